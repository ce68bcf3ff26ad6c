"""Kernel-level tests of the exported entry points that no other test calls by name, and of the host-side launcher branches the rest of
the suite never takes: dr_lin_fields_fwd / _bwd (csrc/emb_pool.hip), dr_din_concat_fwd / _bwd and the large-LDS branch of dr_cin_fwd
(csrc/cin.hip), dr_softmax_rows_fwd / _bwd, dr_cce_prob_rows, dr_csr_plan and dr_csr_transpose (csrc/graph.hip), dr_gather_cols and
dr_adam_step_2d (csrc/multitask.hip), dr_sigmoid_fwd / _bwd and dr_bce_prob_fwd_bwd (csrc/fm_loss.hip), the vocabulary lookups
(csrc/hash_bucket.hip: the spill loop past the 4096 entries held in LDS), the in-batch softmax pair and dr_scores_nt
(csrc/dense_scores.hip: every condition of ib_h2_prepare's choice between the f16x2 register-split kernel and the fp32 kernel).

Each kernel is compared with a plain reference of the same operation (ref_*: numpy / float64 torch on the CPU) at sizes where every
loop runs more than once: more than the 2048 x 256 elements one launch of a grid-stride kernel covers (dr_grid_for), one row past the
4 x 65535 rows of graph.hip's rows_grid, rows longer than one 64-lane stride.

Pitches and canaries.  Where an entry point takes a leading dimension, inputs and outputs are views into wider NaN-filled buffers
(pitch = width + 3, or + 4 where a multiple of 4 is required).  Outputs are pre-filled with NaN: afterwards the padding must still be
NaN and no element of the output may be (a NaN read from an input's padding would show there too).

Exact kernels.  din_concat, gather_cols, sigmoid_bwd, csr_transpose, csr_plan and vocab_lookup do one fp32 operation per element or
integer work: they are compared bit for bit with the same operation in numpy.

Float tolerances.  u = 2^-24.  A fp32 sum whose terms each pass through at most d additions is within g(d) * sum|terms|,
g(d) = d u / (1 - d u); d is read from the kernel's reduction shape (wave per row: ceil(C / 64) chained adds + 6 butterfly steps).
Where expf / logf enter, the yardstick is measured on the reference alone: the same formula in plain fp32 torch / numpy on the CPU,
its largest (scaled) error against float64 on the test's own inputs; the tolerance adds four times that.  Every test prints
err / tol for each output.

The reference helpers run without a GPU and are themselves checked against oracle/tf_semantics.py, oracle/torch_ref.py and
hand-written known answers in test_reference_helpers_against_oracle (unmarked)."""
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import tf_semantics as O
from oracle import torch_ref as T

gpu = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
MIN_FLOAT = float(np.float32(O.MIN_FLOAT))
EPS32 = np.float32(1e-7)                                   # the kernels' `1e-7f` ...
ONE_M_EPS32 = np.float32(1) - EPS32                        # ... and their `1.f - eps`, both rounded to fp32 as the compiler does
GRID_ELEMS = 2048 * 256          # elements one launch of a grid-stride kernel covers before its loop wraps (dr_grid_for)
ROWS_GRID = 4 * 65535            # rows one launch of graph.hip's wave-per-row kernels covers (rows_grid)
_GRAPH_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deep_recommenders_amd", "csrc", "graph.hip")


def gamma(d):
    return d * U / (1.0 - d * U)


def _graph_constants():
    """(DR_CSR_LONG_ROW, CHUNK, RADIX_TILE) as csrc/graph.hip defines them -- read from the source, not guessed"""
    src = open(_GRAPH_HIP).read()
    long_row = int(re.search(r"#define\s+DR_CSR_LONG_ROW\s+(\d+)", src).group(1))
    chunk = int(re.search(r"constexpr\s+int64_t\s+CHUNK\s*=\s*(\d+)\s*;", src).group(1))
    a, b = re.search(r"constexpr\s+int\s+RADIX_TILE\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", src).groups()
    return long_row, chunk, int(a) * int(b)


# ----------------------------------------------------------------------------------------------------------------------------------
# reference helpers (CPU only)
# ----------------------------------------------------------------------------------------------------------------------------------
def _bags(F, C, col_start):
    return [(f, f + 1) for f in range(F)] if col_start is None else [(int(col_start[f]), int(col_start[f + 1])) for f in range(F)]


def ref_lin_fields(ids, F, col_start, row_base, lin_w):
    """dr_lin_fields_fwd in float64: out[b, f] = sum over field f's bag of lin_w[row_base[f] + id], ids < 0 skipped.
    Returns (out, sum of the absolute terms, number of terms), each [B, F]."""
    ids = np.asarray(ids, np.int64)
    w = np.asarray(lin_w, np.float64)
    B, C = ids.shape
    out, mag, cnt = np.zeros((B, F)), np.zeros((B, F)), np.zeros((B, F), np.int64)
    for f, (c0, c1) in enumerate(_bags(F, C, col_start)):
        bag = ids[:, c0:c1]
        ok = bag >= 0
        t = np.where(ok, w[np.where(ok, bag + int(row_base[f]), 0)], 0.0)
        out[:, f], mag[:, f], cnt[:, f] = t.sum(1), np.abs(t).sum(1), ok.sum(1)
    return out, mag, cnt


def ref_lin_fields_bwd(ids, F, col_start, row_base, d_out, scale, R):
    """dr_lin_fields_bwd in float64: per row of lin_w the sum of the fp32 products scale * d_out[b, f] (one rounding each, the
    kernel's `scale * d_out`) over every slot that names it.  Returns (sum, sum of the absolute terms, count), each [R]."""
    ids = np.asarray(ids, np.int64)
    B, C = ids.shape
    g = (np.float32(scale) * np.asarray(d_out, np.float32)).astype(np.float64)
    tot, mag, cnt = np.zeros(R), np.zeros(R), np.zeros(R, np.int64)
    for f, (c0, c1) in enumerate(_bags(F, C, col_start)):
        for c in range(c0, c1):
            ok = ids[:, c] >= 0
            rows = ids[ok, c] + int(row_base[f])
            np.add.at(tot, rows, g[ok, f])
            np.add.at(mag, rows, np.abs(g[ok, f]))
            np.add.at(cnt, rows, 1)
    return tot, mag, cnt


def ref_din_concat(x, y, mode):
    """dr_din_concat_fwd: [x, y] (mode 0), [x, y, x - y] (1), [x, y, x * y] (2) -- one fp32 operation per element"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return np.concatenate([x, y] + ([x - y] if mode == 1 else [x * y] if mode == 2 else []), axis=1)


def ref_din_concat_bwd(x, y, mode, g):
    """dr_din_concat_bwd in fp32: (d_x, d_y), each a list of the admissible results.  Mode 1 is one addition / subtraction; mode 2's
    gx + g3 * y is either a multiply and an add (two roundings) or one fused multiply-add (a single rounding of the exact value,
    formed here in 64-bit-significand long double: a 48-bit product plus a 24-bit addend, then rounded once to fp32)."""
    x, y, g = np.asarray(x, np.float32), np.asarray(y, np.float32), np.asarray(g, np.float32)
    D = x.shape[1]
    gx, gy = g[:, :D], g[:, D:2 * D]
    if mode == 0:
        return [gx], [gy]
    g3 = g[:, 2 * D:3 * D]
    if mode == 1:
        return [gx + g3], [gy - g3]
    ld = np.longdouble
    return ([gx + g3 * y, (gx.astype(ld) + g3.astype(ld) * y.astype(ld)).astype(np.float32)],
            [gy + g3 * x, (gy.astype(ld) + g3.astype(ld) * x.astype(ld)).astype(np.float32)])


def ref_softmax(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def ref_softmax_bwd(y, dy):
    """dx = y * (dy - sum_c y dy) in float64, and the scale of its rounding errors |y| (|dy| + sum_c |y dy|)"""
    y, dy = np.asarray(y, np.float64), np.asarray(dy, np.float64)
    return y * (dy - (y * dy).sum(1, keepdims=True)), np.abs(y) * (np.abs(dy) + np.abs(y * dy).sum(1, keepdims=True))


def ref_cce_prob(p, labels, w=None):
    """dr_cce_prob_rows in float64: q = p / sum p, qc = clip(q, 1e-7f, 1 - 1e-7f) (the constants rounded to fp32 first),
    row_loss = w * -sum_c y log qc; grad = d row_loss / d p = w / S * (sum_{c' unclipped} y_c' - [c unclipped] y_c / q_c).
    Returns (row_loss, grad, q, unclipped)."""
    p, y = np.asarray(p, np.float64), np.asarray(labels, np.float64)
    w = np.ones(len(p)) if w is None else np.asarray(w, np.float64)
    S = p.sum(1, keepdims=True)
    q = p / S
    lo, hi = float(EPS32), float(ONE_M_EPS32)
    unc = (q >= lo) & (q <= hi)
    row = -w * (y * np.log(np.clip(q, lo, hi))).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        grad = w[:, None] / S * ((y * unc).sum(1, keepdims=True) - np.where(unc, y / q, 0.0))
    return row, grad, q, unc


def ref_gather_cols(a, b, col_map):
    """out[:, j] = a[:, map[j]] if map[j] >= 0 else b[:, -map[j] - 1]"""
    return np.stack([a[:, s] if s >= 0 else b[:, -s - 1] for s in np.asarray(col_map).tolist()], axis=1)


def ref_sigmoid(x):
    return O.sigmoid(np.asarray(x, np.float64))


def ref_bce_prob(p, z, mode):
    """dr_bce_prob_fwd_bwd in float64, eps = 1e-7f: mode 1 (tf.losses.log_loss) l = -z log(p + eps) - (1 - z) log(1 - p + eps);
    mode 2 (Keras binary_crossentropy) the same on pc = clip(p, eps, 1 - eps), d pc / d p = 0 where clipped.
    Returns (per-element loss, d(mean loss) / dp, clipped)."""
    p, z = np.asarray(p, np.float64), np.asarray(z, np.float64)
    eps = float(EPS32)
    clipped = np.zeros(p.shape, bool)
    if mode == 2:
        clipped = (p < eps) | (p > float(ONE_M_EPS32))
        p = np.clip(p, eps, float(ONE_M_EPS32))
    l = -z * np.log(p + eps) - (1 - z) * np.log(1 - p + eps)
    d = (-z / (p + eps) + (1 - z) / (1 - p + eps)) * (~clipped) / p.size
    return l, d, clipped


def ref_vocab_lookup(values, vocab):
    """O.vocab_lookup with the first of equal vocabulary entries winning (the kernels' rule; [TF] refuses such a vocabulary):
    later duplicates are replaced by entries nothing can match.  -1 / "" are dropped before the lookup."""
    seen, first = set(), []
    for v in vocab:
        first.append(object() if v in seen else v)
        seen.add(v)
    out = O.vocab_lookup(values, first)
    arr = np.asarray(values, dtype=object).ravel()
    out.ravel()[np.array([i for i, v in enumerate(arr) if v == -1 or v == "" or v == b""], dtype=np.int64)] = -1
    return out


def ref_csr_transpose(row_ptr, col, val, n_rows, n_cols):
    """the CSR of A^T with sorted indices, through scipy (no (row, column) pair may repeat: scipy would add them up)"""
    A = sp.csr_matrix((np.asarray(val, np.float32), np.asarray(col, np.int32), np.asarray(row_ptr, np.int64)), shape=(n_rows, n_cols))
    At = A.transpose().tocsr()
    At.sort_indices()
    return At.indptr.astype(np.int64), At.indices.astype(np.int32), At.data.astype(np.float32)


def ref_csr_plan(row_ptr, long_row, chunk):
    """The plan layout csrc/graph.hip documents.  With nnz = row_ptr[-1], Lmax = nnz // (long_row + 1) and
    Cmax = Lmax + ceil(nnz / chunk), the int64 buffer is
        [0] n_long   [1] n_chunks   long_row[Lmax]   long_first[Lmax + 1]   chunk_row[Cmax]   chunk_kb[Cmax]
    long_row[j] = the j-th row (ascending) with more than `long_row` entries; its chunks are q in [long_first[j], long_first[j + 1]),
    chunk q covers the entries [chunk_kb[q], min(chunk_kb[q] + chunk, row end)) of row chunk_row[q]; long_first[n_long] = n_chunks.
    Only the first n_long / n_long + 1 / n_chunks entries of the four arrays are written.  Returns the expected buffer with -99
    where nothing is written."""
    row_ptr = np.asarray(row_ptr, np.int64)
    nnz = int(row_ptr[-1])
    Lmax = nnz // (long_row + 1)
    Cmax = Lmax + (nnz + chunk - 1) // chunk
    plan = np.full(2 + 2 * Lmax + 1 + 2 * Cmax, -99, np.int64)
    o_row, o_first, o_crow, o_ckb = 2, 2 + Lmax, 2 + 2 * Lmax + 1, 2 + 2 * Lmax + 1 + Cmax
    nl = nc = 0
    for r in range(len(row_ptr) - 1):
        n = int(row_ptr[r + 1] - row_ptr[r])
        if n > long_row:
            plan[o_row + nl], plan[o_first + nl] = r, nc
            for k in range((n + chunk - 1) // chunk):
                plan[o_crow + nc], plan[o_ckb + nc] = r, row_ptr[r] + k * chunk
                nc += 1
            nl += 1
    plan[0], plan[1] = nl, nc
    if Lmax > 0:                                                          # (Lmax == 0: the launcher writes the two counts only)
        plan[o_first + nl] = nc
    return plan


def ref_inbatch(q, c, cand_prob, cand_ids, w, inv_t, d_loss):
    """The in-batch sampled softmax in float64: s_ij = (q_i . c_j - log p_j + dup_ij * MIN_FLOAT) * inv_t with dup_ij = (id_i == id_j
    and i != j); lse_i = logsumexp_j s_ij; loss = sum_i w_i (lse_i - s_ii); G = d_loss * w_i * (softmax_ij - delta_ij) * inv_t."""
    q64, c64 = np.asarray(q, np.float64), np.asarray(c, np.float64)
    B = len(q64)
    raw = q64 @ c64.T
    logp = np.zeros(B) if cand_prob is None else np.log(np.asarray(cand_prob, np.float64))
    s = raw - logp[None, :]
    mask = np.zeros((B, B), bool)
    if cand_ids is not None:
        ids = np.asarray(cand_ids)
        mask = (ids[:, None] == ids[None, :]) & ~np.eye(B, dtype=bool)
        s = np.where(mask, s + MIN_FLOAT, s)
    s = s * float(inv_t)
    m = s.max(1)
    e = np.exp(s - m[:, None])
    l = e.sum(1)
    lse, pos = m + np.log(l), np.diag(s).copy()
    ww = np.ones(B) if w is None else np.asarray(w, np.float64)
    P = e / l[:, None]
    return dict(raw=raw, logp=logp, s=s, mask=mask, lse=lse, pos=pos, loss=float((ww * (lse - pos)).sum()), P=P, w=ww,
                G=float(d_loss) * ww[:, None] * (P - np.eye(B)) * float(inv_t))


def _inbatch_tolerances(ref, q, c, inv_t, d_loss, h2):
    """Error budget of the in-batch softmax kernels, from the score outwards.
    Score.  The matrix product: fp32 kernel g(D + 32) (|q| |c|)_ij; f16x2 kernel 3e-6 max|q c^T| (what tests/test_gpu_h2_gemm.py
    asserts for that kernel family).  -logf(p_j): four times the error of fp32 numpy's log on these p.  Then one addition and the
    multiplication by inv_t (and the mask's addition, exact for the unmasked): 3 u |terms|.  ds_ij = all of it times inv_t.
    lse_i moves by at most max_j ds_ij, plus the combination itself: every partial sum-exp goes through 7 additions in the epilogue
    and 2 roundings per part in the finalize pass (at most 2 ceil(B / 128) parts) -- g(2 parts + 16) of the sum, i.e. that much
    absolutely on its log -- plus four times fp32 torch.logsumexp's own error on these scores, plus 2 u |lse|.
    loss = sum w (lse - pos): the two tolerances, plus g(12) sum w (|lse| + |pos|) for the subtraction, the weight and the block sum
    (one addition per thread, 6 + 2 for the block; the blocks are added in double).
    softmax_ij = exp(s_ij - lse_i) moves relatively by ds_ij + tol_lse_i (<= 2 max ds: "2 p times that much"), u |s - lse| for the
    subtraction and four times fp32 numpy exp's relative error; G adds 4 roundings of (softmax - delta) w inv_t d_loss.  The first-order
    bound is enlarged by 1e-3 of itself for the products of these errors."""
    B, D = q.shape
    a64 = np.abs(np.asarray(q, np.float64)) @ np.abs(np.asarray(c, np.float64)).T
    acc = 3e-6 * np.abs(ref["raw"]).max() if h2 else gamma(D + 32) * a64
    e_log = 0.0
    if np.any(ref["logp"] != 0):
        p32 = np.exp(ref["logp"]).astype(np.float32)
        e_log = 4 * float(np.abs(np.log(p32).astype(np.float64) - np.log(p32.astype(np.float64))).max())
    ds = float(inv_t) * (acc + e_log + 3 * U * (np.abs(ref["raw"]) + np.abs(ref["logp"])[None, :]))
    ds = np.where(ref["mask"], 0.0, ds) + np.zeros((B, B))
    s32 = torch.from_numpy(ref["s"].astype(np.float32))
    yard_lse = float((torch.logsumexp(s32, 1).double() - torch.logsumexp(s32.double(), 1)).abs().max())
    parts = 2 * math.ceil(B / 128)
    tol_lse = ds.max(1) + gamma(2 * parts + 16) + 4 * yard_lse + 2 * U * np.abs(ref["lse"])
    tol_pos = np.diag(ds).copy()
    tol_loss = float((ref["w"] * (tol_lse + tol_pos)).sum() + gamma(12) * (ref["w"] * (np.abs(ref["lse"]) + np.abs(ref["pos"]))).sum())
    x = np.maximum(ref["s"] - ref["lse"][:, None], -87.0).astype(np.float32)
    yard_exp = float(np.abs(np.exp(x).astype(np.float64) / np.exp(x.astype(np.float64)) - 1).max())
    rel = ds + tol_lse[:, None] + 4 * yard_exp + U * np.abs(np.where(ref["mask"], 0.0, ref["s"] - ref["lse"][:, None]))
    tol_G = abs(float(d_loss)) * ref["w"][:, None] * float(inv_t) * (ref["P"] * rel + 4 * U * np.abs(ref["P"] - np.eye(B)))
    k = 1 + 1e-3
    return dict(lse=k * tol_lse, pos=k * tol_pos + 1e-45, loss=k * tol_loss, G=k * np.where(ref["mask"], 0.0, tol_G))


def _unique_csr(rng, n_rows, n_cols, nnz):
    """a CSR with `nnz` distinct (row, column) pairs, or about `nnz` where the matrix has too many cells to draw them exactly;
    columns ascending inside a row, non-zero values"""
    cells = n_rows * n_cols
    if cells <= 8_000_000:
        flat = np.sort(rng.choice(cells, size=nnz, replace=False))
    else:
        flat = np.unique(rng.integers(0, cells, size=nnz))
    return _csr_from_flat(rng, flat, n_rows, n_cols)


def _csr_from_flat(rng, flat, n_rows, n_cols):
    rows, col = flat // n_cols, (flat % n_cols).astype(np.int32)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))]).astype(np.int64)
    val = rng.standard_normal(len(flat)).astype(np.float32)
    val[val == 0] = 1
    return row_ptr, col, val


# ----------------------------------------------------------------------------------------------------------------------------------
# CPU: the references themselves
# ----------------------------------------------------------------------------------------------------------------------------------
def test_reference_helpers_against_oracle():
    rng = np.random.default_rng(0)
    # lin_fields: a known answer by hand, and the oracle's first-order gather on single-valued fields
    ids = np.array([[0, 2, -1, 1], [-1, -1, -1, -1], [1, 1, 1, 0]], np.int64)
    cs, rb = np.array([0, 1, 4], np.int32), np.array([0, 2], np.int64)          # field 0: column 0 (2 rows); field 1: columns 1..3
    w = np.array([1.0, 2.0, 10.0, 20.0, 40.0], np.float32)
    out, mag, cnt = ref_lin_fields(ids, 2, cs, rb, w)
    assert out.tolist() == [[1.0, 60.0], [0.0, 0.0], [2.0, 50.0]] and cnt.tolist() == [[1, 2], [0, 0], [1, 3]]
    d = np.array([[1.0, 2.0], [7.0, 7.0], [4.0, 8.0]], np.float32)
    tot, mag, cnt = ref_lin_fields_bwd(ids, 2, cs, rb, d, -0.5, 6)
    assert tot.tolist() == [-0.5, -2.0, -4.0, -9.0, -1.0, 0.0] and cnt.tolist() == [1, 1, 1, 3, 1, 0]
    sv = rng.integers(0, 7, size=(9, 3))
    wf = rng.standard_normal(21).astype(np.float32)
    out, _, _ = ref_lin_fields(sv, 3, None, np.array([0, 7, 14]), wf)
    want = O.first_order_gather([sv[:, f] for f in range(3)], [wf[7 * f:7 * f + 7] for f in range(3)], 0.0)
    assert np.abs(out.sum(1) - np.asarray(want, np.float64).reshape(-1)).max() < 2e-6
    # din_concat: known answers; the backward is the float64 autograd of the forward
    x, y = np.array([[1.0, 2.0]], np.float32), np.array([[5.0, 7.0]], np.float32)
    assert ref_din_concat(x, y, 0).tolist() == [[1, 2, 5, 7]] and ref_din_concat(x, y, 1).tolist() == [[1, 2, 5, 7, -4, -5]]
    assert ref_din_concat(x, y, 2).tolist() == [[1, 2, 5, 7, 5, 14]]
    g = np.array([[1.0, 2.0, 3.0, 4.0, 10.0, 20.0]], np.float32)
    assert [a.tolist() for a in ref_din_concat_bwd(x, y, 1, g)[0] + ref_din_concat_bwd(x, y, 1, g)[1]] == [[[11, 22]], [[-7, -16]]]
    dx, dy = ref_din_concat_bwd(x, y, 2, g)
    assert all(a.tolist() == [[51, 142]] for a in dx) and all(a.tolist() == [[13, 44]] for a in dy)
    # softmax / CCE on probabilities against the oracle's CCE from logits
    B, C = 6, 70
    logits = (rng.standard_normal((B, C)) * 3).astype(np.float32)
    labels = rng.random((B, C)).astype(np.float32)
    wgt = rng.random(B).astype(np.float32)
    sm = ref_softmax(logits)
    want = float(O.categorical_crossentropy_from_logits_sum(labels, logits, wgt))
    assert abs(-(wgt[:, None] * labels * np.log(sm)).sum() - want) < 1e-6 * abs(want)
    assert np.abs(sm.sum(1) - 1).max() < 1e-14
    t = torch.tensor(logits.astype(np.float64), requires_grad=True)
    dyv = rng.standard_normal((B, C))
    (torch.softmax(t, 1) * torch.tensor(dyv)).sum().backward()
    assert np.abs(ref_softmax_bwd(sm, dyv)[0] - t.grad.numpy()).max() < 1e-12
    mild = (logits / 3).astype(np.float32)                                          # (no probability below the clip edge)
    want = float(O.categorical_crossentropy_from_logits_sum(labels, mild, wgt))
    row, grad, qq, unc = ref_cce_prob(ref_softmax(mild) * 3.0, labels, wgt)         # unnormalised: p / sum p is the softmax again
    assert abs(row.sum() - want) < 1e-6 * abs(want) and unc.all()
    pt = torch.tensor(np.abs(rng.standard_normal((B, C))) + 0.02, requires_grad=True)
    p0 = pt.detach().numpy().copy()
    p0[0, 3] = 0.0                                                                  # clipped from below, labelled
    pt = torch.tensor(p0, requires_grad=True)
    qt = torch.clamp(pt / pt.sum(1, keepdim=True), float(EPS32), float(ONE_M_EPS32))
    lt = -(torch.tensor(labels.astype(np.float64)) * torch.log(qt)).sum(1) * torch.tensor(wgt.astype(np.float64))
    lt.sum().backward()
    row, grad, qq, unc = ref_cce_prob(p0, labels, wgt)
    assert not unc[0, 3] and np.abs(row - lt.detach().numpy()).max() < 1e-12 and np.abs(grad - pt.grad.numpy()).max() < 1e-10
    for Cc in (1, 7, 63, 64, 65, 130, 1000, 3):                                    # the GPU test's inputs: 1e-5 inside the clip edges
        pc, yc, wc, hc = _cce_prob_inputs(np.random.default_rng(Cc), 37, Cc)
        qc, uc = ref_cce_prob(pc, yc, wc)[2:]
        assert np.minimum(np.abs(qc - float(EPS32)), np.abs(qc - float(ONE_M_EPS32)))[uc].min(initial=1.0) >= 1e-5
        assert (uc.sum() == 0) == (Cc == 1) and np.isin(qc[~uc], (0.0, 1.0)).all()
    # gather_cols: a known answer
    a, b = np.array([[1.0, 2.0, 3.0]], np.float32), np.array([[10.0, 20.0]], np.float32)
    assert ref_gather_cols(a, b, [2, -1, 0, -2, 2]).tolist() == [[3, 10, 1, 20, 3]]
    # sigmoid and the two losses on probabilities against the oracle
    assert ref_sigmoid(np.array([0.0]))[0] == 0.5
    pr = rng.uniform(0.01, 0.99, size=500).astype(np.float32)
    z = (rng.random(500) < 0.4).astype(np.float32)
    assert abs(ref_bce_prob(pr, z, 1)[0].mean() - float(O.log_loss(z, pr))) < 1e-6
    assert abs(ref_bce_prob(pr, z, 2)[0].mean() - float(O.keras_binary_crossentropy(z, pr))) < 1e-6
    pt = torch.tensor(pr.astype(np.float64), requires_grad=True)
    zt = torch.tensor(z.astype(np.float64))
    (-zt * torch.log(pt + float(EPS32)) - (1 - zt) * torch.log(1 - pt + float(EPS32))).mean().backward()
    assert np.abs(ref_bce_prob(pr, z, 1)[1] - pt.grad.numpy()).max() < 1e-12
    l, dd, cl = ref_bce_prob(np.array([0.0, 1.0, 0.5], np.float32), np.array([1.0, 0.0, 1.0], np.float32), 2)
    assert cl.tolist() == [True, True, False] and dd[0] == 0 and dd[1] == 0 and dd[2] != 0 and np.isfinite(l).all()
    assert (ref_bce_prob(np.array([0.0, 1.0], np.float32), np.array([1.0, 0.0], np.float32), 1)[1] != 0).all()
    # vocabulary lookup: the oracle where no entry repeats, the first match where one does, -1 / "" dropped
    vocab = [5, 9, 7, 9, 11]
    assert ref_vocab_lookup([9, 7, 4, -1, 11], vocab).tolist() == [1, 2, -1, -1, 4]
    assert np.array_equal(ref_vocab_lookup([9, 7, 4, 11], [5, 9, 7, 11]), O.vocab_lookup([9, 7, 4, 11], [5, 9, 7, 11]))
    assert ref_vocab_lookup(["a", "", "ab", "abc"], ["ab", "a", "abd", "a"]).tolist() == [1, -1, 0, -1]
    # CSR transpose: scipy == a stable sort of the entries by column; a known answer
    rp, col, val = _unique_csr(rng, 7, 40, 60)
    order = np.argsort(col, kind="stable")
    rows = np.repeat(np.arange(7), np.diff(rp))
    trp, tcol, tval = ref_csr_transpose(rp, col, val, 7, 40)
    assert np.array_equal(tcol, rows[order]) and np.array_equal(tval, val[order])
    assert np.array_equal(trp, np.searchsorted(col[order], np.arange(41)))
    trp, tcol, tval = ref_csr_transpose([0, 2, 3], [0, 2, 2], [1.0, 2.0, 3.0], 2, 3)       # [[1, 0, 2], [0, 0, 3]]
    assert trp.tolist() == [0, 1, 1, 3] and tcol.tolist() == [0, 0, 1] and tval.tolist() == [1.0, 2.0, 3.0]
    # CSR plan: a known answer with long_row = 2, chunk = 2 (rows of 3, 2 and 5 entries: rows 0 and 2 are long, 2 and 3 chunks)
    plan = ref_csr_plan([0, 3, 5, 10], 2, 2)
    assert plan.tolist() == [2, 5, 0, 2, -99, 0, 2, 5, -99, 0, 0, 2, 2, 2, -99, -99, -99, 0, 2, 5, 7, 9, -99, -99, -99]
    assert ref_csr_plan([0, 1, 2], 2, 2).tolist() == [0, 0, -99, -99, -99]
    # in-batch softmax: the oracle's loss and the float64 autograd of its restatement (dq = G c, dc = G^T q)
    B, D = 9, 5
    q = rng.standard_normal((B, D)).astype(np.float32)
    c = rng.standard_normal((B, D)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, size=B).astype(np.float32)
    p = rng.uniform(0.05, 0.9, size=B).astype(np.float32)
    ids = rng.integers(0, 3, size=B)
    for kw in _inbatch_option_sets(w, p, ids):
        temp = kw.get("temperature")
        inv_t = 1.0 if temp is None else 1.0 / temp
        r = ref_inbatch(q, c, kw.get("cand_prob"), kw.get("cand_ids"), kw.get("sample_weight"), inv_t, 0.37)
        want = float(O.retrieval_loss(q, c, sample_weight=kw.get("sample_weight"), candidate_sampling_probability=kw.get("cand_prob"),
                                      candidate_ids=kw.get("cand_ids"), temperature=temp))
        assert abs(r["loss"] - want) < 2e-5 * abs(want)
        tq, tc = (torch.tensor(v.astype(np.float64), requires_grad=True) for v in (q, c))
        f64 = lambda v: None if v is None else torch.tensor(np.asarray(v, np.float64))
        lo = T.inbatch_softmax_loss(tq, tc, f64(kw.get("sample_weight")), f64(kw.get("cand_prob")),
                                    None if "cand_ids" not in kw else torch.tensor(ids), temp)
        (lo * 0.37).backward()
        assert abs(r["loss"] - float(lo.detach())) < 1e-9 * abs(float(lo.detach()))
        assert np.abs(r["G"] @ c.astype(np.float64) - tq.grad.numpy()).max() < 1e-10
        assert np.abs(r["G"].T @ q.astype(np.float64) - tc.grad.numpy()).max() < 1e-10
        tol = _inbatch_tolerances(r, q, c, inv_t, 0.37, h2=False)
        assert (tol["lse"] > 0).all() and (tol["G"] >= 0).all() and (tol["G"][r["mask"]] == 0).all() and tol["lse"].max() < 1e-3
    r = ref_inbatch(q, c, None, np.zeros(B, np.int64), w, 2.0, 0.37)                  # every off-diagonal entry masked
    assert r["loss"] == 0.0 and not r["G"].any()
    # the constants of csrc/graph.hip are where the tests look for them
    long_row, chunk, tile = _graph_constants()
    assert long_row > 0 and chunk > 0 and tile % 256 == 0


def _inbatch_option_sets(w, p, ids):
    """the option sets of test_gpu_retrieval.py's _retrieval_loss_and_gradients"""
    return [dict(), dict(temperature=0.5), dict(sample_weight=w), dict(cand_prob=p), dict(cand_ids=ids),
            dict(temperature=0.7, sample_weight=w, cand_prob=p, cand_ids=ids)]


# ----------------------------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ----------------------------------------------------------------------------------------------------------------------------------
def _ops():
    from deep_recommenders_amd import ops
    return ops


def _L():
    from deep_recommenders_amd import _lib
    return _lib


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device="cuda")
    return torch.from_numpy(a).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _nan_buf(rows, width, pad):
    """(view [rows, width], the NaN-filled [rows, width + pad] buffer it lives in)"""
    buf = torch.full((rows, width + pad), NAN, dtype=torch.float32, device="cuda")
    return buf[:, :width], buf


def _pitched(a, pad):
    """the fp32 matrix `a` as a view into a wider buffer whose padding is NaN"""
    view, buf = _nan_buf(a.shape[0], a.shape[1], pad)
    view.copy_(_dev(np.asarray(a, np.float32)))
    return view, buf


def _pad_is_nan(buf, width):
    return bool(torch.isnan(buf[:, width:]).all())


def _written(view):
    """the view as numpy, after asserting that no element is NaN (outputs are pre-filled with NaN)"""
    got = view.cpu().numpy()
    assert not np.isnan(got).any(), "%d elements were not written (or are NaN)" % int(np.isnan(got).sum())
    return got


class _Mode:
    """gemm mode / operand split for the duration of a block"""

    def __init__(self, mode=None, split=None):
        self.mode, self.split = mode, split

    def __enter__(self):
        ops = _ops()
        self.prev = (ops.set_gemm_mode(self.mode) if self.mode else None, ops.set_gemm_split(self.split) if self.split else None)

    def __exit__(self, *a):
        ops = _ops()
        if self.mode:
            ops.set_gemm_mode(self.prev[0])
        if self.split:
            ops.set_gemm_split(self.prev[1])


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. dr_lin_fields_fwd / _bwd
# ----------------------------------------------------------------------------------------------------------------------------------
def _lin_fwd(ids, F, col_start, row_base, lin_w):
    """through the C entry point, into a NaN-filled output of pitch F + 3"""
    L = _L()
    B, C = ids.shape
    out, buf = _nan_buf(B, F, 3)
    idd, csd, rbd, wd = _dev(ids), (None if col_start is None else _dev(col_start)), _dev(row_base), _dev(lin_w)    # (alive until read back)
    L.check(L.lib().dr_lin_fields_fwd(L.ptr(idd), B, F, C, L.ptr(csd), L.ptr(rbd), L.ptr(wd), L.ptr(out), out.stride(0), L.stream_ptr()),
            "dr_lin_fields_fwd")
    assert _pad_is_nan(buf, F)
    return _written(out)


@gpu
@pytest.mark.parametrize("B,F", [(1, 5), (777, 5), (90_000, 6)])
def test_lin_fields_fwd_single_valued(B, F):
    """col_start = None (C == F): one term per output, so bit for bit; ids of -1 give 0; B * F = 540000 is past the 524288 elements
    of one launch"""
    rng = np.random.default_rng(B)
    V = 11
    ids = rng.integers(-1, V, size=(B, F)).astype(np.int64)
    row_base = (np.arange(F) * V).astype(np.int64)
    lin_w = rng.standard_normal(F * V).astype(np.float32)
    got = _lin_fwd(ids, F, None, row_base, lin_w)
    want = np.where(ids >= 0, lin_w[np.maximum(ids, 0) + row_base[None, :]], np.float32(0))
    assert np.array_equal(_bits(got), _bits(want))
    if B > 1:
        assert (ids == -1).any() and B * F > (GRID_ELEMS if B == 90_000 else 0)
    assert np.array_equal(_bits(_ops().lin_fields_fwd(_dev(ids), F, None, _dev(row_base), _dev(lin_w)).cpu().numpy()), _bits(want))


def _bag_inputs(rng, B, V):
    """bags Ls = [1, 3, 1, 4], about 15 % of the ids -1, example 1 with every bag empty; id V - 2 of every field is never drawn"""
    Ls = [1, 3, 1, 4]
    F, C = len(Ls), sum(Ls)
    col_start = np.concatenate([[0], np.cumsum(Ls)]).astype(np.int32)
    ids = rng.integers(0, V - 1, size=(B, C)).astype(np.int64)
    ids[ids == V - 2] = V - 1
    ids[rng.random((B, C)) < 0.15] = -1
    if B > 1:
        ids[1, :] = -1
    row_base = (np.arange(F) * V).astype(np.int64)
    return Ls, F, C, col_start, ids, row_base


@gpu
@pytest.mark.parametrize("B", [1, 3000])
def test_lin_fields_fwd_bags(B):
    """a lane chains the terms of its bag: at most `count` roundings, g(count) * sum|terms|; empty bags give exactly 0"""
    rng = np.random.default_rng(10 + B)
    V = 7
    Ls, F, C, col_start, ids, row_base = _bag_inputs(rng, B, V)
    lin_w = rng.standard_normal(F * V + 3).astype(np.float32)
    got = _lin_fwd(ids, F, col_start, row_base, lin_w).astype(np.float64)
    want, mag, cnt = ref_lin_fields(ids, F, col_start, row_base, lin_w)
    bound = gamma(np.maximum(cnt, 1)) * mag
    err = np.abs(got - want)
    print("lin_fields_fwd bags B=%d: max err / tol %.3g" % (B, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert (got[cnt == 0] == 0).all()
    if B > 1:
        assert (cnt[1] == 0).all() and (cnt == 0).sum() > F and cnt.max() == 4


@gpu
@pytest.mark.parametrize("scale", [1.0, -0.01])
@pytest.mark.parametrize("bags", [False, True])
def test_lin_fields_bwd(scale, bags):
    """one 7-row vocabulary per field, so that thousands of slots add into one row (fp32 atomics in any order: each term passes
    through at most `count` additions, g(count) * (|initial value| + sum|terms|), the terms being the fp32 products scale * d_out);
    accumulated into a pre-filled dst_lin; rows no id names keep their bits; d_out with pitch F + 3; the bag case has more
    (example, field) pairs than the 524288 one launch covers"""
    L = _L()
    rng = np.random.default_rng(int(abs(scale) * 100) + bags)
    V, B = 7, (140_000 if bags else 20_000)                                         # bags: B * F = 560000 slots, past one launch
    if bags:
        Ls, F, C, col_start, ids, row_base = _bag_inputs(rng, B, V)
    else:
        F = C = 5
        col_start = None
        ids = rng.integers(-1, V - 1, size=(B, F)).astype(np.int64)
        ids[ids == V - 2] = V - 1
        row_base = (np.arange(F) * V).astype(np.int64)
    R = F * V + 3
    d_out = rng.standard_normal((B, F)).astype(np.float32)
    dst0 = rng.standard_normal(R).astype(np.float32)
    dv, dbuf = _pitched(d_out, 3)
    dst = _dev(dst0).clone()
    idd, csd, rbd = _dev(ids), (None if col_start is None else _dev(col_start)), _dev(row_base)
    L.check(L.lib().dr_lin_fields_bwd(L.ptr(idd), B, F, C, L.ptr(csd), L.ptr(rbd), L.ptr(dv), dv.stride(0), float(scale), L.ptr(dst),
                                      L.stream_ptr()), "dr_lin_fields_bwd")
    got = dst.cpu().numpy()
    tot, mag, cnt = ref_lin_fields_bwd(ids, F, col_start, row_base, d_out, scale, R)
    assert cnt.max() > 1000 and (cnt == 0).sum() >= F + 3 and (B * F > GRID_ELEMS) == bags
    want = dst0.astype(np.float64) + tot
    bound = gamma(cnt) * (np.abs(dst0.astype(np.float64)) + mag)
    err = np.abs(got.astype(np.float64) - want)
    print("lin_fields_bwd scale=%g bags=%s: max err / tol %.3g" % (scale, bags, (err[cnt > 0] / bound[cnt > 0]).max()))
    assert (err <= bound).all()
    assert np.array_equal(_bits(got[cnt == 0]), _bits(dst0[cnt == 0]))
    assert _pad_is_nan(dbuf, F)
    dst2 = _dev(dst0).clone()                                                      # the ops wrapper names the same kernel
    _ops().lin_fields_bwd(idd, F, csd, rbd, dv, scale, dst2)
    assert (np.abs(dst2.cpu().numpy().astype(np.float64) - want) <= bound).all()


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. dr_din_concat_fwd / _bwd: bit for bit
# ----------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,D", [(1, 1), (3, 5), (257, 64), (70_000, 8)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_din_concat(mode, B, D):
    """the output buffer is always 3 D + 3 wide: in mode 0 its third column block must stay NaN like the padding; 70000 x 8 is past
    one launch"""
    L = _L()
    rng = np.random.default_rng(B + D + mode)
    x = rng.standard_normal((B, D)).astype(np.float32)
    y = rng.standard_normal((B, D)).astype(np.float32)
    n = (3 if mode else 2) * D
    out, buf = _nan_buf(B, 3 * D, 3)
    xd, yd = _dev(x), _dev(y)
    L.check(L.lib().dr_din_concat_fwd(L.ptr(xd), L.ptr(yd), B, D, mode, L.ptr(out), out.stride(0), L.stream_ptr()), "dr_din_concat_fwd")
    want = ref_din_concat(x, y, mode)
    assert np.array_equal(_bits(_written(out[:, :n])), _bits(want))
    assert _pad_is_nan(buf, n)
    assert np.array_equal(_bits(_ops().din_concat_fwd(xd, yd, mode).cpu().numpy()), _bits(want))
    # backward: the three column blocks of d_out folded back, against the fp32 formula
    g = rng.standard_normal((B, n)).astype(np.float32)
    gv, gbuf = _pitched(g, 3 * D + 3 - n)
    dx = torch.full((B, D), NAN, dtype=torch.float32, device="cuda")
    dy = torch.full((B, D), NAN, dtype=torch.float32, device="cuda")
    L.check(L.lib().dr_din_concat_bwd(L.ptr(xd), L.ptr(yd), B, D, mode, L.ptr(gv), gv.stride(0), L.ptr(dx), L.ptr(dy), L.stream_ptr()),
            "dr_din_concat_bwd")
    for name, got, cands in zip(("d_x", "d_y"), (_written(dx), _written(dy)), ref_din_concat_bwd(x, y, mode, g)):
        ok = np.zeros(got.shape, bool)
        for cnd in cands:
            ok |= _bits(got) == _bits(cnd)
        assert ok.all(), "%s mode %d: %d elements are neither the fused nor the unfused fp32 result" % (name, mode, int((~ok).sum()))
    assert _pad_is_nan(gbuf, n)
    ox, oy = _ops().din_concat_bwd(xd, yd, mode, gv)
    assert torch.equal(ox, dx) and torch.equal(oy, dy)


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. dr_softmax_rows_fwd / _bwd
# ----------------------------------------------------------------------------------------------------------------------------------
def _softmax_input(rng, B, C):
    """by row r % 4: N(0, 3) / logits +-80 offset by 1e4 / a constant row / one -inf entry (C > 1)"""
    x = (rng.standard_normal((B, C)) * 3).astype(np.float32)
    kind = np.arange(B) % 4
    big = kind == 1
    x[big] = (rng.choice([-80.0, 80.0], size=(int(big.sum()), C)) + 1.0e4).astype(np.float32)
    x[kind == 2] = np.float32(1.25)
    if C > 1:
        rows = np.nonzero(kind == 3)[0]
        x[rows, rng.integers(0, C, size=len(rows))] = -np.inf
    return x, kind


@gpu
@pytest.mark.parametrize("B,C", [(5, 1), (5, 7), (5, 63), (5, 64), (1, 65), (5, 65), (5, 130), (5, 1000), (ROWS_GRID + 5, 3)])
def test_softmax_rows(B, C):
    """every C around the 64-lane stride (1 .. 3 strides, and 16); B = 262145 is past the 4 x 65535 rows of one launch; x, y, dy and
    dx all pitched.  Forward error on the scale max(y, u): the row sum (ceil(C / 64) + 6 additions), the reciprocal and the product,
    plus four times the fp32 formula's own error.  Backward against float64 fed the kernel's own y: the fma chain of the row sum
    (ceil(C / 64) + 6, one more for the product), the subtraction and the product -- g(d + 3) |y| (|dy| + sum|y dy|), no libm."""
    L = _L()
    rng = np.random.default_rng(B + C)
    x, kind = _softmax_input(rng, B, C)
    d = math.ceil(C / 64) + 6
    xv, xbuf = _pitched(x, 3)
    y, ybuf = _nan_buf(B, C, 4)
    L.check(L.lib().dr_softmax_rows_fwd(L.ptr(xv), xv.stride(0), B, C, L.ptr(y), y.stride(0), L.stream_ptr()), "dr_softmax_rows_fwd")
    got = _written(y)
    assert _pad_is_nan(ybuf, C) and _pad_is_nan(xbuf, C)
    want = ref_softmax(x)
    t = torch.from_numpy(x)
    e = torch.exp(t - t.max(1, keepdim=True).values)
    f32 = (e / e.sum(1, keepdim=True)).numpy().astype(np.float64)
    mag = np.maximum(want, U)
    yard = float((np.abs(f32 - want) / mag).max())
    tol = gamma(d + 3) + 4 * yard
    err = np.abs(got - want) / mag
    sums = np.abs(got.astype(np.float64).sum(1) - 1)
    print("softmax_rows_fwd B=%d C=%d: err / tol %.3g (yardstick %.3g), row sum err / g(d) %.3g" %
          (B, C, err.max() / tol, yard, sums.max() / gamma(d)))
    assert (got >= 0).all() and (got <= 1).all() and err.max() <= tol
    assert (sums <= gamma(d)).all()
    if C & (C - 1) == 0 and (kind == 2).any():
        assert (got[kind == 2] == np.float32(1.0 / C)).all()                       # a constant row: exactly 1 / C
    if C > 1 and (kind == 3).any():
        assert (got[np.isinf(x)] == 0).all() and np.isinf(x).sum() == (kind == 3).sum()
    assert np.array_equal(_bits(_ops().softmax_rows_fwd(xv).cpu().numpy()), _bits(got))
    # backward
    dy = rng.standard_normal((B, C)).astype(np.float32)
    dyv, dybuf = _pitched(dy, 5)
    dx, dxbuf = _nan_buf(B, C, 3)
    L.check(L.lib().dr_softmax_rows_bwd(L.ptr(y), y.stride(0), L.ptr(dyv), dyv.stride(0), B, C, L.ptr(dx), dx.stride(0), L.stream_ptr()),
            "dr_softmax_rows_bwd")
    gdx = _written(dx)
    assert _pad_is_nan(dxbuf, C) and _pad_is_nan(dybuf, C) and _pad_is_nan(ybuf, C)
    wdx, scale = ref_softmax_bwd(got, dy)
    bound = gamma(d + 3) * scale
    errb = np.abs(gdx - wdx)
    print("softmax_rows_bwd B=%d C=%d: err / tol %.3g" % (B, C, (errb / np.maximum(bound, 1e-300)).max()))
    assert (errb <= bound).all()
    assert np.array_equal(_bits(_ops().softmax_rows_bwd(y, dyv).cpu().numpy()), _bits(gdx))


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. dr_cce_prob_rows
# ----------------------------------------------------------------------------------------------------------------------------------
def _cce_prob_inputs(rng, B, C):
    """unnormalised p = |N(0, 1)| + 0.02 (q = p / sum p then stays 1e-5 inside both clip edges for C up to 1000); labels one-hot on
    even rows, sparse soft on odd ones; row 4: the labelled probability is 0 (clipped from below); row 6: p is one-hot at the label
    (clipped from above, every other entry from below); weights in [0.5, 2] with zeros"""
    p = (np.abs(rng.standard_normal((B, C))) + 0.02).astype(np.float32)
    labels = np.zeros((B, C), np.float32)
    hot = rng.integers(0, C, size=B)
    labels[np.arange(B), hot] = 1
    soft = (rng.random((B, C)) * (rng.random((B, C)) < 0.3)).astype(np.float32)
    labels[1::2] = soft[1::2]
    if C > 1:                                                                       # (C = 1: q = 1 in every row, clipped from above)
        p[4, hot[4]] = 0
        p[6] = 0
        p[6, hot[6]] = 3.5
    w = rng.uniform(0.5, 2.0, size=B).astype(np.float32)
    w[[2, 9]] = 0
    return p, labels, w, hot


@gpu
@pytest.mark.parametrize("B,C", [(37, 1), (37, 7), (37, 63), (37, 64), (37, 65), (37, 130), (37, 1000), (ROWS_GRID + 5, 3)])
def test_cce_prob_rows(B, C):
    """Error scale of a row's loss: w sum_c y (|log qc| + 1) -- the + 1 carries the relative error of S = sum p (g(d), d =
    ceil(C / 64) + 6) and of the division into log q; the loss's own sum adds g(d + 1), the product and the weight 2 more: g(2 d + 4)
    of that scale, plus four times the error of the same formula in fp32 torch.  The gradient has no libm: S, the unclipped label
    sum, y / q and three products -- g(2 d + 6) of w / S (sum_unclipped y + y_c / q_c).  B = 37 over the C grid, and once one
    batch past the 4 x 65535 rows of a launch."""
    L = _L()
    rng = np.random.default_rng(C)
    p, labels, w, hot = _cce_prob_inputs(rng, B, C)
    row64, grad64, q64, unc = ref_cce_prob(p, labels, w)
    # the fp32 kernel and the float64 reference agree on which side of a clip edge every element lies
    edge = np.minimum(np.abs(q64 - float(EPS32)), np.abs(q64 - float(ONE_M_EPS32)))
    assert edge[unc].min(initial=1.0) >= 1e-5 and (q64[~unc] == 0).sum() + (q64[~unc] == 1).sum() == (~unc).sum()
    if C > 1:
        assert not unc[4, hot[4]] and not unc[6].any() and unc[[0, 1, 2, 3, 5]].all()
    else:
        assert not unc.any()                                                        # C = 1: q = 1, clipped from above in every row
    d = math.ceil(C / 64) + 6
    pv, pbuf = _pitched(p, 3)
    yv, ybuf = _pitched(labels, 4)
    row = torch.full((B,), NAN, dtype=torch.float32, device="cuda")
    grad, gbuf = _nan_buf(B, C, 5)
    wd = _dev(w)
    L.check(L.lib().dr_cce_prob_rows(L.ptr(pv), pv.stride(0), L.ptr(yv), yv.stride(0), B, C, L.ptr(wd), L.ptr(row), L.ptr(grad),
                                     grad.stride(0), L.stream_ptr()), "dr_cce_prob_rows")
    got_row, got_grad = _written(row), _written(grad)
    assert _pad_is_nan(gbuf, C) and _pad_is_nan(pbuf, C) and _pad_is_nan(ybuf, C)
    tp, ty = torch.from_numpy(p), torch.from_numpy(labels)
    qc32 = torch.clamp(tp / tp.sum(1, keepdim=True), float(EPS32), float(ONE_M_EPS32))
    f32 = (-(ty * torch.log(qc32)).sum(1) * torch.from_numpy(w)).numpy().astype(np.float64)
    lq = np.abs(np.log(np.clip(q64, float(EPS32), float(ONE_M_EPS32))))
    mag1 = (labels.astype(np.float64) * (lq + 1)).sum(1)
    mag = w.astype(np.float64) * mag1
    ok = mag > 0
    yard = float((np.abs(f32 - row64)[ok] / mag[ok]).max())
    tol = gamma(2 * d + 4) + 4 * yard
    err = np.abs(got_row - row64)
    print("cce_prob_rows B=%d C=%d: loss err / tol %.3g (yardstick %.3g)" % (B, C, (err[ok] / mag[ok]).max() / tol, yard))
    assert (err <= tol * mag).all() and np.isfinite(got_row).all()
    assert (got_row[w == 0] == 0).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        gmag = w.astype(np.float64)[:, None] / p.astype(np.float64).sum(1, keepdims=True) * \
            ((labels * unc).sum(1, keepdims=True) + np.where(unc, labels / q64, 0.0))
    gerr = np.abs(got_grad - grad64)
    print("cce_prob_rows B=%d C=%d: grad err / tol %.3g" % (B, C, (gerr / np.maximum(gamma(2 * d + 6) * gmag, 1e-300)).max()))
    assert (gerr <= gamma(2 * d + 6) * gmag).all()
    # grad = NULL: the same losses; no weights: w = 1; the ops wrapper
    row2 = torch.full((B,), NAN, dtype=torch.float32, device="cuda")
    L.check(L.lib().dr_cce_prob_rows(L.ptr(pv), pv.stride(0), L.ptr(yv), yv.stride(0), B, C, L.ptr(wd), L.ptr(row2), None, 0,
                                     L.stream_ptr()), "dr_cce_prob_rows")
    assert torch.equal(row2.view(torch.int32), row.view(torch.int32))
    r3, g3 = _ops().cce_prob_rows(pv, yv, None, want_grad=True)
    row1 = ref_cce_prob(p, labels, None)[0]
    assert (np.abs(r3.cpu().numpy() - row1) <= tol * mag1).all()
    r4, g4 = _ops().cce_prob_rows(pv, yv, wd, want_grad=False)
    assert g4 is None and torch.equal(r4.view(torch.int32), row.view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. dr_gather_cols: bit for bit
# ----------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M,N", [(1, 1), (300, 33), (9000, 60)])
def test_gather_cols(M, N):
    """a map mixing columns of a (>= 0) and of b (< 0) with repeated sources, three different pitches; b = None with a map that names
    a only (a map pointing into a NULL operand is outside the contract); 9000 x 60 is past one launch"""
    ops = _ops()
    rng = np.random.default_rng(M + N)
    Na, Nb = 7, 4
    a = rng.standard_normal((M, Na)).astype(np.float32)
    b = rng.standard_normal((M, Nb)).astype(np.float32)
    cmap = np.where(rng.random(N) < 0.5, rng.integers(0, Na, size=N), -rng.integers(1, Nb + 1, size=N)).astype(np.int32)
    if N > 4:
        cmap[:4] = [Na - 1, -Nb, Na - 1, -1]
    av, abuf = _pitched(a, 3)
    bv, bbuf = _pitched(b, 5)
    out, obuf = _nan_buf(M, N, 4)
    ops.gather_cols(av, bv, _dev(cmap), out)
    assert np.array_equal(_bits(_written(out)), _bits(ref_gather_cols(a, b, cmap)))
    assert _pad_is_nan(obuf, N) and _pad_is_nan(abuf, Na) and _pad_is_nan(bbuf, Nb)
    amap = rng.integers(0, Na, size=N).astype(np.int32)
    out2, obuf2 = _nan_buf(M, N, 3)
    ops.gather_cols(av, None, _dev(amap), out2)
    assert np.array_equal(_bits(_written(out2)), _bits(a[:, amap])) and _pad_is_nan(obuf2, N)
    bmap = (-rng.integers(1, Nb + 1, size=N)).astype(np.int32)
    out3, obuf3 = _nan_buf(M, N, 3)
    ops.gather_cols(None, bv, _dev(bmap), out3)
    assert np.array_equal(_bits(_written(out3)), _bits(b[:, -bmap - 1])) and _pad_is_nan(obuf3, N)


# ----------------------------------------------------------------------------------------------------------------------------------
# 6. dr_adam_step_2d
# ----------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 5), (300, 33), (2049, 1025)])
def test_adam_step_2d(rows, cols):
    """the column slice [:, 3:3 + cols] of a wider parameter and gradient, contiguous m / v, three steps with grad_scale = 0.5:
    bit-equal to dr_adam_step on contiguous copies (the header promises its arithmetic), within test_adam_step_dense's bounds of the
    float64 restatement, and the columns outside the slice keep their bits; 2049 x 1025 is past one launch (2048 x 256 threads)"""
    ops = _ops()
    rng = np.random.default_rng(rows + cols)
    Wp, Wg = cols + 8, cols + 5
    p0 = rng.standard_normal((rows, Wp)).astype(np.float32)
    P = _dev(p0).clone()
    m = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    v = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    pc = P[:, 3:3 + cols].clone().reshape(-1)                                        # (a copy even where the slice is one row)
    mc, vc = torch.zeros(rows * cols, device="cuda"), torch.zeros(rows * cols, device="cuda")
    tp = torch.tensor(p0[:, 3:3 + cols].astype(np.float64))
    tm, tv = torch.zeros_like(tp), torch.zeros_like(tp)
    for step in range(1, 4):
        g = rng.standard_normal((rows, Wg)).astype(np.float32)
        G = _dev(g)
        lr_t = ops.adam_lr_t(0.01, 0.9, 0.999, step)
        ops.adam_step_2d(P[:, 3:3 + cols], G[:, 3:3 + cols], m, v, lr_t, 0.9, 0.999, 1e-8, grad_scale=0.5)
        ops.adam_step(pc, G[:, 3:3 + cols].contiguous().reshape(-1), mc, vc, lr_t, 0.9, 0.999, 1e-8, grad_scale=0.5)
        T.adam_dense_step(tp, torch.tensor(g[:, 3:3 + cols].astype(np.float64)) * 0.5, tm, tv, 0.01, step)
        assert torch.equal(P[:, 3:3 + cols].reshape(-1).view(torch.int32), pc.view(torch.int32)), step
        assert torch.equal(m.reshape(-1).view(torch.int32), mc.view(torch.int32))
        assert torch.equal(v.reshape(-1).view(torch.int32), vc.view(torch.int32))
    got = P.cpu().numpy()
    np.testing.assert_allclose(got[:, 3:3 + cols], tp.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(m.cpu().numpy(), tm.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(v.cpu().numpy(), tv.numpy(), rtol=1e-5, atol=1e-7)
    print("adam_step_2d %dx%d: max |p - float64| %.3g (bound 2e-5)" % (rows, cols, np.abs(got[:, 3:3 + cols] - tp.numpy()).max()))
    assert np.array_equal(_bits(got[:, :3]), _bits(p0[:, :3])) and np.array_equal(_bits(got[:, 3 + cols:]), _bits(p0[:, 3 + cols:]))
    assert not np.array_equal(got[:, 3:3 + cols], p0[:, 3:3 + cols])


# ----------------------------------------------------------------------------------------------------------------------------------
# 7. dr_sigmoid_fwd / _bwd, dr_bce_prob_fwd_bwd
# ----------------------------------------------------------------------------------------------------------------------------------
SPECIAL_X = [-104.0, -88.0, -20.0, 0.0, 20.0, 88.0, 104.0]
ELEM_SIZES = [1, 255, 257, 600_000]                        # 600000 is past one launch (524288) of the sigmoid kernels and past the
#                                                            512 x 256 threads of the loss kernel


@gpu
@pytest.mark.parametrize("n", ELEM_SIZES)
def test_sigmoid_fwd_bwd(n):
    """forward within four times the error of fp32 torch's 1 / (1 + exp(-x)) and the rtol = 2e-5, atol = 2e-6 the suite asks of
    sigmoid elsewhere; finite, in [0, 1] and monotone over 0, +-20, +-88, +-104 (exp overflows past 88.7: exactly 0 / 1, no NaN);
    backward dy * y * (1 - y): two products and an exact-or-rounded subtraction in this order, bit for bit"""
    ops = _ops()
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 4).astype(np.float32)
    k = min(n, len(SPECIAL_X))
    x[:k] = SPECIAL_X[:k] if n >= len(SPECIAL_X) else [0.0]
    guard = torch.full((n + 64,), NAN, dtype=torch.float32, device="cuda")
    L = _L()
    xd = _dev(x)
    L.check(L.lib().dr_sigmoid_fwd(L.ptr(xd), n, L.ptr(guard), L.stream_ptr()), "dr_sigmoid_fwd")
    got = _written(guard[:n])
    assert bool(torch.isnan(guard[n:]).all())
    want = ref_sigmoid(x)
    tx = torch.from_numpy(x)
    yard = float(np.abs((1 / (1 + torch.exp(-tx))).numpy().astype(np.float64) - want).max())
    err = np.abs(got - want)
    print("sigmoid_fwd n=%d: err %.3g tol %.3g (yardstick %.3g)" % (n, err.max(), 4 * yard, yard))
    assert err.max() <= 4 * yard and (err <= 2e-6 + 2e-5 * want).all()
    assert (got >= 0).all() and (got <= 1).all()
    if n >= len(SPECIAL_X):
        s = got[:len(SPECIAL_X)]
        assert (np.diff(s) >= 0).all() and s[0] == 0 and s[3] == 0.5 and s[-1] == 1 and s[-2] == 1
    assert np.array_equal(_bits(ops.sigmoid_fwd(xd).cpu().numpy()), _bits(got))
    dy = rng.standard_normal(n).astype(np.float32)
    dxg = torch.full((n + 64,), NAN, dtype=torch.float32, device="cuda")
    dyd = _dev(dy)
    L.check(L.lib().dr_sigmoid_bwd(L.ptr(guard), L.ptr(dyd), n, L.ptr(dxg), L.stream_ptr()), "dr_sigmoid_bwd")
    wdx = dy * got * (np.float32(1) - got)
    assert wdx.dtype == np.float32 and np.array_equal(_bits(_written(dxg[:n])), _bits(wdx)) and bool(torch.isnan(dxg[n:]).all())
    assert np.array_equal(_bits(ops.sigmoid_bwd(guard[:n], dyd).cpu().numpy()), _bits(wdx))


@gpu
@pytest.mark.parametrize("n", ELEM_SIZES)
@pytest.mark.parametrize("mode", [1, 2])
def test_bce_prob_fwd_bwd(mode, n):
    """probabilities in (0.01, 0.99) and exactly 0 and 1, each with the matching and the opposite label.  The mean loss: every
    element's loss is off by at most four times the largest element error of the same formula in fp32 torch, so the mean is too; the
    sum itself adds g(ceil(n / (512 x 256)) + 9) of mean|l| (a thread's chain, 6 butterfly steps, 2 for the four waves; the blocks are
    added in double and the mean is rounded to fp32 once).  d_prob element by element on the scale (z / (pc + eps) + (1 - z) / (1 - pc + eps)) / n: four times the fp32
    formula's relative error plus g(4).  Mode 2's clipped elements have d_prob == 0 exactly, mode 1's do not; two runs agree bit for
    bit."""
    ops = _ops()
    rng = np.random.default_rng(10 * n + mode)
    p = rng.uniform(0.01, 0.99, size=n).astype(np.float32)
    z = (rng.random(n) < 0.4).astype(np.float32)
    if n >= 255:
        p[:4], z[:4] = [0.0, 0.0, 1.0, 1.0], [0.0, 1.0, 0.0, 1.0]
    else:
        p[0], z[0] = 0.0, 1.0
    l64, d64, clipped = ref_bce_prob(p, z, mode)
    assert clipped.sum() == ((4 if n >= 255 else 1) if mode == 2 else 0) and np.isfinite(l64).all()
    pd, zd = _dev(p), _dev(z)
    loss, d_prob = ops.bce_prob_fwd_bwd(pd, zd, mode)
    loss_b, d_prob_b = ops.bce_prob_fwd_bwd(pd, zd, mode)
    assert torch.equal(loss.view(torch.int32), loss_b.view(torch.int32))
    assert torch.equal(d_prob.view(torch.int32), d_prob_b.view(torch.int32))
    assert float(ops.bce_prob_fwd_bwd(pd, zd, mode, want_grad=False)[0]) == float(loss)
    # the same formula in fp32 torch
    tp, tz, eps = torch.from_numpy(p), torch.from_numpy(z), float(EPS32)
    pc = torch.clamp(tp, eps, float(ONE_M_EPS32)) if mode == 2 else tp
    l32 = (-tz * torch.log(pc + eps) - (1 - tz) * torch.log(1 - pc + eps)).numpy().astype(np.float64)
    yard = float(np.abs(l32 - l64).max())
    tol = 4 * yard + gamma(math.ceil(n / (512 * 256)) + 9) * np.abs(l64).mean()
    got = float(loss)
    print("bce_prob mode=%d n=%d: loss err / tol %.3g (yardstick %.3g)" % (mode, n, abs(got - l64.mean()) / tol, yard))
    assert np.isfinite(got) and abs(got - l64.mean()) <= tol
    ref = float(O.log_loss(z, p) if mode == 1 else O.keras_binary_crossentropy(z, p))
    if not clipped.any():
        assert abs(got - ref) <= tol + 1e-6 * abs(ref)
    gd = d_prob.cpu().numpy()
    assert np.isfinite(gd).all()
    with np.errstate(divide="ignore"):
        pc64 = np.clip(p.astype(np.float64), eps, float(ONE_M_EPS32)) if mode == 2 else p.astype(np.float64)
        mag = (z / (pc64 + eps) + (1 - z) / (1 - pc64 + eps)) / n
    d32 = ((-tz / (pc + eps) + (1 - tz) / (1 - pc + eps)) / n).numpy().astype(np.float64) * (~clipped)
    yard_d = float((np.abs(d32 - d64) / mag).max())
    derr = np.abs(gd - d64) / mag
    print("bce_prob mode=%d n=%d: d_prob err / tol %.3g (yardstick %.3g)" % (mode, n, derr.max() / (4 * yard_d + gamma(4)), yard_d))
    assert derr.max() <= 4 * yard_d + gamma(4)
    edge = (p == 0) | (p == 1)
    if mode == 2:
        assert (gd[clipped] == 0).all() and (gd[~clipped] != 0).all()
    else:
        assert (gd[edge] != 0).all()


# ----------------------------------------------------------------------------------------------------------------------------------
# 8. vocabulary lookups: exact
# ----------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [0, 1, 3000, GRID_ELEMS + 1000])
def test_vocab_lookup_i64_past_the_lds_copy(n):
    """a vocabulary of 5000 keys: the first 4096 are searched in LDS, the rest by the spill loop over global memory; probes on both
    sides of entry 4096; one key at 4090 and again at 4100 (the first wins), one only past 4096 twice; -1 -> -1; misses; more probes
    than one launch covers"""
    ops = _ops()
    rng = np.random.default_rng(n)
    vocab = (rng.permutation(20_000)[:5000].astype(np.int64) - 3000) * 7919
    vocab[vocab == -1] = -2
    vocab[4100] = vocab[4090]
    vocab[4700] = vocab[4200]
    keys = np.concatenate([vocab[[0, 4095, 4096, 4999, 4090, 4100, 4200, 4700]], [-1, 1, 2 ** 62],
                           rng.choice(vocab, size=max(0, n - 11)), ])[:n].astype(np.int64)
    if n > 100:
        miss = (rng.random(n) < 0.2) & (np.arange(n) >= 11)
        keys[miss] = keys[miss] + 1                                                # 7919 apart: a neighbour is never a key
        keys[(rng.random(n) < 0.05) & (np.arange(n) >= 11)] = -1
    got = ops.vocab_lookup_i64(_dev(keys), _dev(vocab)).cpu().numpy()
    want = ref_vocab_lookup(keys.tolist(), vocab.tolist())
    assert np.array_equal(got, want)
    if n >= 3000:
        assert got[:11].tolist() == [0, 4095, 4096, 4999, 4090, 4090, 4200, 4200, -1, -1, -1]
        assert (got > 4096).sum() > 100 and (got == -1).sum() > 100 and ((got >= 0) & (got < 4096)).sum() > 100
    if n:
        assert (ops.vocab_lookup_i64(_dev(keys), torch.empty(0, dtype=torch.int64, device="cuda")).cpu().numpy() == -1).all()   # vocab_len = 0
        small = vocab[:21].copy()                                                  # a vocabulary of the reference's size
        assert np.array_equal(ops.vocab_lookup_i64(_dev(keys), _dev(small)).cpu().numpy(), ref_vocab_lookup(keys.tolist(), small.tolist()))


@gpu
def test_vocab_lookup_strings():
    """entries that are prefixes of one another, equal-length near-misses differing in the last byte, "" -> -1, a duplicate
    vocabulary entry (the first wins), an empty vocabulary, more values than one launch covers"""
    ops = _ops()
    vocab = ["ab", "a", "abc", "abd", "a", "", "xyz", "abcdefghijklmnopqrstuvwxy1"]
    values = ["a", "ab", "abc", "abd", "abe", "abcd", "", "b", "xyz", "xy", "xyzz", "abcdefghijklmnopqrstuvwxy1",
              "abcdefghijklmnopqrstuvwxy2", "A"]
    got = ops.vocab_lookup_strings(values, vocab).cpu().numpy()
    want = ref_vocab_lookup(values, vocab)
    assert want.tolist() == [1, 0, 2, 3, -1, -1, -1, -1, 6, -1, -1, 7, -1, -1]
    assert np.array_equal(got, want)
    assert (ops.vocab_lookup_strings(values, []).cpu().numpy() == -1).all()
    rng = np.random.default_rng(5)
    many = [values[i] for i in rng.integers(0, len(values), size=GRID_ELEMS + 300)]
    assert np.array_equal(ops.vocab_lookup_strings(many, vocab).cpu().numpy(), ref_vocab_lookup(many, vocab))


# ----------------------------------------------------------------------------------------------------------------------------------
# 9. dr_csr_transpose, dr_csr_plan called directly
# ----------------------------------------------------------------------------------------------------------------------------------
def _transpose_direct(row_ptr, col, val, n_rows, n_cols):
    """through the C entry point into guarded outputs (8 extra elements behind each, which must keep their fill)"""
    L = _L()
    nnz = len(col)
    t_row_ptr = torch.full((n_cols + 1 + 8,), -7, dtype=torch.int64, device="cuda")
    t_col = torch.full((nnz + 8,), -7, dtype=torch.int32, device="cuda")
    t_val = torch.full((nnz + 8,), NAN, dtype=torch.float32, device="cuda")
    nbytes = L.lib().dr_csr_transpose_workspace_bytes(nnz, n_cols)
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device="cuda")
    rpd, cold, vald = _dev(row_ptr), _dev(col), _dev(val)
    L.check(L.lib().dr_csr_transpose(L.ptr(rpd), L.ptr(cold), L.ptr(vald), n_rows, n_cols, nnz, L.ptr(t_row_ptr),
                                     L.ptr(t_col), L.ptr(t_val), L.ptr(ws), nbytes, L.stream_ptr()), "dr_csr_transpose")
    assert bool((t_row_ptr[n_cols + 1:] == -7).all()) and bool((t_col[nnz:] == -7).all()) and bool(torch.isnan(t_val[nnz:]).all())
    return t_row_ptr[:n_cols + 1].cpu().numpy(), t_col[:nnz].cpu().numpy(), _written(t_val[:nnz])


def _assert_transpose(row_ptr, col, val, n_rows, n_cols):
    got = _transpose_direct(row_ptr, col, val, n_rows, n_cols)
    want = ref_csr_transpose(row_ptr, col, val, n_rows, n_cols)
    assert np.array_equal(got[0], want[0]), "t_row_ptr"
    assert np.array_equal(got[1], want[1]), "t_col"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), "t_val"
    ops_got = _ops().csr_transpose(_dev(row_ptr), _dev(col), _dev(val), n_rows, n_cols, len(col))
    assert np.array_equal(ops_got[0].cpu().numpy(), want[0]) and np.array_equal(ops_got[1].cpu().numpy(), want[1])


@gpu
def test_csr_transpose_four_radix_passes():
    """n_cols = 2^24 + 3 needs four 8-bit passes (the widest case elsewhere, 150000 columns, needs three): with an even number of
    passes the payload starts in the outputs and must end there.  About 5000 entries spread over the whole column range, two of them
    in column 2^24 + 2 (the only column whose fourth digit is not 0)"""
    rng = np.random.default_rng(24)
    n_rows, n_cols = 50, 2 ** 24 + 3
    flat = rng.integers(0, n_rows * n_cols, size=5000)
    flat = np.unique(np.concatenate([flat, [3 * n_cols + 2 ** 24 + 2, 40 * n_cols + 2 ** 24 + 2, 7 * n_cols, 9 * n_cols + 2 ** 24]]))
    row_ptr, col, val = _csr_from_flat(rng, flat, n_rows, n_cols)
    assert (col == 2 ** 24 + 2).sum() == 2 and col.min() == 0 and len(np.unique(col >> 16)) > 200
    _assert_transpose(row_ptr, col, val, n_rows, n_cols)


@gpu
@pytest.mark.parametrize("n_cols", [200, 300, 70_000])
@pytest.mark.parametrize("tiles", [1, 2])
def test_csr_transpose_whole_radix_tiles(tiles, n_cols):
    """nnz equal to exactly one and exactly two radix tiles (RADIX_TILE of csrc/graph.hip, read from the source: 256 x 8 = 2048
    entries), where the last tile has no remainder to mask; 200 / 300 / 70000 columns: one, two and three passes"""
    tile = _graph_constants()[2]
    rng = np.random.default_rng(tiles * n_cols)
    row_ptr, col, val = _unique_csr(rng, 64, n_cols, tiles * tile)
    assert len(col) == tiles * tile
    _assert_transpose(row_ptr, col, val, 64, n_cols)


@gpu
def test_csr_transpose_degenerate_shapes():
    """a single entry; a matrix whose entries all sit in one column (every key equal: the scatter is stable, rows stay ascending),
    one entry past a radix tile, in more rows than one launch of the row expansion covers"""
    rng = np.random.default_rng(1)
    tile = _graph_constants()[2]
    _assert_transpose(np.array([0, 0, 1, 1], np.int64), np.array([4], np.int32), np.array([2.5], np.float32), 3, 6)
    _assert_transpose(np.array([0, 1], np.int64), np.array([0], np.int32), np.array([-1.0], np.float32), 1, 1)
    nnz, n_rows = tile + 1, 9500                                                     # (2048 x 4 rows: one launch of the row expansion)
    rows_with = np.sort(rng.choice(n_rows, size=nnz, replace=False))
    rows_with[-1] = n_rows - 1
    row_ptr = np.searchsorted(rows_with, np.arange(n_rows + 1)).astype(np.int64)
    col = np.full(nnz, 37, np.int32)
    val = rng.standard_normal(nnz).astype(np.float32)
    got = _transpose_direct(row_ptr, col, val, n_rows, 300)
    assert np.array_equal(got[1], rows_with.astype(np.int32)) and np.array_equal(_bits(got[2]), _bits(val))
    _assert_transpose(row_ptr, col, val, n_rows, 300)


def _plan_csr(rng, lens, n_cols):
    lens = np.asarray(lens, np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(n_cols, size=int(lens[r]), replace=False)) for r in np.nonzero(lens)[0]] +
                         [np.zeros(0, np.int64)]).astype(np.int32)
    val = rng.standard_normal(len(col)).astype(np.float32)
    return row_ptr, col, val


@gpu
@pytest.mark.parametrize("case", ["no-long-rows", "too-few-entries", "one-long-row", "three-long-rows", "many-rows"])
def test_csr_plan_layout_and_spmm(case):
    """The plan buffer against ref_csr_plan's restatement of the layout csrc/graph.hip documents (int64: [0] n_long, [1] n_chunks,
    long_row[Lmax], long_first[Lmax + 1], chunk_row[Cmax], chunk_kb[Cmax]; Lmax = nnz // (LONG + 1), Cmax = Lmax + ceil(nnz / CHUNK);
    entries past the counts are not written), LONG = DR_CSR_LONG_ROW and CHUNK read from the source.  Rows exactly at the threshold
    (not long), one entry above it (two chunks, the second of one entry), of exactly two chunks, and of three chunks and a remainder;
    600000 rows (the plan kernels' launch covers 2048 x 256) with long rows on both sides of that seam.
    dr_csr_spmm with that plan against float64 at D = 5: a short row is one fma chain of its entries, a long row chains a chunk and
    then adds the chunks in order -- g(min(len, CHUNK) + chunks + 1) sum|val x|."""
    L = _L()
    ops = _ops()
    LONG, CHUNK, _ = _graph_constants()
    rng = np.random.default_rng(len(case))
    lens = {"no-long-rows": [LONG, 3, 0, LONG - 1, 40, LONG],
            "too-few-entries": [LONG - 1, 0, 1],                                        # nnz <= LONG: the launcher's early branch
            "one-long-row": [5, LONG + 1, 0, 7],
            "three-long-rows": [LONG, LONG + 1, 2, 3 * CHUNK + 5, 0, max(2 * CHUNK, LONG + 1), 1],
            "many-rows": None}[case]
    if lens is None:
        lens = np.zeros(600_000, np.int64)
        lens[rng.choice(600_000, size=1500, replace=False)] = 1
        lens[[3, GRID_ELEMS - 1, GRID_ELEMS, 599_990]] = [LONG + 1, LONG, 2 * CHUNK + 1, LONG + 2]
    n_rows, n_cols, D = len(lens), 4 * CHUNK + 50, 5
    row_ptr, col, val = _plan_csr(rng, lens, n_cols)
    nnz = len(col)
    want = ref_csr_plan(row_ptr, LONG, CHUNK)
    assert want[0] == {"no-long-rows": 0, "too-few-entries": 0, "one-long-row": 1, "three-long-rows": 3, "many-rows": 3}[case]
    nbytes = L.lib().dr_csr_plan_bytes(nnz)
    assert nbytes == 8 * len(want)
    plan = torch.full((len(want) + 4,), -99, dtype=torch.int64, device="cuda")
    wbytes = L.lib().dr_csr_plan_workspace_bytes(n_rows)
    ws = torch.empty(max(1, wbytes // 8), dtype=torch.int64, device="cuda")
    rp = _dev(row_ptr)
    L.check(L.lib().dr_csr_plan(L.ptr(rp), n_rows, nnz, L.ptr(plan), nbytes, L.ptr(ws), wbytes, L.stream_ptr()), "dr_csr_plan")
    got = plan.cpu().numpy()
    assert np.array_equal(got[:len(want)], want), (got[:len(want)].tolist(), want.tolist())
    assert (got[len(want):] == -99).all()
    nl, nc = int(want[0]), int(want[1])
    oplan = ops.csr_plan(rp, n_rows, nnz).cpu().numpy()
    Lmax = nnz // (LONG + 1)
    assert oplan[:2].tolist() == [nl, nc] and np.array_equal(oplan[2:2 + nl], want[2:2 + nl])
    if Lmax:
        assert np.array_equal(oplan[2 + Lmax:2 + Lmax + nl + 1], want[2 + Lmax:2 + Lmax + nl + 1])
    # the product with this plan
    X = rng.standard_normal((n_cols, D)).astype(np.float32)
    Xv, Xbuf = _pitched(X, 3)                                                        # pitch 8: a multiple of 4 floats
    out, obuf = _nan_buf(n_rows, D, 3)
    ops.csr_spmm(rp, _dev(col), _dev(val), n_rows, nnz, Xv, plan[:len(want)], out=out)
    res = _written(out)
    assert _pad_is_nan(obuf, D) and _pad_is_nan(Xbuf, D)
    A = sp.csr_matrix((val.astype(np.float64), col, row_ptr), shape=(n_rows, n_cols))
    ref = A @ X.astype(np.float64)
    mag = abs(A) @ np.abs(X.astype(np.float64))
    ln = np.asarray(lens)
    d = np.minimum(ln, CHUNK) + np.where(ln > LONG, (ln + CHUNK - 1) // CHUNK, 0) + 1
    bound = gamma(d)[:, None] * mag
    err = np.abs(res - ref)
    print("csr_spmm with the %s plan: err / tol %.3g" % (case, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all() and (res[ln == 0] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------------------
# 10. in-batch softmax, element by element
# ----------------------------------------------------------------------------------------------------------------------------------
def _takes_h2(split, B, D):
    """ib_h2_prepare (csrc/dense_scores.hip): the f16x2 register-split kernel iff the split is f16x2, D % 4 == 0, D <= 512, B >= 256"""
    return split == "f16x2" and D % 4 == 0 and D <= 512 and B >= 256


def _inbatch_inputs(B, D):
    rng = np.random.default_rng(B * 1000 + D)
    q = (rng.standard_normal((B, D)) / np.sqrt(D)).astype(np.float32)
    c = (rng.standard_normal((B, D)) / np.sqrt(D)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, size=B).astype(np.float32)
    p = rng.uniform(0.05, 0.9, size=B).astype(np.float32)
    ids = rng.integers(0, max(2, B // 3), size=B).astype(np.int64)
    return q, c, w, p, ids


def _run_inbatch(q, c, kw, d_loss):
    ops = _ops()
    dv = lambda v: None if v is None else _dev(v)
    temp = kw.get("temperature")
    inv_t = 1.0 if temp is None else 1.0 / temp
    args = dict(cand_prob=dv(kw.get("cand_prob")), cand_ids=dv(kw.get("cand_ids")), sample_weight=dv(kw.get("sample_weight")),
                inv_temperature=inv_t)
    qd, cd = _dev(q), _dev(c)
    loss, row_lse, pos = ops.inbatch_softmax_fwd(qd, cd, **args)
    G = ops.inbatch_softmax_grad_scores(qd, cd, row_lse, d_loss, **args)
    return float(loss), row_lse, pos, G, float(np.float32(inv_t))


# every B of {255, 256, 257, 385} and every D of {4, 6, 30, 512, 516} once, B = 257 with D = 30 and with D = 512, and B = 256 with a D
# the f16x2 kernel takes so that B = 255 / 256 differ in nothing but the B >= 256 condition
INBATCH_SHAPES = [(255, 4), (256, 4), (256, 6), (257, 30), (257, 512), (385, 516)]


@gpu
@pytest.mark.parametrize("B,D", INBATCH_SHAPES)
@pytest.mark.parametrize("split", ["f16x2", "bf16x3"])
def test_inbatch_softmax_elementwise(split, B, D):
    """row_lse, pos_score, loss and every element of G against float64 (budget: _inbatch_tolerances) for the six option sets of
    test_retrieval_loss_and_gradients with d_loss = 0.37.  The dispatch: under the f16x2 split with D % 4 == 0, D <= 512 and
    B >= 256 the register-split kernel runs, and its bits differ from the fp32 kernel's; in every other case (B = 255; D = 6 and 30:
    the fp32 kernel's unaligned loads; D = 516) the result is bit for bit the fp32 kernel's, i.e. what the bf16x3 split gives."""
    q, c, w, p, ids = _inbatch_inputs(B, D)
    d_loss = 0.37
    h2 = _takes_h2(split, B, D)
    for kw in _inbatch_option_sets(w, p, ids):
        with _Mode(split=split):
            loss, row_lse, pos, G, inv_t = _run_inbatch(q, c, kw, d_loss)
        ref = ref_inbatch(q, c, kw.get("cand_prob"), kw.get("cand_ids"), kw.get("sample_weight"), inv_t, d_loss)
        # G was computed from the kernel's own row_lse: the reference gets it too, its deviation is inside tol["G"]
        tol = _inbatch_tolerances(ref, q, c, inv_t, d_loss, h2)
        g_lse, g_pos, g_G = (t.cpu().numpy().astype(np.float64) for t in (row_lse, pos, G))
        assert np.isfinite(g_lse).all() and np.isfinite(g_pos).all() and np.isfinite(g_G).all() and np.isfinite(loss)
        r_lse, r_pos = np.abs(g_lse - ref["lse"]) / tol["lse"], np.abs(g_pos - ref["pos"]) / tol["pos"]
        r_loss = abs(loss - ref["loss"]) / tol["loss"]
        unm = ~ref["mask"]
        r_G = (np.abs(g_G - ref["G"])[unm] / tol["G"][unm]).max()
        print("inbatch %s B=%d D=%d %s: err / tol lse %.3g pos %.3g loss %.3g G %.3g" %
              (split, B, D, sorted(kw), r_lse.max(), r_pos.max(), r_loss, r_G))
        assert r_lse.max() <= 1 and r_pos.max() <= 1 and r_loss <= 1 and r_G <= 1
        assert (g_G[ref["mask"]] == 0).all()                                        # masked pairs: softmax exactly 0
        if split == "f16x2":
            with _Mode(split="bf16x3"):
                loss3, lse3, pos3, G3, _ = _run_inbatch(q, c, kw, d_loss)
            same = torch.equal(lse3.view(torch.int32), row_lse.view(torch.int32)) and \
                torch.equal(pos3.view(torch.int32), pos.view(torch.int32))
            same_G = torch.equal(G3.contiguous().view(torch.int32), G.contiguous().view(torch.int32))
            assert (same, same_G) == ((False, False) if h2 else (True, True)), "dispatch: f16x2 kernel expected %s" % h2


@gpu
@pytest.mark.parametrize("B,D", [(257, 30), (257, 512)])
@pytest.mark.parametrize("split", ["f16x2", "bf16x3"])
def test_inbatch_softmax_all_candidates_equal(split, B, D):
    """all cand_ids equal: every off-diagonal entry is masked (its exp is taken as exactly 0), so lse_i = s_ii bit for bit, the loss
    is exactly 0, every masked entry of G is exactly 0 and nothing is NaN.  The diagonal of G is exp(s_ii - lse_i) - 1 with s_ii
    recomputed by the gradient kernel: exactly 0 where the product by 1 / T is exact (T = 0.5), otherwise within the score's own
    budget (s_ii - lse_i may be formed as one fused multiply-add, which leaves the product's rounding error)"""
    q, c, w, p, _ = _inbatch_inputs(B, D)
    for temp in (0.5, 0.7):
        kw = dict(temperature=temp, sample_weight=w, cand_prob=p, cand_ids=np.full(B, 5, np.int64))
        with _Mode(split=split):
            loss, row_lse, pos, G, inv_t = _run_inbatch(q, c, kw, 0.37)
        assert loss == 0.0 and torch.equal(row_lse, pos) and bool(torch.isfinite(row_lse).all())
        g = G.cpu().numpy()
        ref = ref_inbatch(q, c, p, kw["cand_ids"], w, inv_t, 0.37)
        assert ref["loss"] == 0.0 and not ref["G"].any()
        tol = _inbatch_tolerances(ref, q, c, inv_t, 0.37, _takes_h2(split, B, D))
        assert np.isfinite(g).all() and not g[ref["mask"]].any(), "masked entries: %d are not zero" % int((g[ref["mask"]] != 0).sum())
        print("inbatch all-equal %s B=%d D=%d T=%g: max |G_ii| / tol %.3g" % (split, B, D, temp, (np.abs(np.diag(g)) / np.diag(tol["G"])).max()))
        assert (np.abs(np.diag(g)) <= np.diag(tol["G"])).all()
        if temp == 0.5:
            assert not g.any()
        assert (np.abs(pos.cpu().numpy() - ref["pos"]) <= tol["pos"]).all()


@gpu
@pytest.mark.parametrize("B,D", [(256, 4), (257, 512)])
def test_inbatch_grad_scores_without_workspace_stays_on_the_fp32_kernel(B, D):
    """dr_inbatch_softmax_grad_scores with workspace = NULL while the split is f16x2: the fp32 kernel, bit for bit what the bf16x3
    split computes on the same inputs (with the workspace, the f16x2 kernel's different bits); G pitched and pre-filled with NaN"""
    L = _L()
    q, c, w, p, ids = _inbatch_inputs(B, D)
    qd, cd, wd, pd, idd = (_dev(v) for v in (q, c, w, p, ids))
    ld_g = (B + 3) // 4 * 4 + 4
    nbytes = L.lib().dr_inbatch_softmax_workspace_bytes(B)
    out = {}
    for split, use_ws in (("bf16x3", True), ("f16x2", False), ("f16x2", True)):
        with _Mode(split=split):
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
            row_lse = torch.full((B,), NAN, device="cuda")
            pos = torch.full((B,), NAN, device="cuda")
            loss = torch.full((1,), NAN, device="cuda")
            L.check(L.lib().dr_inbatch_softmax_fwd(L.ptr(qd), L.ptr(cd), B, D, L.ptr(pd), L.ptr(idd), L.ptr(wd), 2.0, L.ptr(row_lse), L.ptr(pos),
                                                   L.ptr(loss), L.ptr(ws), nbytes, L.stream_ptr()), "dr_inbatch_softmax_fwd")
            _written(row_lse), _written(pos), _written(loss)
            if split == "bf16x3":
                lse3 = row_lse                                                      # the same row_lse for the three gradient calls
            G, Gbuf = _nan_buf(B, B, ld_g - B)
            L.check(L.lib().dr_inbatch_softmax_grad_scores(L.ptr(qd), L.ptr(cd), B, D, L.ptr(pd), L.ptr(idd), L.ptr(wd), 2.0, L.ptr(lse3), 0.37,
                                                           L.ptr(G), G.stride(0), L.ptr(ws) if use_ws else None, nbytes if use_ws else 0,
                                                           L.stream_ptr()), "dr_inbatch_softmax_grad_scores")
            out[(split, use_ws)] = _written(G)
            assert _pad_is_nan(Gbuf, B)
    assert np.array_equal(_bits(out[("f16x2", False)]), _bits(out[("bf16x3", True)]))
    assert not np.array_equal(_bits(out[("f16x2", True)]), _bits(out[("bf16x3", True)]))
    ref = ref_inbatch(q, c, p, ids, w, 2.0, 0.37)
    t32, th2 = (_inbatch_tolerances(ref, q, c, 2.0, 0.37, h2)["G"] for h2 in (False, True))
    for key, tol in ((("f16x2", False), t32), (("f16x2", True), t32 + th2)):      # (row_lse is the fp32 kernel's in both)
        unm = ~ref["mask"]
        assert (np.abs(out[key] - ref["G"])[unm] <= tol[unm]).all() and (out[key][ref["mask"]] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------------------
# 11. dr_scores_nt
# ----------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["bf16x3", "native"])
@pytest.mark.parametrize("M,N,D", [(1, 1, 4), (130, 257, 20), (300, 129, 6), (513, 64, 128)])
def test_scores_nt_direct(mode, M, N, D):
    """a @ b^T with lda, ldb and ld_out wider than the widths (NaN padding; D = 6 and pitch D + 3: rows that are not 16-byte aligned),
    both gemm modes, N = 1 (the narrow tile) to 257 (an edge tile), against float64 with the per-element bound of
    test_gemm_componentwise_error_bound_per_row: 4 sqrt(D) u (|a| |b|^T)_ij, rows of a spanning e^+-6 in magnitude"""
    L = _L()
    rng = np.random.default_rng(M + N + D)
    a = (rng.standard_normal((M, D)) * np.exp(2 * rng.standard_normal((M, 1)))).astype(np.float32)
    b = rng.standard_normal((N, D)).astype(np.float32)
    av, abuf = _pitched(a, 3)
    bv, bbuf = _pitched(b, 4)
    out, obuf = _nan_buf(M, N, 3)
    with _Mode(mode=mode):
        L.check(L.lib().dr_scores_nt(L.ptr(av), av.stride(0), L.ptr(bv), bv.stride(0), M, N, D, L.ptr(out), out.stride(0), L.stream_ptr()),
                "dr_scores_nt")
        via_ops = _ops().scores_nt(_dev(a), _dev(b))
    got = _written(out)
    assert _pad_is_nan(obuf, N) and _pad_is_nan(abuf, D) and _pad_is_nan(bbuf, D)
    ref = a.astype(np.float64) @ b.astype(np.float64).T
    bound = 4 * math.sqrt(D) * U * (np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64)).T)
    err = np.abs(got - ref)
    print("scores_nt %s %dx%dx%d: err / tol %.3g" % (mode, M, N, D, (err / bound).max()))
    assert (err <= bound).all()
    assert np.array_equal(_bits(via_ops.cpu().numpy()), _bits(got))                  # the pitch changes nothing


# ----------------------------------------------------------------------------------------------------------------------------------
# 12. dr_cin_fwd with more than 64 KiB of LDS
# ----------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_cin_large_lds_branch():
    """H0 + Hk = 255: (H0 + Hk) * 65 * 4 = 66300 bytes of LDS, past the 64 KiB a kernel gets without hipFuncSetAttribute.  Forward and
    backward against the float64 einsum of test_cin_forward_backward_match_oracle, with that test's tolerances; then a small shape again:
    the raised limit must not disturb the ordinary launch"""
    ops = _ops()
    B, H0, Hk, D, Fm = 3, 130, 125, 7, 5
    assert (H0 + Hk) * 65 * 4 > 64 * 1024
    rng = np.random.default_rng(12)
    for (b_, h0, hk) in ((B, H0, Hk), (2, 4, 3)):
        x0 = rng.standard_normal((b_, h0, D)).astype(np.float32)
        x = rng.standard_normal((b_, hk, D)).astype(np.float32)
        W = (rng.standard_normal((h0 * hk, Fm)) * 0.2).astype(np.float32)
        bias = rng.standard_normal(Fm).astype(np.float32)
        out = ops.cin_fwd(_dev(x0), _dev(x), _dev(W), _dev(bias), ops.ACT_CODES["relu"])
        want = O.cin(x0, x, W, bias, "relu")
        scale = np.abs(x0).max() * np.abs(x).max() * np.abs(W).max() * np.sqrt(h0 * hk)
        got = out.cpu().numpy()
        print("cin_fwd H0=%d Hk=%d: max err %.3g (atol %.3g)" % (h0, hk, np.abs(got - want).max(), 2e-6 * scale))
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6 * scale)
        assert 0.2 < (got > 0).mean() < 0.8
        dd = torch.float64
        X0, X, Wt, Bt = (torch.tensor(v, dtype=dd, requires_grad=True) for v in (x0, x, W, bias))
        o = torch.relu(torch.einsum("bid,bjd,ijf->bfd", X0, X, Wt.reshape(h0, hk, Fm)) + Bt[None, :, None])
        gout = rng.standard_normal((b_, Fm, D)).astype(np.float32)
        o.backward(torch.tensor(gout, dtype=dd))
        d_x0, d_x, dW, dbias = ops.cin_bwd(_dev(x0), _dev(x), _dev(W), ops.ACT_CODES["relu"], out, _dev(gout), want_bias=True)
        for name, g, r in (("d_x0", d_x0, X0.grad), ("d_x", d_x, X.grad), ("dW", dW, Wt.grad), ("dbias", dbias, Bt.grad)):
            r = r.numpy()
            np.testing.assert_allclose(g.cpu().numpy(), r, rtol=2e-4, atol=2e-5 * np.abs(r).max(), err_msg=name)


# ----------------------------------------------------------------------------------------------------------------------------------
# argument contracts: refused (DR_EINVAL / DR_ESHAPE) or empty (DR_OK) before any launch; `p` is a valid device pointer, 0 is NULL
# ----------------------------------------------------------------------------------------------------------------------------------
EINVAL, OK, ESHAPE = -1, 0, -3
BIG = 1 << 20
CONTRACTS = [
    # dr_lin_fields_fwd(ids, B, F, C, col_start, row_base, lin_w, out, ld_out)
    ("dr_lin_fields_fwd", lambda p: (p, -1, 2, 2, p, p, p, p, 2), EINVAL),
    ("dr_lin_fields_fwd", lambda p: (p, 1, 0, 2, p, p, p, p, 2), EINVAL),
    ("dr_lin_fields_fwd", lambda p: (p, 1, 3, 2, p, p, p, p, 3), EINVAL),                   # C < F
    ("dr_lin_fields_fwd", lambda p: (p, 1, 2, 3, 0, p, p, p, 2), EINVAL),                   # col_start == NULL and C != F
    ("dr_lin_fields_fwd", lambda p: (p, 1, 2, 2, p, p, p, p, 1), EINVAL),                   # ld_out < F
    ("dr_lin_fields_fwd", lambda p: (0, 1, 2, 2, p, p, p, p, 2), EINVAL),
    ("dr_lin_fields_fwd", lambda p: (p, 1, 2, 2, p, 0, p, p, 2), EINVAL),
    ("dr_lin_fields_fwd", lambda p: (p, 1, 2, 2, p, p, 0, p, 2), EINVAL),
    ("dr_lin_fields_fwd", lambda p: (p, 1, 2, 2, p, p, p, 0, 2), EINVAL),
    ("dr_lin_fields_fwd", lambda p: (p, 0, 2, 2, p, p, p, p, 2), OK),
    # dr_lin_fields_bwd(ids, B, F, C, col_start, row_base, d_out, ld_dout, scale, dst_lin)
    ("dr_lin_fields_bwd", lambda p: (p, -1, 2, 2, p, p, p, 2, 1.0, p), EINVAL),
    ("dr_lin_fields_bwd", lambda p: (p, 1, 0, 2, p, p, p, 2, 1.0, p), EINVAL),
    ("dr_lin_fields_bwd", lambda p: (p, 1, 3, 2, p, p, p, 3, 1.0, p), EINVAL),              # C < F
    ("dr_lin_fields_bwd", lambda p: (p, 1, 2, 3, 0, p, p, 2, 1.0, p), EINVAL),              # col_start == NULL and C != F
    ("dr_lin_fields_bwd", lambda p: (p, 1, 2, 2, p, p, p, 1, 1.0, p), EINVAL),              # ld_dout < F
    ("dr_lin_fields_bwd", lambda p: (p, 1, 2, 2, p, p, 0, 2, 1.0, p), EINVAL),
    ("dr_lin_fields_bwd", lambda p: (p, 1, 2, 2, p, p, p, 2, 1.0, 0), EINVAL),
    ("dr_lin_fields_bwd", lambda p: (p, 0, 2, 2, p, p, p, 2, 1.0, p), OK),
    # dr_din_concat_fwd(x, y, B, D, mode, out, ld_out)
    ("dr_din_concat_fwd", lambda p: (p, p, -1, 4, 1, p, 12), EINVAL),
    ("dr_din_concat_fwd", lambda p: (p, p, 1, 0, 1, p, 12), EINVAL),
    ("dr_din_concat_fwd", lambda p: (p, p, 1, 4, 3, p, 12), EINVAL),                        # mode 3
    ("dr_din_concat_fwd", lambda p: (p, p, 1, 4, -1, p, 12), EINVAL),
    ("dr_din_concat_fwd", lambda p: (p, p, 1, 4, 1, p, 11), EINVAL),                        # ld_out < 3 D
    ("dr_din_concat_fwd", lambda p: (p, p, 1, 4, 2, p, 11), EINVAL),
    ("dr_din_concat_fwd", lambda p: (p, p, 1, 4, 0, p, 7), EINVAL),                         # mode 0: ld_out < 2 D
    ("dr_din_concat_fwd", lambda p: (0, p, 1, 4, 1, p, 12), EINVAL),
    ("dr_din_concat_fwd", lambda p: (p, p, 1, 4, 1, 0, 12), EINVAL),
    ("dr_din_concat_fwd", lambda p: (p, p, 0, 4, 1, p, 12), OK),
    # dr_din_concat_bwd(x, y, B, D, mode, d_out, ld_dout, d_x, d_y)
    ("dr_din_concat_bwd", lambda p: (p, p, -1, 4, 1, p, 12, p, p), EINVAL),
    ("dr_din_concat_bwd", lambda p: (p, p, 1, 4, 3, p, 12, p, p), EINVAL),                  # mode 3
    ("dr_din_concat_bwd", lambda p: (p, p, 1, 4, 1, p, 11, p, p), EINVAL),                  # ld_dout < 3 D
    ("dr_din_concat_bwd", lambda p: (p, p, 1, 4, 0, p, 7, p, p), EINVAL),
    ("dr_din_concat_bwd", lambda p: (p, p, 1, 4, 1, 0, 12, p, p), EINVAL),
    ("dr_din_concat_bwd", lambda p: (p, p, 1, 4, 1, p, 12, p, 0), EINVAL),
    ("dr_din_concat_bwd", lambda p: (p, p, 0, 4, 1, p, 12, p, p), OK),
    # dr_softmax_rows_fwd(x, ld_x, B, C, y, ld_y) / _bwd(y, ld_y, dy, ld_dy, B, C, dx, ld_dx)
    ("dr_softmax_rows_fwd", lambda p: (p, 4, -1, 4, p, 4), EINVAL),
    ("dr_softmax_rows_fwd", lambda p: (p, 4, 1, 0, p, 4), EINVAL),
    ("dr_softmax_rows_fwd", lambda p: (p, 3, 1, 4, p, 4), EINVAL),
    ("dr_softmax_rows_fwd", lambda p: (p, 4, 1, 4, p, 3), EINVAL),
    ("dr_softmax_rows_fwd", lambda p: (0, 4, 1, 4, p, 4), EINVAL),
    ("dr_softmax_rows_fwd", lambda p: (p, 4, 1, 4, 0, 4), EINVAL),
    ("dr_softmax_rows_fwd", lambda p: (p, 4, 0, 4, p, 4), OK),
    ("dr_softmax_rows_bwd", lambda p: (p, 4, p, 4, -1, 4, p, 4), EINVAL),
    ("dr_softmax_rows_bwd", lambda p: (p, 4, p, 4, 1, 0, p, 4), EINVAL),
    ("dr_softmax_rows_bwd", lambda p: (p, 3, p, 4, 1, 4, p, 4), EINVAL),
    ("dr_softmax_rows_bwd", lambda p: (p, 4, p, 3, 1, 4, p, 4), EINVAL),
    ("dr_softmax_rows_bwd", lambda p: (p, 4, p, 4, 1, 4, p, 3), EINVAL),
    ("dr_softmax_rows_bwd", lambda p: (p, 4, 0, 4, 1, 4, p, 4), EINVAL),
    ("dr_softmax_rows_bwd", lambda p: (p, 4, p, 4, 0, 4, p, 4), OK),
    # dr_cce_prob_rows(p, ld_p, labels, ld_labels, B, C, sample_weight, row_loss, grad, ld_grad)
    ("dr_cce_prob_rows", lambda p: (p, 4, p, 4, -1, 4, 0, p, p, 4), EINVAL),
    ("dr_cce_prob_rows", lambda p: (p, 4, p, 4, 1, 0, 0, p, p, 4), EINVAL),
    ("dr_cce_prob_rows", lambda p: (p, 3, p, 4, 1, 4, 0, p, p, 4), EINVAL),
    ("dr_cce_prob_rows", lambda p: (p, 4, p, 3, 1, 4, 0, p, p, 4), EINVAL),
    ("dr_cce_prob_rows", lambda p: (p, 4, p, 4, 1, 4, 0, p, p, 3), EINVAL),                 # grad given and ld_grad < C
    ("dr_cce_prob_rows", lambda p: (p, 4, 0, 4, 1, 4, 0, p, p, 4), EINVAL),
    ("dr_cce_prob_rows", lambda p: (p, 4, p, 4, 1, 4, 0, 0, p, 4), EINVAL),
    ("dr_cce_prob_rows", lambda p: (p, 4, p, 4, 0, 4, 0, p, p, 4), OK),
    # dr_gather_cols(a, lda, b, ldb, map, M, N, out, ldo)
    ("dr_gather_cols", lambda p: (p, 4, p, 4, p, -1, 4, p, 4), EINVAL),
    ("dr_gather_cols", lambda p: (p, 4, p, 4, p, 1, -1, p, 4), EINVAL),
    ("dr_gather_cols", lambda p: (p, 4, p, 4, p, 1, 4, p, 3), EINVAL),                      # ldo < N
    ("dr_gather_cols", lambda p: (0, 4, 0, 4, p, 1, 4, p, 4), EINVAL),                      # neither operand
    ("dr_gather_cols", lambda p: (p, 4, p, 4, 0, 1, 4, p, 4), EINVAL),
    ("dr_gather_cols", lambda p: (p, 4, p, 4, p, 1, 4, 0, 4), EINVAL),
    ("dr_gather_cols", lambda p: (p, 4, p, 4, p, 0, 4, p, 4), OK),
    ("dr_gather_cols", lambda p: (p, 4, p, 4, p, 1, 0, p, 4), OK),
    # dr_adam_step_2d(param, ld_p, grad, ld_g, m, v, ld_mv, rows, cols, lr_t, beta1, beta2, eps, grad_scale)
    ("dr_adam_step_2d", lambda p: (p, 4, p, 4, p, p, 4, -1, 4, 0.1, 0.9, 0.999, 1e-8, 1.0), EINVAL),
    ("dr_adam_step_2d", lambda p: (p, 4, p, 4, p, p, 4, 1, -1, 0.1, 0.9, 0.999, 1e-8, 1.0), EINVAL),
    ("dr_adam_step_2d", lambda p: (p, 3, p, 4, p, p, 4, 1, 4, 0.1, 0.9, 0.999, 1e-8, 1.0), EINVAL),
    ("dr_adam_step_2d", lambda p: (p, 4, p, 3, p, p, 4, 1, 4, 0.1, 0.9, 0.999, 1e-8, 1.0), EINVAL),
    ("dr_adam_step_2d", lambda p: (p, 4, p, 4, p, p, 3, 1, 4, 0.1, 0.9, 0.999, 1e-8, 1.0), EINVAL),
    ("dr_adam_step_2d", lambda p: (0, 4, p, 4, p, p, 4, 1, 4, 0.1, 0.9, 0.999, 1e-8, 1.0), EINVAL),
    ("dr_adam_step_2d", lambda p: (p, 4, p, 4, p, 0, 4, 1, 4, 0.1, 0.9, 0.999, 1e-8, 1.0), EINVAL),
    ("dr_adam_step_2d", lambda p: (p, 4, p, 4, p, p, 4, 0, 4, 0.1, 0.9, 0.999, 1e-8, 1.0), OK),
    ("dr_adam_step_2d", lambda p: (p, 4, p, 4, p, p, 4, 1, 0, 0.1, 0.9, 0.999, 1e-8, 1.0), OK),
    # dr_sigmoid_fwd(x, n, y) / dr_sigmoid_bwd(y, dy, n, dx)
    ("dr_sigmoid_fwd", lambda p: (p, -1, p), EINVAL),
    ("dr_sigmoid_fwd", lambda p: (0, 4, p), EINVAL),
    ("dr_sigmoid_fwd", lambda p: (p, 4, 0), EINVAL),
    ("dr_sigmoid_fwd", lambda p: (p, 0, p), OK),
    ("dr_sigmoid_bwd", lambda p: (p, p, -1, p), EINVAL),
    ("dr_sigmoid_bwd", lambda p: (p, 0, 4, p), EINVAL),
    ("dr_sigmoid_bwd", lambda p: (p, p, 4, 0), EINVAL),
    ("dr_sigmoid_bwd", lambda p: (p, p, 0, p), OK),
    # dr_bce_prob_fwd_bwd(prob, labels, n, mode, d_prob, loss_out, workspace): the mean of no elements does not exist
    ("dr_bce_prob_fwd_bwd", lambda p: (p, p, 4, 0, p, p, p), EINVAL),                       # mode 0
    ("dr_bce_prob_fwd_bwd", lambda p: (p, p, 4, 3, p, p, p), EINVAL),
    ("dr_bce_prob_fwd_bwd", lambda p: (p, p, 0, 1, p, p, p), EINVAL),                       # n = 0
    ("dr_bce_prob_fwd_bwd", lambda p: (p, p, -1, 1, p, p, p), EINVAL),
    ("dr_bce_prob_fwd_bwd", lambda p: (0, p, 4, 1, p, p, p), EINVAL),
    ("dr_bce_prob_fwd_bwd", lambda p: (p, p, 4, 1, p, 0, p), EINVAL),
    ("dr_bce_prob_fwd_bwd", lambda p: (p, p, 4, 1, p, p, 0), EINVAL),
    # dr_vocab_lookup_i64(keys, n, vocab, vocab_len, ids_out) / _bytes(bytes, offsets, n, vocab_bytes, vocab_offsets, vocab_len, ids_out)
    ("dr_vocab_lookup_i64", lambda p: (p, -1, p, 4, p), EINVAL),
    ("dr_vocab_lookup_i64", lambda p: (p, 4, p, -1, p), EINVAL),
    ("dr_vocab_lookup_i64", lambda p: (0, 4, p, 4, p), EINVAL),
    ("dr_vocab_lookup_i64", lambda p: (p, 4, 0, 4, p), EINVAL),
    ("dr_vocab_lookup_i64", lambda p: (p, 4, p, 4, 0), EINVAL),
    ("dr_vocab_lookup_i64", lambda p: (p, 0, p, 4, p), OK),
    ("dr_vocab_lookup_bytes", lambda p: (p, p, -1, p, p, 4, p), EINVAL),
    ("dr_vocab_lookup_bytes", lambda p: (p, p, 4, p, p, -1, p), EINVAL),
    ("dr_vocab_lookup_bytes", lambda p: (p, 0, 4, p, p, 4, p), EINVAL),
    ("dr_vocab_lookup_bytes", lambda p: (p, p, 4, p, 0, 4, p), EINVAL),
    ("dr_vocab_lookup_bytes", lambda p: (p, p, 4, p, p, 4, 0), EINVAL),
    ("dr_vocab_lookup_bytes", lambda p: (p, p, 0, p, p, 4, p), OK),
    # dr_csr_plan(row_ptr, n_rows, nnz, plan, plan_bytes, workspace, workspace_bytes)
    ("dr_csr_plan", lambda p: (p, -1, 1000, p, BIG, p, BIG), EINVAL),
    ("dr_csr_plan", lambda p: (p, 4, -1, p, BIG, p, BIG), EINVAL),
    ("dr_csr_plan", lambda p: (0, 4, 1000, p, BIG, p, BIG), EINVAL),
    ("dr_csr_plan", lambda p: (p, 4, 1000, 0, BIG, p, BIG), EINVAL),
    ("dr_csr_plan", lambda p: (p, 4, 1000, p, 8, p, BIG), EINVAL),                          # a plan buffer too small for nnz
    ("dr_csr_plan", lambda p: (p, 4, 1000, p, BIG, 0, 0), EINVAL),                          # long rows possible: needs the workspace
    ("dr_csr_plan", lambda p: (p, 4, 1000, p, BIG, p, 8), EINVAL),
    # dr_csr_transpose(row_ptr, col, val, n_rows, n_cols, nnz, t_row_ptr, t_col, t_val, workspace, workspace_bytes)
    ("dr_csr_transpose", lambda p: (p, p, p, -1, 4, 10, p, p, p, p, BIG), EINVAL),
    ("dr_csr_transpose", lambda p: (p, p, p, 4, -1, 10, p, p, p, p, BIG), EINVAL),
    ("dr_csr_transpose", lambda p: (p, p, p, 4, 4, -1, p, p, p, p, BIG), EINVAL),
    ("dr_csr_transpose", lambda p: (p, p, p, 4, 1 << 31, 10, p, p, p, p, BIG), EINVAL),
    ("dr_csr_transpose", lambda p: (p, p, p, 1 << 31, 4, 10, p, p, p, p, BIG), EINVAL),
    ("dr_csr_transpose", lambda p: (p, p, p, 4, 4, 10, 0, p, p, p, BIG), EINVAL),
    ("dr_csr_transpose", lambda p: (p, 0, p, 4, 4, 10, p, p, p, p, BIG), EINVAL),
    ("dr_csr_transpose", lambda p: (p, p, p, 4, 4, 10, p, p, 0, p, BIG), EINVAL),
    ("dr_csr_transpose", lambda p: (p, p, p, 4, 4, 10, p, p, p, 0, BIG), EINVAL),
    ("dr_csr_transpose", lambda p: (p, p, p, 4, 4, 10, p, p, p, p, 16), EINVAL),            # a workspace too small for nnz
    # dr_inbatch_softmax_fwd(q, c, B, D, cand_prob, cand_ids, sample_weight, inv_temperature, row_lse, pos_score, loss_out, workspace, bytes)
    ("dr_inbatch_softmax_fwd", lambda p: (p, p, 0, 4, 0, 0, 0, 1.0, p, p, p, p, BIG), EINVAL),      # no in-batch problem without a batch
    ("dr_inbatch_softmax_fwd", lambda p: (p, p, 8, 3, 0, 0, 0, 1.0, p, p, p, p, BIG), EINVAL),      # D < 4
    ("dr_inbatch_softmax_fwd", lambda p: (0, p, 8, 4, 0, 0, 0, 1.0, p, p, p, p, BIG), EINVAL),
    ("dr_inbatch_softmax_fwd", lambda p: (p, p, 8, 4, 0, 0, 0, 1.0, 0, p, p, p, BIG), EINVAL),
    ("dr_inbatch_softmax_fwd", lambda p: (p, p, 8, 4, 0, 0, 0, 1.0, p, p, 0, p, BIG), EINVAL),
    ("dr_inbatch_softmax_fwd", lambda p: (p, p, 8, 4, 0, 0, 0, 1.0, p, p, p, 0, BIG), EINVAL),
    ("dr_inbatch_softmax_fwd", lambda p: (p, p, 8, 4, 0, 0, 0, 1.0, p, p, p, p, 64), EINVAL),       # a workspace too small
    # dr_inbatch_softmax_grad_scores(q, c, B, D, cand_prob, cand_ids, sample_weight, inv_temperature, row_lse, d_loss, G, ld_g, ws, bytes)
    ("dr_inbatch_softmax_grad_scores", lambda p: (p, p, 0, 4, 0, 0, 0, 1.0, p, 1.0, p, 8, 0, 0), EINVAL),
    ("dr_inbatch_softmax_grad_scores", lambda p: (p, p, 8, 3, 0, 0, 0, 1.0, p, 1.0, p, 8, 0, 0), EINVAL),
    ("dr_inbatch_softmax_grad_scores", lambda p: (p, p, 8, 4, 0, 0, 0, 1.0, p, 1.0, p, 7, 0, 0), EINVAL),   # ld_g < B
    ("dr_inbatch_softmax_grad_scores", lambda p: (p, 0, 8, 4, 0, 0, 0, 1.0, p, 1.0, p, 8, 0, 0), EINVAL),
    ("dr_inbatch_softmax_grad_scores", lambda p: (p, p, 8, 4, 0, 0, 0, 1.0, 0, 1.0, p, 8, 0, 0), EINVAL),
    ("dr_inbatch_softmax_grad_scores", lambda p: (p, p, 8, 4, 0, 0, 0, 1.0, p, 1.0, 0, 8, 0, 0), EINVAL),
    # dr_scores_nt(a, lda, b, ldb, M, N, D, out, ld_out)
    ("dr_scores_nt", lambda p: (p, 4, p, 4, 2, 2, 3, p, 4), EINVAL),                        # D = 3
    ("dr_scores_nt", lambda p: (p, 4, p, 4, 2, 5, 4, p, 4), EINVAL),                        # ld_out < N
    ("dr_scores_nt", lambda p: (p, 3, p, 4, 2, 2, 4, p, 4), EINVAL),
    ("dr_scores_nt", lambda p: (p, 4, p, 3, 2, 2, 4, p, 4), EINVAL),
    ("dr_scores_nt", lambda p: (p, 4, p, 4, -1, 2, 4, p, 4), EINVAL),
    ("dr_scores_nt", lambda p: (p, 4, p, 4, 2, 0, 4, p, 4), EINVAL),
    ("dr_scores_nt", lambda p: (0, 4, p, 4, 2, 2, 4, p, 4), EINVAL),
    ("dr_scores_nt", lambda p: (p, 4, p, 4, 2, 2, 4, 0, 4), EINVAL),
    ("dr_scores_nt", lambda p: (p, 4, p, 4, 0, 2, 4, p, 4), OK),
    # dr_cin_fwd(x0, x, B, H0, Hk, D, W, Fm, bias, act, out): (H0 + Hk) * 65 * 4 bytes of LDS, at most 160 KiB
    ("dr_cin_fwd", lambda p: (p, p, 1, 600, 31, 1, p, 1, 0, 1, p), ESHAPE),                 # 631 fields: 164060 bytes
    ("dr_cin_fwd", lambda p: (p, p, -1, 4, 4, 2, p, 2, 0, 1, p), EINVAL),
    ("dr_cin_fwd", lambda p: (p, p, 1, 0, 4, 2, p, 2, 0, 1, p), EINVAL),
    ("dr_cin_fwd", lambda p: (p, p, 1, 4, 4, 2, p, 2, 0, 4, p), EINVAL),
    ("dr_cin_fwd", lambda p: (p, p, 1, 4, 4, 2, 0, 2, 0, 1, p), EINVAL),
    ("dr_cin_fwd", lambda p: (p, p, 1, 4, 4, 2, p, 2, 0, 1, 0), EINVAL),
    ("dr_cin_fwd", lambda p: (p, p, 0, 4, 4, 2, p, 2, 0, 1, p), OK),
]


@gpu
@pytest.mark.parametrize("case", range(len(CONTRACTS)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(CONTRACTS)])
def test_argument_contracts(case):
    """the invalid arguments each launcher documents come back as DR_EINVAL / DR_ESHAPE and empty inputs as DR_OK, in both cases before
    anything is launched: the buffer every pointer argument names keeps its contents"""
    L = _L()
    name, make, want = CONTRACTS[case]
    buf = torch.full((BIG // 4,), 0x5A5A5A5, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    rc = getattr(L.lib(), name)(*make(buf.data_ptr()), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == want
    assert bool((buf == 0x5A5A5A5).all())


@gpu
def test_cin_fwd_at_the_lds_limit_is_accepted():
    """630 fields need 163800 bytes, just inside the 160 KiB the launcher allows (631 are refused: test_argument_contracts)"""
    ops = _ops()
    rng = np.random.default_rng(630)
    x0 = rng.standard_normal((1, 600, 2)).astype(np.float32)
    x = rng.standard_normal((1, 30, 2)).astype(np.float32)
    W = (rng.standard_normal((600 * 30, 3)) * 0.05).astype(np.float32)
    out = ops.cin_fwd(_dev(x0), _dev(x), _dev(W), None, ops.ACT_CODES[None]).cpu().numpy()
    want = O.cin(x0, x, W, None, None)
    scale = np.abs(x0).max() * np.abs(x).max() * np.abs(W).max() * np.sqrt(600 * 30)
    np.testing.assert_allclose(out, want, rtol=1e-5, atol=2e-6 * scale)
