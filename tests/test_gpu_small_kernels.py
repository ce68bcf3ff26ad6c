"""Kernel-level tests of the small entry points of csrc/retrieval.hip, csrc/ivf.hip and csrc/elementwise.hip: the top-k list
machinery (dr_topk_select / _merge / _mips' index_base and init arguments), the IVF pack + scan, the integer gathers, the
wave-per-row float kernels and the element-wise helpers -- each against a plain reference (exact integer logic for the selection and
gather kernels, float64 for the float kernels) at sizes where every loop of the kernel runs more than once: rows longer than one lane
stride (64), batches beyond one launch of the capped grids (2048 blocks: 8192 rows of the wave-per-row kernels, 524288 elements of
the grid-stride ones), lists on both sides of the slot 63 -> 64 seam of csrc/topk_list.h, index offsets on both sides of 2^31.

Selection tests use small-integer-valued scores: every product mode then computes them exactly, many of them tie, and the expected
result is unique under the list's total order (score descending, index ascending) -- scores and indices are asserted bit for bit.

Float tolerances.  u = 2^-24.  A fp32 sum whose terms each pass through at most d additions is within g(d) * sum|terms|,
g(d) = d u / (1 - d u); d is read from the kernel's reduction shape (wave per row: ceil(C / 64) chained adds + 6 butterfly steps).
Where expf / logf / tanhf enter, the yardstick is measured on the reference alone: the same formula in plain fp32 torch on the CPU,
its largest (scaled) error against float64 on the test's own inputs; the tolerance is four times that (another reduction order, device
libm a few ulp from the host's) plus the derivable g(d) of the kernel's own sums.

The reference helpers (ref_*) run without a GPU and are themselves checked against oracle/tf_semantics.py and the golden known
answers in test_reference_helpers_against_oracle (unmarked)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import tf_semantics as O

gpu = pytest.mark.gpu

U = 2.0 ** -24
MIN_FLOAT = np.float32(O.MIN_FLOAT)
MAX_FLOAT = np.float32(O.MAX_FLOAT)
GRID_ELEMS = 2048 * 256          # elements one launch of a grid-stride kernel covers before its loop wraps (dr_grid_for)
GRID_ROWS = 2048 * 4             # rows one launch of a wave-per-row kernel covers


def gamma(d):
    return d * U / (1.0 - d * U)


# ----------------------------------------------------------------------------------------------------------------------------------
# reference helpers (CPU only)
# ----------------------------------------------------------------------------------------------------------------------------------
def ref_topk(s, idx, k):
    """k best (score, index) pairs per row under the total order (score descending, index ascending); entries with index < 0 are
    empty; missing results are (-inf, -1).  s [B, m] float32, idx [B, m] int64."""
    s = np.asarray(s, np.float32)
    idx = np.asarray(idx, np.int64)
    B, m = s.shape
    out_s = np.full((B, k), -np.inf, np.float32)
    out_i = np.full((B, k), -1, np.int64)
    if m == 0 or B == 0:
        return out_s, out_i
    order = np.lexsort((idx, -s.astype(np.float64), (idx < 0).astype(np.int8)), axis=1)[:, :k]
    ti = np.take_along_axis(idx, order, 1)
    ts = np.where(ti < 0, np.float32(-np.inf), np.take_along_axis(s, order, 1))
    out_s[:, :ts.shape[1]] = ts
    out_i[:, :ti.shape[1]] = ti
    return out_s, out_i


def ref_select(scores, k, index_base=0, state=None):
    """dr_topk_select: fold scores[B, n] (index = index_base + column) into `state` (None: a new search)."""
    scores = np.asarray(scores, np.float32)
    B, n = scores.shape
    idx = np.broadcast_to(np.arange(n, dtype=np.int64) + np.int64(index_base), (B, n))
    if state is not None:
        scores = np.concatenate([state[0], scores], axis=1)
        idx = np.concatenate([state[1], idx], axis=1)
    return ref_topk(scores, idx, k)


def ref_merge(sa, ia, sb, ib, k):
    """dr_topk_merge: two-pointer merge of two sorted lists per row (an index < 0 ends a list), list a first on equal scores."""
    B = sa.shape[0]
    out_s = np.full((B, k), -np.inf, np.float32)
    out_i = np.full((B, k), -1, np.int64)
    for r in range(B):
        a = b = 0
        for t in range(k):
            av = a < sa.shape[1] and ia[r, a] >= 0
            bv = b < sb.shape[1] and ib[r, b] >= 0
            if av and (not bv or sa[r, a] >= sb[r, b]):
                out_s[r, t], out_i[r, t] = sa[r, a], ia[r, a]
                a += 1
            elif bv:
                out_s[r, t], out_i[r, t] = sb[r, b], ib[r, b]
                b += 1
    return out_s, out_i


def ref_ivf_pack(cand, order, list_start, ids=None):
    """The packed IVF layout of include/dr_hotpath.h: list l owns blocks [blk_off[l], blk_off[l + 1]) of 64 slots,
    packed[(blk * D + d) * 64 + lane] = component d of the vector in slot (blk, lane), zeros and id -1 in padding slots."""
    cand = np.asarray(cand, np.float32)
    D = cand.shape[1]
    counts = np.diff(list_start)
    blk_off = np.concatenate([[0], np.cumsum((counts + 63) // 64)]).astype(np.int64)
    total = int(blk_off[-1])
    packed = np.zeros((total, D, 64), np.float32)
    pids = np.full(total * 64, -1, np.int64)
    for l in range(len(counts)):
        pos = np.arange(int(counts[l]))
        src = np.asarray(order, np.int64)[int(list_start[l]) + pos]
        blk, lane = int(blk_off[l]) + pos // 64, pos % 64
        packed[blk, :, lane] = cand[src]
        pids[blk * 64 + lane] = src if ids is None else np.asarray(ids)[src]
    return packed.reshape(-1), pids, blk_off


def ref_ivf_scan(q, probes, packed, pids, blk_off, k):
    """dr_ivf_scan over a packed layout: float64 inner products of the members of the probed lists (negative probes skipped),
    top k by (score descending, identifier ascending), (-inf, -1) where fewer than k members were reached."""
    q = np.asarray(q, np.float32)
    Bq, D = q.shape
    vec = packed.reshape(-1, D, 64)
    out_s = np.full((Bq, k), -np.inf, np.float32)
    out_i = np.full((Bq, k), -1, np.int64)
    for r in range(Bq):
        sc, ids = [], []
        for l in probes[r]:
            if l < 0:
                continue
            for blk in range(int(blk_off[l]), int(blk_off[l + 1])):
                sc.append((q[r].astype(np.float64) @ vec[blk].astype(np.float64)).astype(np.float32))
                ids.append(pids[blk * 64:(blk + 1) * 64])
        if sc:
            out_s[r], out_i[r] = (x[0] for x in ref_topk(np.concatenate(sc)[None], np.concatenate(ids)[None], k))
    return out_s, out_i


def ref_cce_rows(logits, labels, inv_t, w=None):
    """dr_softmax_ce_rows' per-row loss in float64: w_r * (lse_r * sum_j y_rj - sum_j y_rj s_rj), s = logits * inv_t."""
    s = np.asarray(logits, np.float64) * float(np.float32(inv_t))
    y = np.asarray(labels, np.float64)
    m = s.max(axis=1)
    lse = m + np.log(np.exp(s - m[:, None]).sum(axis=1))
    row = lse * y.sum(axis=1) - (y * s).sum(axis=1)
    return row if w is None else row * np.asarray(w, np.float64)


def ref_cce_rows_bwd(logits, labels, inv_t, w=None, d_loss=1.0):
    """d(sum of ref_cce_rows) / d logits * d_loss = w_r inv_t d_loss (sum_j(y_r) softmax_rj - y_rj), float64."""
    s = np.asarray(logits, np.float64) * float(np.float32(inv_t))
    y = np.asarray(labels, np.float64)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    k = float(np.float32(inv_t)) * float(np.float32(d_loss)) * (np.ones(len(s)) if w is None else np.asarray(w, np.float64))
    return k[:, None] * (y.sum(axis=1, keepdims=True) * p - y)


def _int_scores(rng, B, n, shift=0):
    """small-integer scores with many ties; by row (r + shift) % 4: plain / sprinkled with -inf / all equal / all -inf"""
    s = rng.integers(-3, 4, size=(B, n)).astype(np.float32)
    for r in range(B):
        role = (r + shift) % 4
        if role == 1:
            s[r, rng.random(n) < 0.3] = -np.inf
        elif role == 2:
            s[r] = 1.0
        elif role == 3:
            s[r] = -np.inf
    return s


def _sorted_list(rng, B, k, id_pool, full_rows=False):
    """B sorted lists of k slots: a random number of valid entries (integer scores descending, distinct ids from id_pool in random
    order), then (-inf, -1) tails; row 0 is entirely empty unless full_rows."""
    s = np.full((B, k), -np.inf, np.float32)
    i = np.full((B, k), -1, np.int64)
    for r in range(B):
        v = k if full_rows else (0 if r == 0 else int(rng.integers(0, k + 1)))
        s[r, :v] = np.sort(rng.integers(-2, 3, size=v))[::-1]
        i[r, :v] = rng.choice(id_pool, size=v, replace=False)
    return s, i


# ----------------------------------------------------------------------------------------------------------------------------------
# CPU: the references themselves
# ----------------------------------------------------------------------------------------------------------------------------------
def test_reference_helpers_against_oracle():
    rng = np.random.default_rng(0)
    G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")))
    # top-k under the total order == tf.math.top_k (stable argsort) when the index is the column
    s = _int_scores(rng, 9, 300)
    for k in (1, 64, 65, 128):
        ws, wi = O.top_k(s, k)
        gs, gi = ref_select(s, k)
        assert np.array_equal(gs, ws) and np.array_equal(gi, wi)
        gs, gi = ref_select(s, k, index_base=2 ** 40)
        assert np.array_equal(gi, wi + 2 ** 40)
    gs, gi = ref_select(s[:, :5], 8)                                    # fewer columns than k: (-inf, -1) tails
    assert np.array_equal(gi[:, :5], O.top_k(s[:, :5], 5)[1]) and (gi[:, 5:] == -1).all() and np.isinf(gs[:, 5:]).all()
    assert (ref_select(s[:, :0], 3)[1] == -1).all()
    # folding column slices with increasing index_base == the single call == Streaming's map + reduce
    q = rng.integers(-2, 3, size=(9, 8)).astype(np.float32)
    cand = rng.integers(-2, 3, size=(300, 8)).astype(np.float32)
    sc = q @ cand.T
    state = None
    for a, b in ((0, 100), (100, 130), (130, 300)):
        state = ref_select(sc[:, a:b], 40, index_base=a, state=state)
    ws, wi = O.streaming_top_k(q, [cand[0:100], cand[100:130], cand[130:300]], k=40)
    assert np.array_equal(state[0], ws) and np.array_equal(state[1], wi)
    assert np.array_equal(state[1], ref_select(sc, 40)[1])
    # merge: list a first on ties == a stable top-k of the concatenation [a, b]
    sa, ia = _sorted_list(rng, 20, 7, np.arange(0, 100, 2), full_rows=True)
    sb, ib = _sorted_list(rng, 20, 12, np.arange(1, 100, 2), full_rows=True)
    for k in (5, 19, 25):
        gs, gi = ref_merge(sa, ia, sb, ib, k)
        ws, order = O.top_k(np.concatenate([sa, sb], 1), min(k, 19))
        wi = O.take_long_axis(np.concatenate([ia, ib], 1), order)
        assert np.array_equal(gs[:, :19], ws) and np.array_equal(gi[:, :19], wi)
        assert (gi[:, 19:] == -1).all()
    sa, ia = _sorted_list(rng, 20, 7, np.arange(0, 100, 2))            # with -1 tails: an empty slot never precedes a valid one
    gs, gi = ref_merge(sa, ia, sb, ib, 19)
    assert (np.diff((gi < 0).astype(int), axis=1) >= 0).all() and (gs[:, 1:] <= gs[:, :-1]).all()
    assert ((gi >= 0).sum(1) == (ia >= 0).sum(1) + 12).all()
    # packed IVF layout + scan == the oracle's IVF-Flat search over the same assignment
    N, D, nlist, nprobe, k = 200, 5, 6, 2, 70
    cand = rng.integers(-2, 3, size=(N, D)).astype(np.float32)
    cent = rng.integers(-2, 3, size=(nlist, D)).astype(np.float32)
    assign = rng.integers(0, nlist - 1, size=N)                         # the last list stays empty
    ids = rng.permutation(N).astype(np.int64) + 1000
    q = rng.integers(-2, 3, size=(7, D)).astype(np.float32)
    order = np.argsort(assign, kind="stable")
    list_start = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=nlist))])
    packed, pids, blk_off = ref_ivf_pack(cand, order, list_start, ids)
    assert packed.size == blk_off[-1] * D * 64 and (pids >= 0).sum() == N and blk_off[-1] == blk_off[-2]
    src = int(order[list_start[2] + 1])                                 # slot (list 2, position 1)
    assert pids[blk_off[2] * 64 + 1] == ids[src] and packed[(blk_off[2] * D + 3) * 64 + 1] == cand[src, 3]
    cs = q.astype(np.float64) @ cent.astype(np.float64).T
    probes = np.stack([np.lexsort((np.arange(nlist), -cs[r]))[:nprobe] for r in range(len(q))])
    gs, gi = ref_ivf_scan(q, probes, packed, pids, blk_off, k)
    ws, wi = O.ivf_flat_search(q, cand, ids, cent, assign, nprobe, k)
    assert np.array_equal(gs, ws) and np.array_equal(gi, wi)
    # CCE rows: forward against the oracle's sum, backward against float64 autograd of the forward
    B, C = 6, 70
    logits = rng.standard_normal((B, C)).astype(np.float32) * 3
    labels = rng.random((B, C)).astype(np.float32)
    w = rng.random(B).astype(np.float32)
    assert abs(ref_cce_rows(logits, labels, 1.0, w).sum() - float(O.categorical_crossentropy_from_logits_sum(labels, logits, w))) \
        < 1e-6 * abs(ref_cce_rows(logits, labels, 1.0, w)).sum()
    want = _autograd_cce_bwd(logits, labels, 20.0, w, 0.5)
    assert np.abs(ref_cce_rows_bwd(logits, labels, 20.0, w, 0.5) - want).max() < 1e-12 * np.abs(want).max()
    # the golden known answers of the gathers
    g = G["take_long_axis"]
    assert np.array_equal(O.take_long_axis(np.array(g["arr"]), np.array(g["indices"])), np.array(g["expected"]))
    g = G["exclude"]
    adj = _ref_exclude_adjust(np.array(g["scores"], np.float32), np.array(g["identifiers"]), np.array(g["exclude"]))
    _, order = ref_select(adj, g["k"])
    assert O.take_long_axis(np.array(g["identifiers"]), order).tolist() == g["expected_ids"]
    np.testing.assert_allclose(O.take_long_axis(np.array(g["scores"]), order), np.array(g["expected_scores"]))
    x, y = O.exclude(np.array(g["scores"], np.float32), np.array(g["identifiers"]), np.array(g["exclude"]), g["k"])
    assert y.tolist() == g["expected_ids"]


def _autograd_cce_bwd(logits, labels, inv_t, w, d_loss):
    """float64 autograd of the forward's formula"""
    x = torch.tensor(np.asarray(logits, np.float64), requires_grad=True)
    y = torch.tensor(np.asarray(labels, np.float64))
    s = x * float(np.float32(inv_t))
    row = torch.logsumexp(s, dim=1) * y.sum(1) - (y * s).sum(1)
    if w is not None:
        row = row * torch.tensor(np.asarray(w, np.float64))
    (row.sum() * float(np.float32(d_loss))).backward()
    return x.grad.numpy()


def _ref_exclude_adjust(scores, ids, excl):
    isin = (ids[:, :, None] == excl[:, None, :]).any(-1) if excl.shape[1] else np.zeros(ids.shape, bool)
    return (scores - isin.astype(np.float32) * np.float32(1.0e5)).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ----------------------------------------------------------------------------------------------------------------------------------
def _ops():
    from deep_recommenders_amd import ops
    return ops


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.size == 0:                                                        # (an empty numpy array carries zero strides)
        return torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device="cuda")
    return torch.from_numpy(a).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_same_list(got, want, what=""):
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    bad = np.argwhere(gi != want[1])
    assert bad.size == 0, "%s index differs first at %s: got %s want %s" % (what, bad[0], gi[tuple(bad[0])], want[1][tuple(bad[0])])
    assert np.array_equal(_bits(gs), _bits(want[0])), "%s scores differ" % what


def _padded(a, pad, poison):
    """a [B, n] as a view of a [B, n + pad] device buffer whose padding holds `poison`"""
    B, n = a.shape
    if pad == 0:
        return _dev(a), None
    buf = torch.full((B, n + pad), poison, dtype=torch.from_numpy(a).dtype, device="cuda")
    buf[:, :n] = _dev(a)
    return buf[:, :n], buf


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. selection: exact
# ----------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 127, 128])
def test_topk_select_shapes(k):
    """every n of {0, 1, k-1, k, 255, 256, 257, 1025} (the 256-entry round and its remainders) x Bq of {1, 3, 4, 5} (surplus waves of
    the last block) x ld of {n, n + 5} with +inf in the padding; rows with -inf, all-equal rows, empty slots (-inf, -1)"""
    ops = _ops()
    rng = np.random.default_rng(100 + k)
    for t, n in enumerate(sorted({0, 1, k - 1, k, 255, 256, 257, 1025})):
        for u, Bq in enumerate((1, 3, 4, 5)):
            pad = 5 * ((t + u) % 2)
            s = _int_scores(rng, Bq, n, shift=t)
            view, _ = _padded(s, pad, float("inf"))
            got = ops.topk_select(view, k)
            _assert_same_list(got, ref_select(s, k), "k=%d n=%d Bq=%d pad=%d" % (k, n, Bq, pad))


@gpu
@pytest.mark.parametrize("k,n,pad", [(65, 1025, 5), (128, 257, 0), (1, 256, 5)])
def test_topk_select_many_rows(k, n, pad):
    ops = _ops()
    rng = np.random.default_rng(7)
    s = _int_scores(rng, 1031, n)
    view, _ = _padded(s, pad, float("inf"))
    _assert_same_list(ops.topk_select(view, k), ref_select(s, k))


@gpu
@pytest.mark.parametrize("pieces", [2, 3, 7])
@pytest.mark.parametrize("k", [1, 64, 65, 128])
def test_topk_select_continued_and_index_base(pieces, k):
    """init = False: the same matrix folded in 2, 3 or 7 column slices with increasing index_base equals the single call, for
    index_base on both sides of 2^31 (the 64-bit list must carry it untruncated) and at 2^40"""
    ops = _ops()
    rng = np.random.default_rng(1000 * pieces + k)
    Bq, n = 5, 1025
    s = _int_scores(rng, Bq, n)
    sd = _dev(s)
    cuts = [0] + sorted(rng.choice(np.arange(1, n), size=pieces - 1, replace=False).tolist()) + [n]
    if pieces == 7:
        cuts[1] = 1                                                     # a first slice of one column: the list starts almost empty
        cuts = sorted(set(cuts))
    for base in (0, 2 ** 31 - 1 - n, 2 ** 31 - n, 2 ** 40):
        want = ref_select(s, k, index_base=base)
        _assert_same_list(ops.topk_select(sd, k, index_base=base), want, "single call base=%d" % base)
        state = ops.topk_init(Bq, k, "cuda")
        ref_state = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            state = ops.topk_select(sd[:, a:b], k, index_base=base + a, init=False, state=state)     # (ld = n > b - a)
            ref_state = ref_select(s[:, a:b], k, index_base=base + a, state=ref_state)
            _assert_same_list(state, ref_state, "after slice [%d, %d) base=%d" % (a, b, base))
        _assert_same_list(state, want, "folded base=%d" % base)
        first = ops.topk_select(sd[:, :cuts[1]], k, index_base=base, init=True)                    # init = True on the first slice
        _assert_same_list(first, ref_select(s[:, :cuts[1]], k, index_base=base))


@gpu
@pytest.mark.parametrize("Bq", [1, 255, 256, 257])
def test_topk_merge(Bq):
    """ka != kb; k smaller than, equal to and larger than ka + kb; -1 tails in either list and entirely empty lists (row 0 of each,
    and ka = 0); equal scores across the lists: list a first"""
    ops = _ops()
    rng = np.random.default_rng(Bq)
    for ka, kb in ((7, 12), (128, 3), (5, 5), (0, 9)):
        sa, ia = _sorted_list(rng, Bq, ka, np.arange(0, 400, 2))
        sb, ib = _sorted_list(rng, Bq, kb, np.arange(1, 400, 2) + 2 ** 33)
        if Bq > 1:
            sb[0, :], ib[0, :] = -np.inf, -1
            sa[1, :ka], ia[1, :ka] = 1.0, np.arange(ka) * 2                # full a of equal scores against b
        for k in sorted({1, max(1, ka + kb - 4), ka + kb, ka + kb + 6}):
            got = ops.topk_merge(_dev(sa), _dev(ia), _dev(sb), _dev(ib), k)
            _assert_same_list(got, ref_merge(sa, ia, sb, ib, k), "ka=%d kb=%d k=%d" % (ka, kb, k))


def _int_corpus(rng, N, D):
    return rng.integers(-2, 3, size=(N, D)).astype(np.float32)


def _modes():
    """(gemm mode, split): both operand splits of the matrix-pipe mode, and the native fp32 mode"""
    return [("bf16x3", "f16x2"), ("bf16x3", "bf16x3"), ("native", "f16x2")]


class _Mode:
    def __init__(self, mode, split):
        self.mode, self.split = mode, split

    def __enter__(self):
        ops = _ops()
        self.prev = (ops.set_gemm_mode(self.mode), ops.set_gemm_split(self.split))

    def __exit__(self, *a):
        ops = _ops()
        ops.set_gemm_mode(self.prev[0])
        ops.set_gemm_split(self.prev[1])


@gpu
@pytest.mark.parametrize("Bq,N,D,k,small_ws", [(64, 170_001, 64, 50, False),      # dense first chunk (32768) + three filtered chunks
                                               (77, 5003, 20, 100, True),         # small workspace: generic kernel, 128-column chunks
                                               (5, 300, 4, 128, False),
                                               (33, 1000, 30, 65, False)])        # D not a multiple of 4: generic kernel
def test_topk_mips_exact_with_index_base(Bq, N, D, k, small_ws):
    """integer-valued q and corpus: every product mode computes the scores exactly, thousands of them tie, and the index matrix is
    unique; the result at index_base = b is the result at 0 plus b on both sides of the 32/64-bit list switch and at 2^40; the same
    through a TopKIndex"""
    ops = _ops()
    rng = np.random.default_rng(N)
    q, cand = _int_corpus(rng, Bq, D), _int_corpus(rng, N, D)
    cand[N - 1] = cand[0]                                                   # a duplicate in the last chunk
    want_s, want_i = ref_select(q @ cand.T, k)
    assert (np.diff(want_s, axis=1) == 0).mean() > 0.2                      # ties are everywhere
    qd, cd = _dev(q), _dev(cand)
    for mode, split in _modes():
        with _Mode(mode, split):
            for corpus in (cd, ops.TopKIndex(cd)):
                for base in (0, 2 ** 31 - 1 - N, 2 ** 31 - N, 2 ** 40):
                    ws = torch.empty(Bq * 512, dtype=torch.float32, device="cuda") if small_ws else None
                    got = ops.topk_mips(qd, corpus, k, index_base=base, workspace=ws)
                    _assert_same_list(got, (want_s, want_i + base), "%s/%s index=%s base=%d" % (mode, split, corpus is not cd, base))


@gpu
@pytest.mark.parametrize("sizes,Bq,D,k", [((300, 290, 400, 10), 9, 8, 64),
                                          ((40_000, 40_000, 40_001), 64, 32, 100),
                                          ((128, 1, 500, 128), 3, 4, 128)])
def test_topk_mips_continued_search(sizes, Bq, D, k):
    """a corpus cut into 3 or 4 batches, searched with init = True then init = False and increasing index_base (the contract of
    include/dr_hotpath.h for a continued search), equals the one-call search of the concatenation and Streaming's map + reduce;
    duplicates of a corpus row sit in every batch, so ties span the batch boundaries"""
    ops = _ops()
    rng = np.random.default_rng(sum(sizes))
    N = sum(sizes)
    q, cand = _int_corpus(rng, Bq, D), _int_corpus(rng, N, D)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    best = int(np.argmax((q @ cand[:sizes[0]].T).max(axis=0)))              # a row of batch 0 that is some query's best ...
    for b in starts[1:-1]:
        cand[b] = cand[best]                                                # ... duplicated at the head of every later batch
    want = ref_select(q @ cand.T, k)
    spans = (want[1] == best).any(1)
    for b in starts[1:-1]:
        spans &= (want[1] == b).any(1)
    assert spans.any()                                                      # some row's list holds the tie across every boundary
    ws, wi = O.streaming_top_k(q, [cand[a:b] for a, b in zip(starts[:-1], starts[1:])], k=k)
    assert np.array_equal(ws, want[0]) and np.array_equal(wi, want[1])
    qd, cd = _dev(q), _dev(cand)
    for mode, split in _modes():
        with _Mode(mode, split):
            for base in (0, 2 ** 31 - 1 - sizes[0], 2 ** 40):                 # second: the first batch still fits 32 bits, the rest do not
                for indexed in (False, True):
                    state = None
                    for a, b in zip(starts[:-1], starts[1:]):
                        part = cd[a:b]
                        state = ops.topk_mips(qd, ops.TopKIndex(part) if indexed else part, k, index_base=base + int(a),
                                              init=(a == 0), state=state)
                    _assert_same_list(state, (want[0], want[1] + base), "%s/%s indexed=%s base=%d" % (mode, split, indexed, base))
                _assert_same_list(ops.topk_mips(qd, cd, k, index_base=base), (want[0], want[1] + base))


@gpu
@pytest.mark.parametrize("D", [1, 3, 4, 33, 130])
@pytest.mark.parametrize("with_ids", [False, True])
def test_ivf_pack_and_scan(D, with_ids):
    """lists of 0, 1, 63, 64, 65 and 129 members (block padding on both sides of a full block); the packed layout of the header;
    probes with -1; nprobe = 1 and nprobe = nlist; k of {1, 64, 128}; fewer reachable members than k; D = 130: the query's copy
    into LDS takes three lane strides and the scan's 8-wide unrolled loop has a remainder"""
    ops = _ops()
    rng = np.random.default_rng(10 * D + with_ids)
    sizes = np.array([0, 1, 63, 64, 65, 129, 0, 5])
    nlist, N = len(sizes), int(sizes.sum())
    assign = rng.permutation(np.repeat(np.arange(nlist), sizes))
    order = np.argsort(assign, kind="stable").astype(np.int64)
    list_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cand = _int_corpus(rng, N, D)
    ids = (rng.permutation(N).astype(np.int64) * 7 + 2 ** 35) if with_ids else None
    packed, pids, blk_off = ops.ivf_pack(_dev(cand), _dev(order), _dev(list_start), ids=_dev(ids) if with_ids else None)
    w_packed, w_pids, w_blk = ref_ivf_pack(cand, order, list_start, ids)
    assert np.array_equal(blk_off.cpu().numpy(), w_blk)
    assert np.array_equal(pids.cpu().numpy(), w_pids)
    assert np.array_equal(_bits(packed.cpu().numpy()), _bits(w_packed))
    Bq = 7
    q = _int_corpus(rng, Bq, D)
    all_lists = np.stack([rng.permutation(nlist) for _ in range(Bq)])
    some = all_lists.copy()
    some[rng.random(some.shape) < 0.3] = -1
    some[0, :] = -1                                                        # a query that probes nothing
    single = np.array([[0], [1], [2], [3], [4], [5], [-1]])
    for probes in (all_lists, some, single):
        for k in (1, 64, 128):
            got = ops.ivf_scan(_dev(q), _dev(probes.astype(np.int64)), blk_off, packed, pids, k)
            want = ref_ivf_scan(q, probes, w_packed, w_pids, w_blk, k)
            gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
            assert np.array_equal(gi, want[1]), "nprobe=%d k=%d" % (probes.shape[1], k)
            assert np.array_equal(gs, want[0])
    want = ref_ivf_scan(q, single, w_packed, w_pids, w_blk, 64)            # list 1 has one member, list 0 none: (-inf, -1) tails
    assert (want[1][0] == -1).all() and (want[1][1, 1:] == -1).all() and want[1][1, 0] >= 0 and (want[1][3] >= 0).all()


@gpu
def test_ivf_pack_and_scan_of_a_list_longer_than_one_launch():
    """a list of 16386 blocks: more than the 4096 x 256 slots one launch of the pack kernel covers, so its grid-stride loop wraps;
    the scan walks all of it"""
    ops = _ops()
    rng = np.random.default_rng(3)
    sizes = np.array([5, 4096 * 256 + 70, 0, 64])
    N, D = int(sizes.sum()), 2
    assign = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    order = np.argsort(assign, kind="stable").astype(np.int64)
    list_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cand = _int_corpus(rng, N, D)
    packed, pids, blk_off = ops.ivf_pack(_dev(cand), _dev(order), _dev(list_start))
    w_packed, w_pids, w_blk = ref_ivf_pack(cand, order, list_start)
    assert w_blk.tolist() == [0, 1, 16387, 16387, 16388]
    assert np.array_equal(blk_off.cpu().numpy(), w_blk) and np.array_equal(pids.cpu().numpy(), w_pids)
    assert np.array_equal(_bits(packed.cpu().numpy()), _bits(w_packed))
    q = _int_corpus(rng, 2, D)
    q[0] = 1
    probes = np.array([[1, 3], [-1, 1]], np.int64)
    got = ops.ivf_scan(_dev(q), _dev(probes), blk_off, packed, pids, 128)
    members = [np.concatenate([order[5:5 + sizes[1]], order[-64:]]), order[5:5 + sizes[1]]]
    for r in range(2):
        sc = (cand[members[r]].astype(np.float64) @ q[r].astype(np.float64)).astype(np.float32)
        want = ref_topk(sc[None], members[r][None], 128)
        assert np.array_equal(got[1][r].cpu().numpy(), want[1][0]) and np.array_equal(got[0][r].cpu().numpy(), want[0][0])


@gpu
@pytest.mark.parametrize("B,K", [(5, 3), (2048, 256), (2049, 256), (4099, 301)])
def test_take_along_rows_and_gather(B, K):
    """B * K on both sides of the 2048 x 256 elements one launch covers; arr with ld > C (poisoned padding); indices that are negative
    or past C give the documented 0 (take_along_rows) / -1 (gather_i64)"""
    ops = _ops()
    rng = np.random.default_rng(B)
    C = 37
    idx = rng.integers(-3, C + 3, size=(B, K)).astype(np.int64)
    idx[0, 0], idx[-1, -1] = -2 ** 40, 2 ** 40
    ok = (idx >= 0) & (idx < C)
    for dtype in (np.float32, np.int64):
        arr = rng.integers(1, 1000, size=(B, C)).astype(dtype) + (2 ** 40 if dtype == np.int64 else 0)
        for pad in (0, 3):
            view, _ = _padded(arr, pad, 777)
            got = ops.take_along_rows(view, _dev(idx)).cpu().numpy()
            want = np.where(ok, np.take_along_axis(arr, np.clip(idx, 0, C - 1), 1), 0).astype(dtype)
            assert got.dtype == dtype and np.array_equal(got, want)
            rows = ok.all(1)
            if rows.any():
                assert np.array_equal(want[rows], O.take_long_axis(arr[rows], idx[rows]))
    src = rng.integers(-2 ** 62, 2 ** 62, size=1000, dtype=np.int64)
    flat = rng.integers(-3, 1003, size=B * K).astype(np.int64)
    flat[0], flat[-1] = -2 ** 40, 2 ** 40
    got = ops.gather_i64(_dev(src), _dev(flat)).cpu().numpy()
    okf = (flat >= 0) & (flat < 1000)
    assert np.array_equal(got, np.where(okf, src[np.clip(flat, 0, 999)], -1))
    assert ops.gather_i64(_dev(src), _dev(flat[:0])).numel() == 0
    assert ops.take_along_rows(_dev(np.ones((B, C), np.float32)), _dev(idx[:, :0])).shape == (B, 0)


@gpu
@pytest.mark.parametrize("B,K,E", [(4, 6, 0), (2048, 256, 3), (2049, 256, 2), (3000, 200, 5)])
def test_exclude_adjust(B, K, E):
    """integer scores: scores - 1e5 is exact; E = 0; B * K on both sides of one launch; composed with topk_select and take_along_rows
    it is the reference's _exclude"""
    ops = _ops()
    rng = np.random.default_rng(B + E)
    scores = rng.integers(-50, 51, size=(B, K)).astype(np.float32)
    ids = np.stack([rng.permutation(K) for _ in range(B)]).astype(np.int64) + 2 ** 33
    excl = (rng.integers(0, K + 5, size=(B, E)) + 2 ** 33).astype(np.int64)
    got = ops.exclude_adjust(_dev(scores), _dev(ids), _dev(excl))
    want = _ref_exclude_adjust(scores, ids, excl)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    if E:
        assert (want != scores).any()
    k = min(K, 10)
    _, order = ops.topk_select(got, k)
    ws, wi = O.exclude(scores, ids, excl if E else np.full((B, 1), -1), k)
    assert np.array_equal(ops.take_along_rows(_dev(ids), order).cpu().numpy(), wi)
    assert np.array_equal(ops.take_along_rows(_dev(scores), order).cpu().numpy(), ws)


@gpu
@pytest.mark.parametrize("B,K", [(7, 0), (7, 5), (GRID_ELEMS - 1, 3), (GRID_ELEMS, 3), (GRID_ELEMS + 1, 3), (2 * GRID_ELEMS + 77, 2)])
def test_topk_hits(B, K):
    """[TF] in_top_k counting on integer scores (ties with the positive do not count against it); K = 0; B on both sides of the
    2048 x 256 rows one launch covers; hits accumulate across two calls"""
    ops = _ops()
    rng = np.random.default_rng(B % 1000 + K)
    pos = rng.integers(-2, 3, size=(B, 1)).astype(np.float32)
    topk = -np.sort(-rng.integers(-2, 3, size=(B, K)).astype(np.float32), axis=1)
    ks = np.array([1, 2, 5, 100], np.int32)
    hits = torch.tensor([3, 0, 2 ** 40, 0], dtype=torch.int64, device="cuda")
    ops.topk_hits(_dev(pos), _dev(topk), _dev(ks), hits)
    pred = np.concatenate([pos, topk], axis=1)
    once = np.array([int(O.in_top_k(np.zeros(B, np.int64), pred, int(kk)).sum()) for kk in ks])
    assert hits.cpu().tolist() == (once + np.array([3, 0, 2 ** 40, 0])).tolist()
    ops.topk_hits(_dev(pos), _dev(topk), _dev(ks), hits)
    assert hits.cpu().tolist() == (2 * once + np.array([3, 0, 2 ** 40, 0])).tolist()
    if K and B > 100:
        assert 0 < once[0] < B


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. row-wise float kernels against float64
# ----------------------------------------------------------------------------------------------------------------------------------
# every C / D of {1, 2, 63, 64, 65, 129, 1000} and every B of {1, 5, 8191, 8192, 8193, 20000}; the largest B meets the largest C once
ROW_SHAPES = [(1, 1), (5, 2), (8191, 63), (8192, 64), (8193, 65), (20000, 129), (5, 1000), (1, 129), (20000, 1000)]


@gpu
@pytest.mark.parametrize("B,D", ROW_SHAPES)
def test_rowdot(B, D):
    ops = _ops()
    rng = np.random.default_rng(B + D)
    a = rng.standard_normal((B, D)).astype(np.float32)
    b = rng.standard_normal((B, D)).astype(np.float32)
    got = ops.rowdot(_dev(a), _dev(b)).cpu().numpy().reshape(-1).astype(np.float64)
    t = a.astype(np.float64) * b.astype(np.float64)
    # one lane chains ceil(D / 64) fused multiply-adds, then 6 butterfly additions
    err = np.abs(got - t.sum(1))
    bound = gamma(math.ceil(D / 64) + 6) * np.abs(t).sum(1)
    assert (err <= bound).all(), "max err / bound %g" % (err / bound).max()


@gpu
@pytest.mark.parametrize("M,D", ROW_SHAPES + [(524288, 1), (524289, 1)])
def test_rows_scale(M, D):
    """the three modes bit for bit against the same fp32 expression (one correctly rounded multiply / divide / square root each), rows
    with s == 0, out aliasing x; M * D on both sides of one launch"""
    ops = _ops()
    rng = np.random.default_rng(M + D)
    x = rng.standard_normal((M, D)).astype(np.float32)
    s = (rng.random(M).astype(np.float32) * 4).astype(np.float32)
    s[::3] = 0
    fb = rng.standard_normal((M, D)).astype(np.float32)
    safe = np.where(s > 0, s, np.float32(1))[:, None]
    want = {0: x * s[:, None],
            1: np.where(s[:, None] > 0, x / np.sqrt(safe), x),
            2: np.where(s[:, None] > 0, x / safe, fb)}
    for mode in (0, 1, 2):
        assert want[mode].dtype == np.float32
        got = ops.rows_scale(_dev(x), _dev(s), mode=mode, fallback=_dev(fb) if mode == 2 else None)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want[mode])), mode
        xd = _dev(x)
        out = ops.rows_scale(xd, _dev(s), mode=mode, fallback=_dev(fb) if mode == 2 else None, out=xd)       # in place
        assert out.data_ptr() == xd.data_ptr() and np.array_equal(_bits(xd.cpu().numpy()), _bits(want[mode])), mode


def _labels_with_equal_maxima(rng, B, C):
    """0 / 0.5 / 1 labels whose row maximum (1) appears one to four times at random columns: the first one is the positive"""
    y = (rng.random((B, C)) < 0.1).astype(np.float32) * np.float32(0.5)
    n = rng.integers(1, 5, size=B)
    for r in range(B if B < 64 else 64):
        y[r, rng.choice(C, size=min(C, int(n[r])), replace=False)] = 1
    if B > 64:                                                             # vectorised for the long batches: up to three maxima
        rows = np.arange(64, B)
        for _ in range(3):
            y[rows, rng.integers(0, C, size=rows.size)] = 1
    return y


@gpu
@pytest.mark.parametrize("B,C", ROW_SHAPES)
def test_logits_adjust(B, C):
    """each of the three terms alone and all together; labels with several equal maxima (the first must win, across lanes too)"""
    ops = _ops()
    rng = np.random.default_rng(B * 7 + C)
    logits = (rng.standard_normal((B, C)) * 3).astype(np.float32)
    labels = _labels_with_equal_maxima(rng, B, C)
    prob = rng.uniform(0.01, 0.9, size=C).astype(np.float32)
    ids = rng.integers(0, max(2, C // 3), size=C).astype(np.int64) + 2 ** 33
    if C > 64:
        assert ((labels == 1).sum(1) > 1).any()
    l64, y64 = logits.astype(np.float64), labels.astype(np.float64)
    lt = torch.from_numpy(logits)

    def terms(use_p, use_ids, scale):
        """float64 result, its scale (sum of the absolute terms) and the same formula in fp32 torch, in the kernel's order"""
        want, mag, f32 = l64.copy(), np.abs(l64), lt.clone()
        if use_p:
            want = want - np.log(prob.astype(np.float64))                        # (the oracle's restatement takes the log in fp32)
            mag = mag + np.abs(np.log(prob.astype(np.float64)))
            f32 = f32 - torch.log(torch.from_numpy(prob))
        if use_ids:
            dup = O.remove_accidental_negative(np.zeros_like(l64), y64, ids) / float(MIN_FLOAT)       # (dup - labels), exactly
            assert np.array_equal(dup, np.round(dup * 2) / 2)
            want = want + dup * float(MIN_FLOAT)
            mag = mag + np.abs(dup) * abs(float(MIN_FLOAT))
            f32 = f32 + torch.from_numpy(dup.astype(np.float32)) * float(MIN_FLOAT)
        if scale:
            want = want + y64 * float(np.float32(scale))
            mag = mag + y64 * abs(float(np.float32(scale)))
            f32 = f32 + torch.from_numpy(labels) * float(np.float32(scale))
        return want, mag, f32.numpy().astype(np.float64)

    combos = ((True, False, 0.0), (False, True, 0.0), (False, False, float(MAX_FLOAT)), (True, True, float(MAX_FLOAT)))
    for use_p, use_ids, scale in combos[3 if B * C > 5_000_000 else 0:]:        # (the largest shape: all together only)
        got = ops.logits_adjust(_dev(logits), _dev(labels) if (use_ids or scale) else None, cand_prob=_dev(prob) if use_p else None,
                                cand_ids=_dev(ids) if use_ids else None, add_label_scale=scale).cpu().numpy().astype(np.float64)
        want, mag, f32 = terms(use_p, use_ids, scale)
        assert np.isfinite(got).all()
        yard = float((np.abs(f32 - want) / mag).max())
        # without logf every term is exact and at most three additions round: 3 u of the terms' magnitudes.  With logf: four times
        # the fp32 formula's own error on these inputs (measured: 7e-8 .. 1.3e-7 of the scale) on top of it; never above the 1e-6 the
        # suite already asks of this operation (test_remove_accidental_negative_and_sampling_correction)
        tol = min(gamma(3) + (4 * yard if use_p else 0.0), 1e-6)
        err = np.abs(got - want) / mag
        print("logits_adjust %s B=%d C=%d: err %.3g yardstick %.3g tol %.3g" % ((use_p, use_ids, bool(scale)), B, C, err.max(), yard, tol))
        assert err.max() <= tol, "terms %s: err %g yard %g tol %g" % ((use_p, use_ids, scale), err.max(), yard, tol)
        if use_ids and not use_p and not scale:
            np.testing.assert_allclose(got, O.remove_accidental_negative(l64, y64, ids), rtol=1e-6)
            # where nothing is masked the logit passes through bit for bit; the first maximum's column is never masked
            first = np.argmax(labels, axis=1)
            assert np.array_equal(got[np.arange(B), first], l64[np.arange(B), first])


def _cce_inputs(rng, B, C, masked, soft):
    logits = (rng.standard_normal((B, C)) * 3).astype(np.float32)
    if soft:
        labels = (rng.random((B, C)) * (rng.random((B, C)) < 0.3)).astype(np.float32)
    else:
        labels = np.zeros((B, C), np.float32)
        labels[:, 0] = 1                                                   # the hard-negative branch: the positive sits in column 0
    if masked and C > 1:
        # the masks dr_logits_adjust itself produces (logit + MIN_FLOAT), label 0 there
        m = rng.random((B, C)) < 0.2
        m[:, 0] = False
        logits = np.where(m, logits + MIN_FLOAT, logits).astype(np.float32)
        labels[m] = 0
    w = rng.uniform(0.5, 2.0, size=B).astype(np.float32)
    return logits, labels, w


CCE_CASES = [(B, C, (1.0, 20.0)[i % 2], i % 3 != 0, i % 2 == 0, i % 4 == 1) for i, (B, C) in enumerate(ROW_SHAPES)] + \
            [(8193, 65, 1.0, False, True, False), (5, 1000, 20.0, True, False, True)]


@gpu
@pytest.mark.parametrize("B,C,inv_t,weighted,masked,soft", CCE_CASES)
def test_softmax_ce_rows(B, C, inv_t, weighted, masked, soft):
    from deep_recommenders_amd import _lib
    ops = _ops()
    rng = np.random.default_rng(B * 3 + C)
    logits, labels, w = _cce_inputs(rng, B, C, masked, soft)
    if not weighted:
        w = None
    ld, yd, wd = _dev(logits), _dev(labels), (_dev(w) if weighted else None)
    row = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().dr_softmax_ce_rows(_lib.ptr(ld), _lib.ptr(yd), B, C, float(inv_t), _lib.ptr(wd), _lib.ptr(row), _lib.ptr(loss),
                                             _lib.stream_ptr()), "dr_softmax_ce_rows")
    got = row.cpu().numpy().astype(np.float64)
    want = ref_cce_rows(logits, labels, inv_t, w)
    # the fp32 formula on the CPU, the kernel's expression: (m + log(sum exp(s - m))) * sum(y) - sum(y * s), s = logits * inv_t
    s = torch.from_numpy(logits) * float(np.float32(inv_t))
    y = torch.from_numpy(labels)
    m = s.max(1).values
    f32 = (m + torch.log(torch.exp(s - m[:, None]).sum(1))) * y.sum(1) - (y * s).sum(1)
    f32 = (f32 * torch.from_numpy(w) if weighted else f32).numpy().astype(np.float64)
    s64 = logits.astype(np.float64) * float(np.float32(inv_t))
    lse = s64.max(1) + np.log(np.exp(s64 - s64.max(1, keepdims=True)).sum(1))
    mag = (np.abs(lse) * labels.astype(np.float64).sum(1) + np.abs(labels * s64).sum(1)) * (w.astype(np.float64) if weighted else 1.0)
    mag = mag + 1e-30
    yard = float((np.abs(f32 - want) / mag).max())
    # derivable part: the three sums of a row (ceil(C / 64) chained adds + 6 butterfly steps) and the four roundings of the final
    # expression; measured part: four times the fp32 formula's error (measured: 1e-8 .. 2.4e-7 of the scale; expf / logf and the
    # rounding of s = logits * inv_t, which the softmax amplifies by |s|)
    tol = gamma(math.ceil(C / 64) + 6 + 4) + 4 * yard
    err = np.abs(got - want) / mag
    print("softmax_ce_rows B=%d C=%d inv_t=%g: err %.3g yardstick %.3g tol %.3g" % (B, C, inv_t, err.max(), yard, tol))
    assert np.isfinite(got).all() and err.max() <= tol, "err %g yard %g tol %g" % (err.max(), yard, tol)
    # the total: the rows are summed in double and rounded once
    total = float(loss.cpu()[0])
    assert abs(total - got.sum()) <= 2 * U * abs(got.sum()) + 1e-37
    assert abs(total - float(ops.softmax_ce_rows(ld, yd, inv_t, wd))) == 0.0
    if not masked and inv_t == 1.0:
        ref = float(O.categorical_crossentropy_from_logits_sum(labels, logits, w))
        assert abs(total - ref) <= (tol + 2 * U) * mag.sum()


@gpu
@pytest.mark.parametrize("B,C,inv_t,weighted,masked,soft", CCE_CASES)
def test_softmax_ce_rows_bwd(B, C, inv_t, weighted, masked, soft):
    """dense, and scattered through `cols` into a pre-zeroed wider matrix whose other entries must stay zero"""
    ops = _ops()
    rng = np.random.default_rng(B * 5 + C)
    logits, labels, w = _cce_inputs(rng, B, C, masked, soft)
    if not weighted:
        w = None
    d_loss = 0.75
    ld, yd, wd = _dev(logits), _dev(labels), (_dev(w) if weighted else None)
    out = torch.full((B, C), float("nan"), dtype=torch.float32, device="cuda")
    dense = ops.softmax_ce_rows_bwd(ld, yd, inv_t, wd, d_loss, out=out).cpu().numpy()
    want = ref_cce_rows_bwd(logits, labels, inv_t, w, d_loss)
    if B * C <= 5_000_000:
        auto = _autograd_cce_bwd(logits, labels, inv_t, w, d_loss)
        assert np.abs(auto - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    s = torch.from_numpy(logits) * float(np.float32(inv_t))
    y = torch.from_numpy(labels)
    e = torch.exp(s - s.max(1, keepdim=True).values)
    kk = torch.full((B,), float(np.float32(inv_t)) * float(np.float32(d_loss)))
    kk = kk * torch.from_numpy(w) if weighted else kk
    f32 = (kk[:, None] * (y.sum(1, keepdim=True) * e / e.sum(1, keepdim=True) - y)).numpy().astype(np.float64)
    s64 = logits.astype(np.float64) * float(np.float32(inv_t))
    p = np.exp(s64 - s64.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    k64 = float(np.float32(inv_t)) * d_loss * (w.astype(np.float64) if weighted else np.ones(B))
    y1 = labels.astype(np.float64).sum(1, keepdims=True)
    # scale of an entry: |k| (y1 max(p_j, u) + y_j): the softmax term carries the row sum's relative error, entries that underflow
    # to zero (masked columns) are compared on the scale of one ulp of the row's probability mass
    mag = np.abs(k64)[:, None] * (y1 * np.maximum(p, U) + labels) + 1e-30
    yard = float((np.abs(f32 - want) / mag).max())
    # derivable: the two row sums (ceil(C / 64) + 6 additions) and the five roundings of the entry; measured: four times the fp32
    # formula's own error (measured 1.2e-6 of the scale at inv_t = 1, 1.5e-5 at 20: the rounding of s = logits * inv_t is
    # amplified by |s| <= ~300)
    tol = gamma(math.ceil(C / 64) + 6 + 5) + 4 * yard
    err = np.abs(dense.astype(np.float64) - want) / mag
    print("softmax_ce_rows_bwd B=%d C=%d inv_t=%g: err %.3g yardstick %.3g tol %.3g" % (B, C, inv_t, err.max(), yard, tol))
    assert np.isfinite(dense).all() and err.max() <= tol, "err %g yard %g tol %g" % (err.max(), yard, tol)
    # scattered: distinct columns per row of a wider pre-zeroed matrix
    W = C + 37
    if B * W <= 1_000_000:
        cols = np.stack([rng.permutation(W)[:C] for _ in range(B)]).astype(np.int64)
    else:
        cols = np.argsort(rng.random((B, W), dtype=np.float32), axis=1)[:, :C].astype(np.int64)
    wide = torch.zeros((B, W), dtype=torch.float32, device="cuda")
    ops.softmax_ce_rows_bwd(ld, yd, inv_t, wd, d_loss, cols=_dev(cols), out=wide)
    wide = wide.cpu().numpy()
    expect = np.zeros((B, W), np.float32)
    np.put_along_axis(expect, cols, dense, axis=1)
    assert np.array_equal(_bits(wide), _bits(expect))                        # the same values at cols, exact zeros elsewhere


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. elementwise.hip
# ----------------------------------------------------------------------------------------------------------------------------------
ACT_SHAPES = [(300, 20), (1024, 512), (1025, 512), (3, 400_000)]             # M * N: below, at and past 524288 = one launch


def _act_input(rng, M, N):
    x = (rng.standard_normal((M, N)) * 3).astype(np.float32)
    x.reshape(-1)[:8] = [100, -100, 0, -0.0, 1e-30, -1e-30, 20, -20]
    return x


@gpu
@pytest.mark.parametrize("M,N", ACT_SHAPES)
@pytest.mark.parametrize("pad", [0, 3])
def test_act_fwd(M, N, pad):
    ops = _ops()
    rng = np.random.default_rng(M + N)
    x = _act_input(rng, M, N)
    x64 = x.astype(np.float64)
    for act in (0, 1, 2, 3):
        view, buf = _padded(x, pad, 777.0)
        ops.act_fwd_(view, act)
        got = view.cpu().numpy()
        if pad:
            assert bool((buf[:, N:] == 777.0).all())
        assert np.isfinite(got).all()
        if act == 0:
            assert np.array_equal(_bits(got), _bits(x))
        elif act == 1:
            assert np.array_equal(got, np.maximum(x, 0))
        else:
            want = 1 / (1 + np.exp(-x64)) if act == 2 else np.tanh(x64)
            t = torch.from_numpy(x)
            f32 = (torch.sigmoid(t) if act == 2 else torch.tanh(t)).numpy().astype(np.float64)
            yard = float(np.abs(f32 - want).max())
            # four times the fp32 formula's largest error on these inputs (measured: sigmoid 8.9e-8, tanh 3.1e-8 absolute), and never above
            # the rtol=2e-5, atol=2e-6 the suite already asks of sigmoid / tanh
            err = np.abs(got - want)
            print("act_fwd act=%d M=%d N=%d: err %.3g yardstick %.3g" % (act, M, N, err.max(), yard))
            assert err.max() <= 4 * yard, "act %d err %g yard %g" % (act, err.max(), yard)
            assert (err <= 2e-6 + 2e-5 * np.abs(want)).all()
            assert got.reshape(-1)[0] == 1.0 and got.reshape(-1)[1] == (0.0 if act == 2 else -1.0)       # saturated, no NaN
    empty = torch.empty((0, N), dtype=torch.float32, device="cuda")
    assert ops.act_fwd_(empty, 2).shape == (0, N)


@gpu
@pytest.mark.parametrize("M,N", ACT_SHAPES)
def test_act_bwd(M, N):
    """dy *= act'(y) through the saved output: relu exactly; sigmoid y (1 - y) and tanh 1 - y^2 within the roundings of the
    expression (at most three, of terms bounded by |dy| (1 + |y|)^2)"""
    ops = _ops()
    rng = np.random.default_rng(M * 3 + N)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    for act in (0, 1, 2, 3):
        y = _act_input(rng, M, N)
        if act == 2:
            y = (1 / (1 + np.exp(-y.astype(np.float64)))).astype(np.float32)
        elif act == 3:
            y = np.tanh(y.astype(np.float64)).astype(np.float32)
        yv, ybuf = _padded(y, 3, 777.0)
        dv, dbuf = _padded(dy, 5, 555.0)
        ops.act_bwd_(yv, dv, act)
        got = dv.cpu().numpy()
        assert bool((dbuf[:, N:] == 555.0).all()) and bool((ybuf[:, N:] == 777.0).all()) and np.array_equal(yv.cpu().numpy(), y)
        y64, d64 = y.astype(np.float64), dy.astype(np.float64)
        if act == 0:
            assert np.array_equal(_bits(got), _bits(dy))
        elif act == 1:
            assert np.array_equal(got, np.where(y > 0, dy, np.float32(0) * dy))
        else:
            want = d64 * (y64 * (1 - y64) if act == 2 else 1 - y64 * y64)
            assert (np.abs(got - want) <= gamma(3) * np.abs(d64) * (1 + np.abs(y64)) ** 2).all()
    e = torch.empty((0, N), dtype=torch.float32, device="cuda")
    ops.act_bwd_(e, e.clone(), 3)


@gpu
@pytest.mark.parametrize("M,N,rate", [(7, 5, 0.0), (2000, 64, 0.5), (2048, 256, 0.3), (2000, 300, 0.3), (1025, 512, 0.9)])
def test_dropout(M, N, rate):
    from deep_recommenders_amd import _lib
    ops = _ops()
    rng = np.random.default_rng(M + N)
    x = rng.standard_normal((M, N)).astype(np.float32)
    x[x == 0] = 1
    seed = 0x1234_5678_9ABC_DEF0 + M
    y, mask = ops.dropout_fwd(_dev(x), rate, seed)
    y, mask = y.cpu().numpy(), mask.cpu().numpy().reshape(M, N)
    scale = np.float32(1) / (np.float32(1) - np.float32(rate))
    assert set(np.unique(mask).tolist()) <= {0, 1}
    assert np.array_equal(mask == 1, y != 0)
    assert np.array_equal(_bits(y), _bits(np.where(mask == 1, x * scale, np.float32(0))))       # kept: x * (1 / (1 - rate)) in fp32
    if rate == 0.0:
        assert mask.all() and np.array_equal(_bits(y), _bits(x))
    # kept fraction: binomial(n, p), p = 1 - floor(rate 2^32) / 2^32; six standard deviations
    n, p = M * N, 1.0 - math.floor(float(np.float32(rate)) * 2.0 ** 32) / 2.0 ** 32
    assert abs(int(mask.sum()) - n * p) <= 6 * math.sqrt(n * p * (1 - p))
    # same seed, same mask -- also when x and y have a row pitch: the mask depends on the dense element index
    xv, _ = _padded(x, 3, 777.0)
    ybuf = torch.full((M, N + 5), 555.0, dtype=torch.float32, device="cuda")
    mask2 = torch.empty(M * N, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().dr_dropout_fwd(_lib.ptr(xv), xv.stride(0), M, N, float(rate), seed, _lib.ptr(ybuf), ybuf.stride(0),
                                         _lib.ptr(mask2), _lib.stream_ptr()), "dr_dropout_fwd")
    assert np.array_equal(mask2.cpu().numpy().reshape(M, N), mask)
    assert np.array_equal(_bits(ybuf[:, :N].cpu().numpy()), _bits(y)) and bool((ybuf[:, N:] == 555.0).all())
    if rate > 0:
        other = ops.dropout_fwd(_dev(x), rate, seed + 1)[1].cpu().numpy().reshape(M, N)
        assert (other != mask).mean() > 0.5 * min(p, 1 - p)
    # backward: the saved mask decides, kept gradients are scaled the same way
    dy = rng.standard_normal((M, N)).astype(np.float32)
    dyv, _ = _padded(dy, 3, 777.0)
    dx = ops.dropout_bwd(dyv, _dev(mask.reshape(-1)), rate).cpu().numpy()
    assert np.array_equal(_bits(dx), _bits(np.where(mask == 1, dy * scale, np.float32(0))))


@gpu
@pytest.mark.parametrize("n", [0, 1, 255, 4096, 4097, 256 * 16 * 1024 + 3])
def test_reduce_sum(n):
    ops = _ops()
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    xd = _dev(x) if n else torch.empty(0, dtype=torch.float32, device="cuda")
    # reduction shape: stage 1 has min(ceil(n / 4096), 1024) blocks of 256 threads, a thread chains ceil(n / (256 blocks)) additions,
    # then 6 butterfly steps and 2 for the four waves; stage 2 the same over the block partials; then alpha and the accumulate
    nb = max(1, min(math.ceil(n / 4096), 1024))
    d = (math.ceil(n / (256 * nb)) + 8) + (math.ceil(nb / 256) + 8) + 2
    for squared in (False, True):
        t = x.astype(np.float64) ** 2 if squared else x.astype(np.float64)
        for alpha, acc, out0 in ((1.0, False, 0.0), (-0.375, False, 5.0), (2.5, True, -7.25)):
            out = torch.full((1,), out0, dtype=torch.float32, device="cuda")
            got = float(ops.reduce_sum(xd, squared=squared, alpha=alpha, out=out, accumulate=acc).cpu()[0])
            want = alpha * t.sum() + (out0 if acc else 0.0)
            bound = gamma(d + int(squared)) * (abs(alpha) * np.abs(t).sum() + (abs(out0) if acc else 0.0))
            print("reduce_sum n=%d squared=%d alpha=%g: err %.3g bound %.3g" % (n, squared, alpha, abs(got - want), bound))
            assert abs(got - want) <= bound, "squared %s alpha %g: err %g bound %g" % (squared, alpha, abs(got - want), bound)
            out2 = torch.full((1,), out0, dtype=torch.float32, device="cuda")
            again = ops.reduce_sum(xd, squared=squared, alpha=alpha, out=out2, accumulate=acc)
            assert torch.equal(again.view(torch.int32), out.view(torch.int32))               # fixed order: the same bits


@gpu
@pytest.mark.parametrize("nbytes", [0, 16, 16 * 1023, 16 * 1024 * 4096 + 16])
def test_copy_nt(nbytes):
    from deep_recommenders_amd import _lib
    ops = _ops()
    L = _lib.lib()
    g = torch.Generator(device="cuda")
    g.manual_seed(nbytes)
    n, guard = nbytes // 4, 1024
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + guard,), dtype=torch.int32, device="cuda", generator=g)
    dst = torch.full((n + guard,), 0x5A5A5A5, dtype=torch.int32, device="cuda")
    assert L.dr_copy_nt(_lib.ptr(src), _lib.ptr(dst), nbytes, _lib.stream_ptr()) == _lib.DR_OK
    assert torch.equal(dst[:n], src[:n]) and bool((dst[n:] == 0x5A5A5A5).all())
    if n:
        dst2 = torch.zeros_like(dst)
        ops.copy_nt(src[:n], dst2[:n])
        assert torch.equal(dst2[:n], src[:n]) and bool((dst2[n:] == 0).all())
    # a misaligned pointer or a length that is not a multiple of 16 is refused before anything is launched
    before = dst.clone()
    assert L.dr_copy_nt(_lib.ptr(src) + 4, _lib.ptr(dst), 16, _lib.stream_ptr()) == _lib.DR_EINVAL
    assert L.dr_copy_nt(_lib.ptr(src), _lib.ptr(dst) + 8, 16, _lib.stream_ptr()) == _lib.DR_EINVAL
    assert L.dr_copy_nt(_lib.ptr(src), _lib.ptr(dst), 24, _lib.stream_ptr()) == _lib.DR_EINVAL
    assert L.dr_copy_nt(_lib.ptr(src), _lib.ptr(dst), -16, _lib.stream_ptr()) == _lib.DR_EINVAL
    assert torch.equal(dst, before)


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. argument contracts: refused (DR_EINVAL) or empty (DR_OK) before any launch; `p` is a valid device pointer, 0 is NULL
# ----------------------------------------------------------------------------------------------------------------------------------
EINVAL, OK, ESHAPE = -1, 0, -3
BIG = 1 << 20
CONTRACTS = [
    # dr_topk_select(scores, ld, Bq, n, k, index_base, init, out_s, out_i)
    ("dr_topk_select", lambda p: (p, 4, -1, 4, 2, 0, 1, p, p), EINVAL),
    ("dr_topk_select", lambda p: (p, 4, 1, -1, 2, 0, 1, p, p), EINVAL),
    ("dr_topk_select", lambda p: (p, 4, 1, 4, 0, 0, 1, p, p), EINVAL),
    ("dr_topk_select", lambda p: (p, 4, 1, 4, 129, 0, 1, p, p), EINVAL),
    ("dr_topk_select", lambda p: (p, 3, 1, 4, 2, 0, 1, p, p), EINVAL),                      # ld < n
    ("dr_topk_select", lambda p: (0, 4, 1, 4, 2, 0, 1, p, p), EINVAL),
    ("dr_topk_select", lambda p: (p, 4, 1, 4, 2, 0, 1, 0, p), EINVAL),
    ("dr_topk_select", lambda p: (p, 4, 1, 4, 2, 0, 1, p, 0), EINVAL),
    ("dr_topk_select", lambda p: (p, 4, 0, 4, 2, 0, 1, p, p), OK),
    # dr_topk_merge(sa, ia, ka, sb, ib, kb, Bq, k, out_s, out_i)
    ("dr_topk_merge", lambda p: (p, p, 2, p, p, 2, -1, 2, p, p), EINVAL),
    ("dr_topk_merge", lambda p: (p, p, -1, p, p, 2, 1, 2, p, p), EINVAL),
    ("dr_topk_merge", lambda p: (p, p, 2, p, p, -1, 1, 2, p, p), EINVAL),
    ("dr_topk_merge", lambda p: (p, p, 2, p, p, 2, 1, 0, p, p), EINVAL),
    ("dr_topk_merge", lambda p: (0, p, 2, p, p, 2, 1, 2, p, p), EINVAL),
    ("dr_topk_merge", lambda p: (p, p, 2, p, 0, 2, 1, 2, p, p), EINVAL),
    ("dr_topk_merge", lambda p: (p, p, 2, p, p, 2, 1, 2, 0, p), EINVAL),
    ("dr_topk_merge", lambda p: (p, p, 2, p, p, 2, 0, 2, p, p), OK),
    # dr_topk_mips(q, Bq, cand, N, D, k, index_base, init, out_s, out_i, workspace, workspace_bytes)
    ("dr_topk_mips", lambda p: (p, -1, p, 8, 4, 2, 0, 1, p, p, p, BIG), EINVAL),
    ("dr_topk_mips", lambda p: (p, 1, p, -1, 4, 2, 0, 1, p, p, p, BIG), EINVAL),
    ("dr_topk_mips", lambda p: (p, 1, p, 8, 3, 2, 0, 1, p, p, p, BIG), EINVAL),             # D < 4
    ("dr_topk_mips", lambda p: (p, 1, p, 8, 4, 0, 0, 1, p, p, p, BIG), EINVAL),
    ("dr_topk_mips", lambda p: (p, 1, p, 200, 4, 129, 0, 1, p, p, p, BIG), EINVAL),
    ("dr_topk_mips", lambda p: (0, 1, p, 8, 4, 2, 0, 1, p, p, p, BIG), EINVAL),
    ("dr_topk_mips", lambda p: (p, 1, 0, 8, 4, 2, 0, 1, p, p, p, BIG), EINVAL),
    ("dr_topk_mips", lambda p: (p, 1, p, 8, 4, 2, 0, 1, 0, p, p, BIG), EINVAL),
    ("dr_topk_mips", lambda p: (p, 1, p, 8, 4, 2, 0, 1, p, p, 0, BIG), EINVAL),
    ("dr_topk_mips", lambda p: (p, 1, p, 8, 4, 2, 0, 1, p, p, p, 16), EINVAL),              # a workspace without room for a chunk
    ("dr_topk_mips", lambda p: (p, 1, p, 8, 4, 9, 0, 1, p, p, p, BIG), ESHAPE),             # init and k > N
    ("dr_topk_mips", lambda p: (p, 0, p, 8, 4, 2, 0, 1, p, p, p, BIG), OK),
    # dr_topk_mips_indexed(q, Bq, cand, index, N, D, k, index_base, init, out_s, out_i, workspace, workspace_bytes)
    ("dr_topk_mips_indexed", lambda p: (p, 1, p, 0, 8, 4, 2, 0, 1, p, p, p, BIG), EINVAL),
    ("dr_topk_mips_indexed", lambda p: (p, 1, p, p + 16, 8, 4, 2, 0, 1, p, p, p, BIG), EINVAL),      # index not 256-byte aligned
    ("dr_topk_mips_indexed", lambda p: (p, 1, p, p, 8, 4, 129, 0, 1, p, p, p, BIG), EINVAL),
    ("dr_topk_mips_indexed", lambda p: (p, 0, p, p, 8, 4, 2, 0, 1, p, p, p, BIG), OK),
    # dr_ivf_pack(cand, N, D, order, list_start, blk_off, nlist, total_blocks, ids, packed, packed_ids)
    ("dr_ivf_pack", lambda p: (p, -1, 4, p, p, p, 2, 1, 0, p, p), EINVAL),
    ("dr_ivf_pack", lambda p: (p, 8, 0, p, p, p, 2, 1, 0, p, p), EINVAL),
    ("dr_ivf_pack", lambda p: (p, 8, 4, p, p, p, 0, 1, 0, p, p), EINVAL),
    ("dr_ivf_pack", lambda p: (p, 8, 4, p, p, p, 2, -1, 0, p, p), EINVAL),
    ("dr_ivf_pack", lambda p: (0, 8, 4, p, p, p, 2, 1, 0, p, p), EINVAL),
    ("dr_ivf_pack", lambda p: (p, 8, 4, p, p, 0, 2, 1, 0, p, p), EINVAL),
    ("dr_ivf_pack", lambda p: (p, 8, 4, p, p, p, 2, 1, 0, p, 0), EINVAL),
    ("dr_ivf_pack", lambda p: (p, 0, 4, p, p, p, 2, 0, 0, p, p), OK),                       # nothing to pack
    # dr_ivf_scan(q, Bq, D, probes, nprobe, blk_off, packed, packed_ids, k, out_s, out_i)
    ("dr_ivf_scan", lambda p: (p, -1, 4, p, 1, p, p, p, 2, p, p), EINVAL),
    ("dr_ivf_scan", lambda p: (p, 1, 0, p, 1, p, p, p, 2, p, p), EINVAL),
    ("dr_ivf_scan", lambda p: (p, 1, 4097, p, 1, p, p, p, 2, p, p), EINVAL),
    ("dr_ivf_scan", lambda p: (p, 1, 4, p, 0, p, p, p, 2, p, p), EINVAL),
    ("dr_ivf_scan", lambda p: (p, 1, 4, p, 1, p, p, p, 0, p, p), EINVAL),
    ("dr_ivf_scan", lambda p: (p, 1, 4, p, 1, p, p, p, 129, p, p), EINVAL),
    ("dr_ivf_scan", lambda p: (p, 1, 4, 0, 1, p, p, p, 2, p, p), EINVAL),
    ("dr_ivf_scan", lambda p: (p, 1, 4, p, 1, p, p, p, 2, p, 0), EINVAL),
    ("dr_ivf_scan", lambda p: (p, 0, 4, p, 1, p, p, p, 2, p, p), OK),
    # dr_rowdot(a, b, B, D, out)
    ("dr_rowdot", lambda p: (p, p, -1, 4, p), EINVAL),
    ("dr_rowdot", lambda p: (p, p, 1, 0, p), EINVAL),
    ("dr_rowdot", lambda p: (p, 0, 1, 4, p), EINVAL),
    ("dr_rowdot", lambda p: (p, p, 1, 4, 0), EINVAL),
    ("dr_rowdot", lambda p: (p, p, 0, 4, p), OK),
    # dr_rows_scale(x, s, mode, fallback, M, D, out)
    ("dr_rows_scale", lambda p: (p, p, 0, 0, -1, 4, p), EINVAL),
    ("dr_rows_scale", lambda p: (p, p, 0, 0, 1, 0, p), EINVAL),
    ("dr_rows_scale", lambda p: (p, p, -1, 0, 1, 4, p), EINVAL),
    ("dr_rows_scale", lambda p: (p, p, 3, p, 1, 4, p), EINVAL),
    ("dr_rows_scale", lambda p: (p, p, 2, 0, 1, 4, p), EINVAL),                             # mode 2 needs the fallback
    ("dr_rows_scale", lambda p: (p, 0, 0, 0, 1, 4, p), EINVAL),
    ("dr_rows_scale", lambda p: (p, p, 0, 0, 0, 4, p), OK),
    # dr_gather_i64(src, nsrc, idx, n, out)
    ("dr_gather_i64", lambda p: (p, 4, p, -1, p), EINVAL),
    ("dr_gather_i64", lambda p: (p, -1, p, 1, p), EINVAL),
    ("dr_gather_i64", lambda p: (0, 4, p, 1, p), EINVAL),
    ("dr_gather_i64", lambda p: (p, 4, p, 1, 0), EINVAL),
    ("dr_gather_i64", lambda p: (p, 4, p, 0, p), OK),
    # dr_take_along_rows_{f32,i64}(arr, ld, B, C, idx, K, out)
    ("dr_take_along_rows_f32", lambda p: (p, 4, -1, 4, p, 2, p), EINVAL),
    ("dr_take_along_rows_f32", lambda p: (p, 4, 1, 0, p, 2, p), EINVAL),
    ("dr_take_along_rows_f32", lambda p: (p, 4, 1, 4, p, -1, p), EINVAL),
    ("dr_take_along_rows_f32", lambda p: (p, 3, 1, 4, p, 2, p), EINVAL),                     # ld < C
    ("dr_take_along_rows_f32", lambda p: (0, 4, 1, 4, p, 2, p), EINVAL),
    ("dr_take_along_rows_f32", lambda p: (p, 4, 0, 4, p, 2, p), OK),
    ("dr_take_along_rows_f32", lambda p: (p, 4, 1, 4, p, 0, p), OK),
    ("dr_take_along_rows_i64", lambda p: (p, 4, -1, 4, p, 2, p), EINVAL),
    ("dr_take_along_rows_i64", lambda p: (p, 4, 1, 0, p, 2, p), EINVAL),
    ("dr_take_along_rows_i64", lambda p: (p, 4, 1, 4, p, -1, p), EINVAL),
    ("dr_take_along_rows_i64", lambda p: (p, 3, 1, 4, p, 2, p), EINVAL),
    ("dr_take_along_rows_i64", lambda p: (p, 4, 1, 4, 0, 2, p), EINVAL),
    ("dr_take_along_rows_i64", lambda p: (p, 4, 0, 4, p, 2, p), OK),
    # dr_topk_hits(pos, topk, B, K, ks, nk, hits)
    ("dr_topk_hits", lambda p: (p, p, -1, 2, p, 1, p), EINVAL),
    ("dr_topk_hits", lambda p: (p, p, 1, -1, p, 1, p), EINVAL),
    ("dr_topk_hits", lambda p: (p, p, 1, 2, p, 0, p), EINVAL),
    ("dr_topk_hits", lambda p: (p, 0, 1, 2, p, 1, p), EINVAL),
    ("dr_topk_hits", lambda p: (p, p, 1, 2, p, 1, 0), EINVAL),
    ("dr_topk_hits", lambda p: (p, p, 0, 2, p, 1, p), OK),
    # dr_exclude_adjust(scores, ids, B, K, exclude, E, adjusted)
    ("dr_exclude_adjust", lambda p: (p, p, -1, 2, p, 1, p), EINVAL),
    ("dr_exclude_adjust", lambda p: (p, p, 1, 0, p, 1, p), EINVAL),
    ("dr_exclude_adjust", lambda p: (p, p, 1, 2, p, -1, p), EINVAL),
    ("dr_exclude_adjust", lambda p: (p, p, 1, 2, 0, 1, p), EINVAL),
    ("dr_exclude_adjust", lambda p: (p, p, 1, 2, p, 1, 0), EINVAL),
    ("dr_exclude_adjust", lambda p: (p, p, 0, 2, p, 1, p), OK),
    # dr_logits_adjust(logits, labels, B, C, cand_prob, cand_ids, add_label_scale, out)
    ("dr_logits_adjust", lambda p: (p, p, -1, 4, p, p, 0.0, p), EINVAL),
    ("dr_logits_adjust", lambda p: (p, p, 1, 0, p, p, 0.0, p), EINVAL),
    ("dr_logits_adjust", lambda p: (0, p, 1, 4, p, p, 0.0, p), EINVAL),
    ("dr_logits_adjust", lambda p: (p, 0, 1, 4, 0, p, 0.0, p), EINVAL),                      # cand_ids needs labels
    ("dr_logits_adjust", lambda p: (p, 0, 1, 4, 0, 0, 1.0, p), EINVAL),                      # ... and so does add_label_scale
    ("dr_logits_adjust", lambda p: (p, p, 1, 4, p, p, 0.0, 0), EINVAL),
    ("dr_logits_adjust", lambda p: (p, p, 0, 4, p, p, 0.0, p), OK),
    # dr_softmax_ce_rows(logits, labels, B, C, inv_temperature, sample_weight, row_loss, loss_out)
    ("dr_softmax_ce_rows", lambda p: (p, p, -1, 4, 1.0, 0, p, p), EINVAL),
    ("dr_softmax_ce_rows", lambda p: (p, p, 1, 0, 1.0, 0, p, p), EINVAL),
    ("dr_softmax_ce_rows", lambda p: (0, p, 1, 4, 1.0, 0, p, p), EINVAL),
    ("dr_softmax_ce_rows", lambda p: (p, 0, 1, 4, 1.0, 0, p, p), EINVAL),
    ("dr_softmax_ce_rows", lambda p: (p, p, 1, 4, 1.0, 0, 0, p), EINVAL),
    ("dr_softmax_ce_rows", lambda p: (p, p, 1, 4, 1.0, 0, p, 0), EINVAL),
    # dr_softmax_ce_rows_bwd(logits, labels, B, C, inv_temperature, sample_weight, d_loss, cols, out, ld_out)
    ("dr_softmax_ce_rows_bwd", lambda p: (p, p, -1, 4, 1.0, 0, 1.0, 0, p, 4), EINVAL),
    ("dr_softmax_ce_rows_bwd", lambda p: (p, p, 1, 0, 1.0, 0, 1.0, 0, p, 4), EINVAL),
    ("dr_softmax_ce_rows_bwd", lambda p: (p, p, 1, 4, 1.0, 0, 1.0, 0, p, 0), EINVAL),
    ("dr_softmax_ce_rows_bwd", lambda p: (p, p, 1, 4, 1.0, 0, 1.0, 0, p, 3), EINVAL),        # dense and ld_out < C
    ("dr_softmax_ce_rows_bwd", lambda p: (p, 0, 1, 4, 1.0, 0, 1.0, 0, p, 4), EINVAL),
    ("dr_softmax_ce_rows_bwd", lambda p: (p, p, 1, 4, 1.0, 0, 1.0, 0, 0, 4), EINVAL),
    ("dr_softmax_ce_rows_bwd", lambda p: (p, p, 0, 4, 1.0, 0, 1.0, 0, p, 4), OK),
    # dr_act_fwd(x, M, N, ld, act) / dr_act_bwd(y, ld_y, dy, ld_dy, M, N, act)
    ("dr_act_fwd", lambda p: (p, -1, 4, 4, 2), EINVAL),
    ("dr_act_fwd", lambda p: (p, 1, 0, 4, 2), EINVAL),
    ("dr_act_fwd", lambda p: (p, 1, 4, 3, 2), EINVAL),
    ("dr_act_fwd", lambda p: (p, 1, 4, 4, -1), EINVAL),
    ("dr_act_fwd", lambda p: (p, 1, 4, 4, 4), EINVAL),
    ("dr_act_fwd", lambda p: (0, 1, 4, 4, 2), EINVAL),
    ("dr_act_fwd", lambda p: (p, 0, 4, 4, 2), OK),
    ("dr_act_bwd", lambda p: (p, 4, p, 4, -1, 4, 2), EINVAL),
    ("dr_act_bwd", lambda p: (p, 4, p, 4, 1, 0, 2), EINVAL),
    ("dr_act_bwd", lambda p: (p, 3, p, 4, 1, 4, 2), EINVAL),
    ("dr_act_bwd", lambda p: (p, 4, p, 3, 1, 4, 2), EINVAL),
    ("dr_act_bwd", lambda p: (p, 4, p, 4, 1, 4, 4), EINVAL),
    ("dr_act_bwd", lambda p: (p, 4, 0, 4, 1, 4, 2), EINVAL),
    ("dr_act_bwd", lambda p: (p, 4, p, 4, 0, 4, 2), OK),
    # dr_dropout_fwd(x, ld_x, M, N, rate, seed, y, ld_y, mask) / dr_dropout_bwd(dy, ld_dy, mask, M, N, rate, dx, ld_dx)
    ("dr_dropout_fwd", lambda p: (p, 4, -1, 4, 0.5, 1, p, 4, p), EINVAL),
    ("dr_dropout_fwd", lambda p: (p, 4, 1, 0, 0.5, 1, p, 4, p), EINVAL),
    ("dr_dropout_fwd", lambda p: (p, 3, 1, 4, 0.5, 1, p, 4, p), EINVAL),
    ("dr_dropout_fwd", lambda p: (p, 4, 1, 4, 0.5, 1, p, 3, p), EINVAL),
    ("dr_dropout_fwd", lambda p: (p, 4, 1, 4, -0.1, 1, p, 4, p), EINVAL),
    ("dr_dropout_fwd", lambda p: (p, 4, 1, 4, 1.0, 1, p, 4, p), EINVAL),
    ("dr_dropout_fwd", lambda p: (p, 4, 1, 4, float("nan"), 1, p, 4, p), EINVAL),
    ("dr_dropout_fwd", lambda p: (p, 4, 1, 4, 0.5, 1, p, 4, 0), EINVAL),
    ("dr_dropout_fwd", lambda p: (p, 4, 0, 4, 0.5, 1, p, 4, p), OK),
    ("dr_dropout_bwd", lambda p: (p, 4, p, -1, 4, 0.5, p, 4), EINVAL),
    ("dr_dropout_bwd", lambda p: (p, 4, p, 1, 0, 0.5, p, 4), EINVAL),
    ("dr_dropout_bwd", lambda p: (p, 3, p, 1, 4, 0.5, p, 4), EINVAL),
    ("dr_dropout_bwd", lambda p: (p, 4, p, 1, 4, 0.5, p, 3), EINVAL),
    ("dr_dropout_bwd", lambda p: (p, 4, p, 1, 4, 1.0, p, 4), EINVAL),
    ("dr_dropout_bwd", lambda p: (p, 4, 0, 1, 4, 0.5, p, 4), EINVAL),
    ("dr_dropout_bwd", lambda p: (p, 4, p, 0, 4, 0.5, p, 4), OK),
    # dr_reduce_sum(x, n, squared, alpha, accumulate, out, workspace)
    ("dr_reduce_sum", lambda p: (p, -1, 0, 1.0, 0, p, p), EINVAL),
    ("dr_reduce_sum", lambda p: (p, 4, 0, 1.0, 0, 0, p), EINVAL),
    ("dr_reduce_sum", lambda p: (p, 4, 0, 1.0, 0, p, 0), EINVAL),
    ("dr_reduce_sum", lambda p: (0, 4, 0, 1.0, 0, p, p), EINVAL),
]


@gpu
@pytest.mark.parametrize("case", range(len(CONTRACTS)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(CONTRACTS)])
def test_argument_contracts(case):
    """the documented invalid arguments come back as DR_EINVAL and empty inputs as DR_OK, in both cases before anything is launched:
    the buffer every pointer argument names keeps its contents"""
    from deep_recommenders_amd import _lib
    name, make, want = CONTRACTS[case]
    buf = torch.full((BIG // 4,), 0x5A5A5A5, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    rc = getattr(_lib.lib(), name)(*make(buf.data_ptr()), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == want
    assert bool((buf == 0x5A5A5A5).all())


@gpu
def test_softmax_ce_rows_of_an_empty_batch():
    """B = 0 is an empty input like everywhere else in the library: DR_OK, the loss of no rows is 0, row_loss is not touched"""
    from deep_recommenders_amd import _lib
    buf = torch.full((64,), float("nan"), dtype=torch.float32, device="cuda")
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    assert _lib.lib().dr_softmax_ce_rows(p, p, 0, 4, 1.0, None, p, loss.data_ptr(), _lib.stream_ptr()) == _lib.DR_OK
    assert float(loss.cpu()[0]) == 0.0 and bool(torch.isnan(buf).all())
    assert _lib.lib().dr_softmax_ce_rows(p, p, 0, 4, 1.0, None, p, None, _lib.stream_ptr()) == _lib.DR_EINVAL
