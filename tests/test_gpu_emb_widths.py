"""Every row-width instantiation of the embedding kernels (csrc/emb_pool.hip, csrc/emb_sorted.hip, csrc/shard.hip).

Each of those kernels is a template on LPR, the number of adjacent lanes that hold one table row as float4s (the smallest power of
two with 4 * LPR >= D).  WIDTHS below names every LPR once with a full row (D = 4 * LPR) and, where one exists, once with a partial
row whose lanes past D / 4 are clamped and live (12, 20, 36, 68, 132); the tests are parametrised over it, so every version of
every kernel is launched.  Beside the width axis: the hot-row piece geometry of K4 (single-slot last piece, more than 64 pieces),
the 64-float piece walk and the grid wrap of dr_adam_catchup_rows, and batches past one launch of the capped grids.

Exact comparisons.  Table and first-order values are multiples of 1/8 in [-4, 4], gradients integers in [-4, 4], d_fm_logit an
integer in [-2, 2], the SGD scale -0.125.  Every sum the kernels form is then exact in fp32, so the result does not depend on the
summation order, on atomics or on the slot plan's path, and the device output is compared bit for bit with a float64 reference.
The precondition -- (largest |partial sum| possible) / quantum < 2^24 -- is asserted by every test on its own reference
(`headroom`) and once more for every case by the unmarked test_exactness_preconditions.

Where exactness is impossible (Adam's sqrt and division, a mean over 3, fm_logit's squares) the reference is float64 and the
tolerance is g(d) * sum|terms| with d read off the kernel's reduction shape, or four times the largest error of the same formula
in plain fp32 torch on the CPU against float64, measured at run time on the test's own inputs.

The reference helpers (ref_*) run without a GPU and are checked against oracle/torch_ref.py in
test_reference_helpers_against_oracle (unmarked)."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import torch_ref as T

gpu = pytest.mark.gpu

U = 2.0 ** -24
EXACT = 2.0 ** 24
WIDTHS = [4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256]
SCALE = -0.125
SENTINEL = np.float32(-12345.0)
# Adam's hyper-parameters as the kernels receive them (C floats): the float64 oracle is given the same rounded values
B1, B2, EPS = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8))


def gamma(d):
    return d * U / (1.0 - d * U)


def lpr_of(D):
    l = 1
    while 4 * l < D:
        l <<= 1
    return l


def test_widths_cover_every_lpr_full_and_partial():
    full = {lpr_of(D) for D in WIDTHS if D == 4 * lpr_of(D)}
    part = {lpr_of(D) for D in WIDTHS if D != 4 * lpr_of(D)}
    assert full == {1, 2, 4, 8, 16, 32, 64}
    assert part == {4, 8, 16, 32, 64}                        # (LPR 1 and 2 have no partial row: D = 4 and 8 only)


# ----------------------------------------------------------------------------------------------------------------------------------
# inputs on the exact grid
# ----------------------------------------------------------------------------------------------------------------------------------
def q8(rng, shape):
    """multiples of 1/8 in [-4, 4]"""
    return (rng.integers(-32, 33, size=shape) / 8.0).astype(np.float32)


def ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def on_grid(a, quantum):
    r = np.asarray(a, np.float64) / quantum
    return bool(np.array_equal(r, np.rint(r)))


def rows_of(ids, row_base, col_field=None):
    """global row of every slot, -1 where the id is missing.  ids [B, C]; col_field [C] = field of each column (default: column)."""
    base = np.asarray(row_base, np.int64)
    base = base if col_field is None else base[np.asarray(col_field)]
    return np.where(ids >= 0, ids + base[None, :], -1)


def bag_layout(F):
    """bags of 1, 2 and 4 columns in turn: (col_start [F + 1] int32, col_field [C])"""
    lens = np.array([(1, 2, 4)[f % 3] for f in range(F)])
    cs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return cs, np.repeat(np.arange(F), lens)


def bag_ids(rng, B, F, V, counts_of_len):
    """ids [B, C] for bag_layout(F): bag (b, f) of length L keeps a number of ids drawn from counts_of_len[L], the others are -1 at
    random places of the bag (so some bags are all -1 when 0 is among the counts)"""
    cs, _ = bag_layout(F)
    ids = rng.integers(0, V, size=(B, int(cs[-1])))
    for f in range(F):
        L = int(cs[f + 1] - cs[f])
        keep = rng.choice(np.asarray(counts_of_len[L]), size=B)
        rank = np.argsort(rng.random((B, L)), axis=1)
        ids[:, cs[f]:cs[f + 1]][rank >= keep[:, None]] = -1
    return ids


# ----------------------------------------------------------------------------------------------------------------------------------
# reference helpers (CPU only, float64)
# ----------------------------------------------------------------------------------------------------------------------------------
def ref_pool_fwd(ids, col_start, row_base, table, lin_w, bias):
    """dr_emb_pool_fwd: mean-pooled bags (ids < 0 dropped, empty bag -> zeros), concat [B, F * D], sum_x [B, D],
    fm_logit = bias + sum of first-order weights + 0.5 * sum_d (S_d^2 - SS_d); `terms` = sum of |every term| of fm_logit."""
    B = ids.shape[0]
    F = len(row_base)
    D = table.shape[1]
    cs = np.arange(F + 1) if col_start is None else np.asarray(col_start)
    t64, l64 = table.astype(np.float64), lin_w.astype(np.float64)
    x = np.zeros((B, F, D))
    lin = np.zeros(B)
    lin_abs = np.zeros(B)
    for f in range(F):
        cnt = np.zeros(B)
        for c in range(cs[f], cs[f + 1]):
            m = ids[:, c] >= 0
            r = ids[m, c] + row_base[f]
            x[m, f] += t64[r]
            lin[m] += l64[r]
            lin_abs[m] += np.abs(l64[r])
            cnt += m
        x[:, f] /= np.maximum(cnt, 1)[:, None]
    S, SS = x.sum(1), (x * x).sum(1)
    logit = float(bias) + lin + 0.5 * (S * S - SS).sum(1)
    terms = abs(float(bias)) + lin_abs + 0.5 * (S * S + SS).sum(1)
    return x.reshape(B, F * D), S, logit, terms


def ref_slot_grads(rows, grad, concat, sum_x, dl, fm):
    """per-slot row gradient [B, F, D] = d_concat (+ d_fm_logit * (sum_x - x) with the FM term)"""
    B, F = rows.shape
    D = grad.shape[1] // F
    g = grad.astype(np.float64).reshape(B, F, D)
    if fm:
        g = g + dl.astype(np.float64)[:, None, None] * (sum_x.astype(np.float64)[:, None, :] - concat.astype(np.float64).reshape(B, F, D))
    return g


def ref_scatter(rows, g, gl, R):
    """dense sums of the slot gradients per row: (sum g [R, D], sum |g|, sum gl [R], sum |gl|)"""
    m = rows >= 0
    D = g.shape[-1]
    dense, dabs = np.zeros((R, D)), np.zeros((R, D))
    np.add.at(dense, rows[m], g[m])
    np.add.at(dabs, rows[m], np.abs(g[m]))
    lin, labs = np.zeros(R), np.zeros(R)
    np.add.at(lin, rows[m], gl[m])
    np.add.at(labs, rows[m], np.abs(gl[m]))
    return dense, dabs, lin, labs


def ref_k4_sgd(c, fm):
    """dr_emb_pool_bwd_sorted on case c: table += scale * sum of slot gradients, lin += scale * sum d_fm_logit, bias += scale *
    sum_b d_fm_logit.  headroom = (largest |partial sum| in any order) / quantum, quantum 1/64 = scale * the gradients' 1/8."""
    rows = c["rows"]
    g = ref_slot_grads(rows, c["grad"], c["concat"], c["sum_x"], c["dl"], fm)
    gl = np.broadcast_to(c["dl"].astype(np.float64)[:, None], rows.shape)
    dense, dabs, lin, labs = ref_scatter(rows, g, gl, c["R"])
    s = c["scale"]
    table = c["table"].astype(np.float64) + s * dense
    lin_w = c["lin"].astype(np.float64) + s * lin
    bias = float(c["bias"]) + s * float(c["dl"].astype(np.float64).sum())
    bound = max(float((np.abs(c["table"]) + abs(s) * dabs).max()), float((np.abs(c["lin"]) + abs(s) * labs).max()),
                abs(float(c["bias"])) + abs(s) * float(np.abs(c["dl"]).sum()))
    q = abs(s) / 8.0
    assert on_grid(table, q) and on_grid(lin_w, q) and on_grid(bias, q)
    touched = np.unique(rows[rows >= 0])
    return {"table": table.astype(np.float32), "lin": lin_w.astype(np.float32), "bias": np.float32(bias), "headroom": bound / q,
            "written_amax": float(np.abs(table[touched]).max()) if touched.size else 0.0}


def ref_pool_bwd(ids, col_start, col_field, row_base, R, d_concat, concat, sum_x, dl, scale, table, lin_w, bias):
    """dr_emb_pool_bwd (atomic form): every id of a bag of `cnt` present ids receives scale * g / cnt, g = d_concat + d_fm_logit *
    (sum_x - concat); first-order rows receive scale * d_fm_logit per id; the bias scale * sum_b d_fm_logit.
    Returns (table, lin, bias, |terms| per table element incl. the start value, additions per row)."""
    B, C = ids.shape
    F = len(row_base)
    D = table.shape[1]
    cs = np.asarray(col_start)
    g = ref_slot_grads(np.zeros((B, F), np.int64), d_concat, concat, sum_x, dl, True) * scale
    t, tabs = table.astype(np.float64).copy(), np.abs(table.astype(np.float64))
    l = lin_w.astype(np.float64).copy()
    hits = np.zeros(R)
    for f in range(F):
        present = ids[:, cs[f]:cs[f + 1]] >= 0
        cnt = present.sum(1)
        gf = g[:, f] / np.maximum(cnt, 1)[:, None]
        for c in range(cs[f], cs[f + 1]):
            m = ids[:, c] >= 0
            r = ids[m, c] + row_base[f]
            np.add.at(t, r, gf[m])
            np.add.at(tabs, r, np.abs(gf[m]))
            np.add.at(l, r, scale * dl[m].astype(np.float64))
            np.add.at(hits, r, 1)
    return t, l, float(bias) + scale * float(dl.astype(np.float64).sum()), tabs, hits


def ref_adam_rows(w, m, v, dense_g, rows, lr, step):
    """one row-wise Adam step of the rows named in `rows` with the pre-summed gradient: oracle/torch_ref.py's adam_rows_step, in the
    dtype of the tensors given (float64: the oracle; float32: the yardstick)"""
    T.adam_rows_step(w, dense_g.to(w.dtype), torch.as_tensor(rows).reshape(-1), m, v, lr, step, B1, B2, EPS)


def ref_catchup(w, m, v, old, named, upto, lr):
    """dr_adam_catchup_rows: row r with 0 < old[r] < upto that is named receives the decay-only steps old[r] + 1 .. upto of the dense
    rule (m *= b1, v *= b2, w -= lr_s m / (sqrt(v) + eps)), one after the other, in the dtype of the tensors given.  In place."""
    old = torch.as_tensor(old)
    named = torch.as_tensor(named)
    lo = int(old[named & (old > 0)].min()) if bool((named & (old > 0)).any()) else upto
    for s in range(lo + 1, upto + 1):
        sel = named & (old > 0) & (old < s)
        lr_s = T.adam_lr_t(lr, B1, B2, s)
        m[sel] = m[sel] * B1
        v[sel] = v[sel] * B2
        w[sel] = w[sel] - lr_s * m[sel] / (v[sel].sqrt() + EPS)


# ----------------------------------------------------------------------------------------------------------------------------------
# cases (built once, shared, read only)
# ----------------------------------------------------------------------------------------------------------------------------------
def _k4_case(seed, B, F, V, D, hot_counts=(), empty_field=None, p_missing=0.05):
    """single-valued ids [B, F] over F fields of V rows; hot_counts: row (field 0, id j) is named by hot_counts[j] examples (the first
    ones), the other examples' field-0 ids avoid those rows; concat / sum_x are the forward activations of the table"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, V, size=(B, F))
    if hot_counts:
        ids[:, 0] = rng.integers(len(hot_counts), V, size=B)
    ids[rng.random((B, F)) < p_missing] = -1
    a = 0
    for j, n in enumerate(hot_counts):
        ids[a:a + n, 0] = j
        a += n
    assert a <= B
    if empty_field is not None:
        ids[:, empty_field] = -1
    row_base = (np.arange(F) * V).astype(np.int64)
    R = F * V
    table, lin = q8(rng, (R, D)), q8(rng, R)
    rows = rows_of(ids, row_base)
    x = np.where(rows[:, :, None] >= 0, table[np.maximum(rows, 0)], np.float32(0))
    c = {"ids": ids, "row_base": row_base, "R": R, "B": B, "F": F, "D": D, "V": V, "rows": rows, "table": table, "lin": lin,
         "bias": np.float32(0.375), "grad": ints(rng, -4, 4, (B, F * D)), "dl": ints(rng, -2, 2, B), "scale": SCALE,
         "concat": x.reshape(B, F * D), "sum_x": x.astype(np.float64).sum(1).astype(np.float32), "hot_counts": tuple(hot_counts)}
    assert on_grid(c["sum_x"], 0.125)
    c["ref_plain"] = ref_k4_sgd(c, False)
    c["ref_fm"] = ref_k4_sgd(c, True)
    return c


K4_SHAPES = {"dups": dict(B=700, F=5, V=1500, empty_field=3), "f64": dict(B=150, F=64, V=40)}


@functools.lru_cache(maxsize=None)
def k4_case(D, shape):
    return _k4_case(1000 + D, D=D, **K4_SHAPES[shape])


HOT_WIDTHS = [4, 20, 64, 256]
HOT_COUNTS = [33, 64, 65, 161, 162, 2113]          # 32 + 1, 2 * 32, 2 * 32 + 1, 32 k + 1, 32 k + 2, and 67 pieces (> 64 behind the first)
HOT_SECOND = 75


@functools.lru_cache(maxsize=None)
def hot_case(D, n_hot):
    F = 2 if D >= 64 else 3
    return _k4_case(2000 + D + n_hot, B=2200, F=F, V=1500, D=D, hot_counts=(n_hot, HOT_SECOND))


def hot_geometry(sr, heads, k):
    """(segment start, slots, piece starts) of row k in the sorted row list `sr` with the plan's work list `heads` (sorted)"""
    pos = np.nonzero(sr == k)[0]
    assert pos.size and np.array_equal(pos, np.arange(pos[0], pos[0] + pos.size))
    start, n = int(pos[0]), int(pos.size)
    mine = heads[(heads >= start) & (heads < start + n)]
    return start, n, mine


def want_pieces(start, n):
    """the piece rule of emb_bwd_dups_body: the segment start runs to the first 32-aligned position >= start + 32, then 32 each"""
    first_stop = start + 32 if start % 32 == 0 else ((start + 31) // 32 + 1) * 32
    return [start] + list(range(first_stop, start + n, 32))


FWD_FIELDS = [1, 7, 26, 64]
FWD_B = 67
FWD_PAD = 8


@functools.lru_cache(maxsize=None)
def fwd_case(D, F, bags, B=FWD_B):
    rng = np.random.default_rng(3000 + D * 100 + F + (7 if bags else 0))
    V = 50
    row_base = (np.arange(F) * V).astype(np.int64)
    table, lin = q8(rng, (F * V, D)), q8(rng, F * V)
    if bags:
        col_start, _ = bag_layout(F)
        ids = bag_ids(rng, B, F, V, {1: (0, 1, 1), 2: (0, 1, 2, 2), 4: (0, 1, 2, 4, 4)})      # power-of-two counts: exact means
    else:
        col_start = None
        ids = rng.integers(0, V, size=(B, F))
        ids[rng.random((B, F)) < 0.1] = -1
        if F > 2:
            ids[:, 2] = -1                                  # a field where every id is missing
    concat, S, logit, terms = ref_pool_fwd(ids, col_start, row_base, table, lin, 0.375)
    # a mean over <= 4 rows of 1/8 multiples is a multiple of 1/32; sums over F <= 64 fields of |x| <= 4
    assert on_grid(concat, 1 / 32) and on_grid(S, 1 / 32)
    return {"ids": ids, "col_start": col_start, "row_base": row_base, "table": table, "lin": lin, "bias": np.float32(0.375), "F": F,
            "D": D, "B": B, "concat": concat.astype(np.float32), "sum_x": S.astype(np.float32), "logit": logit, "terms": terms,
            "headroom": float(np.abs(concat).reshape(B, F, D).sum(1).max()) * 32}


BWD_B, BWD_F, BWD_V = 300, 7, 40


@functools.lru_cache(maxsize=None)
def bwd_case(D, ragged=False):
    """ragged bags for the atomic backward; concat / sum_x are independent 1/8-grid inputs (the kernel only reads them).
    ragged=False: every bag holds 0, 1, 2 or 4 ids (exact); True: counts of 3 occur (float64 reference)"""
    rng = np.random.default_rng(4000 + D + (1 if ragged else 0))
    B, F, V = BWD_B, BWD_F, BWD_V
    col_start, col_field = bag_layout(F)
    counts = {1: (0, 1, 1), 2: (0, 1, 2, 2), 4: (0, 1, 2, 3, 3, 4)} if ragged else {1: (0, 1, 1), 2: (0, 1, 2, 2), 4: (0, 1, 2, 4, 4)}
    ids = bag_ids(rng, B, F, V, counts)
    row_base = (np.arange(F) * V).astype(np.int64)
    R = F * V
    c = {"ids": ids, "col_start": col_start, "row_base": row_base, "R": R, "B": B, "F": F, "D": D, "table": q8(rng, (R, D)),
         "lin": q8(rng, R), "bias": np.float32(0.375), "d_concat": ints(rng, -4, 4, (B, F * D)), "concat": q8(rng, (B, F * D)),
         "sum_x": q8(rng, (B, D)) * np.float32(4), "dl": ints(rng, -2, 2, B)}
    for name, scale, start in (("grad", 1.0, False), ("sgd", SCALE, True)):
        t0 = c["table"] if start else np.zeros_like(c["table"])
        l0 = c["lin"] if start else np.zeros_like(c["lin"])
        b0 = c["bias"] if start else np.float32(0)
        t, l, b, tabs, hits = ref_pool_bwd(ids, col_start, col_field, row_base, R, c["d_concat"], c["concat"], c["sum_x"], c["dl"], scale,
                                           t0, l0, b0)
        q = abs(scale) / 8.0 / 4.0                          # gradients on the 1/8 grid, times the scale, over a count of <= 4
        c[name] = {"table": t, "lin": l, "bias": b, "abs": tabs, "hits": hits, "scale": scale, "t0": t0, "l0": l0, "b0": b0,
                   "headroom": max(float(tabs.max()), float(np.abs(l0).max()) + abs(scale) * 2 * float(hits.max()),
                                   abs(float(b0)) + abs(scale) * float(np.abs(c["dl"]).sum())) / q}
        if not ragged:
            assert on_grid(t, q) and on_grid(l, q)
    return c


ADAM_B, ADAM_F, ADAM_VS, ADAM_HOT, ADAM_LR = 400, 4, 120, 80, 0.01


@functools.lru_cache(maxsize=None)
def adam_case(D):
    """Three steps of row-wise Adam whose per-row gradient sums are exact in fp32 at EVERY step although the table leaves the 1/8
    grid after the first: step s draws the ids of its `fresh` examples from rows no earlier step touched (ids in [(s - 1) VS, s VS)
    of every field) -- their x is still on the grid, and only they get d_fm_logit != 0 -- while the examples that revisit the rows of
    step 1 (the hot row of ADAM_HOT slots among them) get d_fm_logit = 0: their FM term is 0 * (finite) = 0 and their gradient is the
    integer d_concat.  The float64 oracle and the fp32 yardstick therefore receive the very sums the device forms."""
    rng = np.random.default_rng(5000 + D)
    B, F, VS = ADAM_B, ADAM_F, ADAM_VS
    V = 3 * VS
    row_base = (np.arange(F) * V).astype(np.int64)
    R = F * V
    table, lin = q8(rng, (R, D)), q8(rng, R)
    state = {dt: [torch.tensor(table, dtype=dt), torch.zeros((R, D), dtype=dt), torch.zeros((R, D), dtype=dt),
                  torch.tensor(lin, dtype=dt), torch.zeros(R, dtype=dt), torch.zeros(R, dtype=dt)] for dt in (torch.float64, torch.float32)}
    steps, headroom = [], 0.0
    for s in (1, 2, 3):
        fresh = np.ones(B, bool) if s == 1 else (np.arange(B) >= B // 2)
        ids = rng.integers(0, VS, size=(B, F))
        ids[fresh] += (s - 1) * VS
        ids[:ADAM_HOT, 0] = 0                               # the hot row: fresh in step 1, revisited afterwards
        ids[rng.random((B, F)) < 0.05] = -1
        rows = rows_of(ids, row_base)
        grad = ints(rng, -4, 4, (B, F * D))
        dl = np.where(fresh, ints(rng, -2, 2, B), np.float32(0)).astype(np.float32)
        t64 = state[torch.float64][0].numpy()
        x = np.where(rows[:, :, None] >= 0, t64[np.maximum(rows, 0)], 0.0)
        assert on_grid(x[fresh], 0.125)                     # the rows the FM term reads are untouched so far
        g = grad.astype(np.float64).reshape(B, F, D) + dl.astype(np.float64)[:, None, None] * (x.sum(1)[:, None, :] - x)
        gl = np.broadcast_to(dl.astype(np.float64)[:, None], rows.shape)
        dense, dabs, dlin, labs = ref_scatter(rows, g, gl, R)
        assert on_grid(dense, 0.125)
        headroom = max(headroom, float(dabs.max()) * 8, float(labs.max()))
        dg, dgl = torch.tensor(dense), torch.tensor(dlin)
        assert torch.equal(dg.float().double(), dg)
        for dt, (w, m, v, lw, ml, vl) in state.items():
            ref_adam_rows(w, m, v, dg, rows, ADAM_LR, s)
            ref_adam_rows(lw, ml, vl, dgl, rows, ADAM_LR, s)
        steps.append({"ids": ids, "grad": grad, "dl": dl})
    want = [a.numpy() for a in state[torch.float64]]
    yard = [float((a32.double() - a64).abs().max()) for a32, a64 in zip(state[torch.float32], state[torch.float64])]
    return {"row_base": row_base, "R": R, "F": F, "D": D, "B": B, "table": table, "lin": lin, "steps": steps, "want": want,
            "yard": yard, "headroom": headroom}


CATCHUP_LR = 0.001
CATCHUP_CASES = {                                             # D, B, F, V, upto, stamps the rows carry
    "near": dict(B=40, F=3, V=50, upto=12, stamps=(0, 12, 3, 7, 11)),
    "far": dict(B=40, F=3, V=50, upto=400, stamps=(0, 400, 100, 399, 250)),        # early stop + closed-form decay of the rest
    "wrap": dict(B=16500, F=8, V=50, upto=12, stamps=(0, 12, 3, 7, 11)),            # 132 000 slots > 8192 blocks * 16 groups
}


@functools.lru_cache(maxsize=None)
def catchup_case(D, kind):
    p = CATCHUP_CASES[kind]
    rng = np.random.default_rng(6000 + D + len(kind))
    B, F, V, upto = p["B"], p["F"], p["V"], p["upto"]
    R = F * V
    row_base = (np.arange(F) * V).astype(np.int64)
    ids = rng.integers(0, V, size=(B, F))
    if kind != "wrap":
        ids[:, 1] = rng.integers(0, 6, size=B)              # the same row named by several slots of one call
        ids[rng.random((B, F)) < 0.1] = -1
    else:
        ids[rng.random((B, F)) < 0.01] = -1
        ids[:, F - 1] = np.where(ids[:, F - 1] >= V // 2, -1, ids[:, F - 1])       # rows that no slot names
    rows = rows_of(ids, row_base)
    named = np.zeros(R, bool)
    named[rows[rows >= 0]] = True
    assert named.any() and not named.all()
    old = rng.choice(np.asarray(p["stamps"], np.int32), size=R).astype(np.int32)
    live = (old > 0)[:, None]
    # made-up state: |w| in [0.5, 4] (an element at zero would never let the early stop fire), moments of a row that has been updated
    w = (rng.uniform(0.5, 4.0, (R, D + 1)) * rng.choice([-1.0, 1.0], (R, D + 1))).astype(np.float32)
    m = np.where(live, rng.standard_normal((R, D + 1)) * 0.1, 0).astype(np.float32)
    v = np.where(live, rng.uniform(1e-4, 1e-2, (R, D + 1)), 0).astype(np.float32)
    out = {}
    for dt in (torch.float64, torch.float32):               # (column D of w / m / v = the row's first-order weight and its moments)
        tw, tm, tv = (torch.tensor(a, dtype=dt) for a in (w, m, v))
        ref_catchup(tw, tm, tv, old, named, upto, CATCHUP_LR)
        out[dt] = (tw, tm, tv)
    w64, m64, v64 = (a.numpy() for a in out[torch.float64])
    w32, m32, v32 = (a.double().numpy() for a in out[torch.float32])

    def rel(a32, a64):
        nz = a64 != 0
        return float((np.abs(a32 - a64)[nz] / np.abs(a64)[nz]).max()) if nz.any() else 0.0
    replay = named & (old > 0) & (old < upto)
    assert replay.any()
    return {"ids": ids, "row_base": row_base, "R": R, "D": D, "F": F, "upto": upto, "old": old, "named": named, "replay": replay,
            "w": w, "m": m, "v": v, "w64": w64, "m64": m64, "v64": v64,
            "yard_w": float(np.abs(w32 - w64).max()), "yard_m": rel(m32, m64), "yard_v": rel(v32, v64)}


@functools.lru_cache(maxsize=None)
def shard_case(D, F):
    """rows_gather / rows_scatter_add / pack inputs at width D.  pos: a permutation for the plain pack; for the de-duplicated pack
    several slots share a destination (uniq = 0 for them)."""
    rng = np.random.default_rng(7000 + D + F)
    R, n = 300, 1003                                        # 1003: odd, no multiple of any RPW * U
    rows = rng.integers(0, R, size=n)
    rows[::11] = -1
    B = 67
    nslots = B * F
    ld = F * D + 8
    c = {"R": R, "n": n, "rows": rows, "table": q8(rng, (R, D)), "lin": q8(rng, R), "gtable": rng.standard_normal((R, D)).astype(np.float32),
         "glin": rng.standard_normal(R).astype(np.float32), "grads": ints(rng, -4, 4, (n, D)), "lgrads": ints(rng, -4, 4, n),
         "B": B, "F": F, "D": D, "ld": ld, "d_concat": ints(rng, -4, 4, (B, F * D)), "concat": q8(rng, (B, F * D)),
         "sum_x": q8(rng, (B, D)) * np.float32(4), "dl": ints(rng, -2, 2, B), "pos": rng.permutation(nslots).reshape(B, F)}
    m = rows >= 0
    want_t, tabs = c["table"].astype(np.float64).copy(), np.abs(c["table"].astype(np.float64))
    want_l, labs = c["lin"].astype(np.float64).copy(), np.abs(c["lin"].astype(np.float64))
    np.add.at(want_t, rows[m], SCALE * c["grads"][m].astype(np.float64))
    np.add.at(tabs, rows[m], abs(SCALE) * np.abs(c["grads"][m]).astype(np.float64))
    np.add.at(want_l, rows[m], SCALE * c["lgrads"][m].astype(np.float64))
    np.add.at(labs, rows[m], abs(SCALE) * np.abs(c["lgrads"][m]).astype(np.float64))
    c["scatter"] = {"table": want_t.astype(np.float32), "lin": want_l.astype(np.float32),
                    "headroom": max(float(tabs.max()), float(labs.max())) * 8}
    # de-duplicated destinations: ndst < nslots, every destination named at least once
    ndst = nslots * 2 // 3
    dst = np.concatenate([np.arange(ndst), rng.integers(0, ndst // 4 + 1, size=nslots - ndst)])
    dst = dst[rng.permutation(nslots)]
    c["dpos"], c["ndst"] = dst.reshape(B, F), ndst
    c["uniq"] = (np.bincount(dst, minlength=ndst)[dst] == 1).astype(np.uint8)
    dlB = np.broadcast_to(c["dl"].astype(np.float64)[:, None], (B, F))
    for fm in (False, True):
        g = ref_slot_grads(np.zeros((B, F), np.int64), c["d_concat"], c["concat"], c["sum_x"], c["dl"], fm)
        plain = np.zeros((nslots, D))
        plain[c["pos"].reshape(-1)] = g.reshape(nslots, D)
        plain_lin = np.zeros(nslots)
        plain_lin[c["pos"].reshape(-1)] = dlB.reshape(-1)
        dd, dabs, dlin, dlabs = ref_scatter(c["dpos"], g, dlB, ndst)
        assert on_grid(dd, 0.125)
        c["pack", fm] = {"rows": plain.astype(np.float32), "lin": plain_lin.astype(np.float32), "drows": dd.astype(np.float32),
                         "dlin": dlin.astype(np.float32), "bias": np.float32(c["dl"].astype(np.float64).sum()),
                         "headroom": max(float(dabs.max()) * 8, float(dlabs.max()), float(np.abs(c["dl"]).sum()))}
    return c


# ----------------------------------------------------------------------------------------------------------------------------------
# CPU: the references themselves, and the exactness precondition of every case
# ----------------------------------------------------------------------------------------------------------------------------------
def test_reference_helpers_against_oracle():
    rng = np.random.default_rng(0)
    B, F, V, D = 9, 5, 6, 12
    col_start, col_field = bag_layout(F)
    ids = bag_ids(rng, B, F, V, {1: (0, 1), 2: (0, 1, 2), 4: (0, 1, 2, 3, 4)})
    row_base = (np.arange(F) * V).astype(np.int64)
    R = F * V
    table, lin, bias = q8(rng, (R, D)), q8(rng, R), np.float32(0.375)
    # forward: mean-pooled bags, sum_x, fm_logit == oracle/torch_ref.py's emb_fm_forward in float64
    concat, S, logit, terms = ref_pool_fwd(ids, col_start, row_base, table, lin, bias)
    tt = torch.tensor(table, dtype=torch.float64, requires_grad=True)
    tl = torch.tensor(lin, dtype=torch.float64, requires_grad=True)
    tb = torch.tensor([float(bias)], dtype=torch.float64, requires_grad=True)
    oc, os_, ol = T.emb_fm_forward(tt, tl, tb, torch.tensor(ids), col_start.tolist(), row_base.tolist())
    assert np.abs(concat - oc.detach().numpy()).max() < 1e-12 and np.abs(S - os_.detach().numpy()).max() < 1e-12
    assert np.abs(logit - ol.detach().numpy()).max() < 1e-11 and (terms >= np.abs(logit)).all()
    # backward with the FM term: the kernels' per-slot gradient d_concat + d_fm_logit * (sum_x - x), scattered, == autograd of
    # sum(concat * d_concat) + sum(fm_logit * d_fm_logit) through the oracle's forward (bags: ref_pool_bwd; single-valued: ref_k4_sgd)
    d_concat, dl = ints(rng, -4, 4, (B, F * D)), ints(rng, -2, 2, B)
    ((oc * torch.tensor(d_concat, dtype=torch.float64)).sum() + (ol * torch.tensor(dl, dtype=torch.float64)).sum()).backward()
    t, l, b, tabs, hits = ref_pool_bwd(ids, col_start, col_field, row_base, R, d_concat, concat, S, dl, SCALE, table, lin, bias)
    assert np.abs(t - (table + SCALE * tt.grad.numpy())).max() < 1e-12
    assert np.abs(l - (lin + SCALE * tl.grad.numpy())).max() < 1e-12 and abs(b - (float(bias) + SCALE * float(tb.grad))) < 1e-12
    assert (tabs >= np.abs(t) - 1e-12).all() and hits.sum() == (ids >= 0).sum()
    c = _k4_case(1, B=20, F=4, V=5, D=8, hot_counts=(7, 3), empty_field=2)
    tt = torch.tensor(c["table"], dtype=torch.float64, requires_grad=True)
    tl = torch.tensor(c["lin"], dtype=torch.float64, requires_grad=True)
    tb = torch.tensor([float(c["bias"])], dtype=torch.float64, requires_grad=True)
    oc, os_, ol = T.emb_fm_forward(tt, tl, tb, torch.tensor(c["ids"]), list(range(5)), c["row_base"].tolist())
    assert np.array_equal(oc.detach().numpy(), c["concat"]) and np.array_equal(os_.detach().numpy(), c["sum_x"])
    ((oc * torch.tensor(c["grad"], dtype=torch.float64)).sum() + (ol * torch.tensor(c["dl"], dtype=torch.float64)).sum()).backward()
    assert np.array_equal(c["ref_fm"]["table"], (c["table"] + SCALE * tt.grad.numpy()).astype(np.float32))
    assert np.array_equal(c["ref_fm"]["lin"], (c["lin"] + SCALE * tl.grad.numpy()).astype(np.float32))
    assert c["ref_fm"]["bias"] == np.float32(float(c["bias"]) + SCALE * float(tb.grad))
    assert np.array_equal(c["ref_plain"]["lin"], c["ref_fm"]["lin"]) and not np.array_equal(c["ref_plain"]["table"], c["ref_fm"]["table"])
    # the exact grid: the same sums in fp32, accumulated slot by slot in two different orders, equal the float64 result bit for bit
    g = ref_slot_grads(c["rows"], c["grad"], c["concat"], c["sum_x"], c["dl"], True).astype(np.float32)
    for order in (np.arange(c["rows"].size), np.arange(c["rows"].size)[::-1]):
        acc = np.zeros((c["R"], c["D"]), np.float32)
        for s in order:
            r = c["rows"].reshape(-1)[s]
            if r >= 0:
                acc[r] += g.reshape(-1, c["D"])[s]
        assert np.array_equal(c["table"] + np.float32(SCALE) * acc, c["ref_fm"]["table"])
    # Adam: with every row touched the row-wise step is the dense step; a decay-only catch-up is the dense step with a zero gradient
    w0, g0 = rng.standard_normal((6, 4)), rng.standard_normal((6, 4))
    w, m, v = torch.tensor(w0), torch.full((6, 4), 0.01, dtype=torch.float64), torch.full((6, 4), 0.002, dtype=torch.float64)
    wd, md, vd = w.clone(), m.clone(), v.clone()
    ref_adam_rows(w, m, v, torch.tensor(g0), np.arange(6), 0.01, 3)
    T.adam_dense_step(wd, torch.tensor(g0), md, vd, 0.01, 3, B1, B2, EPS)
    assert torch.allclose(w, wd, rtol=0, atol=1e-15) and torch.allclose(m, md, rtol=0, atol=1e-15) and torch.allclose(v, vd, rtol=0, atol=1e-15)
    old = np.array([0, 2, 5, 7, 5, 3], np.int32)
    named = np.array([True, True, True, True, False, True])
    wc, mc, vc = wd.clone(), md.clone(), vd.clone()
    ref_catchup(wc, mc, vc, old, named, 7, 0.01)
    for r in range(6):
        wr, mr, vr = wd[r].clone(), md[r].clone(), vd[r].clone()
        if named[r] and old[r] > 0:
            for s in range(old[r] + 1, 8):
                T.adam_dense_step(wr, torch.zeros(4, dtype=torch.float64), mr, vr, 0.01, s, B1, B2, EPS)
        assert torch.allclose(wc[r], wr, rtol=0, atol=1e-15) and torch.allclose(mc[r], mr, rtol=0, atol=1e-18)
        assert torch.allclose(vc[r], vr, rtol=0, atol=1e-18)
    assert torch.equal(wc[0], wd[0]) and torch.equal(wc[3], wd[3]) and torch.equal(wc[4], wd[4]) and not torch.equal(wc[1], wd[1])


def test_exactness_preconditions():
    """every case whose device output is compared bit for bit: the largest partial sum any order can form stays below 2^24 quanta"""
    worst = 0.0
    for D in WIDTHS:
        for shape in K4_SHAPES:
            c = k4_case(D, shape)
            worst = max(worst, c["ref_plain"]["headroom"], c["ref_fm"]["headroom"])
        for F in FWD_FIELDS:
            for bags in (False, True):
                worst = max(worst, fwd_case(D, F, bags)["headroom"])
        worst = max(worst, bwd_case(D)["grad"]["headroom"], bwd_case(D)["sgd"]["headroom"], adam_case(D)["headroom"])
        for F in (5, 64):
            c = shard_case(D, F)
            worst = max(worst, c["scatter"]["headroom"], c["pack", False]["headroom"], c["pack", True]["headroom"])
    for D in HOT_WIDTHS:
        for n_hot in HOT_COUNTS:
            c = hot_case(D, n_hot)
            worst = max(worst, c["ref_plain"]["headroom"], c["ref_fm"]["headroom"])
    for bags in (False, True):
        worst = max(worst, fwd_case(20, 7, bags, FWD_WRAP_B)["headroom"])
    assert 0 < worst < EXACT, worst


def test_hot_piece_rule():
    assert want_pieces(0, 33) == [0, 32] and want_pieces(0, 64) == [0, 32] and want_pieces(0, 65) == [0, 32, 64]
    assert len(want_pieces(0, 2113)) == 67 and want_pieces(0, 2113)[-1] == 2112
    assert want_pieces(33, 75) == [33, 96] and want_pieces(65, 75) == [65, 128] and want_pieces(64, 75) == [64, 96, 128]


# ----------------------------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ----------------------------------------------------------------------------------------------------------------------------------
def _ops():
    from deep_recommenders_amd import ops
    return ops


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device="cuda")
    return torch.from_numpy(a).cuda()


def _padded(a, pad, poison):
    """a [B, n] as a view of a [B, n + pad] device buffer whose padding holds `poison`: (view, buffer)"""
    B, n = a.shape
    buf = torch.full((B, n + pad), float(poison), dtype=torch.float32, device="cuda")
    buf[:, :n] = _dev(a)
    return buf[:, :n], buf


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_array_equal(_bits(got), _bits(np.asarray(want, np.float32).reshape(got.shape)), err_msg=what)


def _record(value):
    rec = torch.zeros(1, dtype=torch.int32, device="cuda")
    rec.view(torch.float32).fill_(float(value))
    return rec


def _plan_path(ops, radix):
    """context: the slot plan's radix path (small limit 0) or its default"""
    class _Ctx:
        def __enter__(self):
            self.prev = ops.emb_plan_set_small_limit(0) if radix else None

        def __exit__(self, *exc):
            if self.prev is not None:
                ops.emb_plan_set_small_limit(self.prev)
    return _Ctx()


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. forward
# ----------------------------------------------------------------------------------------------------------------------------------
FWD_WRAP_B = 8192 + 5


def _check_fwd(c):
    ops = _ops()
    B, F, D = c["B"], c["F"], c["D"]
    assert c["headroom"] < EXACT
    ld = F * D + FWD_PAD
    concat = torch.full((B, ld), float(SENTINEL), dtype=torch.float32, device="cuda")
    cs = None if c["col_start"] is None else _dev(c["col_start"])
    _, sum_x, fm = ops.emb_pool_fwd(_dev(c["ids"]), F, cs, _dev(c["row_base"]), _dev(c["table"]), _dev(c["lin"]),
                                    _dev(np.array([c["bias"]], np.float32)), ld_concat=ld, concat=concat)
    what = "D=%d F=%d %s" % (D, F, "bags" if cs is not None else "single-valued")
    got = concat.cpu().numpy()
    _same(got[:, :F * D], c["concat"], what + ": concat")
    assert (got[:, F * D:] == SENTINEL).all(), what + ": a padding column of concat was written"
    _same(sum_x, c["sum_x"], what + ": sum_x")
    # fm_logit: S_d^2 (1 rounding), - SS_d (1), three adds in the lane, log2(LPR) <= 6 butterfly steps, * 0.5 (exact), + lin, + bias (2);
    # SS_d and lin are themselves exact on this grid
    err = np.abs(fm.cpu().numpy().astype(np.float64) - c["logit"])
    tol = gamma(13) * c["terms"]
    worst = int(np.argmax(err - tol))
    print("%s: fm_logit worst err %.3e tol %.3e" % (what, err[worst], tol[worst]))
    assert (err <= tol).all(), what + ": fm_logit"


@gpu
@pytest.mark.parametrize("bags", [False, True], ids=["sv", "bags"])
@pytest.mark.parametrize("D", WIDTHS)
def test_emb_pool_fwd_every_width(D, bags):
    """F = 1, 7, 26, 64: the f0 += NS * U loop takes a single pass, several passes and a ragged last pass at every width"""
    for F in FWD_FIELDS:
        _check_fwd(fwd_case(D, F, bags))


@gpu
@pytest.mark.parametrize("bags", [False, True], ids=["sv", "bags"])
def test_emb_pool_fwd_past_one_launch(bags):
    _check_fwd(fwd_case(20, 7, bags, FWD_WRAP_B))


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. atomic backward
# ----------------------------------------------------------------------------------------------------------------------------------
def _run_pool_bwd(c, form):
    ops = _ops()
    r = c[form]
    t, l, b = _dev(r["t0"]).clone(), _dev(r["l0"]).clone(), _dev(np.array([r["b0"]], np.float32))
    dc, _ = _padded(c["d_concat"], 4, float("nan"))
    cc, _ = _padded(c["concat"], 8, float("nan"))
    ops.emb_pool_bwd(_dev(c["ids"]), c["F"], _dev(c["col_start"]), _dev(c["row_base"]), c["D"], dc, cc, _dev(c["sum_x"]), _dev(c["dl"]),
                     r["scale"], t, l, b)
    return t.cpu().numpy(), l.cpu().numpy(), float(b.item())


@gpu
@pytest.mark.parametrize("form", ["grad", "sgd"])
@pytest.mark.parametrize("D", WIDTHS)
def test_emb_pool_bwd_every_width(D, form):
    """gradient form (scale 1 into zeros) and fused-SGD form (scale -1/8 into the table); bags of 0, 1, 2 and 4 ids: exact"""
    c = bwd_case(D)
    r = c[form]
    assert r["headroom"] < EXACT
    t, l, b = _run_pool_bwd(c, form)
    _same(t, r["table"], "table")
    _same(l, r["lin"], "first-order weights")
    assert np.float32(b) == np.float32(r["bias"])


@gpu
def test_emb_pool_bwd_count_of_three():
    """bags of 3 ids: g / 3 is rounded once and a row's `hits` contributions meet in any order -> g(hits + 1) * sum|terms|"""
    c = bwd_case(20, ragged=True)
    assert (np.diff(c["col_start"]) == 4).any() and ((c["ids"] >= 0).reshape(c["B"], -1)[:, 3:7].sum(1) == 3).any()
    r = c["sgd"]
    t, l, b = _run_pool_bwd(c, "sgd")
    err = np.abs(t.astype(np.float64) - r["table"])
    tol = gamma(r["hits"] + 1)[:, None] * r["abs"]
    print("count of three: worst err %.3e, tolerance there %.3e" % (err.max(), tol.reshape(-1)[np.argmax(err)]))
    assert (err <= tol).all()
    _same(l, r["lin"].astype(np.float32), "first-order weights")
    assert np.float32(b) == np.float32(r["bias"])


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. K4, SGD form
# ----------------------------------------------------------------------------------------------------------------------------------
K4_VARIANTS = ["plain", "plain_parked", "concat", "snapshot", "nan_scratch", "split_lin"]


def _k4_device(c):
    grad, _ = _padded(c["grad"], 4, float("nan"))
    concat, _ = _padded(c["concat"], 8, float("nan"))
    return {"ids": _dev(c["ids"]), "rb": _dev(c["row_base"]), "grad": grad, "concat": concat, "sum_x": _dev(c["sum_x"]),
            "dl": _dev(c["dl"]), "table": _dev(c["table"]), "lin": _dev(c["lin"])}


def _run_k4_sgd(c, d, plan, variant, amax0=0.0):
    """one variant of dr_emb_pool_bwd_sorted on fresh copies of the tables: (table, lin, bias, amax record or None)"""
    ops = _ops()
    D, R, n = c["D"], c["R"], c["B"] * c["F"]
    t, l, b = d["table"].clone(), d["lin"].clone(), _dev(np.array([c["bias"]], np.float32))
    args = (d["ids"], d["rb"], plan, D, R, d["grad"], d["dl"], c["scale"], t, l, b)
    rec = None
    if variant == "plain":                                   # no FM term, no scratch rows: hot rows' pieces meet through atomics
        ops.emb_pool_bwd_sorted(*args)
    elif variant == "plain_parked":                          # no FM term; hot rows' pieces parked in scratch rows nobody filled
        rec = _record(amax0)
        ops.emb_pool_bwd_sorted(*args, x_sorted=torch.full((n, D), float("nan"), device="cuda"), table_amax=rec)
    elif variant == "concat":                                # x of the shared-row slots from the forward's concat
        ops.emb_pool_bwd_sorted(*args, concat=d["concat"], sum_x=d["sum_x"])
    elif variant == "snapshot":                              # ... from the snapshot of the work list's rows
        rec = _record(amax0)
        xs = torch.full((n, D), float("nan"), device="cuda")
        ops.emb_snapshot_sorted_rows(plan, t, R, xs)
        ops.emb_pool_bwd_sorted(*args, sum_x=d["sum_x"], x_sorted=xs, table_amax=rec)
    elif variant == "nan_scratch":                           # ... from the table itself (deterministic mode): the scratch rows start as NaN
        rec = _record(amax0)
        ops.emb_pool_bwd_sorted(*args, sum_x=d["sum_x"], x_sorted=torch.full((n, D), float("nan"), device="cuda"), table_amax=rec)
    elif variant == "split_lin":                             # first-order weights of unique rows by dr_emb_lin_update_unique
        ops.emb_pool_bwd_sorted(*args, concat=d["concat"], sum_x=d["sum_x"], parts=3 | 4)
        ops.emb_lin_update_unique(d["ids"], d["rb"], plan, d["dl"], c["scale"], l)
    else:
        raise AssertionError(variant)
    return t.cpu().numpy(), l.cpu().numpy(), b.cpu().numpy()[0], (None if rec is None else int(rec.item()))


def _check_k4_sgd(c, d, plan, variant, what, amax0=0.0):
    ref = c["ref_plain"] if variant.startswith("plain") else c["ref_fm"]
    assert ref["headroom"] < EXACT
    t, l, b, rec = _run_k4_sgd(c, d, plan, variant, amax0)
    what = "%s %s" % (what, variant)
    _same(t, ref["table"], what + ": table")
    _same(l, ref["lin"], what + ": first-order weights")
    _same(np.array([b]), np.array([ref["bias"]]), what + ": bias")
    if rec is not None:
        want = int(np.array([max(amax0, ref["written_amax"])], np.float32).view(np.int32)[0])
        assert rec == want, "%s: amax record %#x, want %#x" % (what, rec, want)


@gpu
@pytest.mark.parametrize("radix", [False, True], ids=["default_plan", "radix_plan"])
@pytest.mark.parametrize("shape", list(K4_SHAPES))
@pytest.mark.parametrize("D", WIDTHS)
def test_emb_bwd_sorted_sgd_every_width(D, shape, radix):
    """table, first-order weights and bias bit for bit against the float64 reference in every variant (hence equal across the
    variants and the plan paths); missing ids, a field with no id at all (`dups`), F = 64 (`f64`)"""
    ops = _ops()
    c = k4_case(D, shape)
    with _plan_path(ops, radix):
        d = _k4_device(c)
        plan = ops.emb_sort_slots(d["ids"], d["rb"], c["R"])
        assert int(plan.dup_count[0].item()) > 0                              # both passes have work: shared rows ...
        assert shape != "dups" or int(plan.flags[:c["B"] * c["F"]].sum().item()) > 0      # ... and rows unique in the batch
        for i, variant in enumerate(K4_VARIANTS):
            # the record starts below, or above, everything the call writes
            _check_k4_sgd(c, d, plan, variant, "D=%d %s" % (D, shape), amax0=(0.5, 1.0e6)[i % 2] if shape == "dups" else 0.0)


@gpu
@pytest.mark.parametrize("radix", [False, True], ids=["default_plan", "radix_plan"])
@pytest.mark.parametrize("n_hot", HOT_COUNTS)
@pytest.mark.parametrize("D", HOT_WIDTHS)
def test_emb_bwd_sorted_hot_row_geometry(D, n_hot, radix):
    """A row of n_hot slots at sorted position 0 (pieces at 0, 32, 64, ...: a single-slot last piece when n_hot = 1 mod 32, 67 pieces
    at 2113 so that the apply kernel's 64-piece ballot runs twice) and a row of 75 slots behind it (a segment that starts where the
    first ends).  The geometry is read back from the plan before the results are compared."""
    ops = _ops()
    c = hot_case(D, n_hot)
    with _plan_path(ops, radix):
        d = _k4_device(c)
        plan = ops.emb_sort_slots(d["ids"], d["rb"], c["R"])
        L = plan.sorted_len()
        sr = plan.rows.cpu().numpy()[:L]
        heads = np.sort(plan.dup_heads.cpu().numpy()[:int(plan.dup_count[0].item())])
        start, n, pieces = hot_geometry(sr, heads, 0)
        assert (start, n) == (0, n_hot) and list(pieces) == want_pieces(0, n_hot)
        assert len(pieces) == (n_hot + 31) // 32 and n - int(pieces[-1]) == (n_hot - 1) % 32 + 1
        start2, n2, pieces2 = hot_geometry(sr, heads, 1)
        assert (start2, n2) == (n_hot, HOT_SECOND) and list(pieces2) == want_pieces(n_hot, HOT_SECOND)
        for variant in ("nan_scratch", "snapshot", "plain_parked", "concat"):
            _check_k4_sgd(c, d, plan, variant, "D=%d n_hot=%d" % (D, n_hot))


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. K4, Adam form
# ----------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("radix", [False, True], ids=["default_plan", "radix_plan"])
@pytest.mark.parametrize("D", WIDTHS)
def test_emb_bwd_sorted_adam_every_width(D, radix):
    """three steps with the FM term, first-order moments as two arrays and interleaved in one [R, 2] array; a hot row of 80 slots
    whose segment-start head walks the whole segment.  w, m, v (and the first-order w, m, v) against the float64 oracle, each within
    four times the largest error of the fp32 torch evaluation of the same steps."""
    ops = _ops()
    c = adam_case(D)
    assert c["headroom"] < EXACT
    R, F = c["R"], c["F"]
    rb = _dev(c["row_base"])
    zero_bias = torch.zeros(1, device="cuda")
    with _plan_path(ops, radix):
        for interleaved in (False, True):
            t, l = _dev(c["table"]).clone(), _dev(c["lin"]).clone()
            m, v = torch.zeros_like(t), torch.zeros_like(t)
            if interleaved:
                mv = torch.zeros((R, 2), device="cuda")
                ml, vl = mv[:, 0], mv[:, 1]
            else:
                ml, vl = torch.zeros_like(l), torch.zeros_like(l)
            for s, st in enumerate(c["steps"], start=1):
                ids = _dev(st["ids"])
                plan = ops.emb_sort_slots(ids, rb, R)
                if s == 1:
                    sr = plan.rows.cpu().numpy()[:plan.sorted_len()]
                    assert (sr == 0).sum() > 64              # the hot row's slots are all on the sorted list
                concat, sum_x, _ = ops.emb_pool_fwd(ids, F, None, rb, t, l, zero_bias)
                grad, _ = _padded(st["grad"], 4, float("nan"))
                ops.emb_pool_bwd_sorted_adam(ids, rb, plan, D, R, grad, _dev(st["dl"]), ops.adam_lr_t(ADAM_LR, B1, B2, s), B1, B2, EPS,
                                             t, m, v, l, ml, vl, concat=concat, sum_x=sum_x)
            got = [a.cpu().numpy().astype(np.float64) for a in (t, m, v, l, ml, vl)]
            for name, g, want, yard in zip(("w", "m", "v", "lin w", "lin m", "lin v"), got, c["want"], c["yard"]):
                err = float(np.abs(g - want).max())
                print("D=%d interleaved=%d %s: err %.3e, fp32 yardstick %.3e" % (D, interleaved, name, err, yard))
                assert err <= 4 * yard, (name, err, yard)


@gpu
def test_emb_bwd_sorted_adam_lin_old_t_changes_no_bit():
    """lin_old_t hands the Adam form the first-order weights the forward read, so that a row unique in the batch is not read again:
    the same values by another route.  One step (FM term, non-zero moments) over a batch with a unique row, a row five slots share
    and a missing id: table, m, v and the first-order w, m, v equal the call without lin_old_t bit for bit."""
    ops = _ops()
    rng = np.random.default_rng(77)
    B, F, D, V = 64, 3, 8, 50
    R = F * V
    ids = rng.integers(0, V - 1, size=(B, F))
    ids[0, 0] = V - 1                                       # a row no other slot looks up
    ids[1:6, 1] = 7                                         # a row several slots share
    ids[2, 2] = -1                                          # a missing id
    assert (ids[:, 0] == V - 1).sum() == 1 and (ids[:, 1] == 7).sum() >= 5 and (ids < 0).sum() == 1
    row_base = (np.arange(F) * V).astype(np.int64)
    rb, ids_d = _dev(row_base), _dev(ids)
    plan = ops.emb_sort_slots(ids_d, rb, R)
    flags = plan.flags.cpu().numpy()[:B * F].reshape(B, F)
    assert flags[0, 0] == 1 and not flags[1:6, 1].any()      # the plan sees them as unique / shared
    start = [_dev(a.astype(np.float32)) for a in (rng.standard_normal((R, D)), 0.1 * rng.standard_normal((R, D)), rng.random((R, D)),
                                                  rng.standard_normal(R), 0.1 * rng.standard_normal(R), rng.random(R))]
    grad = _dev(rng.standard_normal((B, F * D)).astype(np.float32))
    dl = _dev(rng.standard_normal(B).astype(np.float32))
    concat, sum_x, _ = ops.emb_pool_fwd(ids_d, F, None, rb, start[0], start[3], torch.zeros(1, device="cuda"))
    lin_old_t = start[3][_dev(np.maximum(ids + row_base[None, :], 0))].t().contiguous()
    results = []
    for lo in (None, lin_old_t):
        t, m, v, l, ml, vl = (a.clone() for a in start)
        ops.emb_pool_bwd_sorted_adam(ids_d, rb, plan, D, R, grad, dl, ops.adam_lr_t(ADAM_LR, B1, B2, 3), B1, B2, EPS, t, m, v, l, ml, vl,
                                     concat=concat, sum_x=sum_x, lin_old_t=lo)
        results.append((t, m, v, l, ml, vl))
    for name, a0, plain, saved in zip(("w", "m", "v", "lin w", "lin m", "lin v"), start, *results):
        assert not torch.equal(plain, a0), name              # the step moved it
        _same(saved, plain.cpu().numpy(), name)


# ----------------------------------------------------------------------------------------------------------------------------------
# 6. dr_adam_catchup_rows
# ----------------------------------------------------------------------------------------------------------------------------------
def _check_catchup(c, stamp, interleaved):
    ops = _ops()
    D, R, upto = c["D"], c["R"], c["upto"]
    t, m, v = (_dev(a[:, :D]) for a in (c["w"], c["m"], c["v"]))
    l = _dev(c["w"][:, D])
    if interleaved:
        mv = _dev(np.stack([c["m"][:, D], c["v"][:, D]], 1))
        ml, vl = mv[:, 0], mv[:, 1]
    else:
        ml, vl = _dev(c["m"][:, D]), _dev(c["v"][:, D])
    step = _dev(c["old"])
    ops.adam_catchup_rows(_dev(c["ids"]), _dev(c["row_base"]), t, m, v, l, ml, vl, step, upto, stamp, CATCHUP_LR, B1, B2, EPS)
    gw = np.concatenate([t.cpu().numpy(), l.cpu().numpy()[:, None]], 1)
    gm = np.concatenate([m.cpu().numpy(), ml.cpu().numpy()[:, None]], 1)
    gv = np.concatenate([v.cpu().numpy(), vl.cpu().numpy()[:, None]], 1)
    np.testing.assert_array_equal(step.cpu().numpy(), np.where(c["named"], stamp, c["old"]))
    same = ~c["replay"]                                      # not named, never updated (stamp 0), or nothing to replay: bit-unchanged
    for got, src in ((gw, c["w"]), (gm, c["m"]), (gv, c["v"])):
        np.testing.assert_array_equal(_bits(got[same]), _bits(src[same]))
    rp = c["replay"]
    # w: the fp32 yardstick, plus what the early stop drops: every later step is smaller than the last by >= b1 / sqrt(b2), and the
    # stop fires once a step is below `tiny` = 2^-26 |w|
    stop = 2.0 ** -26 * np.abs(c["w64"]) / (1.0 - B1 / math.sqrt(B2))
    err_w = np.abs(gw.astype(np.float64) - c["w64"])[rp]
    err_m = np.abs(gm.astype(np.float64) - c["m64"])[rp]
    err_v = np.abs(gv.astype(np.float64) - c["v64"])[rp]
    print("catch-up D=%d: w err %.3e (yard %.3e), m rel %.3e (yard %.3e), v rel %.3e (yard %.3e)" % (
        D, err_w.max(), c["yard_w"], (err_m / np.abs(c["m64"][rp])).max(), c["yard_m"], (err_v / np.abs(c["v64"][rp])).max(), c["yard_v"]))
    assert (err_w <= 4 * c["yard_w"] + stop[rp]).all()
    assert (err_m <= 4 * c["yard_m"] * np.abs(c["m64"][rp])).all()
    assert (err_v <= 4 * c["yard_v"] * np.abs(c["v64"][rp])).all()


@gpu
@pytest.mark.parametrize("interleaved", [False, True], ids=["two_arrays", "interleaved"])
@pytest.mark.parametrize("export", [False, True], ids=["before_step", "export"])
@pytest.mark.parametrize("D", [4, 16, 64, 68, 132, 256])
def test_adam_catchup_rows_every_width(D, export, interleaved):
    """D <= 64: one piece; 68, 132, 256: the 64-float piece walk with a partial, a partial and a full last piece"""
    c = catchup_case(D, "near")
    _check_catchup(c, c["upto"] if export else c["upto"] + 1, interleaved)


@gpu
@pytest.mark.parametrize("D", [16, 132])
def test_adam_catchup_rows_long_gap(D):
    """gaps of up to 300 steps: the replay stops early and m, v take the rest of their decay in closed form"""
    c = catchup_case(D, "far")
    _check_catchup(c, c["upto"] + 1, D == 132)


@gpu
def test_adam_catchup_rows_past_one_launch():
    c = catchup_case(4, "wrap")
    assert c["ids"].size > 8192 * 16
    _check_catchup(c, c["upto"] + 1, False)


# ----------------------------------------------------------------------------------------------------------------------------------
# 7. sharding primitives
# ----------------------------------------------------------------------------------------------------------------------------------
def _check_gather(rows, table, lin):
    ops = _ops()
    n, D = rows.size, table.shape[1]
    present = rows >= 0
    want = np.where(present[:, None], table[np.maximum(rows, 0)], np.float32(0))
    want_lin = np.where(present, lin[np.maximum(rows, 0)], np.float32(0))
    for with_lin in (True, False):
        out = torch.full((n + 1, D), float(SENTINEL), device="cuda")
        out_lin = torch.full((n + 1,), float(SENTINEL), device="cuda") if with_lin else None
        ops.rows_gather(_dev(rows), _dev(table), _dev(lin) if with_lin else None, out_rows=out, out_lin=out_lin)
        got = out.cpu().numpy()
        _same(got[:n], want, "gathered rows (out_lin %s)" % with_lin)
        assert (got[n] == SENTINEL).all()
        if with_lin:
            _same(out_lin.cpu().numpy()[:n], want_lin, "gathered first-order weights")
            assert out_lin[n].item() == SENTINEL


@gpu
@pytest.mark.parametrize("D", WIDTHS)
def test_rows_gather_and_scatter_every_width(D):
    ops = _ops()
    c = shard_case(D, 5)
    _check_gather(c["rows"], c["gtable"], c["glin"])
    assert c["scatter"]["headroom"] < EXACT
    t, l = _dev(c["table"]).clone(), _dev(c["lin"]).clone()
    ops.rows_scatter_add(_dev(c["rows"]), _dev(c["grads"]), _dev(c["lgrads"]), SCALE, t, l)
    _same(t, c["scatter"]["table"], "scattered table")
    _same(l, c["scatter"]["lin"], "scattered first-order weights")
    t2 = _dev(c["table"]).clone()
    ops.rows_scatter_add(_dev(c["rows"]), _dev(c["grads"]), None, SCALE, t2, None)          # no first-order table
    _same(t2, c["scatter"]["table"], "scattered table, no first-order part")


@gpu
def test_rows_gather_past_one_launch():
    rng = np.random.default_rng(8)
    R, D, n = 500, 256, 32768 + 37
    rows = rng.integers(0, R, size=n)
    rows[::13] = -1
    _check_gather(rows, rng.standard_normal((R, D)).astype(np.float32), rng.standard_normal(R).astype(np.float32))


@gpu
@pytest.mark.parametrize("F", [5, 64])
@pytest.mark.parametrize("D", WIDTHS)
def test_emb_pack_grads_every_width(D, F):
    """plain pack (pos a permutation: every destination stored once) and de-duplicated pack (shared destinations add), with and
    without the FM term, gradient rows with a pitch > F * D whose padding is NaN"""
    ops = _ops()
    c = shard_case(D, F)
    B, n = c["B"], c["B"] * F
    dc, _ = _padded(c["d_concat"], 8, float("nan"))
    cc, _ = _padded(c["concat"], 4, float("nan"))
    for fm in (False, True):
        r = c["pack", fm]
        assert r["headroom"] < EXACT
        concat, sum_x = (cc, _dev(c["sum_x"])) if fm else (None, None)
        out = torch.full((n + 1, D), float(SENTINEL), device="cuda")
        out_lin = torch.full((n + 1,), float(SENTINEL), device="cuda")
        bias = torch.full((1,), 3.0, device="cuda")
        ops.emb_pack_grads(_dev(c["pos"]), D, dc, concat, sum_x, _dev(c["dl"]), out, out_lin, bias)
        what = "D=%d F=%d fm=%s" % (D, F, fm)
        _same(out[:n], r["rows"], what + ": packed rows")
        _same(out_lin[:n], r["lin"], what + ": packed first-order gradients")
        assert (out[n] == float(SENTINEL)).all() and out_lin[n].item() == SENTINEL
        assert bias.item() == 3.0 + float(r["bias"])
        nd = c["ndst"]
        out = torch.zeros((nd + 1, D), device="cuda")
        out_lin = torch.zeros(nd + 1, device="cuda")
        out[nd], out_lin[nd] = float(SENTINEL), float(SENTINEL)
        ops.emb_pack_grads(_dev(c["dpos"]), D, dc, concat, sum_x, _dev(c["dl"]), out, out_lin, None, unique_flags=_dev(c["uniq"]))
        _same(out[:nd], r["drows"], what + ": de-duplicated rows")
        _same(out_lin[:nd], r["dlin"], what + ": de-duplicated first-order gradients")
        assert (out[nd] == float(SENTINEL)).all() and out_lin[nd].item() == SENTINEL
        out = torch.full((n + 1, D), float(SENTINEL), device="cuda")
        ops.emb_pack_grads(_dev(c["pos"]), D, dc, concat, sum_x, _dev(c["dl"]), out)          # no out_lin, no bias
        _same(out[:n], r["rows"], what + ": packed rows, no first-order output")
        assert (out[n] == float(SENTINEL)).all()


# ----------------------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ----------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("D", [0, 2, 6, 260])
def test_bad_widths_are_refused(D):
    """every entry point above answers a width outside {4, 8, ..., 256} with DR_EINVAL and leaves its destination alone"""
    ops = _ops()
    rng = np.random.default_rng(9)
    B, F, V = 8, 3, 5
    R = F * V
    W = max(D, 8)                                            # room behind the buffers, whatever the call believes their width to be
    ids = _dev(rng.integers(0, V, size=(B, F)))
    rb = _dev((np.arange(F) * V).astype(np.int64))
    cs = _dev(np.arange(F + 1).astype(np.int32))
    plan = ops.emb_sort_slots(ids, rb, R)

    def buf(*shape):
        return torch.full(shape, float(SENTINEL), device="cuda")

    def narrow(rows):                                        # a [rows, D] view (what the wrappers read D from) of a roomy buffer
        return buf(rows, W)[:, :D] if D > 0 else torch.empty((rows, 0), device="cuda")
    table = torch.full((R, D), float(SENTINEL), device="cuda")
    lin, m_lin, v_lin, bias = buf(R), buf(R), buf(R), buf(1)
    m, v = torch.full((R, D), float(SENTINEL), device="cuda"), torch.full((R, D), float(SENTINEL), device="cuda")
    wide = buf(B, F * W + 8)
    sum_x, dl, fm = buf(B, W), buf(B), buf(B)
    out = buf(B * F, W)
    out_lin = buf(B * F)
    step = torch.full((R,), 3, dtype=torch.int32, device="cuda")
    rows = _dev(rng.integers(0, R, size=B * F))
    pos = _dev(rng.permutation(B * F).reshape(B, F))
    uniq = torch.ones(B * F, dtype=torch.uint8, device="cuda")
    calls = {
        "emb_pool_fwd": lambda: ops.emb_pool_fwd(ids, F, None, rb, table, lin, bias, ld_concat=wide.shape[1], concat=wide, sum_x=sum_x, fm_logit=fm),
        "emb_pool_fwd bags": lambda: ops.emb_pool_fwd(ids, F, cs, rb, table, lin, bias, ld_concat=wide.shape[1], concat=wide, sum_x=sum_x,
                                                      fm_logit=fm),
        "emb_pool_bwd": lambda: ops.emb_pool_bwd(ids, F, cs, rb, D, wide, wide, sum_x, dl, SCALE, table, lin, bias),
        "emb_pool_bwd_sorted": lambda: ops.emb_pool_bwd_sorted(ids, rb, plan, D, R, wide, dl, SCALE, table, lin, bias),
        "emb_pool_bwd_sorted_ex": lambda: ops.emb_pool_bwd_sorted(ids, rb, plan, D, R, wide, dl, SCALE, table, lin, bias, x_sorted=out,
                                                                  table_amax=_record(0.0)),
        "emb_pool_bwd_sorted_parts": lambda: ops.emb_pool_bwd_sorted(ids, rb, plan, D, R, wide, dl, SCALE, table, lin, bias, parts=1),
        "emb_pool_bwd_sorted_adam": lambda: ops.emb_pool_bwd_sorted_adam(ids, rb, plan, D, R, wide, dl, 0.01, B1, B2, EPS, table, m, v, lin,
                                                                         m_lin, v_lin),
        "adam_catchup_rows": lambda: ops.adam_catchup_rows(ids, rb, table, m, v, lin, m_lin, v_lin, step, 7, 8, 0.01, B1, B2, EPS),
        "rows_gather": lambda: ops.rows_gather(rows, table, lin, out_rows=out, out_lin=out_lin),
        "rows_scatter_add": lambda: ops.rows_scatter_add(rows, narrow(B * F), dl.new_ones(B * F), SCALE, table, lin),
        "emb_pack_grads": lambda: ops.emb_pack_grads(pos, D, wide, wide, sum_x, dl, out, out_lin, bias),
        "emb_pack_grads_dedup": lambda: ops.emb_pack_grads(pos, D, wide, wide, sum_x, dl, out, out_lin, bias, unique_flags=uniq),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="DR_EINVAL"):
            call()
        torch.cuda.synchronize()
        for t in (table, m, v, lin, m_lin, v_lin, bias, wide, sum_x, fm, out, out_lin):
            assert bool((t == float(SENTINEL)).all()), "%s wrote to a buffer it refused to work on" % name
        assert bool((step == 3).all()), name
