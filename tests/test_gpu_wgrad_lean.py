"""The register-split wgrad (csrc/bf3_wgrad.hip) bit for bit: all four instantiations of bf3_gemm_tn_rs_kernel and the reduce.

Entry points: dr_h2_wgrad_emb and dr_bf3_wgrad_emb (x gathered from the tables), dr_h2_wgrad and dr_bf3_wgrad (x read from a
buffer).  What the shapes reach: R = 32 * 33 + 5 = 1024 + 37 = 1061 rows give split = 3 slices of 384, 384 and 293 rows -- a last
slice shorter than the others whose last k-tile holds 5 rows; nf = 3 fields + 13 dense features (F = 205) is one f-tile, whose blocks
store the column sums; nf = 5 + 13 (F = 333) adds a second f-tile that does not, with waves whose columns lie past F (and, in the
first tile, the dense features' wave); N = 256 fills the column tile, N = 40 leaves most of it to the padding; some ids are -1; dstb
is given and is NULL; the gathering entry points run as part 1 then part 2 and as one call; dstW sits in a wider buffer whose
leading dimension allows 16-byte accesses (N = 256: ld = 256; N = 40: ld = 44) or does not (N = 40: ld = 41 -- the reduce's scalar form).

Exact comparisons.  Table values and dense features are multiples of 1/8 with |k| <= 64, gradients integers in [-4, 4], dstW / dstb
start on the 1/8 grid and the scale is -1/8.  Seven significant bits fit the first bf16 term and the first fp16 term (the f16x2
scales are powers of two whatever the amax records hold), so every later term is zero, every product is exact and every fp32 sum is
exact in any order: the device output is compared bit for bit with a float64 reference.  The precondition -- (largest |partial sum|
any order can form) / quantum < 2^24 -- is asserted on the reference by every test."""
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

EXACT = 2.0 ** 24
SCALE = -0.125
SENTINEL = -12345.0
R_CASES = sorted({32 * 33 + 5, 1024 + 37})                  # (one number, written both ways)
FIELD_CASES = [3, 5]
ND = 13
N_CASES = [(256, 256), (40, 44), (40, 41)]                  # (N, leading dimension of dstW)
V = 50
BK = 32


def plan(R, F, N):
    """tn_rs_plan of bf3_wgrad.hip: (split, rows per slice, Fp, Np)"""
    tf, tn = (F + 255) // 256, (N + 255) // 256
    sp = max(1, min(256 // (tf * tn), (R + 16 * BK - 1) // (16 * BK)))
    per = ((R + sp - 1) // sp + BK - 1) // BK * BK
    return (R + per - 1) // per, per, tf * 256, tn * 256


def h2_scale(amax):
    """h2_scale_of (csrc/rs_args.h): the power of two an operand with this amax record is multiplied by"""
    e = (int(np.array([amax], np.float32).view(np.uint32)[0]) >> 23) & 0xff
    e = min(max(e, 20), 250)
    return 2.0 ** (140 - e)


@functools.lru_cache(maxsize=None)
def case(R, nf, N):
    rng = np.random.default_rng(100 * nf + N + R)
    F = 64 * nf + ND
    table = (rng.integers(-64, 65, size=(nf * V, 64)) / 8.0).astype(np.float32)
    dense = np.zeros((R, 32), np.float32)
    dense[:, :ND] = rng.integers(-64, 65, size=(R, ND)) / 8.0
    ids = rng.integers(0, V, size=(R, nf))
    ids[rng.random((R, nf)) < 0.1] = -1
    ids[R - 3:, 0] = -1                                      # ... also in the partial last k-tile
    row_base = (np.arange(nf) * V).astype(np.int64)
    rows = np.where(ids >= 0, ids + row_base[None, :], -1)
    x = np.where(rows[:, :, None] >= 0, table[np.maximum(rows, 0)], np.float32(0)).reshape(R, 64 * nf)
    x = np.concatenate([x, dense[:, :ND]], axis=1).astype(np.float32)
    dy = rng.integers(-4, 5, size=(R, N)).astype(np.float32)
    W0 = (rng.integers(-64, 65, size=(F, N)) / 8.0).astype(np.float32)
    b0 = (rng.integers(-64, 65, size=N) / 8.0).astype(np.float32)
    split, per, Fp, Np = plan(R, F, N)
    assert split >= 2 and R - (split - 1) * per < per and (R - (split - 1) * per) % BK != 0
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    part = np.stack([x64[s * per:(s + 1) * per].T @ dy64[s * per:(s + 1) * per] for s in range(split)])
    csum = np.stack([dy64[s * per:(s + 1) * per].sum(0) for s in range(split)])
    # headroom: x dy is a multiple of 1/8, scale * that of 1/64
    bound_w = float((np.abs(W0) + abs(SCALE) * (np.abs(x64).T @ np.abs(dy64))).max()) * 64
    bound_b = float((np.abs(b0) + abs(SCALE) * np.abs(dy64).sum(0)).max()) * 64
    return {"R": R, "nf": nf, "F": F, "N": N, "table": table, "dense": dense, "ids": ids, "ids_t": np.ascontiguousarray(ids.T).astype(np.int32),
            "row_base": row_base, "x": x, "dy": dy, "W0": W0, "b0": b0, "plan": (split, per, Fp, Np), "part": part, "csum": csum,
            "W": (W0 + SCALE * part.sum(0)).astype(np.float32), "b": (b0 + SCALE * csum.sum(0)).astype(np.float32),
            "headroom": max(bound_w, bound_b)}


def test_cases_are_exact_and_reach_the_edges():
    for R in R_CASES:
        for nf in FIELD_CASES:
            for N, _ in N_CASES:
                c = case(R, nf, N)
                assert 0 < c["headroom"] < EXACT
                split, per, Fp, Np = c["plan"]
                assert (split, per) == (3, 384) and Fp == (256 if nf == 3 else 512) and Np == 256
                assert (c["ids"] < 0).any() and (c["ids"][R - R % BK:] < 0).any()
                assert np.array_equal(c["W"].astype(np.float64), c["W0"] + SCALE * c["part"].sum(0))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_array_equal(_bits(got), _bits(np.asarray(want, np.float32).reshape(got.shape)), err_msg=what)


def _record(value):
    rec = torch.zeros(1, dtype=torch.int32, device="cuda")
    rec.view(torch.float32).fill_(float(value))
    return rec


def _dst(c, ld, with_b):
    """dstW as a view of an [F, ld] buffer whose padding holds a sentinel, dstb or None"""
    buf = torch.full((c["F"], ld), SENTINEL, dtype=torch.float32, device="cuda")
    buf[:, :c["N"]] = _dev(c["W0"])
    return buf, buf[:, :c["N"]], (_dev(c["b0"]).clone() if with_b else None)


def _check_dst(c, buf, b, what):
    N = c["N"]
    got = buf.cpu().numpy()
    _same(got[:, :N], c["W"], what + ": dstW")
    assert (got[:, N:] == SENTINEL).all(), what + ": the padding of dstW was written"
    if b is not None:
        _same(b, c["b"], what + ": dstb")


def _check_workspace(c, ws, factor, with_b, what):
    """the used region of the split-K workspace after part 1: partial[s][f < F][n < N] and, with dstb, colsum[s][n < N]"""
    split, per, Fp, Np = c["plan"]
    got = ws.cpu().numpy()
    part = got[:split * Fp * Np].reshape(split, Fp, Np)[:, :c["F"], :c["N"]]
    # (f16x2: the partials carry the two operands' scales, powers of two; the sums stay on the 1/8 grid times that factor)
    _same(part, c["part"] * factor, what + ": partial sums")
    if with_b:
        cs = got[split * Fp * Np:split * Fp * Np + split * Np].reshape(split, Np)[:, :c["N"]]
        _same(cs, c["csum"], what + ": column sums")


@gpu
@pytest.mark.parametrize("with_b", [True, False], ids=["dstb", "no_dstb"])
@pytest.mark.parametrize("N,ld", N_CASES)
@pytest.mark.parametrize("nf", FIELD_CASES)
@pytest.mark.parametrize("R", R_CASES)
@pytest.mark.parametrize("mode", ["h2", "bf3"])
def test_wgrad_emb_parts_and_whole(mode, R, nf, N, ld, with_b):
    """dr_h2_wgrad_emb / dr_bf3_wgrad_emb: part 1 leaves the exact partial sums (and column sums) in a NaN-poisoned
    workspace, part 2 applies them; one call (parts = 3) gives the same bits"""
    from deep_recommenders_amd import ops
    c = case(R, nf, N)
    assert c["headroom"] < EXACT
    ids_t, rb, table, dense, dy = _dev(c["ids_t"]), _dev(c["row_base"]), _dev(c["table"]), _dev(c["dense"]), _dev(c["dy"])
    what = "%s R=%d nf=%d N=%d ld=%d" % (mode, R, nf, N, ld)
    if mode == "h2":
        # records as the engine keeps them: the table's is a running maximum (here: above the values), the others exact
        t_amax, d_amax, y_amax = _record(11.0), ops.h2_amax(dense), ops.h2_amax(dy)
        factor = h2_scale(max(11.0, float(np.abs(c["dense"]).max()))) * h2_scale(float(np.abs(c["dy"]).max()))

        def run(dstW, dstb, ws, parts):
            ops.h2_wgrad_emb(ids_t, rb, table, t_amax, dense, d_amax, dy, y_amax, SCALE, dstW, dstb, workspace=ws, parts=parts)
    else:
        factor = 1.0

        def run(dstW, dstb, ws, parts):
            ops.bf3_wgrad_emb(ids_t, rb, table, dense, dy, SCALE, dstW, dstb, workspace=ws, parts=parts)
    ws = ops.bf3_wgrad_workspace(R, c["F"], N, "cuda").fill_(float("nan"))
    buf, dstW, dstb = _dst(c, ld, with_b)
    run(dstW, dstb, ws, 1)
    _check_workspace(c, ws, factor, with_b, what + " part 1")
    _same(buf[:, :N], c["W0"], what + " part 1: dstW must be untouched")
    run(dstW, dstb, ws, 2)
    _check_dst(c, buf, dstb, what + " parts 1, 2")
    ws.fill_(float("nan"))
    buf, dstW, dstb = _dst(c, ld, with_b)
    run(dstW, dstb, ws, 3)
    _check_dst(c, buf, dstb, what + " parts 3")


@gpu
@pytest.mark.parametrize("with_b", [True, False], ids=["dstb", "no_dstb"])
@pytest.mark.parametrize("N,ld", N_CASES)
@pytest.mark.parametrize("nf", FIELD_CASES)
@pytest.mark.parametrize("R", R_CASES)
@pytest.mark.parametrize("mode", ["h2", "bf3"])
def test_wgrad_from_buffer(mode, R, nf, N, ld, with_b):
    """dr_h2_wgrad / dr_bf3_wgrad on the same product with x = concat(embeddings, dense features) read from a buffer (leading
    dimension F + 3: rows that are not 16-byte aligned)"""
    from deep_recommenders_amd import ops
    c = case(R, nf, N)
    assert c["headroom"] < EXACT
    xbuf = torch.full((R, c["F"] + 3), float("nan"), dtype=torch.float32, device="cuda")
    xbuf[:, :c["F"]] = _dev(c["x"])
    x, dy = xbuf[:, :c["F"]], _dev(c["dy"])
    ws = ops.bf3_wgrad_workspace(R, c["F"], N, "cuda").fill_(float("nan"))
    buf, dstW, dstb = _dst(c, ld, with_b)
    what = "%s R=%d nf=%d N=%d ld=%d" % (mode, R, nf, N, ld)
    if mode == "h2":
        ops.h2_wgrad(x, _record(float(np.abs(c["x"]).max())), dy, ops.h2_amax(dy), SCALE, dstW, dstb, workspace=ws)
        factor = h2_scale(float(np.abs(c["x"]).max())) * h2_scale(float(np.abs(c["dy"]).max()))
    else:
        ops.bf3_wgrad(x, dy, SCALE, dstW, dstb, workspace=ws)
        factor = 1.0
    _check_workspace(c, ws, factor, with_b, what)
    _check_dst(c, buf, dstb, what)
