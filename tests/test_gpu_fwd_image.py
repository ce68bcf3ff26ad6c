"""The fused first layer (csrc/bf3_emb_linear.hip) bit for bit: its activation image in the LDS is written by the gather's LDS-DMA
(every lane chooses the row and the 16-byte chunk it fetches) and read twice, as the MFMA operand and position-wise for the concat
stores; a swizzle that the three places do not share shows up as permuted columns in `out`, `sum_x` or `concat`.

Entry points: dr_h2_emb_linear_fwd and dr_bf3_emb_linear_fwd (with lin_vals_t).  M = 256 + 19 (a full row tile and a ragged one: rows 16-31 of
a wave are the ones the swizzle's second term moves), F = 3 fields with and without 13 dense features (the k-tile that comes from
`dense_pad`), N = 256, `concat` stored and NULL, some ids -1.

Exact comparisons.  Table values, first-order weights, dense features, W and the biases are multiples of 1/8 with |k| <= 64: seven
significant bits fit the first bf16 and the first fp16 term (the f16x2 scales are powers of two), the later terms are zero, every
product and every fp32 sum is exact in any order, and so are the squares and the halving of fm_logit.  out, concat, sum_x, fm_logit
and the saved first-order values are compared bit for bit with a float64 reference; the precondition -- (largest |partial sum| any
order can form) / quantum < 2^24 -- is asserted on the reference."""
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

EXACT = 2.0 ** 24
SENTINEL = -12345.0
M, F, ND, N, V, D = 256 + 19, 3, 13, 256, 50, 64


def q8(rng, shape):
    return (rng.integers(-64, 65, size=shape) / 8.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(nd):
    rng = np.random.default_rng(7 + nd)
    K = F * D + nd
    table, lin_w, lin_b = q8(rng, (F * V, D)), q8(rng, F * V), np.float32(0.375)
    dense = np.zeros((M, 32), np.float32)
    dense[:, :nd] = q8(rng, (M, nd))
    ids = rng.integers(0, V, size=(M, F))
    ids[rng.random((M, F)) < 0.1] = -1
    ids[17, :] = -1                                          # an example without any id
    row_base = (np.arange(F) * V).astype(np.int64)
    rows = np.where(ids >= 0, ids + row_base[None, :], -1)
    x = np.where(rows[:, :, None] >= 0, table[np.maximum(rows, 0)], np.float32(0)).astype(np.float64)     # [M, F, D]
    W, b = q8(rng, (K, N)), q8(rng, N)
    xk = np.concatenate([x.reshape(M, F * D), dense[:, :nd].astype(np.float64)], axis=1)
    pre = xk @ W.astype(np.float64) + b.astype(np.float64)
    S, SS = x.sum(1), (x * x).sum(1)
    lin = np.where(rows >= 0, lin_w[np.maximum(rows, 0)].astype(np.float64), 0.0)
    logit = float(lin_b) + lin.sum(1) + 0.5 * ((S * S).sum(1) - SS.sum(1))
    # quanta: x W 1/64; S 1/8; S^2, x^2 1/64, halved 1/128; the first-order sum 1/8
    headroom = max(float((np.abs(xk) @ np.abs(W).astype(np.float64) + np.abs(b)).max()) * 64, float(np.abs(x).sum(1).max()) * 8,
                   float((S * S).sum(1).max()) * 128, float(SS.sum(1).max()) * 128,
                   float((abs(float(lin_b)) + np.abs(lin).sum(1) + 0.5 * ((S * S).sum(1) + SS.sum(1))).max()) * 128)
    return {"K": K, "nd": nd, "table": table, "lin_w": lin_w, "lin_b": lin_b, "dense": dense, "ids": ids, "row_base": row_base, "W": W, "b": b,
            "concat": x.reshape(M, F * D).astype(np.float32), "sum_x": S.astype(np.float32), "logit": logit.astype(np.float32),
            "out": np.maximum(pre, 0.0).astype(np.float32), "lin_vals": lin.T.astype(np.float32), "present": (rows >= 0).T,
            "headroom": headroom}


def test_cases_are_exact():
    for nd in (0, ND):
        c = case(nd)
        assert 0 < c["headroom"] < EXACT
        assert (c["ids"] < 0).any() and (c["ids"] >= 0).all(1).any() and (c["out"] > 0).any() and (c["out"] == 0).any()
        assert np.array_equal(c["logit"].astype(np.float64) * 128, np.rint(c["logit"].astype(np.float64) * 128))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what):
    got = np.ascontiguousarray(got.cpu().numpy(), np.float32)
    np.testing.assert_array_equal(got.view(np.int32), np.ascontiguousarray(want, np.float32).reshape(got.shape).view(np.int32), err_msg=what)


@gpu
@pytest.mark.parametrize("store_concat", [True, False], ids=["concat", "no_concat"])
@pytest.mark.parametrize("nd", [0, ND], ids=["no_dense", "dense13"])
@pytest.mark.parametrize("mode", ["h2", "bf3"])
def test_fused_first_layer_bit_for_bit(mode, nd, store_concat):
    from deep_recommenders_amd import ops
    c = case(nd)
    assert c["headroom"] < EXACT
    K = c["K"]
    ld = (K + 3) // 4 * 4 + 4
    concat = torch.full((M, ld), SENTINEL, dtype=torch.float32, device="cuda") if store_concat else None
    nan = float("nan")
    sum_x, fm = torch.full((M, D), nan, device="cuda"), torch.full((M,), nan, device="cuda")
    out, lv = torch.full((M, N), nan, device="cuda"), torch.full((F, M), nan, device="cuda")
    ids, rb, table, lin_w = _dev(c["ids"]), _dev(c["row_base"]), _dev(c["table"]), _dev(c["lin_w"])
    lin_b, bias, W = _dev(np.array([c["lin_b"]], np.float32)), _dev(c["b"]), _dev(c["W"])
    dpad = _dev(c["dense"]) if nd else None
    if mode == "h2":
        wp = ops.H2WeightPlanes(W)
        ops.h2_emb_linear_fwd(ids, rb, V, table, ops.h2_amax(table), lin_w, lin_b, dpad, ops.h2_amax(dpad) if nd else None, concat, K, wp.wt,
                              bias, 1, sum_x, fm, out, lin_vals_t=lv)
    else:
        wp = ops.WeightPlanes(W)
        ops.bf3_emb_linear_fwd(ids, rb, V, table, lin_w, lin_b, dpad, concat, K, wp.wt, bias, 1, sum_x, fm, out, lin_vals_t=lv)
    what = "%s nd=%d %s" % (mode, nd, "concat" if store_concat else "no concat")
    _same(out, c["out"], what + ": out")
    _same(sum_x, c["sum_x"], what + ": sum_x")
    _same(fm, c["logit"], what + ": fm_logit")
    got_lv = lv.cpu().numpy()
    np.testing.assert_array_equal(got_lv[c["present"]].view(np.int32), c["lin_vals"][c["present"]].view(np.int32),
                                  err_msg=what + ": saved first-order values")
    if store_concat:
        got = concat.cpu().numpy()
        _same(concat[:, :F * D], c["concat"], what + ": concat")
        assert (got[:, F * D:] == SENTINEL).all(), what + ": a column of concat past the embeddings was written"
