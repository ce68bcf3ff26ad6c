"""The kernels of csrc/attention.hip through `ops`, against the float64 restatement of tests/transformer_ref.py.

Tolerances (the form of tests/test_gpu_small_kernels.py): a derived fp32 running-error bound -- gamma(chain length) times the
formula evaluated on absolute values, with the softmax's sensitivity to the score error (|dp| <= 2 p max|ds|, ds <= gamma(dh)
|q|.|k| / sqrt(dh)) added -- plus four times the error the SAME formula shows in fp32 on the CPU (torch) against float64 on the same
inputs.  The yardstick is the fp32 reference arithmetic, never the kernel; the factor four covers another summation order.  Every
element of every output is compared."""
import math

import numpy as np
import pytest
import torch

import transformer_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# fp32 underflow: a term below 2^-126 loses its bits (exp(s - max) for s - max < -87), in the kernel and in the fp32 yardstick alike;
# a sum of up to 2^20 such terms stays below 2^-100.  Magnitudes are floored there, so that such elements are compared absolutely.
FLOOR = 2.0 ** -100


def gamma(d):
    return d * U / (1.0 - d * U)


def _ops():
    from deep_recommenders_amd import ops
    return ops


def _dev3(x, extra=0):
    """[B, L, W] fp32 on the device as a view of a [B, L, W + extra] buffer (leading dimension larger than the width)"""
    B, L, W = x.shape
    buf = torch.full((B, L, W + extra), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :, :W] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return buf[:, :, :W]


def _pads(B, Lk):
    """padded-key counts per batch row (pre-padding, as the example's sequences): sequence length 0, partial, full"""
    part = max(1, Lk // 3) if Lk > 1 else 0
    return {1: [part], 2: [part, Lk], 3: [Lk, part, 0]}[B]


def _mask(B, Lk):
    m = np.zeros((B, Lk), dtype=bool)
    for b, n in enumerate(_pads(B, Lk)):
        m[b, :n] = True
    return m


_dhp = R.dhp


def _oracle(q, k, v, d_out, H, mask, future, keep, rate, dtype):
    tq, tk, tv = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (q, k, v))
    out = R.attention(tq, tk, tv, H, mask, future, keep, rate, dtype)
    out.backward(torch.from_numpy(d_out).to(dtype))
    return [t.detach().to(torch.float64).numpy() for t in (out, tq.grad, tk.grad, tv.grad)]


_magnitudes = R.attention_magnitudes


def _run(q, k, v, d_out, H, mask, future, rate, seed, extra):
    ops = _ops()
    dq_, dk_, dv_ = _dev3(q, extra), _dev3(k, extra), _dev3(v, extra)
    dm = torch.from_numpy(mask).cuda() if mask is not None else None
    out, stats = ops.attn_fwd(dq_, dk_, dv_, H, dm, future, rate, seed)
    g = ops.attn_bwd(dq_, dk_, dv_, H, _dev3(d_out, extra), stats, dm, future, rate, seed)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (out,) + tuple(g)]


def _check(name, q, k, v, d_out, H, mask, future, rate=0.0, seed=0, extra=0):
    B, Lq, W = q.shape
    Lk = k.shape[1]
    dh = W // H
    keep = R.keep_mask(seed, rate, (B, H, Lq, Lk)) if rate > 0 else None
    got = _run(q, k, v, d_out, H, mask, future, rate, seed, extra)
    want = _oracle(q, k, v, d_out, H, mask, future, keep, rate, torch.float64)
    f32 = _oracle(q, k, v, d_out, H, mask, future, keep, rate, torch.float32)
    mags, es = _magnitudes(q, k, v, d_out, H, mask, future, keep, rate)
    # chain lengths: out = one softmax row (Lk) and one dot (dh); the gradients add the dP dot, delta and the sum over the other axis
    chains = [Lk + _dhp(dh) + 16] + [Lq + Lk + 2 * _dhp(dh) + 32] * 3
    sens = [2 * es, 4 * es, 4 * es, 2 * es]
    for what, g, w, f, mag, n, se in zip(("out", "dq", "dk", "dv"), got, want, f32, mags, chains, sens):
        assert g.shape == w.shape and np.isfinite(g).all(), (name, what)
        yard = float((np.abs(f - w) / (mag + FLOOR)).max())
        rel = gamma(n) + se + 4 * yard
        err = np.abs(g.astype(np.float64) - w)
        worst = float((err / (rel * (mag + FLOOR))).max())
        print("%s %s: max err %.3g, yardstick %.3g, derived %.3g, err / tol %.3g" % (name, what, err.max(), yard, gamma(n) + se, worst))
        assert (err <= rel * (mag + FLOOR)).all(), "%s %s: err / tol %g" % (name, what, worst)
    return got, want


def _inputs(rng, B, H, Lq, Lk, dh, scale=1.0):
    W = H * dh
    return [(rng.standard_normal(s) * c).astype(np.float32) for s, c in
            (((B, Lq, W), scale), ((B, Lk, W), scale), ((B, Lk, W), 1.0), ((B, Lq, W), 1.0))]


# every value of every axis occurs; every dh meets a ragged and a long L          B  H   Lq    Lk   dh  mask   future extra
GRID = [(3, 1, 1, 1, 1, True, False, 0), (3, 2, 7, 7, 4, True, True, 4), (3, 8, 129, 129, 20, True, False, 3),
        (2, 2, 256, 256, 64, True, True, 0), (3, 2, 100, 333, 128, True, False, 8), (2, 1, 1000, 1000, 1, False, False, 0),
        (1, 2, 1000, 1000, 64, True, True, 0), (3, 8, 7, 7, 128, False, True, 0), (2, 2, 1000, 1000, 4, True, False, 0),
        (2, 1, 100, 333, 64, False, False, 4), (1, 2, 1000, 1000, 20, True, True, 0), (2, 2, 129, 129, 1, True, True, 1),
        (1, 1, 1000, 1000, 128, True, False, 0), (3, 2, 100, 333, 4, True, False, 0), (2, 8, 256, 256, 64, False, False, 0)]


@pytest.mark.parametrize("B,H,Lq,Lk,dh,masked,future,extra", GRID)
def test_attention_against_float64(B, H, Lq, Lk, dh, masked, future, extra):
    rng = np.random.default_rng(B * 1000003 + H * 10007 + Lq * 101 + Lk * 7 + dh)
    q, k, v, d_out = _inputs(rng, B, H, Lq, Lk, dh)
    mask = _mask(B, Lk) if masked else None
    got, _ = _check("B%d H%d L%dx%d dh%d" % (B, H, Lq, Lk, dh), q, k, v, d_out, H, mask, future, extra=extra)
    if masked:
        # |s| < 128 here (asserted), so a padded key's probability is exactly 0 next to any unpadded visible key: in the batch rows
        # where EVERY query sees an unpadded key the padded keys' dK and dV rows are exactly zero, not merely small
        s = R.attention_scores(torch.from_numpy(q).double(), torch.from_numpy(k).double(), H).abs().max()
        assert float(s) < 128
        checked = 0
        for b in range(B):
            unpadded = ~mask[b]
            first = int(np.argmax(unpadded)) if unpadded.any() else None
            every_row_sees_one = unpadded.any() and (not future or first == 0)
            if every_row_sees_one and mask[b].any():
                assert (got[2][b, mask[b]] == 0).all() and (got[3][b, mask[b]] == 0).all(), b
                checked += 1
        assert checked > 0 or future or Lk == 1


@pytest.mark.parametrize("future", [False, True])
def test_masking_semantics(future):
    """section 3 items 2-4 of the design: additive key-side mask as an fp32 add (uniform rows, exact zeros, non-saturating scores),
    the replacing future mask on pre-padded rows, the mask shared by the heads and not applied to queries.  Inputs are small
    integers / 2 with dh = 4, so that every score is exact in fp32 and float64 alike and the fp32 rounding of s + M is the same
    in the kernel and in the restatement; `scale` 16 pushes |s| beyond 256."""
    ops = _ops()
    B, H, L, dh = 3, 2, 37, 4
    for scale in (1.0, 16.0):
        rng = np.random.default_rng(int(scale) + 10 * future)
        q = (rng.integers(-4, 5, size=(B, L, H * dh)) * 0.5 * scale).astype(np.float32)
        k = (rng.integers(-4, 5, size=(B, L, H * dh)) * 0.5 * scale).astype(np.float32)
        v = (rng.integers(-8, 9, size=(B, L, H * dh)) * 0.25).astype(np.float32)
        d_out = (rng.integers(-8, 9, size=(B, L, H * dh)) * 0.125).astype(np.float32)
        mask = _mask(B, L)                              # row 0: every key padded; row 1: the first 12 padded; row 2: none
        smax = float(R.attention_scores(torch.from_numpy(q).double(), torch.from_numpy(k).double(), H).abs().max())
        assert smax < 128 if scale == 1.0 else smax > 256
        got, want = _check("semantics future=%d scale=%g" % (future, scale), q, k, v, d_out, H, mask, future)
        out = got[0]
        if scale == 1.0:
            mean_v = v[0].astype(np.float64).mean(0)
            # every key padded: the uniform distribution over all L keys -- the future ones included -- not NaN, not zeros
            assert np.abs(out[0] - mean_v[None]).max() <= 64 * U * np.abs(v[0]).max()
            if future:
                # pre-padded causal rows: queries 0..11 of row 1 see only padded keys and attend uniformly over ALL keys
                mean_v1 = v[1].astype(np.float64).mean(0)
                assert np.abs(out[1, :12] - mean_v1[None]).max() <= 64 * U * np.abs(v[1]).max()
                # query 12 sees exactly one unpadded key: itself
                assert np.abs(out[1, 12] - v[1, 12]).max() <= 4 * U * np.abs(v[1, 12]).max()
            else:
                assert (got[2][1, :12] == 0).all() and (got[3][1, :12] == 0).all()
            # queries at padded positions are not masked: ordinary outputs
            assert np.abs(out[1, :12]).max() > 0
        # one [B, Lk] mask serves every head: per-head calls on the column blocks give the same bits
        dm = torch.from_numpy(mask).cuda()
        for h in range(H):
            sl = slice(h * dh, (h + 1) * dh)
            one, _ = ops.attn_fwd(_dev3(q[:, :, sl]), _dev3(k[:, :, sl]), _dev3(v[:, :, sl]), 1, dm, future)
            assert np.array_equal(one.cpu().numpy(), out[:, :, sl])


@pytest.mark.parametrize("B,H,Lq,Lk,dh,future", [(2, 2, 100, 333, 20, False), (2, 2, 129, 129, 64, True)])
def test_attention_dropout(B, H, Lq, Lk, dh, future):
    ops = _ops()
    rng = np.random.default_rng(Lq + dh)
    q, k, v, d_out = _inputs(rng, B, H, Lq, Lk, dh)
    mask = _mask(B, Lk)
    base = _run(q, k, v, d_out, H, mask, future, 0.0, 0, 0)
    same = _run(q, k, v, d_out, H, mask, future, 0.0, 987654321, 0)
    for a, b in zip(base, same):                         # rate 0 == no dropout, bit for bit, whatever the seed
        assert np.array_equal(a, b)
    for rate in (0.1, 0.5):
        seed = 1234567 + int(rate * 10)
        got, _ = _check("dropout %.1f L%dx%d dh%d" % (rate, Lq, Lk, dh), q, k, v, d_out, H, mask, future, rate, seed)
        again = _run(q, k, v, d_out, H, mask, future, rate, seed, 0)
        other = _run(q, k, v, d_out, H, mask, future, rate, seed + 1, 0)
        for a, b, c in zip(got, again, other):
            assert np.array_equal(a, b) and not np.array_equal(a, c)
        keep = R.keep_mask(seed, rate, (B, H, Lq, Lk))
        n = keep.size
        frac = keep.mean()
        sigma = math.sqrt(rate * (1 - rate) / n)
        print("keep fraction %.6f, expected %.6f, 5 sigma %.2g" % (frac, 1 - rate, 5 * sigma))
        assert abs(frac - (1 - rate)) <= 5 * sigma
        assert not np.array_equal(keep, R.keep_mask(seed + 1, rate, (B, H, Lq, Lk)))


def test_attention_is_bit_reproducible():
    rng = np.random.default_rng(5)
    q, k, v, d_out = _inputs(rng, 2, 8, 200, 300, 64)
    mask = _mask(2, 300)
    a = _run(q, k, v, d_out, 8, mask, False, 0.1, 42, 0)
    b = _run(q, k, v, d_out, 8, mask, False, 0.1, 42, 0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_attention_refused_arguments():
    from deep_recommenders_amd import _lib
    L = _lib.lib()
    t = torch.zeros(4 * 8 * 256, dtype=torch.float32, device="cuda")
    st = torch.zeros(4096, dtype=torch.float32, device="cuda")

    def fwd(B, H, Lq, Lk, dh, future, rate, ld=None):
        ld = H * dh if ld is None else ld
        return L.dr_attn_fwd(_lib.ptr(t), ld, _lib.ptr(t), ld, _lib.ptr(t), ld, None, B, H, Lq, Lk, dh, future, rate, 0, _lib.ptr(t), ld,
                             _lib.ptr(st), _lib.stream_ptr())

    def bwd(B, H, Lq, Lk, dh, future, rate):
        ld = H * dh
        a = (_lib.ptr(t), ld)
        return L.dr_attn_bwd(*a, *a, *a, None, *a, _lib.ptr(st), B, H, Lq, Lk, dh, future, rate, 0, *a, *a, *a, _lib.ptr(st),
                             _lib.stream_ptr())
    assert fwd(1, 1, 4, 4, 8, 0, 0.0) == _lib.DR_OK
    for f in (fwd, bwd):
        assert f(1, 1, 4, 4, 129, 0, 0.0) == _lib.DR_ESHAPE              # dh > 128
        assert f(1, 1, 4, 5, 8, 1, 0.0) == _lib.DR_ESHAPE                # future needs Lq == Lk
        assert f(1, 1, 4, 4, 8, 0, 1.0) == _lib.DR_EINVAL                # rate outside [0, 1)
        assert f(1, 1, 4, 4, 8, 0, -0.1) == _lib.DR_EINVAL
        assert f(1, 1, 4, 4, 8, 0, float("nan")) == _lib.DR_EINVAL
        assert f(1, 1, 0, 4, 8, 0, 0.0) == _lib.DR_EINVAL
    assert fwd(1, 2, 4, 4, 8, 0, 0.0, ld=15) == _lib.DR_EINVAL          # a pitch below H * dh
    torch.cuda.synchronize()
    ops = _ops()
    x = torch.zeros((1, 4, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="DR_EINVAL"):
        ops.attn_fwd(x, x, x, 1, rate=1.5)
    with pytest.raises(RuntimeError, match="DR_ESHAPE"):
        ops.attn_fwd(x, x[:, :3], x[:, :3], 1, future=True)


# ---- residual add + LayerNormalization --------------------------------------------------------------------------------------------
def _ln_inputs(rng, M, D, with_b):
    a = rng.standard_normal((M, D)).astype(np.float32) * 2 + 0.5
    b = rng.standard_normal((M, D)).astype(np.float32) if with_b else None
    a[3 % M, :] = 2.5                                   # a constant row: variance 0, the epsilon path (1.5 * D is exact in fp32)
    if with_b:
        b[3 % M, :] = -1.0
    gamma_ = (rng.standard_normal(D) + 1).astype(np.float32)
    beta = rng.standard_normal(D).astype(np.float32)
    dy = rng.standard_normal((M, D)).astype(np.float32)
    return a, b, gamma_, beta, dy


def _ln_oracle(a, b, g, be, dy, dtype):
    ta = torch.from_numpy(a).to(dtype).requires_grad_(True)
    tb = torch.from_numpy(b).to(dtype).requires_grad_(True) if b is not None else None
    tg, tbe = (torch.from_numpy(x).to(dtype).requires_grad_(True) for x in (g, be))
    y = R.layer_norm(ta, tb, tg, tbe, 1e-8, dtype)
    y.backward(torch.from_numpy(dy).to(dtype))
    if tb is not None:
        assert torch.equal(ta.grad, tb.grad)
    return [t.detach().double().numpy() for t in (y, ta.grad, tg.grad, tbe.grad)]


@pytest.mark.parametrize("M,D,with_b", [(300, 8, True), (257, 50, True), (130, 512, True), (5, 50, False), (1, 8, True)])
def test_add_layernorm(M, D, with_b):
    ops = _ops()
    rng = np.random.default_rng(M + D)
    a, b, g, be, dy = _ln_inputs(rng, M, D, with_b)
    dev = lambda x: torch.from_numpy(x).cuda() if x is not None else None       # noqa: E731
    da, db, dg, dbe, ddy = dev(a), dev(b), dev(g), dev(be), dev(dy)
    y, stats = ops.add_layernorm_fwd(da, db, dg, dbe, 1e-8)
    d_s, d_g, d_b = ops.add_layernorm_bwd(da, db, dg, stats, ddy)
    y2, stats2 = ops.add_layernorm_fwd(da, db, dg, dbe, 1e-8)
    again = ops.add_layernorm_bwd(da, db, dg, stats2, ddy)
    assert torch.equal(y, y2) and all(torch.equal(p, r) for p, r in zip((d_s, d_g, d_b), again))    # bit-reproducible
    got = [t.cpu().numpy().astype(np.float64) for t in (y, d_s, d_g, d_b)]
    want = _ln_oracle(a, b, g, be, dy, torch.float64)
    f32 = _ln_oracle(a, b, g, be, dy, torch.float32)
    # magnitudes: the formulas on absolute values, with the conditioning of xhat = (s - mean) * rstd made explicit: its absolute
    # error is gamma * A, A = (|s| + |mean|) rstd + |xhat| mean_c(|s - mean| (|s| + |mean|)) / (var + eps)
    s = a.astype(np.float64) + (b.astype(np.float64) if b is not None else 0.0)
    mean = s.mean(1, keepdims=True)
    d = s - mean
    var = (d * d).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + 1e-8)
    xh = d * rstd
    spread = np.abs(s) + np.abs(mean)
    A = spread * rstd + np.abs(xh) * (np.abs(d) * spread).mean(1, keepdims=True) / (var + 1e-8)
    Ar = A.max(1, keepdims=True)
    g64, dy64 = g.astype(np.float64)[None], dy.astype(np.float64)
    gg = np.abs(dy64 * g64)
    m1, m2 = gg.mean(1, keepdims=True), (gg * np.abs(xh)).mean(1, keepdims=True)
    mags = [np.abs(g64) * (np.abs(xh) + A) + np.abs(be)[None],
            rstd * (gg + m1 + np.abs(xh) * m2 + Ar * (m2 + m1 + np.abs(xh) * m1)) + Ar * np.abs(want[1]),
            (np.abs(dy64) * (np.abs(xh) + A)).sum(0), np.abs(dy64).sum(0)]
    chains = [D + 32, 2 * D + 48, M + D + 32, M + 8]
    for what, gt, w, f, mag, n in zip(("y", "d_s", "d_gamma", "d_beta"), got, want, f32, mags, chains):
        yard = float((np.abs(f - w) / (mag + FLOOR)).max())
        rel = gamma(n) + 4 * yard
        err = np.abs(gt - w)
        print("add_layernorm M=%d D=%d %s: max err %.3g yardstick %.3g err / tol %.3g" % (M, D, what, err.max(), yard,
                                                                                             (err / (rel * (mag + FLOOR))).max()))
        assert np.isfinite(gt).all() and (err <= rel * (mag + FLOOR)).all(), what
    assert np.array_equal(got[0][3 % M], be.astype(np.float64))           # the constant row: s - mean == 0 exactly -> beta


# ---- token embedding ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,D,B,L,rate,ids_kind", [(11, 8, 4, 7, 0.0, "dup"), (100, 50, 3, 33, 0.1, "dup"), (5000, 512, 2, 128, 0.5, "rand"),
                                                   (7, 50, 5, 40, 0.1, "equal"), (16, 8, 128, 128, 0.1, "padded")])
def test_token_embedding(V, D, B, L, rate, ids_kind):
    ops = _ops()
    rng = np.random.default_rng(V + D + L)
    if ids_kind == "equal":
        ids = np.full((B, L), 3, dtype=np.int64)                            # all-equal ids: one owner sums every position
    elif ids_kind == "padded":
        ids = rng.integers(1, V, size=(B, L))
        for r in range(B):
            ids[r, :rng.integers(0, L + 1)] = 0                             # pre-padding: id 0 is the heavy hitter
    else:
        ids = rng.integers(0, V if ids_kind == "rand" else min(V, 5), size=(B, L))
    ids = ids.astype(np.int64)
    table = rng.standard_normal((V, D)).astype(np.float32)
    pos = R.position_encoding(L, D)
    d_out = rng.standard_normal((B, L, D)).astype(np.float32)
    seed = 77
    keep = R.keep_mask(seed, rate, (B, L, D))
    dids, dtab, dpos, dd = (torch.from_numpy(x).cuda() for x in (ids, table, pos, d_out))
    out = ops.token_embedding_fwd(dids, dtab, dpos, rate, seed)
    d_table = torch.zeros((V, D), dtype=torch.float32, device="cuda")
    ops.token_embedding_bwd(dids, dd, d_table, rate, seed)
    again = torch.zeros((V, D), dtype=torch.float32, device="cuda")
    ops.token_embedding_bwd(dids, dd, again, rate, seed)
    assert torch.equal(d_table, again) and torch.equal(out, ops.token_embedding_fwd(dids, dtab, dpos, rate, seed))
    ops.token_embedding_bwd(dids, dd, again, rate, seed)                    # accumulates: a second call doubles (exactly)
    assert torch.equal(again, d_table * 2)

    def oracle(dtype):
        t = torch.from_numpy(table).to(dtype).requires_grad_(True)
        o = R.token_embedding(t, ids, pos, keep, rate, dtype)
        o.backward(torch.from_numpy(d_out).to(dtype))
        return o.detach().double().numpy(), t.grad.double().numpy()
    want, f32 = oracle(torch.float64), oracle(torch.float32)
    inv = 1.0 / (1.0 - float(np.float32(rate)))
    kept = np.abs(d_out.astype(np.float64)) * keep * inv
    mag_dt = np.zeros((V, D))
    np.add.at(mag_dt, ids.reshape(-1), kept.reshape(-1, D))
    mags = [(np.abs(table.astype(np.float64))[ids] * math.sqrt(D) + np.abs(pos)[None]) * inv, mag_dt * math.sqrt(D)]
    counts = np.bincount(ids.reshape(-1), minlength=V).max()
    for what, gt, w, f, mag, n in zip(("out", "d_table"), (out, d_table), want, f32, mags, (6, int(counts) + 8)):
        gt = gt.cpu().numpy().astype(np.float64)
        yard = float((np.abs(f - w) / (mag + FLOOR)).max())
        rel = gamma(n) + 4 * yard
        err = np.abs(gt - w)
        print("token_embedding %s %s: max err %.3g yardstick %.3g err / tol %.3g" % (ids_kind, what, err.max(), yard,
                                                                                    (err / (rel * (mag + FLOOR))).max()))
        assert (err <= rel * (mag + FLOOR)).all(), what
    assert (out.cpu().numpy()[~keep] == 0).all()
    untouched = np.setdiff1d(np.arange(V), ids.reshape(-1))
    assert (d_table.cpu().numpy()[untouched] == 0).all()
