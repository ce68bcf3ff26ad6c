"""GPU tests of AFM on the fused attention-pooling kernels (csrc/afm_pool.hip): the entry points against the float64 restatement
(tests/afm_ref.py), bit-reproducibility, independence of an example from its batch, strides and padding, the argument errors, memory
growth, the autograd glue, AttentionalPooling and AFM end to end.  The inputs are afm_ref.CASES; tests/test_afm_cpu.py asserts on the
restatement alone that their relu mask z > 0 cannot be changed by fp32 rounding (grid cases: z is exact; random-normal cases:
min |z| >= 4 eps_z).

Forward bound.  u = 2^-24.  z is a sum of D products of a rounded product plus the bias: |dz| <= eps_z = (D + 2) u (|p| |W| + |b|).
s = sum_a max(z, 0) h adds its own A products and carries dz through the 1-Lipschitz relu:
    |ds_q| <= eps_s = (A + 2) u sum_a max(z, 0) |h| + sum_a eps_z |h|.
exp(s_q - lse) changes by at most the factor exp(2 max_q eps_s) when every s moves by at most max eps_s (numerator and denominator
each by one), and the P-term sum, the exp, the log and the division add (P + 8) u:  the weights are off by at most the relative
    w = 2 max eps_s + (P + 8) u,
out = sum_q a_q p_q adds P products and their sum:  |d out| <= (2 max eps_s + (2 P + 10) u) sum_q a_q |p_q|,
|d lse| <= max eps_s + (P + 8) u (1 + |lse|), and a row of attn sums to 1 within (P + 8) u.
The fp32 run of the restatement stays below 0.08 of the out bound at every shape here (0.076 at 8200 x 3 x 4 x 2); on an MI355X the
kernel read at most 0.072 (out), 0.131 (attn) and 0.084 (lse) of its bounds.

Backward limit.  No absolute number: for each of d_emb, dW, db, dh the error is normalised by the largest absolute value of the float64
gradient, r32 is the same figure for the float32 run of the restatement against the float64 run (reference only), and the limit is
16 max(r32, 8 u).  The kernel sums in another order than torch (MFMA chains of 4, per-block partials) and uses the device's exp; a
deliberately different fp32 association (reversed pairs, k-chunks of 4, sequential sums, exp2) read at most 6.7 max(r32, 8 u) over 21
cases, while a dropped pair, a wrong mask or a bf16 product is off by 1e-3 or more.  On an MI355X the kernel read at most
1.65 max(r32, 8 u) (dh at 4 x 3 x 8 x 4)."""
import numpy as np
import pytest
import torch

import afm_ref as R

pytestmark = pytest.mark.gpu

DD = torch.float64
U = 2.0 ** -24
ALL = list(range(len(R.CASES)))
IDS = ["%dx%dx%dx%d" % R.CASES[i][0] for i in ALL]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cuda(a):
    return a.to(torch.float32).cuda()


def _params(index):
    c = R.case(index)
    return _cuda(c["W"]), _cuda(c["b"]), _cuda(c["h"])


def _fwd(index, lo=None, hi=None, want_attention=True):
    from deep_recommenders_amd import ops
    c = R.case(index)
    return ops.afm_pool_fwd(_cuda(c["e"])[lo:hi], *_params(index), c["shape"][1], want_attention)


def _bwd(index, lo=None, hi=None):
    from deep_recommenders_amd import ops
    c = R.case(index)
    out, lse, _ = _fwd(index, lo, hi, False)
    return ops.afm_pool_bwd(_cuda(c["e"])[lo:hi], *_params(index), c["shape"][1], out, lse, _cuda(c["g"])[lo:hi])


def _within(got, want, bound, what):
    err = (got.detach().double().cpu() - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print("%s: max |err| / bound = %.3f" % (what, ratio))
    assert (err <= bound).all(), "%s: max |err| / bound = %.3f" % (what, ratio)


@pytest.mark.parametrize("index", ALL, ids=IDS)
def test_forward(index):
    c = R.case(index)
    B, F, D, A = c["shape"]
    P = F * (F - 1) // 2
    f = c["fwd"]
    out, lse, attn = _fwd(index)
    assert out.shape == (B, D) and lse.shape == (B,) and attn.shape == (B, P)
    eps_z = R.eps_z(c["e"], c["W"], c["b"])
    eps_s = (A + 2) * U * (torch.relu(f["z"]) @ c["h"].abs()) + eps_z @ c["h"].abs()
    es = eps_s.max(dim=1).values                                                               # [B]
    weight = 2 * es + (P + 8) * U
    out_bound = (2 * es + (2 * P + 10) * U)[:, None] * (f["attn"][:, :, None] * f["p"].abs()).sum(1)
    _within(out, f["out"], out_bound, "out %s" % (c["shape"],))
    _within(attn, f["attn"], weight[:, None] * f["attn"], "attn %s" % (c["shape"],))
    _within(lse, f["lse"], es + (P + 8) * U * (1 + f["lse"].abs()), "lse %s" % (c["shape"],))
    assert ((attn.double().sum(1) - 1).abs().cpu() <= (P + 8) * U).all()
    if P == 1:
        e32 = _cuda(c["e"])
        assert _bits_equal(out, e32[:, 0] * e32[:, 1]) and (attn == 1).all()
    again = _fwd(index)                                                                        # run to run
    assert all(_bits_equal(x, y) for x, y in zip((out, lse, attn), again))
    assert _bits_equal(_fwd(index, want_attention=False)[0], out)                              # attn is an output only


@pytest.mark.parametrize("index", ALL, ids=IDS)
def test_backward(index):
    c = R.case(index)
    B, F, D, A = c["shape"]
    got = _bwd(index)
    assert got[0].shape == (B, F * D) and got[1].shape == (D, A) and got[2].shape == (A,) and got[3].shape == (A,)
    with torch.no_grad():
        ref32 = R.backward(*[c[k].float() for k in ("e", "W", "b", "h", "g")])
    for name, x, w32, want in zip(("d_emb", "dW", "db", "dh"), got, ref32, c["grads"]):
        x = x.double().cpu().reshape(want.shape)
        scale = want.abs().max().item()
        if scale == 0.0:                                                                       # P = 1: ds = a (<g, p> - <g, out>) = 0
            assert F == 2 and name != "d_emb" and (x == 0).all(), name
            continue
        r32 = (w32.double() - want).abs().max().item() / scale
        err = (x - want).abs().max().item() / scale
        limit = 16 * max(r32, 8 * U)
        print("%s %s: error %.3g = %.2f max(r32, 8u), %.3f of the limit" % (name, c["shape"], err, err / max(r32, 8 * U), err / limit))
        assert err <= limit, (name, err, limit)
    if F == 2:
        assert all((x == 0).all() for x in got[1:])
    again = _bwd(index)                                                                        # run to run
    assert all(_bits_equal(x, y) for x, y in zip(got, again))


@pytest.mark.parametrize("index", ALL, ids=IDS)
def test_an_example_does_not_depend_on_its_batch(index):
    full, alone = _fwd(index), _fwd(index, 1, 2)
    assert alone[0].shape[0] == 1
    for x, y in zip(full, alone):
        assert _bits_equal(x[1:2], y)
    assert _bits_equal(_bwd(index)[0][1:2], _bwd(index, 1, 2)[0])


@pytest.mark.parametrize("index", ALL, ids=IDS)
def test_strides_and_padding(index):
    from deep_recommenders_amd import _lib, ops
    c = R.case(index)
    B, F, D, A = c["shape"]
    P = F * (F - 1) // 2
    W, b, h = _params(index)
    nan = float("nan")
    ld_emb = F * D + 12
    emb = torch.full((B, ld_emb), nan, device="cuda")[:, :F * D]
    emb.copy_(_cuda(c["e"]).reshape(B, F * D))
    buf = torch.full((B + 1, D + 8), nan, device="cuda")                                       # the last row is a guard
    want = _fwd(index)
    out, lse, attn = ops.afm_pool_fwd(emb, W, b, h, F, True, out=buf[:B, :D])
    assert out.data_ptr() == buf.data_ptr() and all(_bits_equal(x, y) for x, y in zip((out, lse, attn), want))
    assert torch.isnan(buf[:B, D:]).all() and torch.isnan(buf[B]).all()
    abuf = torch.full((B + 1, P + 3), nan, device="cuda")                                      # attn at a pitch, through the entry point
    lse2 = torch.empty(B, device="cuda")
    st = _lib.lib().dr_afm_pool_fwd(emb.data_ptr(), ld_emb, W.data_ptr(), b.data_ptr(), h.data_ptr(), B, F, D, A, buf.data_ptr(), D + 8,
                                    lse2.data_ptr(), abuf.data_ptr(), P + 3, _lib.stream_ptr())
    assert st == _lib.DR_OK and _bits_equal(abuf[:B, :P], want[2]) and _bits_equal(lse2, want[1])
    assert torch.isnan(abuf[:B, P:]).all() and torch.isnan(abuf[B]).all()
    d_out = torch.full((B, D + 4), nan, device="cuda")[:, :D]
    d_out.copy_(_cuda(c["g"]))
    dbuf = torch.full((B + 1, ld_emb), nan, device="cuda")
    got = ops.afm_pool_bwd(emb, W, b, h, F, out, lse, d_out, d_emb=dbuf[:B, :F * D])
    wantb = _bwd(index)
    assert got[0].data_ptr() == dbuf.data_ptr() and torch.isfinite(got[0]).all()
    assert all(_bits_equal(x, y) for x, y in zip(got, wantb))
    assert torch.isnan(dbuf[:B, F * D:]).all() and torch.isnan(dbuf[B]).all()                  # untouched beyond F * D and beyond B


def test_argument_errors_and_the_empty_batch():
    from deep_recommenders_amd import _lib, ops
    z = lambda *s: torch.zeros(s, device="cuda")                                              # noqa: E731
    with pytest.raises(ValueError):                                                           # D = 6
        ops.afm_pool_fwd(z(2, 3, 6), z(6, 4), z(4), z(4), 3)
    with pytest.raises(ValueError):                                                           # F = 1
        ops.afm_pool_fwd(z(2, 1, 8), z(8, 4), z(4), z(4), 1)
    with pytest.raises(ValueError):                                                           # A = 129
        ops.afm_pool_fwd(z(2, 3, 8), z(8, 129), z(129), z(129), 3)
    with pytest.raises(ValueError):                                                           # D 256 with A 64
        ops.afm_pool_fwd(z(2, 3, 256), z(256, 64), z(64), z(64), 3)
    with pytest.raises(ValueError):                                                           # ld_emb = 25
        ops.afm_pool_fwd(z(2, 25)[:, :24], z(8, 4), z(4), z(4), 3)
    with pytest.raises(ValueError):                                                           # a short workspace
        ops.afm_pool_bwd(z(2, 3, 8), z(8, 4), z(4), z(4), 3, z(2, 8), z(2), z(2, 8), workspace=z(8))
    # the entry points themselves: DR_EINVAL / DR_ESHAPE before anything is launched
    L, s = _lib.lib(), _lib.stream_ptr()
    p = lambda t: t.data_ptr()                                                                 # noqa: E731
    emb, W, b, h, out, lse, g, demb = z(2, 24), z(8, 4), z(4), z(4), z(2, 8), z(2), z(2, 8), z(2, 24)
    dW, db, dh = z(8, 4), z(4), z(4)
    need = L.dr_afm_pool_bwd_workspace_bytes(2, 3, 8, 4)
    assert need == 4 * 1 * (8 * 4 + 2 * 4)                                                    # one block of 4 waves
    assert L.dr_afm_pool_bwd_workspace_bytes(70, 7, 20, 5) == 4 * 18 * (20 * 5 + 2 * 5)
    assert L.dr_afm_pool_bwd_workspace_bytes(1 << 20, 26, 64, 32) == 4 * 512 * (64 * 32 + 2 * 32)   # does not grow with B
    ws = z(need // 4)

    def fwd(ld_emb=24, B=2, F=3, D=8, A=4, ld_out=8, ld_attn=3, emb_=emb, out_=out, attn_=None):
        return L.dr_afm_pool_fwd(p(emb_), ld_emb, p(W), p(b), p(h), B, F, D, A, p(out_), ld_out, p(lse), attn_, ld_attn, s)

    def bwd(ld_emb=24, B=2, F=3, D=8, A=4, ld_out=8, ld_dout=8, ld_demb=24, ws_bytes=need, ws_=ws, dW_=dW):
        return L.dr_afm_pool_bwd(p(emb), ld_emb, p(W), p(b), p(h), p(out), ld_out, p(lse), p(g), ld_dout, B, F, D, A, p(demb), ld_demb,
                                 p(dW_) if dW_ is not None else None, p(db), p(dh), p(ws_), ws_bytes, s)

    assert fwd() == _lib.DR_OK and bwd() == _lib.DR_OK
    for kw in (dict(D=6), dict(D=260), dict(D=0), dict(F=1), dict(F=65), dict(A=0), dict(A=129), dict(B=-1), dict(ld_emb=25),
               dict(ld_emb=20), dict(ld_out=4), dict(ld_out=10)):
        assert fwd(**kw) == _lib.DR_EINVAL, kw
        assert bwd(**kw) == _lib.DR_EINVAL, kw
    assert fwd(attn_=p(z(2, 3)), ld_attn=2) == _lib.DR_EINVAL
    assert fwd(emb_=z(2, 25)[:, 1:]) == _lib.DR_EINVAL                                         # a base that is not 16-byte aligned
    for kw in (dict(ld_dout=4), dict(ld_dout=9), dict(ld_demb=20), dict(ld_demb=26), dict(ws_bytes=need - 4), dict(ws_bytes=0),
               dict(dW_=None)):
        assert bwd(**kw) == _lib.DR_EINVAL, kw
    for kw in (dict(D=256, A=64), dict(D=128, A=128), dict(F=64, D=256, A=32)):                # registers, registers, LDS
        assert fwd(**kw) == _lib.DR_ESHAPE, kw
        assert bwd(**kw) == _lib.DR_ESHAPE, kw
        assert L.dr_afm_pool_bwd_workspace_bytes(2, kw.get("F", 3), kw["D"], kw["A"]) == _lib.DR_ESHAPE
    assert L.dr_afm_pool_bwd_workspace_bytes(2, 3, 6, 4) == _lib.DR_EINVAL
    # B = 0: empty tensors, nothing launched
    assert L.dr_afm_pool_fwd(None, 24, None, None, None, 0, 3, 8, 4, None, 8, None, None, 0, s) == _lib.DR_OK
    assert L.dr_afm_pool_bwd(None, 24, None, None, None, None, 8, None, None, 8, 0, 3, 8, 4, None, 24, None, None, None, None, 0, s) == _lib.DR_OK
    assert L.dr_afm_pool_bwd_workspace_bytes(0, 3, 8, 4) == 0
    o, l, a = ops.afm_pool_fwd(z(0, 3, 8), z(8, 4), z(4), z(4), 3, True)
    assert o.shape == (0, 8) and l.shape == (0,) and a.shape == (0, 3)
    grads = ops.afm_pool_bwd(z(0, 3, 8), z(8, 4), z(4), z(4), 3, o, l, z(0, 8))
    assert grads[0].shape == (0, 24) and all((x == 0).all() for x in grads[1:])


def test_no_batch_sized_buffers():
    """F = 64, D = 4: the pair products [B, P, D] would be 504 times the output; neither call allocates beyond its results (and the
    backward its per-block workspace)"""
    from deep_recommenders_amd import _lib, ops
    B, F, D, A = 256, 64, 4, 16
    emb, g = torch.randn((B, F * D), device="cuda"), torch.randn((B, D), device="cuda")
    W, b, h = torch.randn((D, A), device="cuda") / 2, torch.randn(A, device="cuda") / 10, torch.randn(A, device="cuda") / 4
    out, lse, _ = ops.afm_pool_fwd(emb, W, b, h, F)                                            # code objects loaded before measuring
    ops.afm_pool_bwd(emb, W, b, h, F, out, lse, g)
    torch.cuda.synchronize()
    ws = _lib.lib().dr_afm_pool_bwd_workspace_bytes(B, F, D, A)
    assert 0 < ws <= 4 * 512 * (D * A + 2 * A)
    pairs = B * ops.afm_num_pairs(F) * D * 4
    for fn, results in ((lambda: ops.afm_pool_fwd(emb, W, b, h, F), B * D * 4 + B * 4),
                        (lambda: ops.afm_pool_bwd(emb, W, b, h, F, out, lse, g), B * F * D * 4 + (D * A + 2 * A) * 4 + ws)):
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        keep = fn()
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
        assert grown < results + 4096 and 8 * (results + 4096) < pairs, (grown, results, pairs)
        del keep


@pytest.mark.parametrize("index", [1, 5, 7], ids=[IDS[1], IDS[5], IDS[7]])
def test_autograd_glue_equals_the_entry_points(index):
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd.keras.models.ranking import AttentionalPooling
    c = R.case(index)
    B, F, D, A = c["shape"]
    emb = _cuda(c["e"]).requires_grad_(True)                                                  # [B, F, D]
    W, b, h = (t.requires_grad_(True) for t in _params(index))
    out, attn = L.afm_pooling(emb, W, b, h, want_attention=True)
    want = _fwd(index)
    assert _bits_equal(out, want[0]) and _bits_equal(attn, want[2]) and attn.requires_grad is False
    out2, none = L.afm_pooling(emb, W, b, h)
    assert none is None and _bits_equal(out2, out)
    got = torch.autograd.grad(out, [emb, W, b, h], grad_outputs=_cuda(c["g"]))
    wantb = _bwd(index)
    assert got[0].shape == (B, F, D) and _bits_equal(got[0].reshape(B, F * D), wantb[0])
    assert all(_bits_equal(x, y) for x, y in zip(got[1:], wantb[1:]))
    pitched = torch.zeros((B, F * D + 8), device="cuda")[:, :F * D]                            # the slab's concat layout, with F
    pitched.copy_(emb.detach().reshape(B, F * D))
    assert _bits_equal(L.afm_pooling(pitched, W, b, h, F=F)[0], out)
    layer = AttentionalPooling(A)
    layer.build((B, F, D))
    with torch.no_grad():
        layer.W.copy_(W)
        layer.b.copy_(b)
        layer.h.copy_(h)
    assert _bits_equal(layer(emb.detach()), out)
    o3, a3 = layer.call(c["e"].to(torch.float32).numpy(), want_attention=True)
    assert _bits_equal(o3, out) and _bits_equal(a3, attn) and a3.requires_grad is False
    fresh = AttentionalPooling(A)                                                              # built on the first call
    assert fresh(emb.detach()).shape == (B, D) and tuple(fresh.W.shape) == (D, A) and float(fresh.b.detach().abs().max()) == 0.0


def test_afm_model():
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.keras.models.ranking import AFM
    B, F, D, V, A = 33, 5, 8, 50, 4
    P = F * (F - 1) // 2
    cats = [fc.categorical_column_with_identity("c%d" % i, V) for i in range(F)]
    model = AFM([fc.indicator_column(c) for c in cats], [fc.embedding_column(c, D) for c in cats], attention_factor=A)
    model.pooling.build((B, F, D))
    base = np.asarray([model.slab.base["c%d" % i] for i in range(F)])
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))                          # noqa: E731
    for seed in range(100):                                                                    # redraw until the relu mask is safe
        rng = np.random.default_rng(40 + seed)
        inputs = {"c%d" % i: rng.integers(0, V, size=(B, 1)) for i in range(F)}
        vals = dict(table=f32(rng.standard_normal((F * V, D)) / np.sqrt(D)), lin_w=f32(0.1 * rng.standard_normal(F * V)),
                    lin_bias=f32(0.1 * rng.standard_normal(1)), W=f32(rng.standard_normal((D, A)) / np.sqrt(D)),
                    b=f32(0.1 * rng.standard_normal(A)), h=f32(rng.standard_normal(A) / np.sqrt(A)),
                    w_out=f32(rng.standard_normal((D, 1)) / np.sqrt(D)))
        ids = np.concatenate([inputs["c%d" % i] for i in range(F)], axis=1) + base
        margin = R.mask_margin(vals["table"].double()[torch.from_numpy(ids)], vals["W"].double(), vals["b"].double())
        if margin >= 1.0:
            break
    print("AFM model: seed %d, min |z| / (4 eps_z) = %.2f" % (seed, margin))
    assert margin >= 1.0
    params = dict(table=model.slab.table, lin_w=model.slab.lin_w, lin_bias=model.slab.lin_bias, W=model.pooling.W, b=model.pooling.b,
                  h=model.pooling.h, w_out=model.w_out)
    with torch.no_grad():
        for k, v in vals.items():
            params[k].copy_(v)
    logits = model.logits(inputs)
    assert logits.shape == (B, 1)
    # the restatement with the same parameters, float64
    leaves = {k: v.double().requires_grad_(True) for k, v in vals.items()}
    e = leaves["table"][torch.from_numpy(ids)]                                                # [B, F, D]
    linear = leaves["lin_w"][torch.from_numpy(ids)].sum(1) + leaves["lin_bias"]
    want = R.afm_logits(e, linear, leaves["W"], leaves["b"], leaves["h"], leaves["w_out"])
    with torch.no_grad():                                                                     # the stages' bounds, carried to the logit
        f = R.forward(e, leaves["W"], leaves["b"], leaves["h"])
        eps_s = (A + 2) * U * (torch.relu(f["z"]) @ leaves["h"].abs()) + R.eps_z(e, leaves["W"], leaves["b"]) @ leaves["h"].abs()
        out_bound = (2 * eps_s.max(1).values + (2 * P + 10) * U)[:, None] * (f["attn"][:, :, None] * f["p"].abs()).sum(1)
        atol = (out_bound.max() * leaves["w_out"].abs().sum() + 2e-6 * f["out"].abs().max() * leaves["w_out"].abs().max() * np.sqrt(D)
                + (F + 2) * U * (leaves["lin_w"][torch.from_numpy(ids)].abs().sum(1) + leaves["lin_bias"].abs()).max()).item()
    err = (logits.detach().double().cpu() - want.detach()).abs().max().item()
    print("AFM logits: max |err| = %.3g, atol = %.3g" % (err, atol))
    np.testing.assert_allclose(logits.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-5, atol=atol)
    attn = model.attention(inputs)
    assert attn.shape == (B, P) and attn.requires_grad is False
    np.testing.assert_allclose(attn.cpu().numpy(), f["attn"].numpy(), rtol=1e-4)
    # parameter gradients of sum(logits * gy)
    gy = torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32))
    logits.backward(gy.cuda())
    names = list(vals)
    grads = torch.autograd.grad((want * gy.double()).sum(), [leaves[k] for k in names])
    for k, w in zip(names, grads):
        assert params[k].grad is not None, k
        w = w.numpy()
        np.testing.assert_allclose(params[k].grad.cpu().numpy(), w, rtol=2e-4, atol=2e-5 * np.abs(w).max(), err_msg="gradient of " + k)
    # one fused sparse SGD step changes exactly the looked-up rows
    model.zero_grad(set_to_none=True)
    model.slab.sparse_lr = 0.1
    before = model.slab.table.detach().clone()
    model.logits(inputs).backward(gy.cuda())
    torch.cuda.synchronize()
    assert model.slab.table.grad is None
    changed = (model.slab.table.detach() != before).any(dim=1).cpu().numpy()
    looked_up = np.zeros(F * V, dtype=bool)
    looked_up[np.unique(ids)] = True
    assert np.array_equal(changed, looked_up)
    np.testing.assert_allclose(model.slab.table.detach().cpu().numpy(), (before.cpu().double() - 0.1 * grads[0]).numpy(), rtol=2e-4,
                               atol=2e-5 * 0.1 * grads[0].abs().max().item() + 1e-7)
    model.slab.sparse_lr = None
    prob = model.predict(inputs)
    assert prob.shape == (B, 1) and ((prob > 0) & (prob < 1)).all()
    assert model.get_config() == {"attention_factor": A, "dropout": 0.0}
    # dropout acts on the pooled vector while training only
    dropped = AFM(model._indicator_columns, model._embedding_columns, attention_factor=A, dropout=0.5)
    dropped.pooling.build((B, F, D))
    dropped.load_state_dict(model.state_dict())
    now = model.logits(inputs)
    assert not torch.equal(dropped.logits(inputs), now)
    dropped.eval()
    assert _bits_equal(dropped.logits(inputs), now)
