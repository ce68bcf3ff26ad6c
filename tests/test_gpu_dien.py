"""GPU tests of DIEN on the fused recurrence kernels (csrc/dien.hip): the entry points against the float64 restatement
(tests/dien_ref.py), bit-reproducibility, independence of an example from its batch, strides and padding, masking, the attention
kernels, the argument errors, the autograd glue and the model end to end.  The inputs are dien_ref.CASES.

Limit.  For each of hs, h_last, d_xp, dU, d_h0, d_att (and a, d_hs, d_q of the attention) the error is the largest absolute
difference from the float64 result divided by the largest absolute float64 value; r32 is the same figure for the float32 run of the
restatement (reference only), and the limit is 16 max(r32, 8u), u = 2^-24.  r32 lies between 0.7u and 7.5u at these shapes, so the
floor 8u governs: the limit is 128u.  The kernel sums in another order than torch (MFMA chains of 4 along k, 16-lane xor sums and a
wave-ordered sum for d_att, the dense path's tiles for dU) and uses the device's expf and tanhf; tests/test_dien_cpu.py shows that a
deliberately different fp32 association (k-chunks of 4 added last first, exp2-based gates) reads at most 9.3u (dU at 5 x 200 x 16),
0.073 of the limit, while a dropped step, a wrong mask or a bf16 product is off by 1e-3 or more.
On an MI355X the recurrence kernels read at most 0.048 of the limit (6.1u, dU at 33 x 12 x 128) and the attention kernels 0.100
(14.7u against r32 = 9.2u, d_hs at 33 x 12 x 128, where exp carries the rounding of scores of magnitude 10)."""
import functools

import numpy as np
import pytest
import torch

import dien_ref as R

pytestmark = pytest.mark.gpu

DD = torch.float64
ALL = list(range(len(R.CASES)))
IDS = ["%dx%dx%d-%s" % (R.CASES[i][0] + ("augru" if R.CASES[i][1] else "gru",)) for i in ALL]
PLAIN = [i for i in ALL if not R.CASES[i][1]]


def _bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cuda(t):
    if t is None:
        return None
    return t.cuda() if t.dtype == torch.int32 else t.to(torch.float32).cuda()


@functools.lru_cache(maxsize=None)
def _inputs(index):
    c = R.case(index)
    return {k: _cuda(c[k]) for k in ("xp", "U", "h0", "lengths", "att", "d_hs", "d_h_last", "q", "d_a")}


def _sl(t, lo, hi):
    return None if t is None else t[lo:hi]


def _run(index, lo=None, hi=None, **over):
    """(hs, h_last, d_xp, dU, d_h0, d_att) of the two entry points"""
    from deep_recommenders_amd import ops
    g = dict(_inputs(index), **over)
    a = [_sl(g[k], lo, hi) if k != "U" else g[k] for k in R.ARGS]
    hs, h_last = ops.gru_seq_fwd(*a)
    return (hs, h_last) + tuple(ops.gru_seq_bwd(*a, hs, _sl(g["d_hs"], lo, hi), _sl(g["d_h_last"], lo, hi)))


def _check(name, shape, got, want, ref32):
    r32, err = R.rel_err(ref32, want), R.rel_err(got.detach().cpu(), want)
    lim = R.limit(r32)
    print("%s %s: error %.2f u, r32 %.2f u, %.3f of the limit" % (name, shape, err / R.U24, r32 / R.U24, err / lim))
    assert err <= lim, (name, shape, err, lim)


@pytest.mark.parametrize("index", ALL, ids=IDS)
def test_forward_and_backward_against_float64(index):
    c = R.case(index)
    B, T, H = c["shape"]
    got = _run(index)
    shapes = ((B, T, H), (B, H), (B, T, 3 * H), (H, 3 * H), (B, H), (B, T))
    for name, x, shp, want, ref32 in zip(R.NAMES, got, shapes, c["want"], c["ref32"]):
        if want is None:
            assert x is None and name == "d_att"
            continue
        assert tuple(x.shape) == shp and torch.isfinite(x).all(), name
        _check(name, c["shape"], x, want, ref32)
    again = _run(index)                                                                        # run to run
    assert all(_bits_equal(x, y) for x, y in zip(got, again))
    # masked steps: exact zeros; an empty example passes h0 and d_h_last through
    lens = c["lengths"].long()
    off = (torch.arange(T)[None, :] >= lens[:, None]).cuda()
    assert (got[0][off] == 0).all() and (got[2][off] == 0).all() and (got[5] is None or (got[5][off] == 0).all())
    empty = (lens == 0).cuda()
    g = _inputs(index)
    assert _bits_equal(got[1][empty], g["h0"][empty]) and _bits_equal(got[4][empty], g["d_h_last"][empty])


@pytest.mark.parametrize("index", [i for i in ALL if R.CASES[i][0][0] >= 2], ids=[IDS[i] for i in ALL if R.CASES[i][0][0] >= 2])
def test_an_example_does_not_depend_on_its_batch(index):
    full, alone = _run(index), _run(index, 1, 2)
    assert alone[0].shape[0] == 1
    for k in (0, 1, 2, 4, 5):                                                                  # all but dU, a sum over the batch
        assert _bits_equal(_sl(full[k], 1, 2), alone[k]), R.NAMES[k]
    tail = _run(index, 2, None)                                                                # another position in the tile
    for k in (0, 1, 2, 4, 5):
        assert _bits_equal(_sl(full[k], 2, None), tail[k]), R.NAMES[k]


@pytest.mark.parametrize("index", ALL, ids=IDS)
def test_strides_and_padding(index):
    from deep_recommenders_amd import ops
    c = R.case(index)
    B, T, H = c["shape"]
    g = _inputs(index)
    want = _run(index)
    nan = float("nan")
    xp_p = torch.full((B, T, 3 * H + 8), nan, device="cuda")[:, :, :3 * H]                     # a padded pitch, read in place
    xp_p.copy_(g["xp"])
    xp_v = torch.full((B, T + 1, 3 * H), nan, device="cuda")[:, :-1]                           # a [:, :-1] view: no single pitch
    xp_v.copy_(g["xp"])
    dhs_v = torch.full((B, T + 1, H + 4), nan, device="cuda")[:, :-1, :H]
    dhs_v.copy_(g["d_hs"])
    buf = torch.full((B * T + 1, H + 4), nan, device="cuda")                                   # the last row is a guard
    hs_out = buf[:B * T].reshape(B, T, H + 4)[:, :, :H]
    a = (g["U"], g["h0"], g["lengths"], g["att"])
    hs, h_last = ops.gru_seq_fwd(xp_p, *a, hs=hs_out)
    assert hs.data_ptr() == buf.data_ptr() and _bits_equal(hs, want[0]) and _bits_equal(h_last, want[1])
    assert torch.isnan(buf[:, H:]).all() and torch.isnan(buf[B * T]).all()
    hs2, h_last2 = ops.gru_seq_fwd(xp_v, *a)
    assert _bits_equal(hs2, want[0]) and _bits_equal(h_last2, want[1])
    dbuf = torch.full((B * T + 1, 3 * H + 4), nan, device="cuda")
    dxp_out = dbuf[:B * T].reshape(B, T, 3 * H + 4)[:, :, :3 * H]
    got = ops.gru_seq_bwd(xp_p, *a, hs, dhs_v, g["d_h_last"], d_xp=dxp_out)                    # hs at its padded pitch
    assert got[0].data_ptr() == dbuf.data_ptr() and all(_bits_equal(x, y) for x, y in zip(got, want[2:]))
    assert torch.isnan(dbuf[:, 3 * H:]).all() and torch.isnan(dbuf[B * T]).all()
    got2 = ops.gru_seq_bwd(xp_v, *a, hs2, g["d_hs"], g["d_h_last"])
    assert all(_bits_equal(x, y) for x, y in zip(got2, want[2:]))


@pytest.mark.parametrize("index", ALL, ids=IDS)
def test_masked_steps_are_never_read(index):
    c = R.case(index)
    B, T, H = c["shape"]
    g = _inputs(index)
    off = (torch.arange(T)[None, :] >= c["lengths"].long()[:, None]).cuda()
    xp0, xpn = g["xp"].clone(), g["xp"].clone()
    xp0[off] = 0.0
    xpn[off] = float("nan")
    dh0, dhn = g["d_hs"].clone(), g["d_hs"].clone()
    dh0[off] = 0.0
    dhn[off] = float("nan")
    over0, overn = dict(xp=xp0, d_hs=dh0), dict(xp=xpn, d_hs=dhn)
    if g["att"] is not None:
        over0["att"], overn["att"] = g["att"].clone(), g["att"].clone()
        over0["att"][off] = 0.0
        overn["att"][off] = float("nan")
    zero, nans, plain = _run(index, **over0), _run(index, **overn), _run(index)
    for name, x, y, z in zip(R.NAMES, zero, nans, plain):
        assert x is None or torch.isfinite(y).all(), name
        assert _bits_equal(x, y) and _bits_equal(x, z), name


@pytest.mark.parametrize("index", PLAIN, ids=[IDS[i] for i in PLAIN])
def test_sequence_attention(index):
    from deep_recommenders_amd import ops
    c = R.case(index)
    B, T, H = c["shape"]
    g = _inputs(index)
    hs64 = c["want"][0].float().double()                                                       # float32 values
    hs = hs64.float().cuda()
    lens = c["lengths"]
    a = ops.seq_attn_fwd(hs, g["q"], g["lengths"])
    want = R.attention(hs64, c["q"], lens)
    ref32 = R.attention(hs64.float(), c["q"].float(), lens)
    assert tuple(a.shape) == (B, T)
    _check("a", c["shape"], a, want, ref32)
    sums = a.double().sum(1).cpu()
    empty = lens == 0
    assert ((sums[~empty] - 1).abs() <= (T + 8) * R.U24).all() and (a[empty.cuda()] == 0).all()
    off = (torch.arange(T)[None, :] >= lens.long()[:, None]).cuda()
    assert (a[off] == 0).all()
    d_hs, d_q = ops.seq_attn_bwd(hs, g["q"], g["lengths"], a, g["d_a"])
    wb = R.attention_backward(hs64, c["q"], lens, c["d_a"])
    rb = R.attention_backward(hs64.float(), c["q"].float(), lens, c["d_a"].float())
    _check("attention d_hs", c["shape"], d_hs, wb[0], rb[0])
    _check("attention d_q", c["shape"], d_q, wb[1], rb[1])
    assert (d_hs[off] == 0).all()
    # NaN in the masked rows of hs and d_a changes nothing; run to run
    hsn, dan = hs.clone(), g["d_a"].clone()
    hsn[off] = float("nan")
    dan[off] = float("nan")
    a2 = ops.seq_attn_fwd(hsn, g["q"], g["lengths"])
    assert _bits_equal(a2, a)
    b2 = ops.seq_attn_bwd(hsn, g["q"], g["lengths"], a2, dan)
    assert _bits_equal(b2[0], d_hs) and _bits_equal(b2[1], d_q)
    if B >= 2:
        assert _bits_equal(ops.seq_attn_fwd(hs[1:2], g["q"][1:2], g["lengths"][1:2]), a[1:2])
    pitched = torch.zeros((B, T, H + 4), device="cuda")[:, :, :H]
    pitched.copy_(hs)
    assert _bits_equal(ops.seq_attn_fwd(pitched, g["q"], g["lengths"]), a)
    full = ops.seq_attn_fwd(hs, g["q"], None)                                                  # no lengths: every step is valid
    assert ((full.double().sum(1) - 1).abs() <= (T + 8) * R.U24).all()


def test_argument_errors_and_the_empty_batch():
    from deep_recommenders_amd import _lib, ops
    z = lambda *s: torch.zeros(s, device="cuda")                                              # noqa: E731
    with pytest.raises(ValueError):                                                           # H = 6
        ops.gru_seq_fwd(z(2, 3, 18), z(6, 18))
    with pytest.raises(ValueError):                                                           # H = 132
        ops.gru_seq_fwd(z(2, 3, 396), z(132, 396))
    with pytest.raises(ValueError):                                                           # T = 0
        ops.gru_seq_fwd(z(2, 0, 24), z(8, 24))
    with pytest.raises(ValueError):                                                           # a short workspace
        ops.gru_seq_bwd(z(2, 3, 24), z(8, 24), None, None, None, z(2, 3, 8), z(2, 3, 8), z(2, 8), workspace=z(8))
    with pytest.raises(ValueError):                                                           # a base that is not 16-byte aligned
        ops.gru_seq_fwd(z(2 * 3 * 24 + 1)[1:].view(2, 3, 24), z(8, 24))
    with pytest.raises(ValueError):
        ops.seq_attn_fwd(z(2, 3, 6), z(2, 6))
    # a length above T (or below 0) is clamped by the kernels
    xp, U = torch.randn((4, 3, 24), device="cuda"), torch.randn((8, 24), device="cuda")
    big = ops.gru_seq_fwd(xp, U, lengths=torch.tensor([7, 3, -2, 0], dtype=torch.int32, device="cuda"))
    ok = ops.gru_seq_fwd(xp, U, lengths=torch.tensor([3, 3, 0, 0], dtype=torch.int32, device="cuda"))
    assert _bits_equal(big[0], ok[0]) and _bits_equal(big[1], ok[1])
    # the entry points themselves: DR_EINVAL / DR_ESHAPE before anything is launched
    L, s = _lib.lib(), _lib.stream_ptr()
    p = lambda t: None if t is None else t.data_ptr()                                         # noqa: E731
    xp, U, hs, hl, dhs, dhl, dxp, dU, q, a = z(2, 3, 24), z(8, 24), z(2, 3, 8), z(2, 8), z(2, 3, 8), z(2, 8), z(2, 3, 24), z(8, 24), z(2, 8), z(2, 3)
    need = L.dr_gru_seq_bwd_workspace_bytes(2, 3, 8)
    assert need == 4 * 2 * 4 * 24 + (max(L.dr_linear_bwd_dw_workspace_bytes(6, 8, 24), L.dr_linear_bwd_dw_workspace_bytes(2, 8, 24)) + 15) // 16 * 16
    ws = z(need // 4)
    off1 = z(2 * 3 * 24 + 1)[1:]

    def fwd(B=2, T=3, H=8, ld_xp=24, ld_hs=8, xp_=xp, hs_=hs):
        return L.dr_gru_seq_fwd(p(xp_), ld_xp, p(U), None, None, None, B, T, H, p(hs_), ld_hs, p(hl), s)

    def bwd(B=2, T=3, H=8, ld_xp=24, ld_hs=8, ld_dhs=8, ld_dxp=24, ws_bytes=need, xp_=xp, dU_=dU, ws_=ws):
        return L.dr_gru_seq_bwd(p(xp_), ld_xp, p(U), None, None, None, p(hs), ld_hs, B, T, H, p(dhs), ld_dhs, p(dhl), p(dxp), ld_dxp, p(dU_),
                                None, None, p(ws_), ws_bytes, s)

    assert fwd() == _lib.DR_OK and bwd() == _lib.DR_OK
    for kw in (dict(H=6), dict(H=0), dict(T=0), dict(B=-1), dict(ld_xp=25), dict(ld_xp=20), dict(ld_hs=4), dict(ld_hs=10), dict(xp_=off1)):
        assert fwd(**kw) == _lib.DR_EINVAL, kw
        assert bwd(**kw) == _lib.DR_EINVAL, kw
    for kw in (dict(ld_dhs=4), dict(ld_dxp=26), dict(ld_dxp=20), dict(ws_bytes=need - 4), dict(ws_bytes=0), dict(dU_=None), dict(ws_=None)):
        assert bwd(**kw) == _lib.DR_EINVAL, kw
    assert fwd(H=132) == _lib.DR_ESHAPE and bwd(H=132) == _lib.DR_ESHAPE and L.dr_gru_seq_bwd_workspace_bytes(2, 3, 132) == _lib.DR_ESHAPE
    assert L.dr_seq_attn_fwd(p(hs), 8, p(q), None, 2, 3, 8, p(a), s) == _lib.DR_OK
    assert L.dr_seq_attn_bwd(p(hs), 8, p(q), None, p(a), p(a), 2, 3, 8, p(dhs), 8, p(dhl), s) == _lib.DR_OK
    for kw in (dict(H=6), dict(T=0), dict(ld=4), dict(ld=9)):
        H, T, ld = kw.get("H", 8), kw.get("T", 3), kw.get("ld", 8)
        assert L.dr_seq_attn_fwd(p(hs), ld, p(q), None, 2, T, H, p(a), s) == _lib.DR_EINVAL, kw
        assert L.dr_seq_attn_bwd(p(hs), ld, p(q), None, p(a), p(a), 2, T, H, p(dhs), 8, p(dhl), s) == _lib.DR_EINVAL, kw
    assert L.dr_seq_attn_fwd(p(hs), 132, p(q), None, 2, 3, 132, p(a), s) == _lib.DR_ESHAPE
    assert L.dr_seq_attn_fwd(p(hs), 8, None, None, 2, 3, 8, p(a), s) == _lib.DR_EINVAL
    # B = 0: empty tensors, nothing launched
    hs0, hl0 = ops.gru_seq_fwd(z(0, 3, 24), U)
    assert hs0.shape == (0, 3, 8) and hl0.shape == (0, 8)
    g0 = ops.gru_seq_bwd(z(0, 3, 24), U, None, None, None, hs0, z(0, 3, 8), z(0, 8))
    assert g0[0].shape == (0, 3, 24) and (g0[1] == 0).all() and g0[3] is None
    assert ops.seq_attn_fwd(z(0, 3, 8), z(0, 8)).shape == (0, 3)


def _leaves(vals):
    return {k: v.clone().requires_grad_(True) for k, v in vals.items()}


def test_layers_gradients_against_float64():
    """GRU, AUGRU and InterestEvolution: parameter and input gradients of a random linear functional, B 6, T 5, D 8, H 12, against
    autograd of the restatement in float64; the limit as above with r32 from its float32 run"""
    from deep_recommenders_amd.keras.models.ranking import AUGRU, GRU, InterestEvolution
    B, T, D, H = 6, 5, 8, 12
    rng = np.random.default_rng(77)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).double()       # noqa: E731
    lens = torch.tensor([5, 1, 0, 3, 4, 2], dtype=torch.int32)
    vals = dict(seq=f(B, T, D), W=f(D, 3 * H) / np.sqrt(D), b=0.1 * f(3 * H), U=f(H, 3 * H) / np.sqrt(H), h0=0.5 * f(B, H),
                att=torch.from_numpy(rng.uniform(0, 1, (B, T)).astype(np.float32)).double())
    g_hs, g_last = f(B, T, H), f(B, H)

    def reference(dtype, with_att):
        lv = _leaves({k: v.to(dtype) for k, v in vals.items() if with_att or k != "att"})
        hs, h_last = R.gru_layer(lv["seq"], lv["W"], lv["b"], lv["U"], lens, lv.get("att"), lv["h0"])
        names = list(lv)
        grads = torch.autograd.grad((hs * g_hs.to(dtype)).sum() + (h_last * g_last.to(dtype)).sum(), [lv[k] for k in names])
        return dict(zip(names, grads), hs=hs.detach(), h_last=h_last.detach())

    for cls, with_att in ((GRU, False), (AUGRU, True)):
        want, ref32 = reference(DD, with_att), reference(torch.float32, with_att)
        layer = cls(H)
        layer.build(D)
        with torch.no_grad():
            layer.kernel.copy_(vals["W"])
            layer.bias.copy_(vals["b"])
            layer.recurrent_kernel.copy_(vals["U"])
        lv = _leaves({k: vals[k].float().cuda() for k in (("seq", "h0", "att") if with_att else ("seq", "h0"))})
        args = (lv["seq"], lv["att"]) if with_att else (lv["seq"],)
        hs, h_last = layer(*args, lengths=lens, initial_state=lv["h0"], return_state=True)
        (hs * g_hs.float().cuda()).sum().add((h_last * g_last.float().cuda()).sum()).backward()
        got = dict(seq=lv["seq"].grad, h0=lv["h0"].grad, W=layer.kernel.grad, b=layer.bias.grad, U=layer.recurrent_kernel.grad, hs=hs,
                   h_last=h_last)
        if with_att:
            got["att"] = lv["att"].grad
        for k, x in got.items():
            assert x is not None, k
            _check("%s %s" % (cls.__name__, k), (B, T, D, H), x, want[k], ref32[k])
        mask = torch.arange(T)[None, :] < lens[:, None]                                       # a prefix mask is the same call
        assert _bits_equal(layer(*[t.detach() for t in args], mask=mask, initial_state=lv["h0"].detach()), hs)
    # InterestEvolution: hs [B, T, H] from above as its input, target [B, Da]
    Da = 8
    ev = dict(hs=f(B, T, H) * 0.5, target=f(B, Da), Wa=f(H, Da) / np.sqrt(Da), W=f(H, 3 * H) / np.sqrt(H), b=0.1 * f(3 * H),
              U=f(H, 3 * H) / np.sqrt(H))

    def evolution(dtype):
        lv = _leaves({k: v.to(dtype) for k, v in ev.items()})
        out, a = R.evolution(lv["hs"], lv["target"], lens, lv["Wa"], lv["W"], lv["b"], lv["U"])
        names = list(lv)
        grads = torch.autograd.grad((out * g_last.to(dtype)).sum(), [lv[k] for k in names])
        return dict(zip(names, grads), out=out.detach(), a=a.detach())

    want, ref32 = evolution(DD), evolution(torch.float32)
    layer = InterestEvolution(H)
    layer.build(H, Da)
    layer.augru.build(H)
    with torch.no_grad():
        layer.attention_kernel.copy_(ev["Wa"])
        layer.augru.kernel.copy_(ev["W"])
        layer.augru.bias.copy_(ev["b"])
        layer.augru.recurrent_kernel.copy_(ev["U"])
    lv = _leaves({k: ev[k].float().cuda() for k in ("hs", "target")})
    out, a = layer(lv["hs"], lv["target"], lens, return_attention=True)
    (out * g_last.float().cuda()).sum().backward()
    got = dict(hs=lv["hs"].grad, target=lv["target"].grad, Wa=layer.attention_kernel.grad, W=layer.augru.kernel.grad, b=layer.augru.bias.grad,
               U=layer.augru.recurrent_kernel.grad, out=out, a=a)
    for k, x in got.items():
        assert x is not None, k
        _check("InterestEvolution %s" % k, (B, T, Da, H), x, want[k], ref32[k])
    fresh = InterestEvolution(H)                                                              # built on the first call
    assert fresh(lv["hs"].detach(), lv["target"].detach(), lens).shape == (B, H) and tuple(fresh.attention_kernel.shape) == (H, Da)


def test_auxiliary_loss_against_float64():
    from deep_recommenders_amd.keras.models.ranking import InterestExtractor
    B, T, H = 6, 5, 8
    rng = np.random.default_rng(78)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).double()       # noqa: E731
    lens = torch.tensor([5, 1, 0, 3, 4, 2], dtype=torch.int32)
    vals = dict(hs=f(B, T, H), seq=f(B, T, H), neg=f(B, T, H))
    lv64 = _leaves(vals)
    want = R.auxiliary_loss(lv64["hs"], lv64["seq"], lv64["neg"], lens)
    wg = torch.autograd.grad(want, list(lv64.values()))
    lv = _leaves({k: v.float().cuda() for k, v in vals.items()})
    loss = InterestExtractor(H).auxiliary_loss(lv["hs"], lv["seq"], lv["neg"], lens)
    loss.backward()
    np.testing.assert_allclose(loss.item(), want.item(), rtol=64 * R.U24)                      # 20 terms of a few u each and their mean
    for k, w in zip(vals, wg):
        np.testing.assert_allclose(lv[k].grad.cpu().numpy(), w.numpy(), rtol=1e-5, atol=1e-6 * w.abs().max().item(), err_msg=k)


def test_dien_model_trains_on_one_batch():
    from deep_recommenders_amd import losses
    from deep_recommenders_amd.keras.models.ranking import DIEN
    torch.manual_seed(5)
    B, T, V, D = 64, 10, 50, 8
    rng = np.random.default_rng(9)
    beh, neg, tgt = rng.integers(0, V, (B, T)), rng.integers(0, V, (B, T)), rng.integers(0, V, B)
    lens = rng.integers(0, T + 1, B)
    lens[:3] = (T, 1, 0)
    profile = rng.standard_normal((B, 3)).astype(np.float32)
    y = torch.from_numpy((rng.uniform(size=(B, 1)) < 0.5).astype(np.float32)).cuda()
    model = DIEN(V, D, D, dnn_units_size=(16, 8))
    prob = model(beh, lens, tgt, neg, profile)
    assert prob.shape == (B, 1) and ((prob > 0) & (prob < 1)).all()
    aux = model.auxiliary_loss
    assert aux is not None and aux.dim() == 0 and torch.isfinite(aux)
    (g,) = torch.autograd.grad(aux, [model.item_table], retain_graph=True)
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    assert model(beh, lens, tgt, None, profile).shape == (B, 1) and model.auxiliary_loss is None       # no negatives: no auxiliary loss
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    history = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        loss = losses.binary_crossentropy(y, model(beh, lens, tgt, neg, profile)) + model.auxiliary_loss
        loss.backward()
        opt.step()
        history.append(loss.item())
    print("DIEN on one batch: loss %.4f -> %.4f" % (history[0], history[-1]))
    assert np.isfinite(history).all() and history[-1] < history[0]
    assert all(p.grad is not None for p in model.parameters())
