"""GPU tests of DLRM on the fused pairwise dot-interaction kernels (csrc/dot_interact.hip): the two entry points against the float64
restatement (tests/dlrm_ref.py) and float64 autograd, bit-reproducibility, independence of an example from its batch, strides and
padding, the argument errors, the autograd glue, DotInteraction and DLRM end to end.

Tolerances of the two entry points are derived.  An fp32 sum of n products in any order satisfies
|err| <= n u / (1 - n u) sum_k |a_k b_k| with u = 2^-24.
  forward   every triangle element within (D + 2) u (|T| |T|^T)_ij of the float64 value; the t_0 copy is bit-exact.
  backward  every element of dT within (N + 3) u (|S| |T|)_id.  S is exact (one d_out value per off-diagonal pair, times 2 on the
            diagonal).  Row 0 also adds d_out[:, 0:D]: that value is one more term of the same sum (a_k = d_out, b_k = 1), so |d_out[b, d]|
            is added to (|S| |T|)_0d -- the rounding of the last add is relative to the sum including it, and without that term the
            inequality above does not hold for a correct kernel when |d_out| dominates the row (N = 2).
A plain fp32 accumulation chain stays below 0.34 of the forward and 0.19 of the backward bound, so a correct kernel has room."""
import functools

import numpy as np
import pytest
import torch

import dlrm_ref as R

pytestmark = pytest.mark.gpu

DD = torch.float64
U = 2.0 ** -24
# (B, F, D, dense, self_interaction)
SHAPES = [(3, 1, 4, True, False),        # N = 2, the smallest
          (2, 2, 4, False, False),       # no dense vector
          (4, 15, 8, True, False),       # N = 16
          (4, 16, 8, True, False),       # N = 17, crossing a 16-tile
          (3, 31, 12, True, False),      # N = 32, D not a multiple of 8
          (3, 32, 16, True, True),       # N = 33, crossing a 32-tile, diagonal included
          (2, 63, 4, True, False),       # N = 64
          (2, 5, 256, True, True),       # the largest D
          (1, 3, 128, True, False),      # D = 128
          (5, 26, 64, True, False),      # the workload's row
          (70, 7, 20, False, True)]      # more examples than a block holds, remainder block


def _pad4(n):
    return (n + 3) // 4 * 4


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cuda(a):
    return None if a is None else a.to(torch.float32).cuda()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs (float32 values held in float64), the float64 forward and backward and their bounds; computed once, never modified"""
    B, F, D, has_dense, self_i = shape
    rng = np.random.default_rng(1000 + SHAPES.index(shape))
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DD)         # noqa: E731
    dense = t(B, D) if has_dense else None
    emb = t(B, F, D)
    N = F + int(has_dense)
    c0 = D if has_dense else 0
    rows, cols = R.triangle(N, self_i)
    P = len(rows)
    d_out = t(B, c0 + P)
    leaves = [emb.clone().requires_grad_(True)] + ([dense.clone().requires_grad_(True)] if has_dense else [])
    out = R.dot_interaction(leaves[1] if has_dense else None, leaves[0], self_i)
    grads = torch.autograd.grad((out * d_out).sum(), leaves)
    T = R.stack(dense, emb).abs()
    fwd_bound = (D + 2) * U * torch.einsum("bid,bjd->bij", T, T)[:, rows, cols]
    S = R.symmetric_gradient(d_out[:, c0:], N, self_i).abs()
    sums = torch.einsum("bij,bjd->bid", S, T)
    if has_dense:
        sums[:, 0] += d_out[:, :c0].abs()
    bwd_bound = (N + 3) * U * sums
    return dict(dense=dense, emb=emb, d_out=d_out, out=out.detach(), N=N, c0=c0, P=P, fwd_bound=fwd_bound,
                d_emb=grads[0], d_dense=grads[1] if has_dense else None,
                bound_emb=bwd_bound[:, 1:] if has_dense else bwd_bound, bound_dense=bwd_bound[:, 0] if has_dense else None)


def _fwd(shape, lo=None, hi=None):
    from deep_recommenders_amd import ops
    c = _case(shape)
    B, F, D, has_dense, self_i = shape
    sl = slice(lo, hi)
    return ops.dot_interact_fwd(_cuda(c["dense"])[sl] if has_dense else None, _cuda(c["emb"])[sl], F, D, self_i)


def _bwd(shape, lo=None, hi=None):
    from deep_recommenders_amd import ops
    c = _case(shape)
    B, F, D, has_dense, self_i = shape
    sl = slice(lo, hi)
    g = torch.zeros((B, _pad4(c["c0"] + c["P"])), dtype=torch.float32, device="cuda")[:, :c["c0"] + c["P"]]
    g.copy_(_cuda(c["d_out"]))
    return ops.dot_interact_bwd(_cuda(c["dense"])[sl] if has_dense else None, _cuda(c["emb"])[sl], F, D, g[sl], self_i)


def _within(got, want, bound, what):
    err = (got.detach().double().cpu() - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print("%s: max |err| / bound = %.3f" % (what, ratio))
    assert (err <= bound).all(), "%s: max |err| / bound = %.3f" % (what, ratio)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward(shape):
    c = _case(shape)
    B, F, D, has_dense, self_i = shape
    out = _fwd(shape)
    assert out.shape == (B, c["c0"] + c["P"]) and out.stride(0) == _pad4(c["c0"] + c["P"])
    if has_dense:
        assert _bits_equal(out[:, :D], _cuda(c["dense"]))                                     # the t_0 copy is bit-exact
    _within(out[:, c["c0"]:], c["out"][:, c["c0"]:], c["fwd_bound"], "forward %s" % (shape,))
    assert _bits_equal(out, _fwd(shape))                                                      # run to run


@pytest.mark.parametrize("shape", SHAPES)
def test_backward(shape):
    c = _case(shape)
    B, F, D, has_dense, self_i = shape
    d_dense, d_emb = _bwd(shape)
    assert d_emb.shape == (B, F * D)
    _within(d_emb.reshape(B, F, D), c["d_emb"], c["bound_emb"], "d_emb %s" % (shape,))
    if has_dense:
        assert d_dense.shape == (B, D)
        _within(d_dense, c["d_dense"], c["bound_dense"], "d_dense %s" % (shape,))
    else:
        assert d_dense is None
    again = _bwd(shape)                                                                       # run to run
    assert _bits_equal(d_emb, again[1]) and (not has_dense or _bits_equal(d_dense, again[0]))


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] >= 2])
def test_an_example_does_not_depend_on_its_batch(shape):
    has_dense = shape[3]
    full, alone = _fwd(shape), _fwd(shape, 1, 2)
    assert alone.shape[0] == 1 and _bits_equal(full[1:2], alone)
    gfull, galone = _bwd(shape), _bwd(shape, 1, 2)
    assert _bits_equal(gfull[1][1:2], galone[1])
    if has_dense:
        assert _bits_equal(gfull[0][1:2], galone[0])


@pytest.mark.parametrize("shape", SHAPES)
def test_strides_and_padding(shape):
    from deep_recommenders_amd import ops
    c = _case(shape)
    B, F, D, has_dense, self_i = shape
    w = c["c0"] + c["P"]
    nan = float("nan")
    ld_emb = _pad4(F * D + 13)
    emb = torch.full((B, ld_emb), nan, device="cuda")[:, :F * D]
    emb.copy_(_cuda(c["emb"]).reshape(B, F * D))
    dense = None
    if has_dense:
        dense = torch.full((B, D + 8), nan, device="cuda")[:, :D]
        dense.copy_(_cuda(c["dense"]))
    ld_out = _pad4(w) + 4
    buf = torch.full((B + 1, ld_out), nan, device="cuda")                                      # the last row is a guard
    out = ops.dot_interact_fwd(dense, emb, F, D, self_i, out=buf[:B, :w])
    assert out.data_ptr() == buf.data_ptr() and _bits_equal(out, _fwd(shape))
    assert (buf[:B, w:] == 0).all() and buf[:B, w:].shape[1] >= 4
    assert torch.isnan(buf[B]).all()
    # the same through ld_out alone
    out2 = ops.dot_interact_fwd(dense, emb, F, D, self_i, ld_out=ld_out)
    assert out2.stride(0) == ld_out and _bits_equal(out2, out)
    d_out = torch.full((B, ld_out), nan, device="cuda")[:, :w]
    d_out.copy_(_cuda(c["d_out"]))
    demb_buf = torch.full((B + 1, ld_emb), nan, device="cuda")
    dd_buf = torch.full((B + 1, D + 8), nan, device="cuda") if has_dense else None
    d_dense, d_emb = ops.dot_interact_bwd(dense, emb, F, D, d_out, self_i, d_dense=dd_buf[:B, :D] if has_dense else None,
                                          d_emb=demb_buf[:B, :F * D])
    want = _bwd(shape)
    assert torch.isfinite(d_emb).all() and _bits_equal(d_emb, want[1])
    assert torch.isnan(demb_buf[:B, F * D:]).all() and torch.isnan(demb_buf[B]).all()         # untouched beyond F * D and beyond B
    if has_dense:
        assert torch.isfinite(d_dense).all() and _bits_equal(d_dense, want[0])
        assert torch.isnan(dd_buf[:B, D:]).all() and torch.isnan(dd_buf[B]).all()


def test_argument_errors_and_the_empty_batch():
    from deep_recommenders_amd import _lib, ops
    z = lambda *s: torch.zeros(s, device="cuda")                                              # noqa: E731
    with pytest.raises(ValueError):                                                           # D = 6
        ops.dot_interact_fwd(z(2, 6), z(2, 3 * 6), 3, 6)
    with pytest.raises(ValueError):                                                           # D = 260
        ops.dot_interact_fwd(z(2, 260), z(2, 2 * 260), 2, 260)
    with pytest.raises(ValueError):                                                           # N = 1
        ops.dot_interact_fwd(None, z(2, 8), 1, 8)
    with pytest.raises(ValueError):                                                           # N = 65
        ops.dot_interact_fwd(z(2, 4), z(2, 64 * 4), 64, 4)
    with pytest.raises(ValueError):                                                           # ld_emb = 25
        ops.dot_interact_fwd(z(2, 8), z(2, 25)[:, :24], 3, 8)
    with pytest.raises(ValueError):                                                           # ld_out = 14 for 8 + 6 columns
        ops.dot_interact_fwd(z(2, 8), z(2, 24), 3, 8, ld_out=14)
    with pytest.raises(ValueError):                                                           # ld_dout = 14
        ops.dot_interact_bwd(z(2, 8), z(2, 24), 3, 8, z(2, 14))
    with pytest.raises(ValueError):
        ops.dot_interact_bwd(z(2, 6), z(2, 18), 3, 6, z(2, 12))
    with pytest.raises(ValueError):
        ops.dot_interact_bwd(None, z(2, 8), 1, 8, z(2, 4))
    # the entry points themselves: DR_EINVAL before anything is launched
    L, p, s = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    dense, emb, out = z(2, 8), z(2, 24), z(2, 16)
    assert L.dr_dot_interact_fwd(p(dense), 8, p(emb), 24, 2, 3, 8, 0, p(out), 16, s) == _lib.DR_OK
    for ld_dense, ld_emb, F, D, self_i, ld_out in ((8, 24, 3, 6, 0, 16), (8, 24, 3, 260, 0, 16), (8, 24, 64, 8, 0, 16), (8, 25, 3, 8, 0, 16),
                                                  (8, 20, 3, 8, 0, 16), (4, 24, 3, 8, 0, 16), (8, 24, 3, 8, 0, 12), (8, 24, 3, 8, 0, 15),
                                                  (8, 24, 3, 8, 2, 16)):
        assert L.dr_dot_interact_fwd(p(dense), ld_dense, p(emb), ld_emb, 2, F, D, self_i, p(out), ld_out, s) == _lib.DR_EINVAL
    assert L.dr_dot_interact_fwd(None, 0, p(emb), 8, 2, 1, 8, 0, p(out), 16, s) == _lib.DR_EINVAL                 # N = 1
    assert L.dr_dot_interact_fwd(p(dense), 8, p(emb), 24, -1, 3, 8, 0, p(out), 16, s) == _lib.DR_EINVAL
    assert L.dr_dot_interact_bwd(p(dense), 8, p(emb), 24, p(out), 16, 2, 3, 8, 0, None, 8, p(z(2, 24)), 24, s) == _lib.DR_EINVAL
    assert L.dr_dot_interact_bwd(p(dense), 8, p(emb), 24, p(out), 16, 2, 3, 8, 0, p(z(2, 8)), 8, p(z(2, 24)), 20, s) == _lib.DR_EINVAL
    # B = 0: empty tensors, nothing launched
    out = ops.dot_interact_fwd(z(0, 8), z(0, 24), 3, 8)
    assert out.shape == (0, 8 + 6)
    d_dense, d_emb = ops.dot_interact_bwd(z(0, 8), z(0, 24), 3, 8, z(0, 14))
    assert d_dense.shape == (0, 8) and d_emb.shape == (0, 24)
    assert ops.dot_interact_fwd(None, z(0, 3, 8), 3, 8, True).shape == (0, 6)
    assert L.dr_dot_interact_fwd(None, 0, None, 24, 0, 3, 8, 0, None, 4, s) == _lib.DR_OK


def test_no_batch_sized_square_buffer():
    """N = 64, D = 4: the [B, N, N] matrix would be twice the output; neither call allocates beyond its results"""
    from deep_recommenders_amd import ops
    B, F, D = 256, 63, 4
    dense, emb = torch.randn((B, D), device="cuda"), torch.randn((B, F * D), device="cuda")
    w = ops.dot_interact_width(F, D)
    d_out = torch.randn((B, w), device="cuda")
    ops.dot_interact_fwd(dense, emb, F, D)                                                     # code objects loaded before measuring
    ops.dot_interact_bwd(dense, emb, F, D, d_out)
    torch.cuda.synchronize()
    square = B * 64 * 64 * 4
    for fn, results in ((lambda: ops.dot_interact_fwd(dense, emb, F, D), B * w * 4),
                        (lambda: ops.dot_interact_bwd(dense, emb, F, D, d_out), B * (F + 1) * D * 4)):
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        keep = fn()
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
        assert grown < results + 4096 < square, (grown, results, square)
        del keep


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[5], SHAPES[9]])
def test_autograd_glue_equals_the_backward_entry_point(shape):
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd.keras.models.ranking import DotInteraction
    c = _case(shape)
    B, F, D, has_dense, self_i = shape
    emb = _cuda(c["emb"]).requires_grad_(True)                                                # [B, F, D]
    dense = _cuda(c["dense"]).requires_grad_(True) if has_dense else None
    out = L.dot_interaction(dense, emb, self_i)
    assert _bits_equal(out, _fwd(shape))
    g = _cuda(c["d_out"])                                                                     # contiguous: the glue pads its rows itself
    got = torch.autograd.grad(out, [emb] + ([dense] if has_dense else []), grad_outputs=g)
    want = _bwd(shape)
    assert got[0].shape == (B, F, D) and _bits_equal(got[0].reshape(B, F * D), want[1])
    if has_dense:
        assert _bits_equal(got[1], want[0])
        emb2 = _cuda(c["emb"]).reshape(B, F * D)                                              # the slab's concat layout, D from dense
        assert _bits_equal(L.dot_interaction(dense.detach(), emb2, self_i), out)
    layer = DotInteraction(self_i)
    assert _bits_equal(layer(emb.detach(), dense.detach() if has_dense else None), out)
    assert _bits_equal(layer.call(c["emb"].to(torch.float32).numpy(), None if not has_dense else c["dense"].to(torch.float32).numpy()), out)


def _dense_bound(x, W):
    """test_gpu_xdeepfm.py's convention for one fp32 matrix product: 2e-6 max|x| max|W| sqrt(K)"""
    return 2e-6 * (x.abs().max() * W.abs().max()).item() * np.sqrt(W.shape[0])


def _tower_error(x, Ws, bs, err, last_linear):
    """max-abs error after a Dense tower whose input is off by `err`: every layer multiplies an incoming error by at most
    max_n sum_k |W_kn| (relu is 1-Lipschitz) and adds its own product's bound"""
    for k, (W, b) in enumerate(zip(Ws, bs)):
        err = err * W.abs().sum(0).max().item() + _dense_bound(x, W)
        x = x @ W + b
        if not (last_linear and k == len(Ws) - 1):
            x = torch.relu(x)
    return x, err


def _logit_atol(e, x, bWs, bbs, tWs, tbs, self_i):
    """sum of the per-stage bounds, each carried through the stages after it"""
    D = e.shape[2]
    bottom, err = (None, 0.0) if x is None else _tower_error(x, bWs, bbs, 0.0, False)
    T = R.stack(bottom, e).abs()
    # <t_i, t_0 + d> - <t_i, t_0> <= |d|_inf |t_i|_1 (twice and squared on the diagonal); then the interaction's own bound
    err_z = err * 2 * T.sum(-1).max().item() + D * err * err + ((D + 2) * U * torch.einsum("bid,bjd->bij", T, T)).max().item()
    z = R.dot_interaction(bottom, e, self_i)
    return _tower_error(z, tWs, tbs, max(err, err_z), True)[1]


@pytest.mark.parametrize("has_dense", [True, False])
def test_dlrm_model(has_dense):
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.keras.models.ranking import DLRM
    torch.manual_seed(0)
    rng = np.random.default_rng(4)
    B, F, D, Nd, V = 33, 5, 8, 13, 50
    cols = [fc.embedding_column(fc.categorical_column_with_identity("c%d" % i, V), D) for i in range(F)]
    self_i = not has_dense                                                                     # both triangles are exercised
    model = DLRM(cols, bottom_units_size=[16, 8], top_units_size=[16], dense_features_key="dense" if has_dense else None,
                 self_interaction=self_i)
    inputs = {"c%d" % i: rng.integers(0, V, size=(B, 1)) for i in range(F)}
    if has_dense:
        inputs["dense"] = np.log1p(np.abs(rng.standard_normal((B, Nd)))).astype(np.float32)
    logits = model.logits(inputs)
    assert logits.shape == (B, 1)
    with torch.no_grad():                                                                     # biases start at zero: give them values
        for b in list(model.bottom_biases) + list(model.top_biases):
            b.normal_(0, 0.1)
    logits = model.logits(inputs)
    n = F + int(has_dense)
    width = (D if has_dense else 0) + (n * (n + 1) // 2 if self_i else n * (n - 1) // 2)
    assert [tuple(k.shape) for k in model.top_kernels] == [(width, 16), (16, 1)]
    assert [tuple(k.shape) for k in model.bottom_kernels] == ([(Nd, 16), (16, 8)] if has_dense else [])
    # the restatement with the same parameters, float64
    leaf = lambda t: t.detach().double().cpu().requires_grad_(True)                           # noqa: E731
    ids = np.concatenate([inputs["c%d" % i] for i in range(F)], axis=1) + np.asarray([model.slab.base["c%d" % i] for i in range(F)])
    table = leaf(model.slab.table)
    bWs, bbs = [leaf(k) for k in model.bottom_kernels], [leaf(k) for k in model.bottom_biases]
    tWs, tbs = [leaf(k) for k in model.top_kernels], [leaf(k) for k in model.top_biases]
    e = table[torch.from_numpy(ids)]                                                          # [B, F, D]
    x = torch.from_numpy(inputs["dense"]).double() if has_dense else None
    want = R.dlrm_logits(e, x, bWs, bbs, tWs, tbs, 1, self_i)
    with torch.no_grad():
        atol = _logit_atol(e, x, bWs, bbs, tWs, tbs, self_i)
    err = (logits.detach().double().cpu() - want.detach()).abs().max().item()
    print("DLRM logits (dense %s): max |err| = %.3g, atol = %.3g" % (has_dense, err, atol))
    np.testing.assert_allclose(logits.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-5, atol=atol)
    # parameter gradients of sum(logits * gy)
    gy = torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32))
    logits.backward(gy.cuda())
    leaves = [table] + bWs + bbs + tWs + tbs
    grads = torch.autograd.grad((want * gy.double()).sum(), leaves)
    got = [model.slab.table.grad] + [k.grad for k in list(model.bottom_kernels) + list(model.bottom_biases) + list(model.top_kernels)
                                     + list(model.top_biases)]
    assert all(g is not None for g in got)
    for k, (g, w) in enumerate(zip(got, grads)):
        w = w.numpy()
        np.testing.assert_allclose(g.cpu().numpy(), w, rtol=2e-4, atol=2e-5 * np.abs(w).max(), err_msg="gradient %d" % k)
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
    assert model.get_config()["self_interaction"] is self_i
