"""GPU tests of xDeepFM on the fused CIN + sum-pooling kernels (csrc/cin_pool.hip): the two entry points against the float64 restatement
(tests/xdeepfm_ref.py) and float64 autograd, bit-reproducibility, independence of an example from its batch, agreement with the
existing dr_cin_fwd / dr_cin_bwd, the argument errors, and CINNetwork / XDeepFM end to end.

Tolerances are those of test_gpu_cin_din.py::test_cin_forward_backward_match_oracle for the same arithmetic: out rtol 1e-5, atol
2e-6 * scale with scale = max|x0| max|x| max|W| sqrt(H0 Hk); pooled sums D such values, so its atol is D times that (triangle
inequality); gradients rtol 2e-4, atol 2e-5 * max|ref|."""
import functools

import numpy as np
import pytest
import torch

import xdeepfm_ref as R

pytestmark = pytest.mark.gpu

DD = torch.float64
# (B, H0, Hk, D, Fm)
SHAPES = [(10, 12, 12, 10, 3),       # the reference test's shape; D does not divide 64, Fm < 32
          (33, 7, 5, 16, 70),        # odd Hk (k-pair tail); Fm over two 64-groups, not a multiple of 32; H0 Hk = 35
          (5, 3, 9, 64, 33),         # D = 64
          (3, 4, 6, 80, 5),          # D > 64, not a multiple of 32
          (64, 39, 40, 8, 100),      # workload field counts
          (1, 1, 1, 1, 1),           # smallest possible
          (2, 3, 200, 4, 7),         # Hk = 200: seven j-tiles
          (15, 2, 3, 10, 5)]         # 150 rows: the dW reduction runs over three partials, the last of 22 rows
SPLIT_SHAPE = SHAPES[-1]


def _cuda(a):
    return None if a is None else a.to(torch.float32).cuda()


@functools.lru_cache(maxsize=None)
def _case(shape, act, bias):
    """inputs (float32 values held in float64), the float64 forward and the tolerances; computed once per case, never modified"""
    B, H0, Hk, D, Fm = shape
    rng = np.random.default_rng(1000 * SHAPES.index(shape) + 10 * act + int(bias))
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DD)         # noqa: E731
    x0, x, W = t(B, H0, D), t(B, Hk, D), t(H0 * Hk, Fm) * 0.2
    W = W.to(torch.float32).to(DD)
    b = t(Fm) if bias else None
    d_out, d_pooled = t(B, Fm, D), t(B, Fm)
    out, pooled = R.cin_pool(x0, x, W, b, act)
    scale = (x0.abs().max() * x.abs().max() * W.abs().max()).item() * np.sqrt(H0 * Hk)
    return dict(x0=x0, x=x, W=W, b=b, d_out=d_out, d_pooled=d_pooled, out=out, pooled=pooled, atol=2e-6 * scale)


def _autograd(c, act, use_out, use_pooled):
    leaves = [c[k].clone().requires_grad_(True) for k in ("x0", "x", "W")] + ([c["b"].clone().requires_grad_(True)] if c["b"] is not None else [])
    out, pooled = R.cin_pool(leaves[0], leaves[1], leaves[2], leaves[3] if c["b"] is not None else None, act)
    loss = (out * c["d_out"]).sum() * (1 if use_out else 0) + (pooled * c["d_pooled"]).sum() * (1 if use_pooled else 0)
    return torch.autograd.grad(loss, leaves)


def _check_grads(got, want, what):
    for name, g, w in zip(("d_x0", "d_x", "dW", "dbias"), got, want):
        w = w.numpy()
        np.testing.assert_allclose(g.cpu().numpy(), w, rtol=2e-4, atol=2e-5 * np.abs(w).max(), err_msg="%s (%s)" % (name, what))


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward(shape, act, bias):
    from deep_recommenders_amd import ops
    c = _case(shape, act, bias)
    D = shape[3]
    x0, x, W, b = _cuda(c["x0"]), _cuda(c["x"]), _cuda(c["W"]), _cuda(c["b"])
    out, pooled = ops.cin_pool_fwd(x0, x, W, b, act)
    np.testing.assert_allclose(out.cpu().numpy(), c["out"].numpy(), rtol=1e-5, atol=c["atol"])
    np.testing.assert_allclose(pooled.cpu().numpy(), c["pooled"].numpy(), rtol=1e-5, atol=D * c["atol"])
    none, pooled_only = ops.cin_pool_fwd(x0, x, W, b, act, want_out=False)
    assert none is None and _bits_equal(pooled_only, pooled)
    out_only, none = ops.cin_pool_fwd(x0, x, W, b, act, want_pooled=False)
    assert none is None and _bits_equal(out_only, out)
    again = ops.cin_pool_fwd(x0, x, W, b, act)                                                # run to run
    assert _bits_equal(again[0], out) and _bits_equal(again[1], pooled)
    old = ops.cin_fwd(x0, x, W, b, act)                                                       # the existing kernel
    np.testing.assert_allclose(out.cpu().numpy(), old.cpu().numpy(), rtol=1e-5, atol=c["atol"])


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward(shape, act, bias):
    from deep_recommenders_amd import ops
    c = _case(shape, act, bias)
    x0, x, W, b = _cuda(c["x0"]), _cuda(c["x"]), _cuda(c["W"]), _cuda(c["b"])
    d_out, d_pooled = _cuda(c["d_out"]), _cuda(c["d_pooled"])
    out, _ = ops.cin_pool_fwd(x0, x, W, b, act)
    both = None
    for use_out, use_pooled in ((True, True), (True, False), (False, True)):
        got = ops.cin_pool_bwd(x0, x, W, act, out, d_out if use_out else None, d_pooled if use_pooled else None, want_bias=bias)
        _check_grads(got, _autograd(c, act, use_out, use_pooled), "d_out %s, d_pooled %s" % (use_out, use_pooled))
        if use_out and use_pooled:
            both = got
        if use_out and not use_pooled:                                                        # the existing kernels on the same inputs
            old = ops.cin_bwd(x0, x, W, act, out, d_out, want_bias=bias)
            _check_grads(got, [o.double().cpu() for o in old if o is not None], "against dr_cin_bwd")
    again = ops.cin_pool_bwd(x0, x, W, act, out, d_out, d_pooled, want_bias=bias)              # run to run, dW and dbias included
    assert all(_bits_equal(a, g) for a, g in zip(again, both) if g is not None)
    want = _autograd(c, act, True, True)
    prefill = torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(x0.shape)).astype(np.float32)).cuda()
    acc = ops.cin_pool_bwd(x0, x, W, act, out, d_out, d_pooled, want_bias=bias, d_x0=prefill.clone())
    ref = prefill.double().cpu() + want[0]
    np.testing.assert_allclose(acc[0].cpu().numpy(), ref.numpy(), rtol=2e-4, atol=2e-5 * np.abs(ref.numpy()).max(), err_msg="accumulate_x0")
    assert all(_bits_equal(a, g) for a, g in zip(acc[1:], both[1:]) if g is not None)
    if act == 0:                                                                              # out is not read for a linear layer
        no_out = ops.cin_pool_bwd(x0, x, W, 0, None, d_out, d_pooled, want_bias=bias)
        assert all(_bits_equal(a, g) for a, g in zip(no_out, both) if g is not None)


def test_split_shape_really_splits_the_dw_reduction():
    from deep_recommenders_amd import ops
    B, H0, Hk, D, Fm = SPLIT_SHAPE
    parts = ops.cin_pool_bwd_partials(B, H0, Hk, D, Fm)
    assert parts >= 3
    assert parts == -(-B * D // 64) and (B * D) % 64 != 0                                     # 64-row tiles each, the last one partial


@pytest.mark.parametrize("act", [0, 2])
def test_an_example_does_not_depend_on_its_batch(act):
    """the first 7 examples of the B = 33 case equal, bit for bit, a call on those 7 alone: a block owns whole examples"""
    from deep_recommenders_amd import ops
    c = _case(SHAPES[1], act, True)
    x0, x, W, b = _cuda(c["x0"]), _cuda(c["x"]), _cuda(c["W"]), _cuda(c["b"])
    d_out, d_pooled = _cuda(c["d_out"]), _cuda(c["d_pooled"])
    out, pooled = ops.cin_pool_fwd(x0, x, W, b, act)
    d_x0, d_x, _, _ = ops.cin_pool_bwd(x0, x, W, act, out, d_out, d_pooled)
    n = 7
    out7, pooled7 = ops.cin_pool_fwd(x0[:n], x[:n], W, b, act)
    d_x07, d_x7, _, _ = ops.cin_pool_bwd(x0[:n], x[:n], W, act, out7, d_out[:n], d_pooled[:n])
    for name, part, whole in (("out", out7, out), ("pooled", pooled7, pooled), ("d_x0", d_x07, d_x0), ("d_x", d_x7, d_x)):
        assert _bits_equal(part, whole[:n].contiguous()), name


def test_argument_errors():
    from deep_recommenders_amd import _lib, ops
    dev = "cuda"
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)                            # noqa: E731
    x0, x, W = z(2, 3, 4), z(2, 5, 4), z(15, 6)
    out, pooled = ops.cin_pool_fwd(x0, x, W)
    d_out, d_pooled = z(2, 6, 4), z(2, 6)
    for act in (-1, 4):
        with pytest.raises(RuntimeError, match="DR_EINVAL"):
            ops.cin_pool_fwd(x0, x, W, None, act)
        with pytest.raises(RuntimeError, match="DR_EINVAL"):
            ops.cin_pool_bwd(x0, x, W, act, out, d_out, d_pooled)
    with pytest.raises(RuntimeError, match="DR_EINVAL"):
        ops.cin_pool_fwd(x0, x, W, want_out=False, want_pooled=False)
    with pytest.raises(RuntimeError, match="DR_EINVAL"):
        ops.cin_pool_bwd(x0, x, W, 0, out, None, None)
    with pytest.raises(RuntimeError, match="DR_EINVAL"):
        ops.cin_pool_bwd(x0, x, W, 2, None, d_out, d_pooled)                                  # out may be absent only for act 0
    with pytest.raises(RuntimeError, match="DR_EINVAL"):
        ops.cin_pool_bwd(x0, x, W, 0, out, d_out, d_pooled, workspace=z(16))                  # short workspace
    # null required pointers and bad sizes, straight at the C entry points (every other pointer is a valid device address)
    L, p, s = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    d_x0, d_x, dW = z(2, 3, 4), z(2, 5, 4), z(15, 6)
    ws = z(L.dr_cin_pool_bwd_workspace_bytes(2, 3, 5, 4, 6) // 4)
    fwd = [p(x0), p(x), 2, 3, 5, 4, p(W), 6, None, 0, p(out), p(pooled), s]
    bwd = [p(x0), p(x), 2, 3, 5, 4, p(W), 6, 0, p(out), p(d_out), p(d_pooled), p(d_x0), 0, p(d_x), p(dW), None, p(ws), ws.numel() * 4, s]
    assert L.dr_cin_pool_fwd(*fwd) == _lib.DR_OK and L.dr_cin_pool_bwd(*bwd) == _lib.DR_OK
    for fn, args, what, null_at, size_at in ((L.dr_cin_pool_fwd, fwd, "dr_cin_pool_fwd", (0, 1, 6), (2, 3, 4, 5, 7)),
                                             (L.dr_cin_pool_bwd, bwd, "dr_cin_pool_bwd", (0, 1, 6, 12, 14, 15, 17), (2, 3, 4, 5, 7))):
        for k in null_at:
            with pytest.raises(RuntimeError, match="DR_EINVAL"):
                _lib.check(fn(*(args[:k] + [None] + args[k + 1:])), what)
        for k in size_at:
            for bad in ((-1,) if k == 2 else (-1, 0)):
                with pytest.raises(RuntimeError, match="DR_EINVAL"):
                    _lib.check(fn(*(args[:k] + [bad] + args[k + 1:])), what)
    # the LDS staging limit: (H0 + Hk) fields of 64 rows do not fit 160 KB
    x0, x, W = z(1, 400, 1), z(1, 300, 1), z(120000, 1)
    with pytest.raises(RuntimeError, match="DR_ESHAPE"):
        ops.cin_pool_fwd(x0, x, W)
    with pytest.raises(RuntimeError, match="DR_ESHAPE"):
        ops.cin_pool_bwd(x0, x, W, 0, None, None, z(1, 1))
    # B == 0 launches nothing
    e_out, e_pooled = ops.cin_pool_fwd(z(0, 3, 4), z(0, 5, 4), z(15, 6))
    assert e_out.shape == (0, 6, 4) and e_pooled.shape == (0, 6)
    ops.cin_pool_bwd(z(0, 3, 4), z(0, 5, 4), z(15, 6), 0, None, None, z(0, 6))


@pytest.mark.parametrize("activation", [None, "sigmoid"])
def test_cin_network_matches_the_ref_and_float64_autograd(activation):
    from deep_recommenders_amd import ops
    from deep_recommenders_amd.keras.models.ranking import CINNetwork
    rng = np.random.default_rng(11)
    x0 = torch.from_numpy(rng.standard_normal((9, 4, 8)).astype(np.float32)).cuda().requires_grad_(True)
    net = CINNetwork((6, 5), activation=activation, use_bias=True, kernel_init=lambda t: t.normal_(0, 0.3), bias_init=lambda t: t.normal_(0, 0.3))
    y = net(x0)
    assert y.shape == (9, 11)
    gy = torch.from_numpy(rng.standard_normal((9, 11)).astype(np.float32)).cuda()
    y.backward(gy)
    act = ops.ACT_CODES[activation]
    X0 = x0.detach().double().cpu().requires_grad_(True)
    Ws = [k.detach().double().cpu().requires_grad_(True) for k in net.kernels]
    bs = [k.detach().double().cpu().requires_grad_(True) for k in net.biases]
    want = R.cin_network(X0, Ws, bs, act)
    scale = (X0.abs().max() ** 2 * max(w.abs().max() for w in Ws)).item() * np.sqrt(4 * 6)
    # a second-layer input carries the first layer's error; 8 values are pooled
    np.testing.assert_allclose(y.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-5, atol=8 * 2e-6 * scale * (1 + scale))
    grads = torch.autograd.grad((want * gy.double().cpu()).sum(), [X0] + Ws + bs)
    got = [x0.grad] + [k.grad for k in net.kernels] + [k.grad for k in net.biases]
    assert all(g is not None for g in got)
    for k, (g, w) in enumerate(zip(got, grads)):
        w = w.numpy()
        np.testing.assert_allclose(g.cpu().numpy(), w, rtol=2e-4, atol=2e-5 * np.abs(w).max(), err_msg="gradient %d" % k)


def test_xdeepfm_model():
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.keras.models.ranking import XDeepFM
    torch.manual_seed(0)
    rng = np.random.default_rng(2)
    B, F, D = 32, 4, 8
    base = [fc.categorical_column_with_identity("c%d" % i, 50) for i in range(F)]
    ind, emb = [fc.indicator_column(c) for c in base], [fc.embedding_column(c, D) for c in base]
    model = XDeepFM(ind, emb, cin_layer_sizes=[6, 5], dnn_units_size=[16])
    inputs = {"c%d" % i: rng.integers(0, 50, size=(B, 1)) for i in range(F)}
    labels = torch.from_numpy(rng.integers(0, 2, size=(B, 1)).astype(np.float32)).cuda()
    with torch.no_grad():                                                                     # the linear term starts at zero: give it values
        model.slab.lin_w.normal_(0, 0.1)
        model.slab.lin_bias.fill_(0.05)
    logits = model.logits(inputs)
    assert logits.shape == (B, 1)
    # the ref with the same parameters, float64
    cpu = lambda t: t.detach().double().cpu()                                                 # noqa: E731
    ids = np.concatenate([inputs["c%d" % i] for i in range(F)], axis=1) + np.asarray([model.slab.base["c%d" % i] for i in range(F)])
    table, lin_w = cpu(model.slab.table), cpu(model.slab.lin_w)
    e = table[torch.from_numpy(ids)]                                                          # [B, F, D]
    linear = lin_w[torch.from_numpy(ids)].sum(1) + cpu(model.slab.lin_bias)
    cin_Ws = [cpu(k) for k in model.cin.kernels]
    want = R.xdeepfm_logits(e, linear, cin_Ws, [None, None], 0, cpu(model.w_cin), [cpu(k) for k in model.dnn_kernels],
                            [cpu(k) for k in model.dnn_biases], 1)
    # the forward tolerance, scaled by the logit's own terms: each pooled CIN value (D sums of H0 Hk products, twice) times |w_cin|,
    # plus the DNN's two matrix products at float32
    cin_scale = (e.abs().max() ** 2 * max(w.abs().max() for w in cin_Ws)).item() * np.sqrt(F * 6)
    cin_atol = D * 2e-6 * cin_scale * (1 + cin_scale) * cpu(model.w_cin).abs().sum().item()
    dnn_atol = 2e-6 * (e.abs().max() * max(cpu(k).abs().max() for k in model.dnn_kernels)).item() * np.sqrt(F * D) * 16
    np.testing.assert_allclose(logits.detach().cpu().numpy(), want.numpy(), rtol=1e-5, atol=cin_atol + dnn_atol + 1e-6)

    def loss_fn():
        return torch.nn.functional.binary_cross_entropy(model(inputs), labels)
    l0 = loss_fn()
    l0.backward()
    params = dict(model.named_parameters())
    assert {"slab.table", "slab.lin_w", "slab.lin_bias", "w_cin", "cin.kernels.0", "cin.kernels.1"} <= set(params)
    for name, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert model.slab.table.grad.abs().sum().item() > 0
    with torch.no_grad():
        for p in params.values():
            p -= 0.1 * p.grad
    assert loss_fn().item() < l0.item()
    prob = model.predict(inputs)
    assert prob.shape == (B, 1) and ((prob > 0) & (prob < 1)).all()
    cfg = model.get_config()
    assert cfg["cin_layer_sizes"] == [6, 5] and cfg["dnn_units_size"] == [16] and cfg["cin_activation"] is None
