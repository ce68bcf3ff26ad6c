"""The kernels of csrc/din.hip (Dice, the fused interest pooling) and the layers on them, against the float64 restatement of
tests/din_ref.py.

Tolerance of every comparison with float64: the yardstick is the error of the SAME restatement evaluated in fp32 on the CPU against
its float64 self, per result tensor and relative to that tensor's largest magnitude; the device may differ from float64 by at most
max(8 x yardstick, 2e-6) x max|ref|.  The factor 8 covers what the kernels do differently from the fp32 restatement (the folded
per-example weight, the MFMA's accumulation order, fixed-order block reductions); the floor is a few fp32 roundings of the largest
element.  The yardstick never comes from the kernel.  Each comparison prints err / tol."""
import functools

import numpy as np
import pytest
import torch

import din_ref as R

pytestmark = pytest.mark.gpu

ACTS = {"linear": 0, "relu": 1, "sigmoid": 2, "tanh": 3, "dice": 4}


def _mods():
    from deep_recommenders_amd import layers, ops
    from deep_recommenders_amd.keras.models.ranking import din
    return ops, layers, din


def _check(name, got, ref64, ref32):
    got = got.detach().cpu().to(torch.float64)
    ref64 = ref64.detach().to(torch.float64).reshape(got.shape)
    ref32 = ref32.detach().to(torch.float64).reshape(got.shape)
    assert torch.isfinite(got).all(), name
    scale = ref64.abs().max().item()
    yard = (ref32 - ref64).abs().max().item() / scale if scale > 0 else 0.0
    tol = max(8.0 * yard, 2e-6) * scale
    err = (got - ref64).abs().max().item()
    print("%-28s max|ref| %.3e  yardstick %.2e  err %.3e  err/tol %.3f" % (name, scale, yard, err, err / tol if tol > 0 else float(err > 0)))
    assert err <= tol, "%s: err %.3e > tol %.3e (yardstick %.2e)" % (name, err, tol, yard)


def _view2(x, extra):
    """[M, N] fp32 on the device as a view of a [M, N + extra] buffer whose padding is NaN"""
    M, N = x.shape
    buf = torch.full((M, N + extra), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :N] = x.to(torch.float32).cuda()
    return buf[:, :N]


def _view3(x, extra):
    B, T, D = x.shape
    buf = torch.full((B, T, D + extra), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :, :D] = x.to(torch.float32).cuda()
    return buf[:, :, :D]


# ---------------------------------------------------------------------------------------------------------------------------------
# Dice
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-7, 1e-8, 1e-9, 1e-10])
def test_dice_known_answer_of_the_reference_test(eps):
    """tests/keras/test_din.py:50-64 of the reference on the device, through the layer; assertAllClose's default tolerance"""
    _, _, din = _mods()
    inputs = np.asarray([[-0.2, -0.1, 0.1, 0.2]]).astype(np.float32)
    p = (inputs - inputs.mean()) / np.sqrt(inputs.std() + eps)
    p = 1 / (1 + np.exp(-p))
    x = np.where(inputs > 0, inputs, np.zeros_like(inputs))
    expected = np.where(x > 0, p * x, (1 - p) * x)
    got = din.Dice(epsilon=eps)(inputs).detach().cpu().numpy()
    np.testing.assert_allclose(got, expected, rtol=1e-6, atol=1e-6)


def _dice_case(case):
    if case == "const_rows":
        rng = np.random.default_rng(99)
        x = rng.normal(size=(6, 10))
        x[1, :] = 0.75
        x[4, :] = 0.0
    else:
        rng = np.random.default_rng(case[0] * 1009 + case[1])
        x = rng.normal(size=case)
    M, N = x.shape
    return x.astype(np.float32), (rng.normal(size=N) * 0.5).astype(np.float32), rng.normal(size=(M, N)).astype(np.float32)


@pytest.mark.parametrize("case", [(3, 4), (65, 10), (33, 80), (7, 129), (5, 1000), (4099, 36), (1, 1), "const_rows"], ids=str)
def test_dice_forward_backward(case):
    """(4099, 36) crosses the two-stage dalpha reduction; (1, 1) and the constant rows exercise the s == 0 rule; the inputs are views
    with a pitch above N whose padding is NaN; everything runs twice"""
    ops, _, _ = _mods()
    x, alpha, dy = _dice_case(case)
    eps = 1e-8
    refs = {}
    for dtype in (torch.float64, torch.float32):
        X = torch.from_numpy(x).to(dtype).requires_grad_(True)
        A = torch.from_numpy(alpha).to(dtype).requires_grad_(True)
        y = R.dice(X, A, eps)
        y.backward(torch.from_numpy(dy).to(dtype))
        refs[dtype] = (y.detach(), X.grad, A.grad)
    xd, dyd, ad = _view2(torch.from_numpy(x), 3), _view2(torch.from_numpy(dy), 5), torch.from_numpy(alpha).cuda()
    y1 = ops.dice_fwd(xd, ad, eps)
    dx1, da1 = ops.dice_bwd(xd, ad, dyd, eps)
    y2 = ops.dice_fwd(xd, ad, eps)
    dx2, da2 = ops.dice_bwd(xd, ad, dyd, eps)
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2) and torch.equal(da1, da2), "two runs differ"
    for name, got, i in (("y", y1, 0), ("dx", dx1, 1), ("dalpha", da1, 2)):
        _check("dice %s %s" % (case, name), got, refs[torch.float64][i], refs[torch.float32][i])


# ---------------------------------------------------------------------------------------------------------------------------------
# ActivationUnit with the new activations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["dice", "sigmoid"])
def test_activation_unit_with_dice_and_sigmoid(activation):
    _, _, din = _mods()
    rng = np.random.default_rng(3)
    x0, y0 = rng.normal(size=(64, 8)).astype(np.float32), rng.normal(size=(64, 8)).astype(np.float32)
    x = torch.from_numpy(x0).cuda().requires_grad_(True)
    y = torch.from_numpy(y0).cuda().requires_grad_(True)
    act = din.Dice() if activation == "dice" else activation
    unit = din.ActivationUnit(16, interacter=din.Subtract(), activation=act)
    unit(x, y)
    with torch.no_grad():
        unit.dense_kernel_b.normal_(0, 0.1)
        unit.dense_kernel_w.mul_(6.0)
        unit.dense_output_w.mul_(6.0)
        if activation == "dice":
            unit.dice.alpha.normal_(0, 0.5)
    names = ["dense_kernel_w", "dense_kernel_b", "dense_output_w", "dense_output_b"]
    params = [getattr(unit, n) for n in names] + ([unit.dice.alpha] if activation == "dice" else [])
    assert all(any(p is q for q in unit.parameters()) for p in params), "the Dice instance's alpha must be a parameter of the unit"
    g = torch.from_numpy(rng.normal(size=(64, 1)).astype(np.float32))
    out = unit(x, y)
    out.backward(g.cuda())
    refs = {}
    for dtype in (torch.float64, torch.float32):
        X, Y = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (x0, y0))
        P = [p.detach().cpu().to(dtype).requires_grad_(True) for p in params]
        h = torch.cat([X, Y, X - Y], 1) @ P[0] + P[1]
        h = R.dice(h, P[4], 1e-8) if activation == "dice" else torch.sigmoid(h)
        o = h @ P[2] + P[3]
        o.backward(g.to(dtype))
        refs[dtype] = [o.detach(), X.grad, Y.grad] + [p.grad for p in P]
    got = [out, x.grad, y.grad] + [p.grad for p in params]
    for name, gt, r64, r32 in zip(["out", "dx", "dy"] + names + ["alpha"], got, refs[torch.float64], refs[torch.float32]):
        _check("unit[%s] %s" % (activation, name), gt, r64, r32)


# ---------------------------------------------------------------------------------------------------------------------------------
# Interest pooling
# ---------------------------------------------------------------------------------------------------------------------------------
POOL_CASES = {
    "b1_t1_d4_u1_none_relu": (1, 1, 4, 1, 0, "relu", True, "lengths"),
    "b3_t7_d20_u10_sub_relu": (3, 7, 20, 10, 1, "relu", True, "lengths"),
    "b65_t50_d64_u36_mul_dice": (65, 50, 64, 36, 2, "dice", True, "lengths"),
    "b5_t33_d128_u128_sub_dice": (5, 33, 128, 128, 1, "dice", True, "lengths"),
    "b4_t17_d8_u80_mul_sigmoid_holes": (4, 17, 8, 80, 2, "sigmoid", True, "holes"),
    "b2_t200_d16_u5_sub_tanh": (2, 200, 16, 5, 1, "tanh", True, "lengths"),
    "b3_t5_d12_u7_mul_dice_nobias": (3, 5, 12, 7, 2, "dice", False, "lengths"),
}
RESULTS = ["out", "scores", "d_query", "d_keys", "dW", "db", "d_w_out", "d_b_out", "dalpha"]


def _pool_mask(rng, B, T, kind):
    """example 0 is empty and example 1 full (where there are that many); partial lengths elsewhere, or holes in the middle"""
    if kind == "holes":
        m = rng.random((B, T)) < 0.6
    else:
        lengths = rng.integers(1, max(2, T), size=B)
        m = np.arange(T)[None, :] < lengths[:, None]
    if B >= 2:
        m[0, :] = False
        m[1, :] = True
    else:
        m[:] = True
    return m


@functools.lru_cache(maxsize=None)
def _pool_case(name):
    """inputs (fp32 values, as torch CPU tensors) and the float64 / fp32 restatement's nine results; computed once, never modified"""
    B, T, D, U, mode, act, bias, kind = POOL_CASES[name]
    rng = np.random.default_rng(len(name) * 7 + B + T)
    f = lambda *s: torch.from_numpy(rng.normal(size=s).astype(np.float32))                     # noqa: E731
    n_in = 2 if mode == 0 else 3
    a = dict(query=f(B, D), keys=f(B, T, D), W=f(n_in * D, U) * (1.5 / np.sqrt(n_in * D)), b=f(U) * 0.2 if bias else None,
             w_out=f(U, 1) * (1.0 / np.sqrt(U)), b_out=f(1) * 0.2 if bias else None, alpha=f(U) * 0.5 if act == "dice" else None)
    mask = torch.from_numpy(_pool_mask(rng, B, T, kind))
    g_out, g_sc = f(B, D), f(B, T)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        leaf = {k: (v.to(dtype).requires_grad_(True) if v is not None else None) for k, v in a.items()}
        out, scores = R.pool(leaf["query"], leaf["keys"], mask, leaf["W"], leaf["b"], leaf["w_out"], leaf["b_out"], mode, ACTS[act],
                             leaf["alpha"], 1e-8)
        ((out * g_out.to(dtype)).sum() + (scores * g_sc.to(dtype)).sum()).backward()
        gr = lambda k: leaf[k].grad if leaf[k] is not None else None                            # noqa: E731
        refs[dtype] = [out.detach(), scores.detach(), gr("query"), gr("keys"), gr("W"), gr("b"), gr("w_out"), gr("b_out"), gr("alpha")]
    return a, mask, g_out, g_sc, refs


def _pool_run(name, keys_override=None):
    ops, _, _ = _mods()
    B, T, D, U, mode, act, bias, kind = POOL_CASES[name]
    a, mask, g_out, g_sc, _ = _pool_case(name)
    dev = lambda t: None if t is None else t.cuda()                                            # noqa: E731
    q = _view2(a["query"], 3)
    k = _view3(a["keys"] if keys_override is None else keys_override, 4)
    args = (q, k, mask.cuda(), dev(a["W"]), dev(a["b"]), dev(a["w_out"]), dev(a["b_out"]), mode, ACTS[act])
    out, scores = ops.din_pool_fwd(*args, alpha=dev(a["alpha"]), eps=1e-8)
    grads = ops.din_pool_bwd(*args, g_out.cuda(), g_sc.cuda(), alpha=dev(a["alpha"]), eps=1e-8)
    return [out, scores] + list(grads)


@pytest.mark.parametrize("name", list(POOL_CASES))
def test_pool_forward_backward(name):
    _, mask, _, _, refs = _pool_case(name)
    got = _pool_run(name)
    for res, g, r64, r32 in zip(RESULTS, got, refs[torch.float64], refs[torch.float32]):
        assert (g is None) == (r64 is None), res
        if g is not None:
            _check("%s %s" % (name, res), g, r64, r32)
    assert (got[3].cpu()[~mask] == 0).all(), "d_keys must be exactly 0 at masked positions"


@pytest.mark.parametrize("name", ["b65_t50_d64_u36_mul_dice", "b4_t17_d8_u80_mul_sigmoid_holes"])
def test_pool_skips_masked_positions(name):
    """NaN keys at masked positions reach nothing: every result is finite and EQUAL to the run with zeros there"""
    a, mask, _, _, _ = _pool_case(name)
    zeros = torch.where(mask[:, :, None], a["keys"], torch.zeros_like(a["keys"]))
    nans = torch.where(mask[:, :, None], a["keys"], torch.full_like(a["keys"], float("nan")))
    with_zeros, with_nans = _pool_run(name, zeros), _pool_run(name, nans)
    for res, z, n in zip(RESULTS, with_zeros, with_nans):
        if z is not None:
            assert torch.isfinite(n).all(), res
            assert torch.equal(z, n), res
    assert (with_nans[3].cpu()[~mask] == 0).all()
    assert (with_nans[1].cpu()[~mask] == 0).all()


@pytest.mark.parametrize("name", ["b65_t50_d64_u36_mul_dice", "b5_t33_d128_u128_sub_dice", "b2_t200_d16_u5_sub_tanh"])
def test_pool_is_bit_reproducible(name):
    first, second = _pool_run(name), _pool_run(name)
    for res, x, y in zip(RESULTS, first, second):
        if x is not None:
            assert torch.equal(x, y), res


@pytest.mark.parametrize("inter,activation", [("subtract", "dice"), ("multiply", "relu"), (None, "tanh")])
def test_interest_pooling_agrees_with_activation_unit_on_expanded_pairs(inter, activation):
    """the two public paths on shared parameters: InterestPooling == masked sum of ActivationUnit(expanded query, flattened keys) * keys"""
    _, _, din = _mods()
    B, T, D, U = 6, 11, 16, 24
    rng = np.random.default_rng(21)
    q0, k0 = rng.normal(size=(B, D)).astype(np.float32), rng.normal(size=(B, T, D)).astype(np.float32)
    lengths = np.array([0, T, 3, 7, 1, 10])
    mk = lambda: {None: None, "subtract": din.Subtract(), "multiply": din.Multiply()}[inter]   # noqa: E731
    act = din.Dice() if activation == "dice" else activation
    pool = din.InterestPooling(U, interacter=mk(), activation=act)
    q, k = torch.from_numpy(q0).cuda(), torch.from_numpy(k0).cuda().requires_grad_(True)
    pool(q, k, lengths=lengths)
    with torch.no_grad():
        pool.dense_kernel_w.mul_(5.0)
        pool.dense_output_w.mul_(5.0)
        pool.dense_kernel_b.normal_(0, 0.1)
        pool.dense_output_b.normal_(0, 0.1)
        if activation == "dice":
            pool.dice.alpha.normal_(0, 0.5)
    unit = din.ActivationUnit(U, interacter=mk(), activation=act)
    for n in ("dense_kernel_w", "dense_kernel_b", "dense_output_w", "dense_output_b"):
        setattr(unit, n, getattr(pool, n))
    unit.built = True
    g = torch.from_numpy(rng.normal(size=(B, D)).astype(np.float32)).cuda()
    out_p, sc_p = pool(q, k, lengths=lengths, return_scores=True)
    (out_p * g).sum().backward()
    dk_p, dW_p = k.grad.clone(), pool.dense_kernel_w.grad.clone()
    k.grad = None
    pool.dense_kernel_w.grad = None
    valid = torch.arange(T, device="cuda")[None, :] < torch.from_numpy(lengths).cuda()[:, None]
    s = unit(q[:, None, :].expand(B, T, D).reshape(B * T, D), k.reshape(B * T, D)).reshape(B, T)
    sc_u = torch.where(valid, s, torch.zeros_like(s))
    out_u = (sc_u[:, :, None] * k).sum(1)
    (out_u * g).sum().backward()
    mode = {None: 0, "subtract": 1, "multiply": 2}[inter]
    refs = {}
    for dtype in (torch.float64, torch.float32):
        c = lambda t: None if t is None else t.detach().cpu().to(dtype)                        # noqa: E731
        K, W = c(k).requires_grad_(True), c(pool.dense_kernel_w).requires_grad_(True)
        o, sc = R.pool(c(q), K, valid.cpu(), W, c(pool.dense_kernel_b), c(pool.dense_output_w), c(pool.dense_output_b), mode,
                       ACTS[activation], c(pool.dice.alpha) if activation == "dice" else None, 1e-8)
        (o * g.cpu().to(dtype)).sum().backward()
        refs[dtype] = [o.detach(), sc.detach(), K.grad, W.grad]
    for name, gp, gu, r64, r32 in zip(["out", "scores", "d_keys", "dW"], [out_p, sc_p, dk_p, dW_p], [out_u, sc_u, k.grad, pool.dense_kernel_w.grad],
                                      refs[torch.float64], refs[torch.float32]):
        _check("pooling %s" % name, gp, r64, r32)
        _check("unit    %s" % name, gu, r64, r32)


@pytest.mark.parametrize("D,U", [(6, 8), (132, 8), (8, 129)])
def test_pool_domain_errors_name_the_domain(D, U):
    _, _, din = _mods()
    q, k = torch.zeros(2, D, device="cuda"), torch.zeros(2, 3, D, device="cuda")
    with pytest.raises(ValueError, match="D % 4 == 0, 4 <= D <= 128, 1 <= U <= 128"):
        din.InterestPooling(U, interacter=din.Multiply())(q, k)


def test_pool_never_allocates_the_pair_matrix():
    """forward + backward at B 2048, T 64, D 64, U 32 stay below the bytes of the [B * T, 3D] concat the layer avoids (100.7 MB):
    d_keys (33.5 MB), the [B * T, U] hidden gradient (16.8 MB), scores and the reduction workspaces fit under that, a pair matrix
    does not"""
    _, L, _ = _mods()
    B, T, D, U = 2048, 64, 64, 32
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)                                  # noqa: E731
    q, k = r(B, D).requires_grad_(True), r(B, T, D).requires_grad_(True)
    W, b, wo, bo, al = (t.requires_grad_(True) for t in (r(3 * D, U) * 0.1, r(U) * 0.1, r(U, 1) * 0.2, r(1), r(U) * 0.3))
    mask = torch.rand(B, T, device="cuda", generator=g) < 0.8
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, scores = L.din_interest_pooling(q, k, mask, W, b, wo, bo, 2, 4, al, 1e-8)
    (out.sum() + scores.sum()).backward()
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    print("peak extra allocation %.1f MB of %.1f MB" % (used / 1e6, B * T * 3 * D * 4 / 1e6))
    assert used < B * T * 3 * D * 4
    assert all(torch.isfinite(t.grad).all() for t in (q, k, W, b, wo, bo, al))


def test_small_din_model_trains():
    """embedding table -> InterestPooling -> concat with the query -> layers.mlp -> BCE; five SGD steps"""
    _, L, din = _mods()
    B, T, D, V = 256, 20, 16, 50
    g = torch.Generator().manual_seed(4)
    items = torch.randint(0, V, (B,), generator=g).cuda()
    hist = torch.randint(0, V, (B, T), generator=g).cuda()
    lengths = torch.randint(0, T + 1, (B,), generator=g).cuda()
    labels = ((items % 2) == 0).float().cuda()
    table = torch.nn.Parameter((torch.randn(V, D, generator=g) * 0.3).cuda())
    pool = din.InterestPooling(36, interacter=din.Multiply(), activation=din.Dice())
    W1 = torch.nn.Parameter((torch.randn(2 * D, 32, generator=g) * 0.2).cuda())
    b1 = torch.nn.Parameter(torch.zeros(32).cuda())
    W2 = torch.nn.Parameter((torch.randn(32, 1, generator=g) * 0.2).cuda())
    b2 = torch.nn.Parameter(torch.zeros(1).cuda())

    def loss_fn():
        qe = table[items]
        pooled = pool(qe, table[hist], lengths=lengths)
        logit = L.mlp(torch.cat([pooled, qe], dim=1), [W1, W2], [b1, b2], [1, 0])
        return torch.nn.functional.binary_cross_entropy_with_logits(logit.reshape(-1), labels)

    loss_fn()                                        # builds the lazily created parameters
    params = [table, W1, b1, W2, b2] + list(pool.parameters())
    assert len(list(pool.parameters())) == 5         # two kernels, two biases, Dice's alpha
    opt = torch.optim.SGD(params, lr=0.2)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        for p in params:
            assert p.grad is not None and torch.isfinite(p.grad).all()
        opt.step()
        losses.append(loss.item())
    print("losses", losses)
    assert losses[-1] < losses[0]
