"""Multi-task learning on the GPU: the grouped dense layers, the gate softmax + mixture, the MSE / ESMM heads, MMoE and ESMM against a
float64 restatement written here, the variables, the two-apply Adam recipe and the example script."""
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multitask_ref import _gate_mix_ref, _ref_esmm_x, _ref_input, _ref_mmoe      # the float64 restatements

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)


@pytest.fixture(params=["native", "bf16x3"])
def gemm_mode(request):
    from deep_recommenders_amd import ops
    old = ops.get_gemm_mode()
    ops.set_gemm_mode(ops.GEMM_NATIVE_F32 if request.param == "native" else ops.GEMM_BF16X3)
    yield request.param
    ops.set_gemm_mode(old)


# ---------------------------------------------------------------------------------------------------------------------------------
# grouped dense layers
# ---------------------------------------------------------------------------------------------------------------------------------
def _close(got, want, what):
    got = got.double().cpu()
    err = (got - want).abs().max().item() if got.numel() else 0.0
    scale = max(1.0, want.abs().max().item() if want.numel() else 1.0)
    assert err <= 1e-4 * scale, "%s: max err %g (scale %g)" % (what, err, scale)


GROUPED_SHAPES = [(G, M, K, N) for G in (1, 2, 3, 8) for M in (1, 1000, 4096) for K in (10, 32, 256) for N in (1, 10, 32, 64)
                  if not (M == 4096 and G == 8 and K == 256)]
GROUPED_SHAPES.append((2, 130, 3, 1))                   # skinny (K < 4, N < 4) kernels, two row slabs per group


@pytest.mark.parametrize("G,M,K,N", GROUPED_SHAPES)
def test_grouped_linear_matches_float64(gemm_mode, G, M, K, N):
    from deep_recommenders_amd import ops
    g = torch.Generator().manual_seed(G * 1000 + M + K + N)
    pad = 3                                             # strided layouts: row pitch beyond G*K / G*N
    ldx, ldy = G * K + pad, G * N + pad
    x = torch.randn(M, ldx, generator=g)
    W = torch.randn(G, K, N, generator=g) / math.sqrt(K)
    b = torch.randn(G, N, generator=g)
    dy = torch.randn(M, ldy, generator=g)
    xd, Wd, bd, dyd = x.cuda(), W.cuda(), b.cuda(), dy.cuda()
    y = torch.full((M, ldy), 7.0, device="cuda")
    ops.linear_fwd_grouped(xd, ldx, K, Wd, N, K * N, bd, N, M, K, N, G, 1, y, ldy, N)
    relu_src = x.clone()
    dx = torch.zeros(M, ldx, device="cuda")
    ops.linear_bwd_dx_grouped(dyd, ldy, N, Wd, N, K * N, M, K, N, G, xd, ldx, K, False, dx, ldx, K)
    gW = torch.zeros(G, K, N, device="cuda")
    gb = torch.zeros(G, N, device="cuda")
    ws = ops.linear_bwd_dw_grouped_workspace(M, K, N, G, "cuda")
    ops.linear_bwd_dw_grouped(xd, ldx, K, dyd, ldy, N, M, K, N, G, 1.0, gW, N, K * N, gb, N, workspace=ws)
    # a second launch on the same inputs: bit-identical
    y2 = torch.full((M, ldy), 7.0, device="cuda")
    ops.linear_fwd_grouped(xd, ldx, K, Wd, N, K * N, bd, N, M, K, N, G, 1, y2, ldy, N)
    dx2 = torch.zeros(M, ldx, device="cuda")
    ops.linear_bwd_dx_grouped(dyd, ldy, N, Wd, N, K * N, M, K, N, G, xd, ldx, K, False, dx2, ldx, K)
    gW2 = torch.zeros(G, K, N, device="cuda")
    gb2 = torch.zeros(G, N, device="cuda")
    ops.linear_bwd_dw_grouped(xd, ldx, K, dyd, ldy, N, M, K, N, G, 1.0, gW2, N, K * N, gb2, N, workspace=ws)
    # without a workspace: the atomic form of the weight gradient (any summation order)
    gW3 = torch.zeros(G, K, N, device="cuda")
    gb3 = torch.zeros(G, N, device="cuda")
    ops.linear_bwd_dw_grouped(xd, ldx, K, dyd, ldy, N, M, K, N, G, 1.0, gW3, N, K * N, gb3, N)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(gW, gW2) and torch.equal(gb, gb2)
    assert torch.all(y[:, G * N:] == 7.0), "wrote past the groups"
    for z in range(G):
        xz = x[:, z * K:(z + 1) * K].double()
        dyz = dy[:, z * N:(z + 1) * N].double()
        Wz = W[z].double()
        _close(y[:, z * N:(z + 1) * N], torch.relu(xz @ Wz + b[z].double()), "fwd g%d" % z)
        _close(dx[:, z * K:(z + 1) * K], (dyz @ Wz.T) * (relu_src[:, z * K:(z + 1) * K] > 0).double(), "dx g%d" % z)
        _close(gW[z], xz.T @ dyz, "dW g%d" % z)
        _close(gb[z], dyz.sum(0), "db g%d" % z)
        _close(gW3[z], xz.T @ dyz, "dW (no workspace) g%d" % z)
        _close(gb3[z], dyz.sum(0), "db (no workspace) g%d" % z)


@pytest.mark.parametrize("G,M,K,N", [(2, 1000, 32, 64), (3, 4096, 256, 32), (8, 1000, 10, 10), (2, 4096, 64, 128)])
def test_grouped_linear_groups_equal_single_calls(gemm_mode, G, M, K, N):
    """a group runs the same tile kernel as dr_linear_* on that group's slice: fwd, dx and the deterministic dW agree bit for bit"""
    from deep_recommenders_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, G * K, generator=g).cuda()
    W = (torch.randn(G, K, N, generator=g) / math.sqrt(K)).cuda()
    b = torch.randn(G, N, generator=g).cuda()
    dy = torch.randn(M, G * N, generator=g).cuda()
    y = torch.empty(M, G * N, device="cuda")
    ops.linear_fwd_grouped(x, G * K, K, W, N, K * N, b, N, M, K, N, G, 1, y, G * N, N)
    dx = torch.empty(M, G * K, device="cuda")
    ops.linear_bwd_dx_grouped(dy, G * N, N, W, N, K * N, M, K, N, G, x, G * K, K, False, dx, G * K, K)
    gW = torch.zeros(G, K, N, device="cuda")
    ops.linear_bwd_dw_grouped(x, G * K, K, dy, G * N, N, M, K, N, G, 1.0, gW, N, K * N, None, 0,
                              workspace=ops.linear_bwd_dw_grouped_workspace(M, K, N, G, "cuda"))
    for z in range(G):
        xs, dys = x[:, z * K:(z + 1) * K], dy[:, z * N:(z + 1) * N]
        ys = ops.linear_fwd(xs, W[z], b[z], 1)
        dxs = ops.linear_bwd_dx(dys, W[z], xs)
        gWs = torch.zeros(K, N, device="cuda")
        ops.linear_bwd_dw(xs, dys, 1.0, gWs, None, workspace=ops.linear_bwd_dw_workspace(M, K, N, "cuda"))
        torch.cuda.synchronize()
        assert torch.equal(y[:, z * N:(z + 1) * N], ys), "fwd group %d" % z
        assert torch.equal(dx[:, z * K:(z + 1) * K], dxs), "dx group %d" % z
        assert torch.equal(gW[z], gWs), "dW group %d" % z


def test_grouped_dw_fused_sgd_form(gemm_mode):
    from deep_recommenders_amd import ops
    G, M, K, N, lr = 2, 1000, 32, 10, 0.05
    x = torch.randn(M, G * K).cuda()
    dy = torch.randn(M, G * N).cuda()
    W = torch.randn(G, K, N).cuda()
    b = torch.randn(G, N).cuda()
    W0, b0 = W.double().cpu(), b.double().cpu()
    ops.linear_bwd_dw_grouped(x, G * K, K, dy, G * N, N, M, K, N, G, -lr, W, N, K * N, b, N,
                              workspace=ops.linear_bwd_dw_grouped_workspace(M, K, N, G, "cuda"))
    for z in range(G):
        xz, dyz = x[:, z * K:(z + 1) * K].double().cpu(), dy[:, z * N:(z + 1) * N].double().cpu()
        _close(W[z], W0[z] - lr * xz.T @ dyz, "sgd W")
        _close(b[z], b0[z] - lr * dyz.sum(0), "sgd b")


# ---------------------------------------------------------------------------------------------------------------------------------
# gate softmax + mixture
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,T,U,B", [(E, T, U, B) for E in (1, 2, 3, 8, 64) for T in (1, 2, 3) for U in (1, 7, 64, 130)
                                     for B in (1, 33, 4096) if not (E == 64 and B == 4096 and U == 130)])
def test_gate_mix_matches_float64(E, T, U, B):
    from deep_recommenders_amd import ops
    g = torch.Generator().manual_seed(E * 100 + T * 10 + U + B)
    h = torch.randn(B, E * U, generator=g)
    l = torch.randn(B, T * E, generator=g) * 3
    d_out = torch.randn(B, T * U, generator=g)
    p, out = ops.mmoe_gate_mix_fwd(h.cuda(), l.cuda(), E, T, U)
    d_h, d_l = ops.mmoe_gate_mix_bwd(h.cuda(), p, d_out.cuda(), E, T, U)
    p2, out2 = ops.mmoe_gate_mix_fwd(h.cuda(), l.cuda(), E, T, U)
    d_h2, d_l2 = ops.mmoe_gate_mix_bwd(h.cuda(), p, d_out.cuda(), E, T, U)
    assert torch.equal(p, p2) and torch.equal(out, out2) and torch.equal(d_h, d_h2) and torch.equal(d_l, d_l2)
    hd, ld = h.double().requires_grad_(True), l.double().requires_grad_(True)
    pr, outr = _gate_mix_ref(hd, ld, E, T, U)
    outr.backward(d_out.double())
    _close(p, pr.detach(), "p")
    _close(out, outr.detach(), "out")
    _close(d_h, hd.grad, "d_h")
    _close(d_l, ld.grad, "d_l")
    if E == 1:
        assert torch.all(p == 1.0) and torch.all(d_l == 0.0)


def test_gate_mix_saturated_logits_finite():
    from deep_recommenders_amd import ops
    B, E, T, U = 64, 8, 2, 16
    l = torch.where(torch.rand(B, T * E) < 0.5, torch.tensor(80.0), torch.tensor(-80.0)).cuda()
    h = torch.randn(B, E * U).cuda()
    p, out = ops.mmoe_gate_mix_fwd(h, l, E, T, U)
    d_h, d_l = ops.mmoe_gate_mix_bwd(h, p, torch.randn(B, T * U).cuda(), E, T, U)
    for t in (p, out, d_h, d_l):
        assert torch.isfinite(t).all()


def test_gate_mix_domain():
    from deep_recommenders_amd import _lib, ops
    h = torch.randn(4, 65 * 2).cuda()
    with pytest.raises(RuntimeError, match="DR_ESHAPE"):
        ops.mmoe_gate_mix_fwd(h, torch.randn(4, 65).cuda(), 65, 1, 2)
    with pytest.raises(RuntimeError, match="DR_ESHAPE"):
        ops.mmoe_gate_mix_fwd(torch.randn(4, 4).cuda(), torch.randn(4, 17 * 2).cuda(), 2, 17, 2)
    assert _lib.DR_ESHAPE == -3


# ---------------------------------------------------------------------------------------------------------------------------------
# heads
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(1, 1), (512, 2), (4099, 3)])
def test_mse_matches_float64(B, T):
    from deep_recommenders_amd import ops
    pred = torch.randn(B, T) * 3
    y = torch.randn(B, T)
    loss, d = ops.mse_fwd_bwd(pred.cuda(), y.cuda())
    loss2, d2 = ops.mse_fwd_bwd(pred.cuda(), y.cuda())
    assert torch.equal(loss, loss2) and torch.equal(d, d2)
    r = pred.double() - y.double()
    _close(loss, (r * r).mean(0), "loss")
    _close(d, 2 * r / B, "d_pred")


def test_esmm_head_matches_float64_and_saturates():
    from deep_recommenders_amd import ops
    B = 1000
    lg = torch.randn(B, 2) * 4
    lg[:4] = torch.tensor([[90.0, -90.0], [-95.0, 95.0], [120.0, 120.0], [-120.0, -120.0]])
    p_cvr, p_ctr, p_ctcvr = ops.esmm_head_fwd(lg.cuda())
    assert torch.equal(p_ctcvr, p_ctr * p_cvr)
    ld = lg.double().requires_grad_(True)
    pc, pt = torch.sigmoid(ld[:, 0]), torch.sigmoid(ld[:, 1])
    _close(p_cvr, pc.detach(), "p_cvr")
    _close(p_ctr, pt.detach(), "p_ctr")
    g = [torch.randn(B) for _ in range(3)]
    (pc * g[0] + pt * g[1] + pc * pt * g[2]).sum().backward()
    d = ops.esmm_head_bwd(p_cvr, p_ctr, *[t.cuda() for t in g])
    _close(d, ld.grad, "d_logits")
    d_only = ops.esmm_head_bwd(p_cvr, p_ctr, None, None, g[2].cuda())
    for t in (p_cvr, p_ctr, p_ctcvr, d, d_only):
        assert torch.isfinite(t).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# models against a float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def _numeric_features(n, B, seed):
    r = np.random.RandomState(seed)
    return {"C%d" % i: r.normal(size=(B, 1)).astype(np.float32) for i in range(n)}


def _check_model_parity(model, ref_fn, features, out_grads, tol=2e-4):
    V = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in model.export_variables().items()}
    outs = model(features)
    refs = ref_fn(V)
    total, total_ref = 0, 0
    for o, r, g in zip(outs, refs, out_grads):
        _close(o, r.detach(), "output")
        total = total + (o * g.cuda()).sum()
        total_ref = total_ref + (r * g.double()).sum()
    total.backward()
    total_ref.backward()
    for name in model.var_names:
        if not name.startswith("input_layer/"):
            grad = model.variable(name).grad
        else:
            key = name.split("/")[1][:-len("_embedding")]
            sl = model.input_layer.slab
            grad = sl.table.grad[sl.base[key]:sl.base[key] + sl.columns[key].num_buckets]
        want = V[name].grad
        if want is None:
            assert grad is None, "%s should receive no gradient" % name
            continue
        assert grad is not None, "%s got no gradient" % name
        g64 = grad.double().cpu()
        err = (g64 - want).abs().max().item()
        assert err <= tol * max(1.0, want.abs().max().item()), "%s: gradient err %g" % (name, err)


@pytest.mark.parametrize("E,T,act", [(2, 2, "relu"), (3, 2, "relu"), (8, 3, "tanh")])
def test_mmoe_parity(gemm_mode, E, T, act):
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.estimator.models.feature_interaction.dnn import relu, tanh
    from deep_recommenders_amd.estimator.models.multi_task_learning import MMoE
    torch.manual_seed(E * 10 + T)
    a = relu if act == "relu" else tanh
    cols = [fc.numeric_column("C%d" % i) for i in range(20)]
    eu, tu = [32, 16], [10]
    m = MMoE(cols, num_tasks=T, num_experts=E, expert_hidden_units=eu, task_hidden_units=tu, task_hidden_activation=a,
             expert_hidden_activation=a)
    B = 300
    feats = _numeric_features(20, B, 1)
    _check_model_parity(m, lambda V: _ref_mmoe(feats, cols, V, E, T, eu, tu, act, act), feats, [torch.randn(B, 1) for _ in range(T)])
    if E > T:       # the unused gates exist and get nothing
        for t in range(T, E):
            assert m.variable("multi_gate/dense_%d/kernel" % t).grad is None


def test_mmoe_parity_mixed_embedding_and_numeric(gemm_mode):
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.estimator.models.multi_task_learning import MMoE
    torch.manual_seed(3)
    cols = [fc.numeric_column("a_num"), fc.numeric_column("z_num", shape=(3,)),
            fc.embedding_column(fc.categorical_column_with_identity("m_cat", 50), 8),
            fc.embedding_column(fc.categorical_column_with_identity("b_cat", 30), 8)]
    m = MMoE(cols, num_tasks=2, num_experts=3, expert_hidden_units=[16, 8], task_hidden_units=[4])
    B = 200
    r = np.random.RandomState(2)
    feats = {"a_num": r.normal(size=(B, 1)).astype(np.float32), "z_num": r.normal(size=(B, 3)).astype(np.float32),
             "m_cat": r.randint(0, 50, size=(B, 1)), "b_cat": r.randint(0, 30, size=(B, 1))}
    _check_model_parity(m, lambda V: _ref_mmoe(feats, cols, V, 3, 2, [16, 8], [4]), feats, [torch.randn(B, 1) for _ in range(2)])


def test_esmm_parity(gemm_mode):
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.estimator.models.multi_task_learning import ESMM
    torch.manual_seed(4)
    cols = [fc.numeric_column("C%d" % i) for i in range(12)]
    m = ESMM(cols, [32, 10])
    B = 256
    feats = _numeric_features(12, B, 3)

    def ref(V):
        return _ref_esmm_x(_ref_input(feats, cols, V), V, 3)
    _check_model_parity(m, ref, feats, [torch.randn(B, 1) for _ in range(3)])


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's tests, restated
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_size", [32, 64, 128, 512])
def test_reference_mmoe_and_esmm_shapes(batch_size):
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.datasets import SyntheticForMultiTask
    from deep_recommenders_amd.estimator.models.multi_task_learning import ESMM, MMoE
    cols = [fc.numeric_column("C{}".format(i)) for i in range(100)]
    feats, _ = next(SyntheticForMultiTask(5000, example_dim=100, seed=0).input_fn(batch_size=batch_size))
    outs = MMoE(cols, num_tasks=2, num_experts=2, task_hidden_units=[32, 10], expert_hidden_units=[64, 32])(feats)
    assert len(outs) == 2 and all(tuple(o.shape) == (batch_size, 1) for o in outs)
    p = ESMM(cols, [32, 10])(feats)
    assert len(p) == 3 and all(tuple(o.shape) == (batch_size, 1) for o in p)


def test_model_errors():
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.estimator.models.multi_task_learning import ESMM, MMoE
    cols = [fc.numeric_column("C0")]
    with pytest.raises(IndexError):
        MMoE(cols, num_tasks=3, num_experts=2, expert_hidden_units=[4], task_hidden_units=[4])
    with pytest.raises(TypeError):
        MMoE(cols, num_tasks=1, num_experts=2, expert_hidden_units=[4], task_hidden_units=[4], expert_batch_normalization=True)
    with pytest.raises(TypeError):
        ESMM(cols, [4], batch_normalization=True)


def test_dropout_draws_every_call():
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.estimator.models.multi_task_learning import MMoE
    cols = [fc.numeric_column("C%d" % i) for i in range(8)]
    m = MMoE(cols, 2, 2, [16, 8], [4], expert_dropout=0.5, task_dropout=0.5)
    f = _numeric_features(8, 64, 0)
    a, b = m(f)[0], m(f)[0]
    assert not torch.equal(a, b)


def test_export_variables_example_configuration():
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.estimator.models.multi_task_learning import MMoE
    cols = [fc.numeric_column("C{}".format(i)) for i in range(256)]
    m = MMoE(cols, num_tasks=2, num_experts=2, task_hidden_units=[32, 10], expert_hidden_units=[64, 32])
    v = m.export_variables()
    want = [("mixture_of_experts/dense/kernel", (256, 64)), ("mixture_of_experts/dense/bias", (64,)),
            ("mixture_of_experts/dense_1/kernel", (64, 32)), ("mixture_of_experts/dense_1/bias", (32,)),
            ("mixture_of_experts/dense_2/kernel", (256, 64)), ("mixture_of_experts/dense_2/bias", (64,)),
            ("mixture_of_experts/dense_3/kernel", (64, 32)), ("mixture_of_experts/dense_3/bias", (32,)),
            ("multi_gate/dense/kernel", (256, 2)), ("multi_gate/dense_1/kernel", (256, 2))]
    for t in range(2):
        for j, (k, n) in enumerate([(32, 32), (32, 10), (10, 1)]):
            nm = "task%d/dense%s" % (t, "" if j == 0 else "_%d" % j)
            want += [(nm + "/kernel", (k, n)), (nm + "/bias", (n,))]
    assert [(k, tuple(a.shape)) for k, a in v.items()] == want
    m2 = MMoE(cols, num_tasks=2, num_experts=2, task_hidden_units=[32, 10], expert_hidden_units=[64, 32])
    m2.import_variables(v)
    f = _numeric_features(256, 64, 5)
    for a, b in zip(m(f), m2(f)):
        assert torch.equal(a, b)
    v2 = m2.export_variables()
    assert all(np.array_equal(v[k], v2[k]) for k in v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the training recipe: two Adam applies per step, one shared step counter
# ---------------------------------------------------------------------------------------------------------------------------------
def _ref_adam_apply(V, grads, m, v, t, lr=0.01, b1=0.9, b2=0.999, eps=1e-8):
    lr_t = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    for k, g in grads.items():
        if g is None:
            continue
        m[k] = b1 * m[k] + (1 - b1) * g
        v[k] = b2 * v[k] + (1 - b2) * g * g
        V[k] = V[k] - lr_t * m[k] / (torch.sqrt(v[k]) + eps)


def test_training_recipe_matches_float64_two_apply_adam():
    """30 steps of the example's recipe.  Each step starts the float64 restatement from the model's current parameters (so fp32
    rounding does not compound through 30 Adam steps into a different trajectory); its moments and step counter run on their own."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_mmoe_on_synthetic_estimator as ex
    from deep_recommenders_amd.datasets import SyntheticForMultiTask
    torch.manual_seed(0)
    model = ex.build_model()
    opt = ex.make_optimizer(model)
    cols = ex.build_columns()
    names = list(model.export_variables())
    m = {k: torch.zeros(model.variable(k).shape, dtype=torch.float64) for k in names}
    v = {k: torch.zeros(model.variable(k).shape, dtype=torch.float64) for k in names}
    it = SyntheticForMultiTask(512 * 30, example_dim=256, seed=7).input_fn(batch_size=512)
    t = 0
    for step in range(30):
        feats, labels = next(it)
        V = {k: torch.tensor(a, dtype=torch.float64) for k, a in model.export_variables().items()}
        l0, l1 = ex.train_step(model, opt, feats, labels)
        Vg = {k: a.clone().requires_grad_(True) for k, a in V.items()}
        outs = _ref_mmoe(feats, cols, Vg, 2, 2, [64, 32], [32, 10])
        y0 = torch.as_tensor(labels["labels0"]).double().reshape(-1, 1)
        y1 = torch.as_tensor(labels["labels1"]).double().reshape(-1, 1)
        r0 = ((outs[0] - y0) ** 2).mean()
        r1 = ((outs[1] - y1) ** 2).mean()
        assert abs(l0.item() - r0.item()) <= 1e-4 * abs(r0.item()), (step, l0.item(), r0.item())
        assert abs(l1.item() - r1.item()) <= 1e-4 * abs(r1.item()), (step, l1.item(), r1.item())
        g0 = dict(zip(names, torch.autograd.grad(r0, [Vg[k] for k in names], retain_graph=True, allow_unused=True)))
        g1 = dict(zip(names, torch.autograd.grad(r1, [Vg[k] for k in names], allow_unused=True)))
        assert g0["task1/dense/kernel"] is None and g1["task0/dense/kernel"] is None and g1["multi_gate/dense/kernel"] is None
        t += 1
        _ref_adam_apply(V, g0, m, v, t)
        t += 1
        _ref_adam_apply(V, g1, m, v, t)
        got = model.export_variables()
        for k in names:
            d = np.abs(got[k] - V[k].numpy())
            assert (d > 1e-4).mean() <= 1e-3 and d.max() <= 2e-3, (step, k, d.max())
    assert opt.t == 60
    assert opt.state[model.variable("task1/dense/kernel")]["t"] == 30


def test_task1_first_update_uses_shared_t2():
    """one step on a model whose task-1 tower sees gradient only from loss1: its update equals Adam at t = 2, not t = 1"""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_mmoe_on_synthetic_estimator as ex
    from deep_recommenders_amd.datasets import SyntheticForMultiTask
    torch.manual_seed(1)
    model = ex.build_model()
    opt = ex.make_optimizer(model)
    feats, labels = next(SyntheticForMultiTask(512, example_dim=256, seed=3).input_fn(batch_size=512))
    before = model.export_variables()["task1/dense_2/bias"].astype(np.float64)
    _, l0, l1 = ex.model_losses(model, feats, labels)
    g1 = torch.autograd.grad(l1, [model.variable("task1/dense_2/bias")])[0].double().cpu().numpy()
    ex.train_step(model, opt, feats, labels)
    after = model.export_variables()["task1/dense_2/bias"].astype(np.float64)
    lr_t2 = 0.01 * math.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2)
    m = 0.1 * g1
    v = 0.001 * g1 * g1
    want = before - lr_t2 * m / (np.sqrt(v) + 1e-8)
    assert np.allclose(after, want, rtol=1e-4, atol=1e-6), (after, want)


def test_example_runs_and_loss_decreases():
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_mmoe_on_synthetic_estimator.py"), "--examples", str(512 * 60),
           "--steps", "50", "--eval-steps", "5", "--log-every", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    import json
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    tr = [x["total_loss"] for x in lines if "total_loss" in x]
    assert len(tr) == 50
    assert np.mean(tr[-10:]) < np.mean(tr[:5]), tr
    assert "task0_mse" in lines[-1] and "task1_mse" in lines[-1]
