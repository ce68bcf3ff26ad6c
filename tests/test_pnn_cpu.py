"""CPU tests of PNN: the torch restatement (tests/pnn_ref.py) against hand-written cases and autograd, the exactness of the grid cases
that tests/test_gpu_pnn.py compares bit for bit, the GPU limit 16 max(r32, 8 u) held against a deliberately different fp32 association,
the inner-product half against the paper's form, and everything of the package that needs no device: configs, constructor errors,
exports, the argument errors of ops.pnn_outer_* and the static half of the kernels' contract."""
import numpy as np
import pytest
import torch

import pnn_ref as R

DD = torch.float64
U = 2.0 ** -24
GRID = [i for i, c in enumerate(R.CASES) if c[1] == "grid"]
NORMAL = [i for i, c in enumerate(R.CASES) if c[1] == "normal"]
ID = lambda i: "%dx%dx%dx%d" % R.CASES[i][0]                                                   # noqa: E731


def _close(a, b, tol=1e-11):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def test_hand_written_case():
    e = torch.tensor([[[1.0, 2.0, 0.0, -1.0], [0.5, 0.0, 1.0, 1.0]]], dtype=DD)                # u = (1.5, 2, 1, 0)
    W = torch.zeros((16, 2), dtype=DD)
    W[0 * 4 + 1, 0] = 1.0                                                                      # u_0 u_1 = 3
    W[2 * 4 + 0, 0] = 2.0                                                                      # 2 u_2 u_0 = 3
    W[1 * 4 + 1, 1] = -1.0                                                                     # -u_1^2 = -4
    W[3 * 4 + 2, 1] = 5.0                                                                      # u_3 = 0
    f = R.forward(e, W, torch.tensor([[10.0, 20.0]], dtype=DD))
    assert f["u"].tolist() == [[1.5, 2.0, 1.0, 0.0]] and f["out"].tolist() == [[16.0, 16.0]]
    d_emb, dW = R.backward(e, W, torch.tensor([[1.0, 0.0]], dtype=DD))
    # out_0 = u_0 u_1 + 2 u_2 u_0: d/du = (u_1 + 2 u_2, u_0, 2 u_0, 0)
    assert d_emb.tolist() == [[[4.0, 1.5, 3.0, 0.0]] * 2]
    assert dW[:, 1].abs().max().item() == 0.0 and dW[1, 0].item() == 3.0 and dW[4, 0].item() == 3.0 and dW[15, 0].item() == 0.0


def test_identity_column_gives_the_squared_norm_and_antisymmetric_w_gives_zero():
    rng = np.random.default_rng(1)
    e = torch.from_numpy(rng.normal(size=(5, 3, 8)))
    A = torch.from_numpy(rng.normal(size=(8, 8, 3)))
    W = (A - A.transpose(0, 1)).reshape(64, 3).clone()
    W[:, 1] = torch.eye(8, dtype=DD).reshape(64)
    out = R.forward(e, W)["out"]
    u = e.sum(1)
    _close(out[:, 1], (u * u).sum(1))
    assert out[:, [0, 2]].abs().max().item() <= 1e-12 * (u * u).sum(1).max().item() * 64


def test_closed_form_backward_equals_autograd():
    rng = np.random.default_rng(2)
    for B, F, D, N in ((3, 1, 4, 1), (4, 3, 8, 5), (2, 2, 12, 7)):
        e = torch.from_numpy(rng.normal(size=(B, F, D))).requires_grad_(True)
        W = torch.from_numpy(rng.normal(size=(D * D, N))).requires_grad_(True)
        add = torch.from_numpy(rng.normal(size=(B, N))).requires_grad_(True)
        g = torch.from_numpy(rng.normal(size=(B, N)))
        want = torch.autograd.grad(R.forward(e, W, add)["out"], [e, W, add], grad_outputs=g)
        with torch.no_grad():
            d_emb, dW = R.backward(e, W, g)
        _close(d_emb, want[0])
        _close(dW, want[1])
        _close(g, want[2])


@pytest.mark.parametrize("index", GRID, ids=ID)
def test_grid_cases_are_exact_in_fp32(index):
    c = R.case(index)
    assert R.grid_conditions(c["shape"]), c["shape"]
    with torch.no_grad():
        f = R.forward(c["e"].float(), c["W"].float(), c["addend"].float())
        d_emb, dW = R.backward(c["e"].float(), c["W"].float(), c["g"].float())
    assert torch.equal(f["u"].double(), c["fwd"]["u"]) and torch.equal(f["out"].double(), c["fwd"]["out"] + c["addend"])
    assert torch.equal(d_emb.double(), c["grads"][0]) and torch.equal(dW.double(), c["grads"][1])
    assert c["fwd"]["out"].abs().max().item() > 0 and c["grads"][0].abs().max().item() > 0 and c["grads"][1].abs().max().item() > 0


def _other_association(e, W, g):
    """fp32 in another order than torch's: the field sum reversed, k in sequential chunks of 4 taken in reverse, the batch in sequential
    chunks of 4.  Reads at most 1.11 max(r32, 8 u) over the six normal shapes (out at 40 x 4 x 32 x 24)."""
    B, F, D = e.shape
    u = torch.zeros((B, D), dtype=torch.float32)
    for i in reversed(range(F)):
        u = u + e[:, i]
    outer = (u[:, :, None] * u[:, None, :]).reshape(B, D * D)
    out = torch.zeros((B, W.shape[1]), dtype=torch.float32)
    for k in reversed(range(0, D * D, 4)):
        out = out + outer[:, k:k + 4] @ W[k:k + 4]
    dW = torch.zeros_like(W)
    for b in range(0, B, 4):
        dW = dW + outer[b:b + 4].T @ g[b:b + 4]
    W3 = W.reshape(D, D, -1)
    S = torch.zeros((B, D, D), dtype=torch.float32)
    for n in reversed(range(0, W.shape[1], 4)):
        S = S + torch.einsum("bn,den->bde", g[:, n:n + 4], W3[:, :, n:n + 4])
    S = S + S.transpose(1, 2)
    du = torch.zeros((B, D), dtype=torch.float32)
    for k in reversed(range(0, D, 4)):
        du = du + torch.einsum("bde,be->bd", S[:, :, k:k + 4], u[:, k:k + 4])
    return dict(u=u, out=out, d_emb=du[:, None, :].expand(B, F, D), dW=dW)


@pytest.mark.parametrize("index", NORMAL, ids=ID)
def test_another_fp32_association_stays_within_the_gpu_limit(index):
    c = R.case(index)
    r32 = R.errors32(index)
    with torch.no_grad():
        got = _other_association(c["e"].float(), c["W"].float(), c["g"].float())
    want = dict(u=c["fwd"]["u"], out=c["fwd"]["out"], d_emb=c["grads"][0], dW=c["grads"][1])
    for name in ("u", "out", "d_emb", "dW"):
        err = (got[name].double() - want[name]).abs().max().item() / want[name].abs().max().item()
        limit = 16 * max(r32[name], 8 * U)
        print("%s %s: %.2f max(r32, 8u)" % (name, c["shape"], err / max(r32[name], 8 * U)))
        assert err <= limit, (name, err, limit)


def test_inner_part_with_rank_one_weights_is_the_papers_squared_norm():
    rng = np.random.default_rng(4)
    B, F, D = 5, 6, 8
    e = torch.from_numpy(rng.normal(size=(B, F, D)))
    theta = torch.from_numpy(rng.normal(size=(F,)))
    w = torch.stack([(theta[i] * theta[j]) * (1.0 if i == j else 2.0) for i in range(F) for j in range(i + 1)])
    assert R.inner(e, True).shape == (B, F * (F + 1) // 2) and R.inner(e, False).shape == (B, F * (F - 1) // 2)
    got = R.inner(e, True) @ w
    want = ((theta[None, :, None] * e).sum(1) ** 2).sum(1)
    _close(got, want)
    assert R.inner(e, False)[:, 1].allclose((e[:, 2] * e[:, 0]).sum(1))                        # (1,0), (2,0), (2,1), ...


def test_pnn_logits_equal_a_written_out_composition():
    rng = np.random.default_rng(5)
    t = lambda *s: torch.from_numpy(rng.normal(size=s))                                        # noqa: E731
    B, F, D, D1, D2 = 4, 3, 4, 5, 3
    e, w_z, b1, w_in, w_out = t(B, F, D), t(F * D, D1), t(D1), t(3, D1), t(D * D, D1)
    k2, c2, k3, c3 = t(D1, D2), t(D2), t(D2, 1), t(1)
    u = e[:, 0] + e[:, 1] + e[:, 2]
    lz = torch.cat([e[:, 0], e[:, 1], e[:, 2]], dim=1) @ w_z
    ips = torch.stack([(e[:, 1] * e[:, 0]).sum(1), (e[:, 2] * e[:, 0]).sum(1), (e[:, 2] * e[:, 1]).sum(1)], dim=1)
    lp = torch.stack([sum(u[:, d] * u[:, f] * w_out[d * D + f, n] for d in range(D) for f in range(D)) for n in range(D1)], dim=1)
    for use_in, use_out in ((True, False), (False, True), (True, True)):
        pre = lz + b1 + (ips @ w_in if use_in else 0) + (lp if use_out else 0)
        want = torch.relu(torch.relu(pre) @ k2 + c2) @ k3 + c3
        got = R.pnn_logits(e, w_z, b1, w_in if use_in else None, w_out if use_out else None, [k2, k3], [c2, c3])
        assert got.shape == (B, 1)
        _close(got, want)
    _close(R.pnn_logits(e, w_z, b1, None, w_out, [torch.ones((D1, 1), dtype=DD)], [c3], activation="tanh"),
           torch.tanh(lz + b1 + lp).sum(1, keepdim=True) + c3)


def _columns(F=4, D=8):
    from deep_recommenders_amd import feature_column as fc
    cats = [fc.categorical_column_with_identity("c%d" % i, 50) for i in range(F)]
    return [fc.embedding_column(c, D) for c in cats]


def test_pnn_config_constructor_errors_and_exports():
    from deep_recommenders_amd.keras.models import ranking
    from deep_recommenders_amd.keras.models.ranking import PNN, OuterProduct
    assert ranking.PNN is PNN and ranking.OuterProduct is OuterProduct
    emb = _columns()
    model = PNN(emb, [16, 8], use_inner=True, use_outer=True, device="cpu", name="p")
    assert model.get_config() == {"name": "p", "dnn_units_size": [16, 8], "use_inner": True, "use_outer": True,
                                  "self_interaction": False, "activation": "relu"}
    assert PNN(emb, [4], device="cpu").get_config() == {"dnn_units_size": [4], "use_inner": True, "use_outer": False,
                                                         "self_interaction": False, "activation": "relu"}
    assert model.slab.lin_w is None and model.outer.get_config() == {"units": 16} and PNN(emb, [4], device="cpu").outer is None
    with pytest.raises(ValueError, match="product layer"):
        PNN(emb, [16], use_inner=False, use_outer=False, device="cpu")
    with pytest.raises(ValueError, match="dnn_units_size"):
        PNN(emb, [], device="cpu")
    with pytest.raises(ValueError, match="activation"):
        PNN(emb, [16], activation="gelu", device="cpu")
    with pytest.raises(ValueError, match="up to 128"):
        PNN(_columns(2, 256), [16], use_outer=True, device="cpu")
    assert OuterProduct(2, name="x").get_config() == {"name": "x", "units": 2}
    for bad in (0, 4097, 2.5):
        with pytest.raises(ValueError, match="units"):
            OuterProduct(bad)
    with pytest.raises(ValueError, match="dim should be 3"):
        OuterProduct(4)(np.zeros((2, 12), np.float32))
    layer = OuterProduct(4)
    layer.build((2, 3, 8), device="cpu")
    assert tuple(layer.W.shape) == (64, 4) and float(layer.W.detach().abs().max()) <= np.sqrt(6.0 / 68)
    with pytest.raises(ValueError, match="dim should be 3"):
        OuterProduct(4).build((2, 24))


def test_argument_errors_need_no_device():
    from deep_recommenders_amd import layers, ops
    z = torch.zeros
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.pnn_outer_fwd(z(2, 3, 6), z(36, 4), 3)
    with pytest.raises(ValueError, match=r"\[4, 128\]"):
        ops.pnn_outer_fwd(z(2, 1, 132), z(132 * 132, 4), 1)
    with pytest.raises(ValueError, match="1 <= F <= 64"):
        ops.pnn_outer_fwd(z(2, 0, 8), z(64, 4), 0)
    with pytest.raises(ValueError, match="1 <= F <= 64"):
        ops.pnn_outer_fwd(z(2, 65 * 4), z(16, 4), 65)
    with pytest.raises(ValueError, match=r"\[1, 4096\]"):
        ops.pnn_outer_fwd(z(2, 3, 4), z(16, 4097), 3)
    with pytest.raises(ValueError, match=r"\[1, 4096\]"):
        ops.pnn_outer_fwd(z(2, 3, 4), z(16, 0), 3)
    with pytest.raises(ValueError, match="W must be"):
        ops.pnn_outer_fwd(z(2, 3, 8), z(60, 4), 3)
    with pytest.raises(ValueError, match="W must be"):
        ops.pnn_outer_fwd(z(2, 3, 8), z(64), 3)
    with pytest.raises(ValueError, match="emb must be"):                                       # 25 columns, F = 3
        ops.pnn_outer_fwd(z(2, 25), z(64, 4), 3)
    with pytest.raises(ValueError, match="3-d emb"):
        ops.pnn_outer_fwd(z(2, 4, 8), z(64, 4), 3)
    with pytest.raises(ValueError, match="fp32"):
        ops.pnn_outer_fwd(z(2, 3, 8, dtype=torch.float64), z(64, 4), 3)
    with pytest.raises(ValueError, match="row stride"):                                        # pitch 25
        ops.pnn_outer_fwd(z(2, 25)[:, :24], z(64, 4), 3)
    with pytest.raises(ValueError, match="addend"):
        ops.pnn_outer_fwd(z(2, 3, 8), z(64, 4), 3, addend=z(2, 5))
    with pytest.raises(ValueError, match="out"):
        ops.pnn_outer_fwd(z(2, 3, 8), z(64, 4), 3, out=z(3, 4))
    with pytest.raises(ValueError, match="row stride"):                                        # an output is not copied
        ops.pnn_outer_fwd(z(2, 3, 8), z(64, 4), 3, out=z(2, 5)[:, :4])
    with pytest.raises(ValueError, match="d_out"):
        ops.pnn_outer_bwd(z(2, 8), z(64, 4), 3, z(2, 6))
    with pytest.raises(ValueError, match="d_emb"):
        ops.pnn_outer_bwd(z(2, 8), z(64, 4), 3, z(2, 4), d_emb=z(2, 16))
    with pytest.raises(ValueError, match="accumulate"):
        ops.pnn_outer_bwd(z(2, 8), z(64, 4), 3, z(2, 4), accumulate=True)
    with pytest.raises(ValueError, match="u must be"):
        ops.pnn_outer_bwd(z(2, 3, 8), z(64, 4), 3, z(2, 4))
    with pytest.raises(ValueError, match="1 <= F <= 64"):
        ops.pnn_outer_bwd(z(2, 8), z(64, 4), 65, z(2, 4))
    with pytest.raises(ValueError, match="together with F"):
        layers.pnn_outer(z(2, 24), z(64, 4))
    with pytest.raises(ValueError, match="does not match"):
        layers.pnn_outer(z(2, 3, 8), z(64, 4), F=4)


def test_kernel_source_has_no_atomics_and_no_allocation():
    """the contract's static half: the products run on the fp32-input MFMA, sums have one owner (no atomic of any kind), and the file
    allocates nothing, copies nothing and reads no environment"""
    import os
    import re
    from deep_recommenders_amd import build
    src = open(os.path.join(build.CSRC, "pnn_outer.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in code
    for word in ("atomic", "hipMalloc", "hipMemcpy", "getenv"):
        assert word not in code, word
