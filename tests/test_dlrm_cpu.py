"""CPU checks of the DLRM restatement the GPU tests compare against (tests/dlrm_ref.py) and of the configuration surface of
DotInteraction and DLRM."""
import numpy as np
import pytest
import torch

import dlrm_ref as R

DD = torch.float64


def _close(got, want, tol=1e-12):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())


def test_triangle_order_on_a_hand_written_case():
    """N = 3, D = 2: t_0 = (1, 2), t_1 = (3, 4), t_2 = (5, 6), so <t_1, t_0> = 11, <t_2, t_0> = 17, <t_2, t_1> = 39 and the squares are
    5, 25, 61.  Row-major lower triangle: (1,0), (2,0), (2,1) without the diagonal; (0,0), (1,0), (1,1), (2,0), (2,1), (2,2) with it."""
    dense = torch.tensor([[1.0, 2.0]], dtype=DD)
    emb = torch.tensor([[[3.0, 4.0], [5.0, 6.0]]], dtype=DD)
    assert R.dot_interaction(dense, emb, False).tolist() == [[1, 2, 11, 17, 39]]
    assert R.dot_interaction(dense, emb, True).tolist() == [[1, 2, 5, 11, 25, 17, 39, 61]]
    all3 = torch.tensor([[[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]], dtype=DD)                      # the same three vectors, no dense one
    assert R.dot_interaction(None, all3, False).tolist() == [[11, 17, 39]]
    assert R.dot_interaction(None, all3, True).tolist() == [[5, 11, 25, 17, 39, 61]]
    # an asymmetric check of (row, col): swapping two fields permutes the triangle, it does not leave it in place
    swapped = all3[:, [1, 0, 2]]
    assert R.dot_interaction(None, swapped, False).tolist() == [[11, 39, 17]]


def test_symmetric_gradient_on_a_hand_written_case():
    g = torch.tensor([[1.0, 2.0, 3.0]], dtype=DD)
    assert R.symmetric_gradient(g, 3, False).tolist() == [[[0, 1, 2], [1, 0, 3], [2, 3, 0]]]
    g = torch.tensor([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]], dtype=DD)
    assert R.symmetric_gradient(g, 3, True).tolist() == [[[2, 2, 4], [2, 6, 5], [4, 5, 12]]]  # the diagonal doubled


@pytest.mark.parametrize("self_interaction", [False, True])
@pytest.mark.parametrize("has_dense", [False, True])
@pytest.mark.parametrize("B,F,D", [(3, 1, 4), (4, 5, 3), (2, 16, 8)])
def test_closed_form_backward_equals_autograd(B, F, D, has_dense, self_interaction):
    if F + int(has_dense) < 2:
        F = 2
    rng = np.random.default_rng(100 * F + 10 * D + 2 * int(has_dense) + int(self_interaction))
    t = lambda *s: torch.from_numpy(rng.normal(size=s))                                       # noqa: E731
    dense = t(B, D).requires_grad_(True) if has_dense else None
    emb = t(B, F, D).requires_grad_(True)
    out = R.dot_interaction(dense, emb, self_interaction)
    N = F + int(has_dense)
    assert out.shape == (B, (D if has_dense else 0) + (N * (N + 1) // 2 if self_interaction else N * (N - 1) // 2))
    d_out = t(*out.shape)
    want = torch.autograd.grad((out * d_out).sum(), [emb] + ([dense] if has_dense else []))
    with torch.no_grad():
        d_dense, d_emb = R.dot_interaction_backward(dense, emb, d_out, self_interaction)
    _close(d_emb, want[0])
    if has_dense:
        _close(d_dense, want[1])
    else:
        assert d_dense is None


def test_dlrm_logits_equal_the_written_out_composition():
    rng = np.random.default_rng(3)
    t = lambda *s: torch.from_numpy(rng.normal(size=s))                                       # noqa: E731
    B, F, D, Nd = 6, 3, 4, 5
    emb, x = t(B, F, D), t(B, Nd)
    W1, b1, W2, b2 = t(Nd, 7) * 0.3, t(7) * 0.1, t(7, D) * 0.3, t(D) * 0.1
    V1, c1, V2, c2 = t(D + 6, 8) * 0.3, t(8) * 0.1, t(8, 1), t(1)
    bottom = torch.relu(torch.relu(x @ W1 + b1) @ W2 + b2)
    T = torch.cat([bottom[:, None], emb], dim=1)
    z = torch.stack([(T[:, i] * T[:, j]).sum(-1) for i, j in ((1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2))], dim=1)
    want = torch.relu(torch.cat([bottom, z], dim=1) @ V1 + c1) @ V2 + c2
    _close(R.dlrm_logits(emb, x, [W1, W2], [b1, b2], [V1, V2], [c1, c2], 1, False), want)
    V1e = t(3, 8) * 0.3
    z = torch.stack([(emb[:, i] * emb[:, j]).sum(-1) for i, j in ((1, 0), (2, 0), (2, 1))], dim=1)
    _close(R.dlrm_logits(emb, None, [], [], [V1e, V2], [c1, c2], 1, False), torch.relu(z @ V1e + c1) @ V2 + c2)


def _columns(F=4, D=8):
    from deep_recommenders_amd import feature_column as fc
    return [fc.embedding_column(fc.categorical_column_with_identity("c%d" % i, 50), D) for i in range(F)]


def test_dlrm_config_and_constructor_errors():
    from deep_recommenders_amd.keras.models.ranking import DLRM, DotInteraction
    model = DLRM(_columns(), bottom_units_size=[16, 8], top_units_size=[16], dense_features_key="dense", device="cpu", name="d")
    assert model.get_config() == {"name": "d", "bottom_units_size": [16, 8], "top_units_size": [16], "dense_features_key": "dense",
                                  "activation": "relu", "self_interaction": False}
    assert model.slab.lin_w is None                                                           # no linear term
    with pytest.raises(ValueError, match="embedding dimension 8"):
        DLRM(_columns(), bottom_units_size=[16, 4], top_units_size=[16], dense_features_key="dense", device="cpu")
    with pytest.raises(ValueError, match="embedding dimension 8"):
        DLRM(_columns(), bottom_units_size=[], top_units_size=[16], dense_features_key="dense", device="cpu")
    with pytest.raises(ValueError, match="activation"):
        DLRM(_columns(), [8], [16], "dense", activation="gelu", device="cpu")
    only = DLRM(_columns(), bottom_units_size=None, top_units_size=[16], dense_features_key=None, self_interaction=True, device="cpu")
    assert only.get_config()["bottom_units_size"] == [] and only.get_config()["self_interaction"] is True
    assert DotInteraction().get_config() == {"self_interaction": False}
    assert DotInteraction(True, name="x").get_config() == {"name": "x", "self_interaction": True}
    with pytest.raises(ValueError, match="dim should be 3"):
        DotInteraction()(np.zeros((2, 12), np.float32))


def test_interaction_width_and_argument_errors_need_no_device():
    from deep_recommenders_amd import ops
    assert ops.dot_interact_width(26, 64) == 64 + 27 * 26 // 2
    assert ops.dot_interact_width(26, 64, dense=False, self_interaction=True) == 26 * 27 // 2
    emb = torch.zeros((2, 3 * 6))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.dot_interact_fwd(None, emb, 3, 6)
    with pytest.raises(ValueError, match="2 <= N <= 64"):
        ops.dot_interact_fwd(None, torch.zeros((2, 8)), 1, 8)


def test_kernel_source_has_no_atomics_and_no_allocation():
    """the contract's static half: sums have one owner (no atomic of any kind) and there is nowhere to put a [B, N, N] matrix -- the entry
    points take no workspace and the file allocates nothing"""
    import os
    import re
    from deep_recommenders_amd import build
    src = open(os.path.join(build.CSRC, "dot_interact.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in code
    for word in ("atomic", "hipMalloc", "hipMemcpy", "getenv"):
        assert word not in code, word
