"""CPU checks of the DIN restatement the GPU tests compare against (tests/din_ref.py) and of the layers' configuration surface."""
import numpy as np
import pytest
import torch

import din_ref as R


@pytest.mark.parametrize("eps", [1e-7, 1e-8, 1e-9, 1e-10])
def test_dice_ref_reproduces_the_reference_test(eps):
    """tests/keras/test_din.py:50-64 of the reference: the numpy expression of its lines 57-61 (alpha is zero), assertAllClose defaults"""
    inputs = np.asarray([[-0.2, -0.1, 0.1, 0.2]]).astype(np.float32)
    p = (inputs - inputs.mean()) / np.sqrt(inputs.std() + eps)
    p = 1 / (1 + np.exp(-p))
    x = np.where(inputs > 0, inputs, np.zeros_like(inputs))
    expected = np.where(x > 0, p * x, (1 - p) * x)
    for dtype in (torch.float64, torch.float32):
        got = R.dice(torch.from_numpy(inputs).to(dtype), torch.zeros(4, dtype=dtype), eps).numpy()
        np.testing.assert_allclose(got, expected, rtol=1e-6, atol=1e-6)


def _pool_inputs(rng, B, T, D, U, mode, bias=True):
    t = lambda *s: torch.from_numpy(rng.normal(size=s))                                       # noqa: E731
    n_in = 2 if mode == 0 else 3
    mask = torch.from_numpy(rng.random((B, T)) < 0.7)
    return dict(query=t(B, D), keys=t(B, T, D), mask=mask, W=t(n_in * D, U) * 0.3, b=t(U) * 0.1 if bias else None, w_out=t(U, 1) * 0.3,
                b_out=t(1) * 0.1 if bias else None, alpha=t(U) * 0.25)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("act", [1, 4])
def test_folded_form_equals_composed_form(mode, act):
    a = _pool_inputs(np.random.default_rng(10 + mode), 5, 9, 8, 6, mode)
    out_c, sc_c = R.pool(mode=mode, act=act, **a)
    out_f, sc_f = R.pool_folded(mode=mode, act=act, **a)
    assert (sc_c - sc_f).abs().max().item() <= 1e-12 * max(1.0, sc_c.abs().max().item())
    assert (out_c - out_f).abs().max().item() <= 1e-12 * max(1.0, out_c.abs().max().item())


def test_dice_closed_form_backward_equals_autograd():
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.normal(size=(7, 11))).requires_grad_(True)
    x.data[2, 3] = 0.0
    alpha = torch.from_numpy(rng.normal(size=11) * 0.5).requires_grad_(True)
    dy = torch.from_numpy(rng.normal(size=(7, 11)))
    R.dice(x, alpha, 1e-8).backward(dy)
    dx, dalpha = R.dice_backward(x.detach(), alpha.detach(), dy, 1e-8)
    assert (dx - x.grad).abs().max().item() <= 1e-12 * x.grad.abs().max().item()
    assert (dalpha - alpha.grad).abs().max().item() <= 1e-12 * alpha.grad.abs().max().item()


def test_dice_backward_is_finite_on_constant_rows():
    x = torch.tensor([[0.5, 0.5, 0.5], [0.0, 0.0, 0.0], [-1.0, 2.0, 0.25]], dtype=torch.float64, requires_grad=True)
    alpha = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64, requires_grad=True)
    dy = torch.ones_like(x)
    R.dice(x, alpha).backward(dy)
    dx, dalpha = R.dice_backward(x.detach(), alpha.detach(), dy)
    assert torch.isfinite(x.grad).all() and torch.isfinite(alpha.grad).all() and torch.isfinite(dx).all() and torch.isfinite(dalpha).all()
    assert (dx - x.grad).abs().max().item() <= 1e-12
    one = torch.tensor([[1.5]], dtype=torch.float64, requires_grad=True)                       # N == 1: always constant
    R.dice(one, torch.zeros(1, dtype=torch.float64)).backward(torch.ones(1, 1, dtype=torch.float64))
    assert torch.isfinite(one.grad).all()


def test_configs_carry_the_reference_keys():
    from deep_recommenders_amd.keras.models.ranking import din
    cfg = din.Dice(epsilon=1e-9).get_config()
    assert set(cfg) >= {"epsilon", "alpha_initializer", "alpha_regularizer"}
    assert cfg["epsilon"] == 1e-9 and cfg["alpha_initializer"] == "zeros" and cfg["alpha_regularizer"] is None
    act = din.Dice()
    pool = din.InterestPooling(36, interacter=din.Multiply(), activation=act)
    cfg = pool.get_config()
    assert set(cfg) >= {"units", "interacter", "use_bias", "activation", "kernel_init", "kernel_regu", "bias_init", "bias_regu"}
    assert cfg["units"] == 36 and cfg["activation"] is act and cfg["use_bias"] is True
    assert set(din.ActivationUnit(4, activation="tanh").get_config()) == set(din.InterestPooling(4).get_config())
    with pytest.raises(NotImplementedError):
        din.Dice(alpha_regularizer="l2")
    with pytest.raises(NotImplementedError):
        din.InterestPooling(4, interacter=lambda xy: xy[0] + xy[1])        # an interacter without a `mode`
    with pytest.raises(NotImplementedError):
        din.ActivationUnit(4, activation="gelu")
