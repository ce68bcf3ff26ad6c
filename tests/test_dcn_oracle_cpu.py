"""The DCN oracle harnesses (tests/dcn_oracle.py) have teeth -- no GPU needed.

dcn_engine.DCNDense runs on the CPU with the oracle-backed primitives of tests/test_sharded_gloo.py (torch fp32 restatements of each
kernel) at the `wide-diag` and `mixed-mlp` shapes of tests/test_gpu_dcn_matrix.py: unmodified it passes harness A (the gradient bucket
against the float64 gradients, two calls) and harness B's update checks (grads=None, three steps), a few per cent inside every bound;
each planted error -- a primitive subclassed to go wrong the way a kernel or its call does -- fails.
"""
import pytest
import torch

import dcn_oracle as DO
from test_sharded_gloo import OraclePrims

SHAPES = {                       # in_dim, L, units, B, diag (the matrix's rows of the same names)
    "wide-diag": (131, 3, [256, 128], 2048, 0.25),
    "mixed-mlp": (131, 3, [64, 128, 32], 2048, 0.0),
}


def _problem(shape, prims, bucket, steps=1):
    in_dim, L, units, B, diag = SHAPES[shape]
    return DO.DenseProblem(in_dim, L, units, B, diag, "cpu", prims=prims, bucket=bucket, steps=steps)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fp32_dense_half_passes_the_bucket_harness(shape):
    pb = _problem(shape, OraclePrims, True)
    assert DO.gates(pb.dense) == {"h2": False, "cross": ["PlainWeight"] * 3, "mlp": ["PlainWeight"] * (len(SHAPES[shape][2]) + 1),
                                  "diag0": SHAPES[shape][4] == 0.0}
    ratios = DO.run_bucket_harness(pb)
    print("%s: harness A, worst error / tolerance (fp32 against float64): %s" % (shape, {k: round(v, 4) for k, v in ratios.items()}))
    assert max(ratios.values()) < 1.0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fp32_dense_half_passes_the_update_checks(shape):
    ratios = DO.run_inplace_harness(_problem(shape, OraclePrims, False, steps=3))
    print("%s: harness B, worst error / tolerance over 3 steps (fp32 against float64): %s" % (shape, {k: round(v, 4) for k, v in ratios.items()}))
    assert max(ratios.values()) < 1.0


class _DropsDiag(OraclePrims):
    @staticmethod
    def cross_combine_bwd(x0, prod, d_out, diag_scale, d_x0_accum, d_x_accum):
        d_prod = d_out * x0
        d_x0_accum.add_(d_out * prod)
        if d_x_accum is not None:
            d_x_accum.add_(d_out)
        return d_prod


class _X0ForProd(OraclePrims):
    @staticmethod
    def cross_combine_bwd(x0, prod, d_out, diag_scale, d_x0_accum, d_x_accum):
        return OraclePrims.cross_combine_bwd(x0, x0, d_out, diag_scale, d_x0_accum, d_x_accum)


class _ProdWithoutBias(OraclePrims):
    @staticmethod
    def cross_fwd(x0, x, W, b, diag_scale=0.0, want_prod=False, prod=None):
        out, pr = OraclePrims.cross_fwd(x0, x, W, b, diag_scale, want_prod, prod)
        return out, pr - b


class _MaskGreaterEqual(OraclePrims):
    @staticmethod
    def linear_bwd_dx(dy, W, relu_src=None, accumulate=False, out=None):
        dx = dy @ W.t()
        if relu_src is not None:
            dx = dx * (relu_src >= 0)
        return out.add_(dx) if accumulate else out.copy_(dx)


class _NoBiasGradient(OraclePrims):
    @staticmethod
    def linear_bwd_dw(x, dy, scale, dstW, dstb=None, workspace=None):
        OraclePrims.linear_bwd_dw(x, dy, scale, dstW, None)


class _HalfScale(OraclePrims):
    @staticmethod
    def linear_bwd_dw(x, dy, scale, dstW, dstb=None, workspace=None):
        OraclePrims.linear_bwd_dw(x, dy, scale / 2, dstW, dstb)


class _StaleDTop(OraclePrims):
    """The first MLP layer's dgrad adds to d_top instead of overwriting it (d_top is the only [B, 131] dgrad target of these shapes):
    right on the first call, where d_top is zero, wrong on every later one."""
    @staticmethod
    def linear_bwd_dx(dy, W, relu_src=None, accumulate=False, out=None):
        return OraclePrims.linear_bwd_dx(dy, W, relu_src, accumulate or out.shape[1] == 131, out)


PLANTS = {"combine drops diag * d_prod": _DropsDiag, "combine adds d_out * x0 to d_x0": _X0ForProd, "cross_fwd's prod lacks the bias": _ProdWithoutBias,
          "dgrad masks with >= 0": _MaskGreaterEqual, "wgrad leaves out the bias": _NoBiasGradient, "wgrad with scale / 2": _HalfScale,
          "second step starts from a non-zero d_top": _StaleDTop}
# (diag is 0 at mixed-mlp: dropping diag * d_prod is no error there)
PLANT_CASES = [(s, p) for s in SHAPES for p in PLANTS if not (s == "mixed-mlp" and p == "combine drops diag * d_prod")]


@pytest.mark.parametrize("shape,plant", PLANT_CASES)
def test_planted_error_fails_the_bucket_harness(shape, plant):
    with pytest.raises(AssertionError) as e:
        DO.run_bucket_harness(_problem(shape, PLANTS[plant], True))
    print("%s / %s fails harness A with: %s" % (shape, plant, str(e.value)[:160]))


@pytest.mark.parametrize("shape,plant", PLANT_CASES)
def test_planted_error_fails_the_update_checks(shape, plant):
    with pytest.raises(AssertionError) as e:
        DO.run_inplace_harness(_problem(shape, PLANTS[plant], False, steps=2))
    print("%s / %s fails harness B with: %s" % (shape, plant, str(e.value)[:160]))
