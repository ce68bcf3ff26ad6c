"""Every DCNEngine / DCNDense kernel path against a float64 oracle.

dcn_engine.DCNDense -- the dense half of DCNEngine (bench.py --model dcn) and sharded.ShardedDCNEngine -- picks a GEMM family per weight
and a buffer arrangement per cross layer from B, in_dim, the layer widths, diag_scale, `grads` and the two process-wide GEMM switches.
The bench shape (all wide, f16x2, diag 0) and a toy with every gate off have their one-step oracle tests; every other arrangement was
only ever compared with another arrangement.  Each row of CASES builds the smallest shape that opens its gates, ASSERTS the gate row
(tests/dcn_oracle.py gates(): a case must not pass on another path) and runs through two harnesses.  "same" = F 2, D 64, Nd 3 (in_dim 131,
ld 132), L 3, units [256, 128], B 2048, split f16x2, diag 0.25; the DCNDense branch a row is there for:

  wide-diag      same.  Cross stack and both hidden layers H2WeightPlanes, head plain: dr_h2_cross_fwd with diag inside the stack,
                 cross_combine_bwd into a SEPARATE zero-filled d_x (`d_x is d_out` false) and with d_prod_amax at the same time
  wide-diag-bf16x3  split bf16x3: the same layers on WeightPlanes (dr_bf3_cross_fwd with diag), h2 off, no record anywhere
  wide-diag0     diag 0, Nd 0 (in_dim 128 = ld): the cross dgrad accumulates into d_out itself (`d_x is d_out`), no padding column
  ragged-32      B 2080: a 256-row tile with 32 rows used (the tile-edge branch of the GEMM epilogues, cross code included)
  ragged-odd     B 2050: the per-element edge epilogue, with diag
  mixed-mlp      units [64, 128, 32], diag 0: MLP layers plain / f16x2 / plain -- the dr_h2_amax pass in front of an f16x2 layer whose
                 producer is plain, forward (`if g.wants_amax and xam is None`) and backward (`... and dyam is None`)
  plain-cross-planes-mlp  F 1, Nd 5 (in_dim 69), L 2, units [128], diag 0.1: cross stack not wide -> PlainWeight, h2 off, so the wide
                 MLP layer runs on WeightPlanes (bf16x3) although the library reports f16x2
  below-2048     B 2016, diag 0: no gate opens, every product on PlainWeight with its deterministic dw workspace
  native         set_gemm_mode("native"): planes_worthwhile is off at the wide shape, everything PlainWeight
  no-cross       L 0: the MLP reads x0 and its record directly, d_x0 is what the first layer's dgrad left in d_top
  cross-only     dnn_units [], L 2, diag 0.1: Dense(1) directly on x_L (no ReLU, no dhs)
  d16-hot        F 8, D 16, Nd 3 (in_dim 131), 40 distinct keys per field: K3 / K4 at another row width, rows shared by ~50 slots

A  gradient bucket (DCNDense with grads=(...), no tables; weights allocated as DCNEngine allocates them): one step() on a zeroed bucket
   -- loss 1e-5 relative; d_x0 and every bucket tensor max |err| <= 2e-5 * max |want| against the float64 gradient (the figure
   tests/test_gpu_h2_gemm.py holds the two splits to; the kernel tests bound one product at 3e-6 - 5e-6; fp32 torch is within 6e-7 at
   these shapes: tests/test_dcn_oracle_cpu.py) -- weights bit-unchanged, bucket padding untouched; a second step() on the same inputs
   without zeroing: loss and d_x0 BIT-identical (d_top and the aliased d_out carry nothing over), bucket = twice the gradient; with h2
   every amax record the step wrote = the float bits of its tensor's true max |.|, every other record still 0.
B  DCNEngine.train_step, three steps at lr 1.0 (tests/test_gpu_benchcfg.py: at 0.01 a row's update is below the row's fp32 spacing),
   each against one float64 step from the device's own state read just before it: ids bit-exact, loss 1e-5 relative, every parameter and
   the touched table rows through _assert_update(rel=1e-2) (the DCN figure of tests/test_gpu_benchcfg.py), every other row of the table
   bit-identical, the oracle's update of every parameter visible in fp32.  wide-diag and wide-diag-bf16x3 write one cross weight and
   one MLP weight from outside (W.mul_(0.5)) between steps 2 and 3: step 3 must run on re-split planes (ensure_fresh).
"""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import dcn_oracle as DO
from oracle import torch_ref as T

H2, WP, PL = "H2WeightPlanes", "WeightPlanes", "PlainWeight"
_S = dict(F=2, V=3000, D=64, Nd=3, L=3, units=[256, 128], B=2048, diag=0.25, split="f16x2", mode=None, keys=None, poke=False)


def _case(h2, cross, mlp, **kw):
    c = dict(_S, h2=h2, cross=cross, mlp=mlp)
    c.update(kw)
    return c


CASES = {
    "wide-diag": _case(True, [H2] * 3, [H2, H2, PL], poke=True),
    "wide-diag-bf16x3": _case(False, [WP] * 3, [WP, WP, PL], split="bf16x3", poke=True),
    "wide-diag0": _case(True, [H2] * 3, [H2, H2, PL], diag=0.0, Nd=0),
    "ragged-32": _case(True, [H2] * 3, [H2, H2, PL], B=2080),
    "ragged-odd": _case(True, [H2] * 3, [H2, H2, PL], B=2050),
    "mixed-mlp": _case(True, [H2] * 3, [PL, H2, PL, PL], units=[64, 128, 32], diag=0.0),
    "plain-cross-planes-mlp": _case(False, [PL] * 2, [WP, PL], F=1, Nd=5, L=2, units=[128], diag=0.1),
    "below-2048": _case(False, [PL] * 3, [PL, PL, PL], B=2016, diag=0.0),
    "native": _case(False, [PL] * 3, [PL, PL, PL], mode="native"),
    "no-cross": _case(True, [], [H2, H2, PL], L=0),
    "cross-only": _case(True, [H2] * 2, [PL], units=[], L=2, diag=0.1),
    "d16-hot": _case(True, [H2] * 3, [H2, H2, PL], F=8, D=16, keys="hot"),
}


def _assert_gates(name, c, dense):
    from deep_recommenders_amd import ops
    assert ops.get_gemm_split() == c["split"] and ops.get_gemm_mode() == (c["mode"] or "bf16x3")
    got = DO.gates(dense)
    want = {"h2": c["h2"], "cross": c["cross"], "mlp": c["mlp"], "diag0": c["diag"] == 0.0}
    assert got == want, "%s runs on another path than its row says: %s, not %s" % (name, got, want)
    in_dim = c["F"] * c["D"] + c["Nd"]
    assert dense.in_dim == in_dim and dense.ld == (in_dim + 3) // 4 * 4 and (dense.ld == in_dim) == (name == "wide-diag0")
    for g in list(dense.cross_gemm) + list(dense.gemm):
        if type(g) is ops.PlainWeight:
            assert g.dw_ws is not None, "a plain product without its deterministic dw workspace"
        else:
            assert g.wgrad_ws is not None


def _with_switches(c, fn, *args):
    """fn(*args) under the case's operand split and product mode; both process-wide switches are put back whatever happens."""
    from deep_recommenders_amd import ops
    prev_split = ops.set_gemm_split(c["split"])
    prev_mode = None
    try:
        if c["mode"]:
            prev_mode = ops.set_gemm_mode(c["mode"])
        return fn(*args)
    finally:
        ops.set_gemm_split(prev_split)
        if prev_mode is not None:
            ops.set_gemm_mode(prev_mode)


@pytest.mark.parametrize("name", list(CASES))
def test_dcn_dense_gradient_bucket_matches_float64_gradients(name):
    """Harness A of the module docstring."""
    _with_switches(CASES[name], _bucket_case, name, CASES[name])


def _bucket_case(name, c):
    t0 = time.time()
    in_dim = c["F"] * c["D"] + c["Nd"]
    pb = DO.DenseProblem(in_dim, c["L"], c["units"], c["B"], c["diag"], "cuda", bucket=True,
                         rows=(c["F"], c["D"], 40) if c["keys"] == "hot" else None)
    _assert_gates(name, c, pb.dense)
    ratios = DO.run_bucket_harness(pb, records=c["h2"])
    worst = max(ratios, key=ratios.get)
    print("%s: bucket harness %.1f s, worst error / tolerance %.3f (%s), loss %.4f" % (name, time.time() - t0, ratios[worst], worst,
                                                                                     ratios["loss"]))
    del pb
    torch.cuda.empty_cache()


def _batches(c, g, n=3):
    F, Nd, B = c["F"], c["Nd"], c["B"]
    out = []
    for _ in range(n):
        if c["keys"] == "hot":
            pool = torch.randint(0, 10**12, (40, F), device="cuda", generator=g)
            pick = torch.randint(0, 40, (B, F), device="cuda", generator=g)
            keys = pool[pick, torch.arange(F, device="cuda")[None, :]].contiguous()
        else:
            keys = torch.randint(0, 10**12, (B, F), device="cuda", generator=g)
        dense = torch.log1p(torch.randn((B, Nd), device="cuda", generator=g).abs()) if Nd else None
        labels = (torch.rand(B, device="cuda", generator=g) < 0.3).float()
        out.append((keys, dense, labels))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_dcn_engine_three_steps_match_float64_oracle(name):
    """Harness B of the module docstring."""
    _with_switches(CASES[name], _engine_case, name, CASES[name])


def _engine_case(name, c):
    t0 = time.time()
    eng, g = DO.make_engine(c["F"], c["V"], c["D"], c["Nd"], c["L"], c["units"], c["B"], c["diag"], lr=1.0)
    _assert_gates(name, c, eng.dense)
    batches = _batches(c, g)
    ratios = {}
    for step, (keys, dense, labels) in enumerate(batches):
        if step == 2 and c["poke"]:
            with torch.no_grad():                       # written from outside: the planes are stale until ensure_fresh re-splits them
                eng.cross_W[1].mul_(0.5)
                eng.Ws[0].mul_(0.5)
        loss, want, ties, params, touched = DO._dcn_step_vs_oracle(eng, keys, dense, labels, all_rows=True)
        T.check_ties(ties)
        ratios["loss"] = max(ratios.get("loss", 0.0), abs(loss - want) / (1e-5 * abs(want)))
        assert abs(loss - want) <= 1e-5 * abs(want), (step, loss, want)
        if c["keys"] == "hot":
            cnt = int(touched.sum())
            assert cnt <= 40 * c["F"] and c["B"] * c["F"] / cnt >= 40, "rows are not shared by ~50 slots each"
        for nm, before, after, want_after in params:
            if nm == "table rows":
                DO._assert_untouched(nm, before, after, touched)
                before, after, want_after = before[touched], after[touched], want_after[touched]
            DO._assert_not_vacuous("step %d %s" % (step, nm), before, want_after)
            ratios[nm] = max(ratios.get(nm, 0.0), DO._assert_update("step %d %s" % (step, nm), before, after, want_after, rel=DO.UPDATE_REL))
    dense_only = {k: v for k, v in ratios.items() if k not in ("loss", "table rows")}
    worst = max(dense_only, key=dense_only.get)
    print("%s: engine harness %.1f s, worst error / tolerance over 3 steps: table rows %.3f, weights %.3f (%s), loss %.4f" % (
        name, time.time() - t0, ratios["table rows"], dense_only[worst], worst, ratios["loss"]))
    del eng
    torch.cuda.empty_cache()
