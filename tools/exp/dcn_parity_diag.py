"""Root cause of GPUTEST_r04's red test: test_dcn_bench_config_matches_oracle[8192-200000], cross W0.

For each operand split (f16x2, bf16x3) the DCN step of the test is run twice against the fp64 oracle -- once with the oracle's own
relu decisions (round 4's comparison) and once tie-aware (the device's decisions) -- and for every parameter the fraction of elements
outside the test's tolerance is printed, with the rows / columns the outliers sit in (a ReLU tie of ONE example moves a rank-one
pattern: the outliers of cross W_l concentrate in the 13 dense-feature rows and columns, whose x is ~1 instead of ~0.1).
Runs each case twice to see whether the outcome is reproducible from run to run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_benchcfg as tb                       # noqa: E402
from engine_oracle import _ulp                     # noqa: E402
from deep_recommenders_amd import ops               # noqa: E402


def report(name, before, after, want, rel=1e-2):
    b64 = before.astype(np.float64)
    d_gpu, d_cpu = after.astype(np.float64) - b64, want.astype(np.float64) - b64
    rms = float(np.sqrt(np.mean(d_cpu * d_cpu)))
    err = np.abs(d_gpu - d_cpu)
    tol = 2 * np.maximum(_ulp(before), _ulp(want)) + rel * np.abs(d_cpu) + 1e-3 * rms
    bad = err > tol
    line = "  %-12s off %.2e of %d   rms err / rms update %.2e   max err / rms %.2e" % (
        name, bad.mean(), bad.size, float(np.sqrt(np.mean(err * err))) / rms, float(err.max()) / rms)
    if bad.any() and bad.ndim == 2:
        r, c = np.nonzero(bad)
        ru, rc_ = np.unique(r, return_counts=True)
        cu, cc_ = np.unique(c, return_counts=True)
        top_r = ru[np.argsort(-rc_)[:6]].tolist()
        top_c = cu[np.argsort(-cc_)[:6]].tolist()
        line += "   outliers in %d rows (top %s) x %d cols (top %s)" % (len(ru), top_r, len(cu), top_c)
    print(line, flush=True)
    return float(bad.mean())


def main():
    Bd, V = int(os.environ.get("DIAG_B", "8192")), int(os.environ.get("DIAG_V", "200000"))
    for split in ("f16x2", "bf16x3"):
        ops.set_gemm_split(split)
        for rep in range(2):
            for tie_aware in ((False, True) if rep == 0 else (True,)):
                loss, want, ties, params = tb._dcn_bench_step(Bd, V, tie_aware=tie_aware)
                print("split %s run %d tie_aware %s: loss %.9f oracle %.9f (rel %.2e); ties %s" % (
                    split, rep, tie_aware, loss, want, abs(loss - want) / abs(want),
                    [(t["layer"], t["disagree"], "%.2e" % t["worst_abs_z"], "%.2e" % t["rms_z"], t["examples"][:8]) for t in ties]), flush=True)
                worst = 0.0
                for name, before, after, want_after in params:
                    if name.startswith(("table", "cross W", "mlp W")):
                        worst = max(worst, report(name, before, after, want_after))
                print("  -> worst outlier fraction %.2e (test allows 1e-4)" % worst, flush=True)
    ops.set_gemm_split("f16x2")


if __name__ == "__main__":
    main()
