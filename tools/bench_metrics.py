"""dr_confusion_hist_update (the streaming state of metrics.AUC / Precision / Recall / StreamingAUC) against the composition a user of
torch would write on the device in fp32 -- torch.bucketize against the same thresholds, then a (weighted) torch.bincount over
label * (T + 1) + bucket, added to the same fp64 state -- in ONE process.

  python tools/bench_metrics.py [--rounds 7] [--iters 10 (the least per window; raised to fill ~20 ms)] [--log profiles/metrics_bench.log]

T = 200 (the default grid).  Twelve cells: n = 65 536 (one evaluation batch of the bench configuration) and n = 2^24; predictions
uniform, sigmoid(N(0, 1)) and all 0.5 (the degenerate case: every example in one bucket); without and with weights.  Labels
Bernoulli(0.4).  Device events; every variant is warmed up; the two implementations alternate inside every round; median, min and the
spread (max - min) / median over the rounds are printed.  `kernel_no_slower` is: kernel median <= torch median + the larger of the
two spreads (in ms).  The n = 2^24 cells also give the kernel's bytes (8 per example, 12 with weights) per second as a fraction of
the copy ceiling ops.copy_nt measures in the same call (read + write bytes of a 256 MiB copy), and the line `degenerate_over_uniform`
gives the ratio of the all-0.5 time to the uniform time.
For context the host path of examples/train_fm_on_movielens_estimator.py -- a device-to-host copy of the batch's labels and
probabilities plus its rank auc() -- is timed on the wall clock at n = 65 536 (its Python loop is not meant for 2^24)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from deep_recommenders_amd import metrics, ops  # noqa: E402

T = 200
SIZES = {"n65536": 1 << 16, "n2^24": 1 << 24}
DISTS = ("uniform", "sigmoid_normal", "all_half")


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def stats(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"median_ms": round(med, 5), "min_ms": round(ms[0], 5), "spread": round((ms[-1] - ms[0]) / med, 4)}


def measure(variants, rounds, iters, fill_ms=20.0):
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = {k: max(iters, int(math.ceil(fill_ms / max(window(fn, iters), 1e-3)))) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():                       # alternating inside every round
            times[k].append(window(fn, reps[k]))
    return {k: stats(v) for k, v in times.items()}, reps


def predictions(dist, n, gen):
    if dist == "uniform":
        return torch.rand(n, device="cuda", generator=gen)
    if dist == "sigmoid_normal":
        return torch.sigmoid(torch.randn(n, device="cuda", generator=gen))
    return torch.full((n,), 0.5, device="cuda")


def copy_ceiling(rounds, iters):
    src = torch.empty(1 << 26, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    res, _ = measure({"copy": lambda: ops.copy_nt(src, dst)}, rounds, iters)
    return 2 * src.numel() * 4 / (res["copy"]["median_ms"] * 1e-3) / 1e9, res["copy"]


def bench_cell(name, n, dist, weighted, thr, rounds, iters, copy_gbps):
    gen = torch.Generator(device="cuda").manual_seed(1)
    p = predictions(dist, n, gen)
    y = (torch.rand(n, device="cuda", generator=gen) < 0.4).to(torch.float32)
    w = torch.rand(n, device="cuda", generator=gen) * 2.0 if weighted else None
    ws = ops.confusion_hist_workspace(n, T)
    h_kernel = torch.zeros((2, T + 1), dtype=torch.float64, device="cuda")
    h_torch = torch.zeros(2 * (T + 1), dtype=torch.float64, device="cuda")

    def kernel():
        ops.confusion_hist_update(p, y, thr, h_kernel, w, False, ws)

    def composed():
        key = torch.bucketize(p, thr) + (y != 0).to(torch.int64) * (T + 1)
        h_torch.add_(torch.bincount(key, weights=w, minlength=2 * (T + 1)))

    kernel()
    composed()
    a, b = h_kernel.reshape(-1).clone(), h_torch.clone()
    diff = float((a - b).abs().max() / b.abs().max())
    if not weighted:
        assert torch.equal(a, b), "the two histograms differ"
    res, reps = measure({"kernel": kernel, "torch": composed}, rounds, iters)
    k, t = res["kernel"], res["torch"]
    slack_ms = max(k["spread"] * k["median_ms"], t["spread"] * t["median_ms"])
    out = {"cell": name, "n": n, "dist": dist, "weighted": weighted, "iters_per_window": reps, "max_rel_diff_kernel_vs_torch": diff,
           "kernel": k, "torch": t, "speedup": round(t["median_ms"] / k["median_ms"], 3),
           "kernel_no_slower": bool(k["median_ms"] <= t["median_ms"] + slack_ms)}
    if n == 1 << 24:
        gbps = n * (12 if weighted else 8) / (k["median_ms"] * 1e-3) / 1e9
        out.update({"kernel_GBps": round(gbps, 1), "kernel_frac_of_copy_ceiling": round(gbps / copy_gbps, 4)})
    return out


def host_path(n, rounds):
    """what examples/train_fm_on_movielens_estimator.py does per evaluation: both tensors to the host, then its rank auc()"""
    from train_fm_on_movielens_estimator import auc
    gen = torch.Generator(device="cuda").manual_seed(1)
    p = predictions("sigmoid_normal", n, gen)
    y = (torch.rand(n, device="cuda", generator=gen) < 0.4).to(torch.float32)
    copy_ms, auc_ms = [], []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        yh, ph = y.cpu().numpy(), p.cpu().numpy()
        t1 = time.perf_counter()
        auc(yh, ph)
        t2 = time.perf_counter()
        copy_ms.append((t1 - t0) * 1e3)
        auc_ms.append((t2 - t1) * 1e3)
    return {"n": n, "copy_to_host": stats(copy_ms), "rank_auc_on_host": stats(auc_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    log = open(a.log, "a") if a.log else None

    def emit(line):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    thr = torch.from_numpy(metrics.auc_thresholds(T)).cuda()
    copy_gbps, copy_stats = copy_ceiling(a.rounds, a.iters)
    emit("copy_ceiling: " + json.dumps({"GBps": round(copy_gbps, 1), **copy_stats}))
    cells = {}
    for size, n in SIZES.items():
        for dist in DISTS:
            for weighted in (False, True):
                name = "%s/%s/%s" % (size, dist, "weighted" if weighted else "unweighted")
                cells[name] = bench_cell(name, n, dist, weighted, thr, a.rounds, a.iters, copy_gbps)
                emit(name + ": " + json.dumps(cells[name]))
    ratio = {w: round(cells["n2^24/all_half/%s" % w]["kernel"]["median_ms"] / cells["n2^24/uniform/%s" % w]["kernel"]["median_ms"], 3)
             for w in ("unweighted", "weighted")}
    emit("degenerate_over_uniform (n = 2^24, kernel): " + json.dumps(ratio))
    host = host_path(1 << 16, min(a.rounds, 3))
    emit("host_path: " + json.dumps(host))
    summary = {"bench": "confusion_hist", "T": T, "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
               "copy_ceiling_GBps": round(copy_gbps, 1), "cells_kernel_no_slower": sum(c["kernel_no_slower"] for c in cells.values()),
               "cells": len(cells), "slower_cells": [k for k, c in cells.items() if not c["kernel_no_slower"]],
               "degenerate_over_uniform": ratio}
    emit(json.dumps(summary))
    if log:
        log.close()


if __name__ == "__main__":
    main()
