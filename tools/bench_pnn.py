"""PNN's outer-product layer: the fused kernels (dr_pnn_outer_fwd / dr_pnn_outer_bwd) against the two compositions a user of torch
would write on the device in fp32, all in ONE process per cell, alternating:
  `mat`     u = emb.sum(1); (u[:, :, None] * u[:, None, :]).reshape(B, D * D) @ W      (the [B, D^2] matrix is written and kept)
  `einsum`  torch.einsum('bd,dek->bek', u, W3) contracted with u                          (a [B, D, N] tensor instead)

  python tools/bench_pnn.py [--rounds 7] [--iters 3 (the least per window; raised to fill ~50 ms)] [--cells b65536,b8192]
                            [--limit 400 (seconds per cell)] [--log profiles/pnn_bench.log]

Cells: `b65536` (B 65 536, F 26, D 64, N 256: the workload's input shape) and `b8192` (B 8 192, F 26, D 32, N 128).

Every cell runs in a fresh child process under its own time limit, and the first failing cell stops the run.  Device events; every
variant is warmed up; the implementations alternate inside every round; median and min over the rounds and the spread (max - min) /
median are printed with every figure.  `wins` says whether the fused median is below the faster composition's by more than both
spreads; `target_met` whether it is no longer than that composition by more than the call's spread.
The forward's arithmetic is 2 B D^2 N FLOP, the backward's twice that (dW and du); the rates are given against the 155 TFLOP/s the
fp32-input MFMA reaches.  Peak memory is torch's max_memory_allocated over one call of each implementation, less what was allocated
before it: the results, the workspace and, for the compositions, what autograd keeps."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# cell -> (B, F, D, N)
CELLS = {"b65536": (65536, 26, 64, 256), "b8192": (8192, 26, 32, 128)}
FP32_MFMA_TFLOPS = 155.0


def stats(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"median_ms": round(med, 4), "min_ms": round(ms[0], 4), "spread": round((ms[-1] - ms[0]) / med, 4), "rounds": len(ms)}


def window(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def measure(variants, rounds, iters):
    """every variant warmed up, windows of >= ~50 ms, the variants alternating inside every round"""
    import torch
    reps = {}
    for n, fn in variants.items():
        for _ in range(3):
            fn()
        reps[n] = max(iters, int(math.ceil(50.0 / max(window(fn, iters), 1e-3))))
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(rounds):
        for n, fn in variants.items():
            times[n].append(window(fn, reps[n]))
    return {n: stats(t) for n, t in times.items()}, reps


def peak_bytes(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    del keep
    return int(grown)


def bench_cell(name, rounds, iters):
    import torch
    from deep_recommenders_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_pnn needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    B, F, D, N = CELLS[name]
    gen = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)                          # noqa: E731
    emb, g = r(B, F * D) / math.sqrt(F), r(B, N)
    W = r(D * D, N) / D
    leaves = [t.clone().requires_grad_(True) for t in (emb, W)]

    def mat(e, W_):
        u = e.reshape(B, F, D).sum(1)
        return (u[:, :, None] * u[:, None, :]).reshape(B, D * D) @ W_

    def ein(e, W_):
        u = e.reshape(B, F, D).sum(1)
        return (torch.einsum("bd,dek->bek", u, W_.reshape(D, D, N)) * u[:, :, None]).sum(1)

    def fused_fwd():
        return ops.pnn_outer_fwd(emb, W, F)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn(emb, W)
        return run

    out, u = fused_fwd()
    ws = ops.pnn_outer_bwd_workspace(B, F, D, N, "cuda")

    def fused_bwd():
        return ops.pnn_outer_bwd(u, W, F, g, workspace=ws)

    def fused_fwd_bwd():
        _, u_ = fused_fwd()
        return ops.pnn_outer_bwd(u_, W, F, g)

    def with_grad(fn):
        def run():
            for t in leaves:
                t.grad = None
            torch.autograd.backward([fn(*leaves)], [g])
        return run

    mat_fwd, ein_fwd, mat_fwd_bwd, ein_fwd_bwd = no_grad(mat), no_grad(ein), with_grad(mat), with_grad(ein)
    # faster and different is not faster: the implementations on these inputs
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())                          # noqa: E731
    diffs = {"out_fused_vs_mat": rel(out, mat_fwd()), "out_einsum_vs_mat": rel(ein_fwd(), mat_fwd())}
    grads = fused_bwd()
    mat_fwd_bwd()
    for k, x, t in zip(("d_emb", "dW"), grads, leaves):
        diffs[k + "_fused_vs_mat"] = rel(x.reshape(t.grad.shape), t.grad)
    del grads
    for t in leaves:
        t.grad = None
    peaks = {"fused_fwd": peak_bytes(fused_fwd), "mat_fwd": peak_bytes(mat_fwd), "einsum_fwd": peak_bytes(ein_fwd),
             "fused_fwd_bwd": peak_bytes(fused_fwd_bwd), "mat_fwd_bwd": peak_bytes(mat_fwd_bwd), "einsum_fwd_bwd": peak_bytes(ein_fwd_bwd)}
    for t in leaves:
        t.grad = None
    variants = {"fused_fwd": fused_fwd, "mat_fwd": mat_fwd, "einsum_fwd": ein_fwd, "fused_bwd": fused_bwd, "fused_fwd_bwd": fused_fwd_bwd,
                "mat_fwd_bwd": mat_fwd_bwd, "einsum_fwd_bwd": ein_fwd_bwd}
    res, reps = measure(variants, rounds, iters)
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    wins = lambda x, y: bool(med(x) * (1 + res[x]["spread"]) < med(y) * (1 - res[y]["spread"]))   # noqa: E731
    met = lambda x, y: bool(med(x) <= med(y) * (1 + max(res[x]["spread"], res[y]["spread"])))     # noqa: E731
    best_f = min(("mat_fwd", "einsum_fwd"), key=med)
    best_fb = min(("mat_fwd_bwd", "einsum_fwd_bwd"), key=med)
    flop_f = 2.0 * B * D * D * N
    rate = lambda flop, n: round(flop / (med(n) * 1e-3) / 1e12, 2)                          # noqa: E731
    out_line = {"shape": {"B": B, "F": F, "D": D, "N": N}, "iters_per_window": reps, "max_rel_diff": diffs, **res,
                "faster_torch_fwd": best_f, "fwd_speedup_vs_torch": round(med(best_f) / med("fused_fwd"), 3),
                "fwd_wins": wins("fused_fwd", best_f), "fwd_target_met": met("fused_fwd", best_f),
                "faster_torch_fwd_bwd": best_fb, "fwd_bwd_speedup_vs_torch": round(med(best_fb) / med("fused_fwd_bwd"), 3),
                "fwd_bwd_wins": wins("fused_fwd_bwd", best_fb), "fwd_bwd_target_met": met("fused_fwd_bwd", best_fb),
                "fused_fwd_TFLOPs": rate(flop_f, "fused_fwd"), "fused_fwd_frac_of_155": round(rate(flop_f, "fused_fwd") / FP32_MFMA_TFLOPS, 4),
                "fused_bwd_TFLOPs": rate(2 * flop_f, "fused_bwd"), "fused_bwd_frac_of_155": round(rate(2 * flop_f, "fused_bwd") / FP32_MFMA_TFLOPS, 4),
                "mat_fwd_TFLOPs": rate(flop_f, "mat_fwd"),
                "peak_bytes": peaks, "gathered_rows_bytes": 4 * B * F * D, "outer_matrix_bytes": 4 * B * D * D}
    print("%s: %s" % (name, json.dumps(out_line)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--cells", default=",".join(CELLS))
    ap.add_argument("--limit", type=float, default=400.0, help="time limit of one cell, seconds")
    ap.add_argument("--log", default=None, help="also append the per-cell lines to this file")
    ap.add_argument("--cell", default=None, help="(internal) run this one cell in this process")
    a = ap.parse_args()
    if a.cell is not None:
        bench_cell(a.cell, a.rounds, a.iters)
        return
    for name in a.cells.split(","):
        if name not in CELLS:
            raise SystemExit("unknown cell %r; known: %s" % (name, ", ".join(CELLS)))
    for name in a.cells.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--cell", name, "--rounds", str(a.rounds), "--iters", str(a.iters)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.limit, text=True)
        except subprocess.TimeoutExpired as e:
            print(e.stdout or "", flush=True)
            raise SystemExit("cell %s did not finish within %.0f s: stopping" % (name, a.limit))
        print(p.stdout, end="", flush=True)
        if p.returncode != 0:
            raise SystemExit("cell %s failed with exit status %d: stopping" % (name, p.returncode))
        if a.log:
            with open(a.log, "a") as log:
                log.writelines(line + "\n" for line in p.stdout.splitlines() if line.startswith(name + ": "))


if __name__ == "__main__":
    main()
