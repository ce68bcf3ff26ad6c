"""AFM's attention pooling: the fused kernels (dr_afm_pool_fwd / dr_afm_pool_bwd) against the composition a user of torch would write on
the device in fp32 (index_select -> mul -> [B, P, D] -> matmul -> relu -> matmul -> softmax -> weighted sum, autograd backward), both in
ONE process per cell, alternating.

  python tools/bench_afm.py [--rounds 7] [--iters 3 (the least per window; raised to fill ~50 ms)] [--cells b65536,b8192]
                            [--limit 400 (seconds per cell)] [--log profiles/afm_bench.log]

Cells: `b65536` (B 65 536, F 26, D 64, A 32: the workload's input shape, P = 325 pairs) and `b8192` (B 8 192, the same row).

Every cell runs in a fresh child process under its own time limit, and the first failing cell stops the run.  Device events; every
variant is warmed up; the implementations alternate inside every round; median and min over the rounds and the spread (max - min) /
median are printed with every figure.  `wins` says whether the fused median is below the composition's by more than both spreads.
The forward's arithmetic is the z product, 2 B P D A FLOP; its rate is given as a fraction of the fp32 matrix peak (157.3 TFLOP/s:
256 CUs x 4 SIMDs x 64 FLOP per clock x 2.4 GHz).  Peak memory is torch's max_memory_allocated over one call of each implementation,
less what was allocated before it: the results, the workspace and, for the composition, the [B, P, .] tensors autograd keeps.
The composition's second product is written as a matmul with h [A, 1]: as a matrix-vector product (`relu(z) @ h`) the torch build this
was measured with returns wrong scores from row 8192 * 325 on at B 65 536 (a chunked evaluation disagrees by 100 %, the matmul form
and the fused kernel agree with it to 7e-7), and a wrong result is not worth timing."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# cell -> (B, F, D, A)
CELLS = {"b65536": (65536, 26, 64, 32), "b8192": (8192, 26, 64, 32)}
FP32_MATRIX_PEAK = 256 * 4 * 64 * 2.4e9


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
        raise SystemExit("bench_afm needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    B, F, D, A = CELLS[name]
    P = ops.afm_num_pairs(F)
    gen = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)                          # noqa: E731
    emb, g = r(B, F * D), r(B, D)
    W, b, h = r(D, A) / math.sqrt(D), 0.1 * r(A), r(A) / math.sqrt(A)
    pairs = [(i, j) for i in range(F) for j in range(i)]
    rows = torch.tensor([p[0] for p in pairs], device="cuda")
    cols = torch.tensor([p[1] for p in pairs], device="cuda")
    leaves = [t.clone().requires_grad_(True) for t in (emb, W, b, h)]

    def compose(e, W_, b_, h_):
        e3 = e.reshape(B, F, D)
        p = e3.index_select(1, rows) * e3.index_select(1, cols)
        s = torch.matmul(torch.relu(torch.matmul(p, W_) + b_), h_[:, None])[:, :, 0]   # not `@ h_`: see the module docstring
        return (torch.softmax(s, dim=1)[:, :, None] * p).sum(1)

    def fused_fwd():
        return ops.afm_pool_fwd(emb, W, b, h, F)

    def torch_fwd():
        with torch.no_grad():
            return compose(emb, W, b, h)

    out, lse, _ = fused_fwd()

    def fused_bwd():
        return ops.afm_pool_bwd(emb, W, b, h, F, out, lse, g)

    def fused_fwd_bwd():
        o, l, _ = fused_fwd()
        return ops.afm_pool_bwd(emb, W, b, h, F, o, l, g)

    def torch_fwd_bwd():
        for t in leaves:
            t.grad = None
        torch.autograd.backward([compose(*leaves)], [g])

    # faster and different is not faster: both implementations on these inputs
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())                          # noqa: E731
    diffs = {"out_fused_vs_torch": rel(out, torch_fwd())}
    grads = fused_bwd()
    torch_fwd_bwd()
    for k, x, t in zip(("d_emb", "dW", "db", "dh"), grads, leaves):
        diffs[k + "_fused_vs_torch"] = rel(x.reshape(t.grad.shape), t.grad)
    del grads
    for t in leaves:
        t.grad = None
    peaks = {"fused_fwd": peak_bytes(fused_fwd), "torch_fwd": peak_bytes(torch_fwd), "fused_fwd_bwd": peak_bytes(fused_fwd_bwd),
             "torch_fwd_bwd": peak_bytes(torch_fwd_bwd)}
    variants = {"fused_fwd": fused_fwd, "torch_fwd": torch_fwd, "fused_bwd": fused_bwd, "fused_fwd_bwd": fused_fwd_bwd,
                "torch_fwd_bwd": torch_fwd_bwd}
    res, reps = measure(variants, rounds, iters)
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    wins = lambda x, y: bool(med(x) * (1 + res[x]["spread"]) < med(y) * (1 - res[y]["spread"]))   # noqa: E731
    flop_f = 2.0 * B * P * D * A
    out_line = {"shape": {"B": B, "F": F, "D": D, "A": A, "P": P}, "iters_per_window": reps, "max_rel_diff": diffs, **res,
                "fwd_speedup_vs_torch": round(med("torch_fwd") / med("fused_fwd"), 3), "fwd_wins": wins("fused_fwd", "torch_fwd"),
                "fwd_bwd_speedup_vs_torch": round(med("torch_fwd_bwd") / med("fused_fwd_bwd"), 3),
                "fwd_bwd_wins": wins("fused_fwd_bwd", "torch_fwd_bwd"),
                "fused_fwd_TFLOPs": round(flop_f / (med("fused_fwd") * 1e-3) / 1e12, 2),
                "fused_fwd_frac_of_fp32_matrix_peak": round(flop_f / (med("fused_fwd") * 1e-3) / FP32_MATRIX_PEAK, 4),
                "fused_bwd_TFLOPs_3_products": round(3 * flop_f / (med("fused_bwd") * 1e-3) / 1e12, 2),
                "peak_bytes": peaks, "gathered_rows_bytes": 4 * B * F * D}
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
