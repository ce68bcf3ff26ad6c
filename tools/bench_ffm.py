"""FFM's field-aware interaction for single-valued fields, three ways in ONE process per cell, alternating, with the copy ceiling
(dr_copy_nt) measured in the same call:

  (a) torch    the fp32 composition a user of torch would write on the device, including its gather:
               table[ids] -> [B, F, F, k] -> transpose -> multiply -> masked sum, autograd backward into a dense table gradient
  (b) rows     K3 (dr_emb_pool_fwd writes concat [B, F * F * k]) followed by dr_ffm_fwd; backward dr_ffm_bwd + K4 (dr_emb_pool_bwd)
  (c) gather   dr_ffm_gather_fwd straight from the table; backward dr_ffm_gather_bwd + K4

  python tools/bench_ffm.py [--rounds 7] [--iters 5 (the least per window; raised to fill ~50 ms)] [--cells b65536_f26_k4,...]
                            [--limit 300 (seconds per cell)] [--log profiles/ffm_bench.log]

Cells: B 65 536, F 26, k 4;  B 65 536, F 39, k 4;  B 8 192, F 26, k 8; 100 000 rows per field, ids uniform.  K4 runs as the fused SGD
step on the table (scale = -lr, nothing materialised), which is how the model trains; torch's backward produces the dense gradient of
the table, which is what `table[ids]` gives its user.

Every cell runs in a fresh child process under its own time limit, and the first failing cell stops the run.  Device events; every
variant is warmed up; the implementations alternate inside every round; median and min over the rounds and the spread (max - min) /
median are printed with every figure, and the peak of torch's allocator over one call of each variant above what was allocated before
it.  Bytes are the algorithm's: forward 4 B (F (F - 1) k + 1) (the needed blocks read once, B floats written); the gather backward
4 B (F (F - 1) k + F F k + 1) (the blocks read, d_rows written).  The fraction is that traffic over the kernel's time, over the traffic
per time of the copy (read + write of a buffer of the forward's size)."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# cell -> (B, F, k)
CELLS = {"b65536_f26_k4": (65536, 26, 4), "b65536_f39_k4": (65536, 39, 4), "b8192_f26_k8": (8192, 26, 8)}
ROWS_PER_FIELD = 100000


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


def peak_mb(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    del keep
    return round(grown / 2 ** 20, 1)


def bench_cell(name, rounds, iters):
    import torch
    from deep_recommenders_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_ffm needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    B, F, k = CELLS[name]
    D, V, lr = F * k, ROWS_PER_FIELD, 1e-3
    gen = torch.Generator(device="cuda").manual_seed(1)
    table = torch.empty((F * V, D), device="cuda").normal_(0, 1.0 / math.sqrt(k), generator=gen)
    ids = torch.randint(0, V, (B, F), device="cuda", generator=gen)
    row_base = torch.arange(F, device="cuda") * V
    col_start = torch.arange(F + 1, dtype=torch.int32, device="cuda")
    d = torch.randn(B, device="cuda", generator=gen)
    rows = ids + row_base[None, :]
    lower = torch.tril(torch.ones((F, F), device="cuda"), -1)[None, :, :, None]
    leaf = table.clone().requires_grad_(True)
    concat = torch.empty((B, F * F * k), device="cuda")
    d_rows = torch.empty((B, F * F * k), device="cuda")

    def compose(t):
        A = t[rows].reshape(B, F, F, k)
        return (A * A.transpose(1, 2) * lower).sum((1, 2, 3))

    def torch_fwd():
        with torch.no_grad():
            return compose(table)

    def torch_fwd_bwd():
        leaf.grad = None
        torch.autograd.backward([compose(leaf)], [d])

    def rows_fwd():
        ops.emb_pool_fwd(ids, F, None, row_base, table, want_sum_x=False, want_fm=False, concat=concat)
        return ops.ffm_fwd(concat, F, k)

    def rows_interaction_only():
        return ops.ffm_fwd(concat, F, k)

    def rows_fwd_bwd():
        rows_fwd()
        ops.ffm_bwd(concat, F, k, d, d_rows=d_rows)
        ops.emb_pool_bwd(ids, F, col_start, row_base, D, d_rows, None, None, None, -lr, table, None)

    def gather_fwd():
        return ops.ffm_gather_fwd(ids, row_base, table, F, k)[0]

    def gather_bwd():
        return ops.ffm_gather_bwd(ids, row_base, table, F, k, d, d_rows=d_rows)

    def gather_fwd_bwd():
        gather_fwd()
        gather_bwd()
        ops.emb_pool_bwd(ids, F, col_start, row_base, D, d_rows, None, None, None, -lr, table, None)

    bytes_f = 4.0 * B * (F * (F - 1) * k + 1)
    bytes_b = 4.0 * B * (F * (F - 1) * k + F * F * k + 1)
    src = torch.empty(int(bytes_f // 4), device="cuda")                                     # the forward's traffic, as one copy
    dst = torch.empty_like(src)

    def copy():
        return ops.copy_nt(src, dst)

    # faster and different is not faster: the three implementations on these inputs
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())                          # noqa: E731
    want = torch_fwd()
    diffs = {"gather_vs_torch": rel(gather_fwd(), want), "rows_vs_torch": rel(rows_fwd(), want),
             "gather_vs_rows_bit_equal": bool(torch.equal(gather_fwd().view(torch.int32), rows_fwd().view(torch.int32)))}
    del want
    peaks = {"torch_fwd": peak_mb(torch_fwd), "rows_fwd": peak_mb(rows_fwd), "gather_fwd": peak_mb(gather_fwd)}
    peaks["rows_fwd_persistent_concat"] = round(concat.numel() * 4 / 2 ** 20, 1)
    peaks["torch_fwd_bwd"] = peak_mb(lambda: (torch_fwd_bwd(), leaf.grad)[1])
    leaf.grad = None
    variants = {"torch_fwd": torch_fwd, "rows_fwd": rows_fwd, "rows_interaction_only": rows_interaction_only, "gather_fwd": gather_fwd,
                "gather_bwd": gather_bwd, "torch_fwd_bwd": torch_fwd_bwd, "rows_fwd_bwd": rows_fwd_bwd, "gather_fwd_bwd": gather_fwd_bwd,
                "copy_nt": copy}
    res, reps = measure(variants, rounds, iters)
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    wins = lambda a, b: bool(med(a) * (1 + res[a]["spread"]) < med(b) * (1 - res[b]["spread"]))   # noqa: E731
    ceiling = 2.0 * src.numel() * 4 / (med("copy_nt") * 1e-3)
    frac = lambda n, nbytes: round(nbytes / (med(n) * 1e-3) / ceiling, 4)                   # noqa: E731
    out = {"shape": {"B": B, "F": F, "k": k, "row_floats": D, "rows_per_field": V, "table_MB": round(table.numel() * 4 / 2 ** 20, 1)},
           "iters_per_window": reps, "max_rel_diff": diffs, "peak_MB": peaks, **res,
           "copy_ceiling_GBps": round(ceiling / 1e9, 1),
           "gather_fwd_speedup_vs_torch": round(med("torch_fwd") / med("gather_fwd"), 3),
           "gather_fwd_speedup_vs_rows": round(med("rows_fwd") / med("gather_fwd"), 3),
           "gather_fwd_wins_over_rows": wins("gather_fwd", "rows_fwd"),
           "gather_fwd_bwd_speedup_vs_torch": round(med("torch_fwd_bwd") / med("gather_fwd_bwd"), 3),
           "gather_fwd_bwd_speedup_vs_rows": round(med("rows_fwd_bwd") / med("gather_fwd_bwd"), 3),
           "gather_fwd_bwd_wins_over_rows": wins("gather_fwd_bwd", "rows_fwd_bwd"),
           "gather_fwd_frac_of_copy_ceiling": frac("gather_fwd", bytes_f),
           "rows_interaction_only_frac_of_copy_ceiling": frac("rows_interaction_only", bytes_f),
           "gather_bwd_frac_of_copy_ceiling": frac("gather_bwd", bytes_b)}
    print("%s: %s" % (name, json.dumps(out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cells", default=",".join(CELLS))
    ap.add_argument("--limit", type=float, default=300.0, help="time limit of one cell, seconds")
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
