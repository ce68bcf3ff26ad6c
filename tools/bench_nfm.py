"""NFM's Bi-Interaction pooling for single-valued fields, three ways in ONE process per cell, alternating, with the copy ceiling
(dr_copy_nt) measured in the same call:

  (a) torch    the fp32 composition a user of torch would write on the device, including its gather:
               e = table[ids] -> 0.5 (e.sum(1)^2 - (e * e).sum(1)), autograd backward into a dense table gradient
  (b) rows     K3 (dr_emb_pool_fwd writes concat [B, F * D]) followed by dr_bi_interact_fwd; backward dr_bi_interact_bwd + K4
  (c) gather   dr_bi_interact_gather_fwd straight from the table; backward dr_bi_interact_gather_bwd + K4 (dr_emb_pool_bwd)

  python tools/bench_nfm.py [--rounds 7] [--iters 5 (the least per window; raised to fill ~50 ms)] [--cells b65536_f26_d64,...]
                            [--limit 300 (seconds per cell)] [--log profiles/nfm_bench.log]

Cells: B 65 536, F 26, D 64;  B 65 536, F 39, D 16;  B 8 192, F 26, D 128; 100 000 rows per field, ids uniform.  Timed: the forward,
forward + backward (d_rows written), and with K4 as the fused SGD step on the table (scale = -lr, nothing materialised), which is how
the model trains; torch's backward produces the dense gradient of the table, which is what `table[ids]` gives its user.

Every cell runs in a fresh child process under its own time limit, and the first failing cell stops the run.  Device events; every
variant is warmed up; the implementations alternate inside every round; median, min and the spread (max - min) / median are printed
with every figure, and the peak of torch's allocator over one call of each variant.  Bytes are the algorithm's, with R = 4 B F D (the
rows) and W = R (d_rows): the gather forward reads R and writes 4 B D; the rows path writes R (K3), reads it back and reads the table:
3 R; the gather backward moves 2 R + W (the rows twice, d_rows once), the rows backward R + W beside K3's own."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ffm import measure, peak_mb                                            # noqa: E402  (the shared measuring loop)

# cell -> (B, F, D)
CELLS = {"b65536_f26_d64": (65536, 26, 64), "b65536_f39_d16": (65536, 39, 16), "b8192_f26_d128": (8192, 26, 128)}
ROWS_PER_FIELD = 100000


def bench_cell(name, rounds, iters):
    import torch
    from deep_recommenders_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_nfm needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    B, F, D = CELLS[name]
    V, lr = ROWS_PER_FIELD, 1e-3
    gen = torch.Generator(device="cuda").manual_seed(1)
    table = torch.empty((F * V, D), device="cuda").normal_(0, 1.0 / math.sqrt(D), generator=gen)
    ids = torch.randint(0, V, (B, F), device="cuda", generator=gen)
    row_base = torch.arange(F, device="cuda") * V
    col_start = torch.arange(F + 1, dtype=torch.int32, device="cuda")
    d = torch.randn((B, D), device="cuda", generator=gen)
    rows = ids + row_base[None, :]
    leaf = table.clone().requires_grad_(True)
    concat = torch.empty((B, F * D), device="cuda")
    d_rows = torch.empty((B, F * D), device="cuda")
    out = torch.empty((B, D), device="cuda")

    def compose(t):
        e = t[rows]
        s = e.sum(1)
        return 0.5 * (s * s - (e * e).sum(1))

    def torch_fwd():
        with torch.no_grad():
            return compose(table)

    def torch_fwd_bwd():
        leaf.grad = None
        torch.autograd.backward([compose(leaf)], [d])

    def k3():
        ops.emb_pool_fwd(ids, F, col_start if F > 64 else None, row_base, table, want_sum_x=False, want_fm=False, concat=concat)

    def rows_fwd():
        k3()
        return ops.bi_interaction_fwd(concat, F, D, out=out)

    def rows_pooling_only():
        return ops.bi_interaction_fwd(concat, F, D, out=out)

    def rows_fwd_bwd():
        rows_fwd()
        return ops.bi_interaction_bwd(concat, F, D, d, d_rows=d_rows)

    def gather_fwd():
        return ops.bi_interaction_gather_fwd(ids, row_base, table, F, D, out=out)[0]

    def gather_bwd():
        return ops.bi_interaction_gather_bwd(ids, row_base, table, F, D, d, d_rows=d_rows)

    def gather_fwd_bwd():
        gather_fwd()
        return gather_bwd()

    def k4():
        ops.emb_pool_bwd(ids, F, col_start, row_base, D, d_rows, None, None, None, -lr, table, None)

    def rows_step():
        rows_fwd_bwd()
        k4()

    def gather_step():
        gather_fwd_bwd()
        k4()

    R = 4.0 * B * F * D
    bytes_f = R + 4.0 * B * D
    bytes_b = 2 * R + R + 4.0 * B * D
    src = torch.empty(int(R // 4), device="cuda")                                           # the rows, as one copy
    dst = torch.empty_like(src)

    def copy():
        return ops.copy_nt(src, dst)

    # faster and different is not faster: the three implementations on these inputs
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())                          # noqa: E731
    want = torch_fwd()
    g = gather_fwd().clone()
    diffs = {"gather_vs_torch": rel(g, want), "rows_vs_torch": rel(rows_fwd(), want),
             "gather_vs_rows_bit_equal": bool(torch.equal(g.view(torch.int32), rows_fwd().view(torch.int32)))}
    del want, g
    peaks = {"torch_fwd": peak_mb(torch_fwd), "rows_fwd": peak_mb(rows_fwd), "gather_fwd": peak_mb(gather_fwd)}
    peaks["rows_fwd_persistent_concat"] = round(concat.numel() * 4 / 2 ** 20, 1)
    peaks["torch_fwd_bwd"] = peak_mb(lambda: (torch_fwd_bwd(), leaf.grad)[1])
    leaf.grad = None
    variants = {"torch_fwd": torch_fwd, "rows_fwd": rows_fwd, "rows_pooling_only": rows_pooling_only, "gather_fwd": gather_fwd,
                "gather_bwd": gather_bwd, "torch_fwd_bwd": torch_fwd_bwd, "rows_fwd_bwd": rows_fwd_bwd, "gather_fwd_bwd": gather_fwd_bwd,
                "rows_step": rows_step, "gather_step": gather_step, "copy_nt": copy}
    res, reps = measure(variants, rounds, iters)
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    wins = lambda a, b: bool(med(a) * (1 + res[a]["spread"]) < med(b) * (1 - res[b]["spread"]))   # noqa: E731
    ceiling = 2.0 * src.numel() * 4 / (med("copy_nt") * 1e-3)
    frac = lambda n, nbytes: round(nbytes / (med(n) * 1e-3) / ceiling, 4)                   # noqa: E731
    line = {"shape": {"B": B, "F": F, "D": D, "rows_per_field": V, "table_MB": round(table.numel() * 4 / 2 ** 20, 1),
                      "rows_MB": round(R / 2 ** 20, 1)},
            "iters_per_window": reps, "max_rel_diff": diffs, "peak_MB": peaks, **res,
            "copy_ceiling_GBps": round(ceiling / 1e9, 1),
            "gather_fwd_speedup_vs_torch": round(med("torch_fwd") / med("gather_fwd"), 3),
            "gather_fwd_speedup_vs_rows": round(med("rows_fwd") / med("gather_fwd"), 3),
            "gather_fwd_wins_over_rows": wins("gather_fwd", "rows_fwd"),
            "gather_fwd_bwd_speedup_vs_torch": round(med("torch_fwd_bwd") / med("gather_fwd_bwd"), 3),
            "gather_fwd_bwd_speedup_vs_rows": round(med("rows_fwd_bwd") / med("gather_fwd_bwd"), 3),
            "gather_fwd_bwd_wins_over_rows": wins("gather_fwd_bwd", "rows_fwd_bwd"),
            "gather_step_speedup_vs_rows": round(med("rows_step") / med("gather_step"), 3),
            "gather_step_wins_over_rows": wins("gather_step", "rows_step"),
            "gather_fwd_frac_of_copy_ceiling": frac("gather_fwd", bytes_f),
            "rows_pooling_only_frac_of_copy_ceiling": frac("rows_pooling_only", bytes_f),
            "gather_bwd_frac_of_copy_ceiling": frac("gather_bwd", bytes_b)}
    print("%s: %s" % (name, json.dumps(line)), flush=True)


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
