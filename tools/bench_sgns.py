"""The skip-gram step with negative sampling, two ways in ONE process per cell, alternating, with the copy ceiling (dr_copy_nt) measured in
the same call:

  (a) torch   the fp32 composition a user of torch would write on the device: in_table[c], out_table[ids] -> [B, 1 + K, D] -> bmm ->
              logsigmoid; the step is autograd back to the gathered rows plus index_add_ of -lr times them into both tables
  (b) sgns    dr_sgns_fwd (forward only), dr_sgns_fwd with the gradient rows (one pass), and the whole step: one pass + K4 on both tables,
              K4 in its atomic form (dr_emb_pool_bwd) and in its planned form (dr_emb_sort_slots + dr_emb_pool_bwd_sorted with x_sorted)

  python tools/bench_sgns.py [--rounds 7] [--iters 5 (the least per window; raised to fill ~50 ms)] [--cells v1m_d128_uniform,...]
                             [--limit 300 (seconds per cell)] [--log profiles/sgns_bench.log]

Cells: B 65 536, K 5; V 1 M with D 128 and V 10 M with D 64; ids uniform, or Zipf with exponent 1 (floor(V^r), r uniform: rank k with
probability ~ 1 / k), centers, contexts and negatives alike.  Every pair is valid and row_scale = 1 / B is known to the host: the one
host read of SkipGram.train_step is not part of any window.

Every cell runs in a fresh child process under its own time limit, and the first failing cell stops the run.  Device events; every
variant is warmed up; the implementations alternate inside every round; median and min over the rounds and the spread (max - min) /
median are printed with every figure, and the peak of torch's allocator over one call of each variant above what was allocated before
it.  Bytes are the algorithm's, per example: forward 4 (2 + K) D of rows + 8 (2 + K) of ids + 4 (2 + K) of results; one pass adds
4 D (d_center) + 4 (1 + K) D (d_ctx); the step adds K4 reading both buffers and their ids again and reading and writing (2 + K) table rows.
d_ctx is c_j u: `d_ctx_share` is what writing it (one pass) and writing + reading it (step) is of those bytes -- what a rank-1 apply
inside K4 would save.  The fraction is a kernel's traffic over its time, over the traffic per time of the copy."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ffm import measure, peak_mb  # noqa: E402

# cell -> (V, D, zipf)
CELLS = {"v1m_d128_uniform": (10 ** 6, 128, False), "v1m_d128_zipf": (10 ** 6, 128, True),
         "v10m_d64_uniform": (10 ** 7, 64, False), "v10m_d64_zipf": (10 ** 7, 64, True)}
B, K = 65536, 5


def plan_bytes(plan):
    return sum(t.numel() * t.element_size() for t in (plan.rows, plan.slots, plan.flags, plan.dup_heads, plan.dup_count, plan.workspace))


def bench_cell(name, rounds, iters):
    import torch
    import torch.nn.functional as F
    from deep_recommenders_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_sgns needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    V, D, zipf = CELLS[name]
    S, lr, inv = 1 + K, 1e-3, 1.0 / B
    gen = torch.Generator(device="cuda").manual_seed(1)
    tin = torch.empty((V, D), device="cuda").normal_(0, 1.0 / math.sqrt(D), generator=gen)
    tout = torch.empty((V, D), device="cuda").normal_(0, 1.0 / math.sqrt(D), generator=gen)

    def draw(*shape):
        if not zipf:
            return torch.randint(0, V, shape, device="cuda", generator=gen)
        r = torch.rand(shape, device="cuda", generator=gen, dtype=torch.float64)
        return ((r * math.log(V)).exp().long() - 1).clamp_(0, V - 1)
    centers, contexts, negatives = draw(B), draw(B), draw(B, K)
    ids_in = centers.reshape(B, 1)
    ids_out = torch.cat([contexts.reshape(B, 1), negatives], dim=1)
    flat_out = ids_out.reshape(-1)
    d_center = torch.empty((B, D), device="cuda")
    d_ctx = torch.empty((B, S * D), device="cuda")
    rb1, rbs = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(S, dtype=torch.int64, device="cuda")
    cs1, css = torch.arange(2, dtype=torch.int32, device="cuda"), torch.arange(S + 1, dtype=torch.int32, device="cuda")
    plan_in, plan_out = ops.SortPlan(B, "cuda"), ops.SortPlan(B * S, "cuda")
    scratch = torch.empty((B * S, D), device="cuda")

    def compose(u, v):
        s = torch.bmm(v, u[:, :, None]).squeeze(2)
        return -(F.logsigmoid(s[:, 0]) + F.logsigmoid(-s[:, 1:]).sum(1))

    def torch_fwd():
        with torch.no_grad():
            return compose(tin[centers], tout[ids_out])

    def torch_step():
        u = tin[centers].requires_grad_(True)
        v = tout[ids_out].requires_grad_(True)
        compose(u, v).mean().backward()
        tin.index_add_(0, centers, u.grad, alpha=-lr)
        tout.index_add_(0, flat_out, v.grad.reshape(-1, D), alpha=-lr)

    def sgns_fwd():
        return ops.sgns_fwd(tin, tout, centers, contexts, negatives, None, False)[0]

    def sgns_fwd_grad():
        return ops.sgns_fwd(tin, tout, centers, contexts, negatives, None, False, row_scale=inv, d_center=d_center, d_ctx=d_ctx)[0]

    def sgns_step_atomic():
        sgns_fwd_grad()
        ops.emb_pool_bwd(ids_in, 1, cs1, rb1, D, d_center, None, None, None, -lr, tin, None)
        ops.emb_pool_bwd(ids_out, S, css, rbs, D, d_ctx, None, None, None, -lr, tout, None)

    def sgns_step_planned():
        sgns_fwd_grad()
        ops.emb_sort_slots(ids_in, rb1, V, plan_in)
        ops.emb_pool_bwd_sorted(ids_in, rb1, plan_in, D, V, d_center, None, -lr, tin, x_sorted=scratch)
        ops.emb_sort_slots(ids_out, rbs, V, plan_out)
        ops.emb_pool_bwd_sorted(ids_out, rbs, plan_out, D, V, d_ctx, None, -lr, tout, x_sorted=scratch)

    bytes_f = 4.0 * B * ((2 + K) * D + 2 * (2 + K) + (2 + K))
    bytes_ctx = 4.0 * B * S * D
    bytes_g = bytes_f + 4.0 * B * D + bytes_ctx
    bytes_step = bytes_g + 4.0 * B * ((2 + K) * D + 2 * (2 + K)) + 8.0 * B * (2 + K) * D
    src = torch.empty(int(bytes_f // 8) * 2, device="cuda")                                 # the forward's traffic, as one copy
    dst = torch.empty_like(src)

    def copy():
        return ops.copy_nt(src, dst)

    # faster and different is not faster: the two forwards on these inputs
    want = torch_fwd()
    diffs = {"sgns_vs_torch_loss": float((sgns_fwd() - want).abs().max() / want.abs().max())}
    del want
    peaks = {"torch_fwd": peak_mb(torch_fwd), "sgns_fwd": peak_mb(sgns_fwd), "torch_step": peak_mb(torch_step),
             "sgns_step_atomic": peak_mb(sgns_step_atomic),
             "sgns_step_persistent_buffers": round((d_center.numel() + d_ctx.numel()) * 4 / 2 ** 20, 1),
             "sgns_step_planned_persistent_extra": round((scratch.numel() * 4 + plan_bytes(plan_in) + plan_bytes(plan_out)) / 2 ** 20, 1)}
    variants = {"torch_fwd": torch_fwd, "sgns_fwd": sgns_fwd, "sgns_fwd_grad": sgns_fwd_grad, "torch_step": torch_step,
                "sgns_step_atomic": sgns_step_atomic, "sgns_step_planned": sgns_step_planned, "copy_nt": copy}
    res, reps = measure(variants, rounds, iters)
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    ceiling = 2.0 * src.numel() * 4 / (med("copy_nt") * 1e-3)
    frac = lambda n, nbytes: round(nbytes / (med(n) * 1e-3) / ceiling, 4)                   # noqa: E731
    out = {"shape": {"B": B, "K": K, "V": V, "D": D, "ids": "zipf" if zipf else "uniform", "table_MB": round(tin.numel() * 4 / 2 ** 20, 1),
                     "distinct_out_rows": int(flat_out.unique().numel())},
           "iters_per_window": reps, "max_rel_diff": diffs, "peak_MB": peaks, **res,
           "copy_ceiling_GBps": round(ceiling / 1e9, 1),
           "algorithmic_MB": {"fwd": round(bytes_f / 1e6, 1), "fwd_grad": round(bytes_g / 1e6, 1), "step": round(bytes_step / 1e6, 1)},
           "d_ctx_share": {"fwd_grad": round(bytes_ctx / bytes_g, 4), "step": round(2 * bytes_ctx / bytes_step, 4)},
           "sgns_fwd_speedup_vs_torch": round(med("torch_fwd") / med("sgns_fwd"), 3),
           "sgns_step_atomic_speedup_vs_torch": round(med("torch_step") / med("sgns_step_atomic"), 3),
           "sgns_step_planned_speedup_vs_torch": round(med("torch_step") / med("sgns_step_planned"), 3),
           "sgns_fwd_frac_of_copy_ceiling": frac("sgns_fwd", bytes_f),
           "sgns_fwd_grad_frac_of_copy_ceiling": frac("sgns_fwd_grad", bytes_g),
           "sgns_step_atomic_frac_of_copy_ceiling": frac("sgns_step_atomic", bytes_step)}
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
