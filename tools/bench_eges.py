"""The skip-gram step with side information (EGES), two ways in ONE process per cell, alternating, with the copy ceiling (dr_copy_nt)
measured in the same call:

  (a) torch   the fp32 composition a user of torch would write on the device: side_table[rows] -> [B, S, D], softmax(att[items]) -> the
              weighted sum u, out_table[ids] -> [B, P + K, D] -> bmm -> logsigmoid; the step is autograd back to the gathered rows and
              logits plus index_add_ of -lr times them into the three tables
  (b) eges    dr_eges_fwd (forward only), dr_eges_fwd with the gradient rows (one pass), and the whole step: one pass + K4 on the three
              tables, K4 in its atomic form (dr_emb_pool_bwd) and in its planned form (dr_emb_sort_slots + dr_emb_pool_bwd_sorted)
  (c) sgns    in the S = 1, P = 1 cells only: dr_sgns_fwd on the same ids, forward and one pass -- the kernel dr_eges_fwd equals bit for
              bit there, and should equal in time within the spread

  python tools/bench_eges.py [--rounds 7] [--iters 5 (the least per window; raised to fill ~50 ms)] [--cells d128_s4,...]
                             [--limit 300 (seconds per cell)] [--log profiles/eges_bench.log]

Cells: B 65 536, K 5, V 1 M items, every side field 1 000 values, ids uniform; D in {64, 128} x S in {1, 4, 8} with P = 1 and attention
(S = 1: without, beside dr_sgns_fwd).  Every pair is valid and row_scale = 1 / B is known to the host.

Every cell runs in a fresh child process under its own time limit, and the first failing cell stops the run.  Device events; every
variant is warmed up; the implementations alternate inside every round; median and min over the rounds and the spread (max - min) /
median are printed with every figure, and the peak of torch's allocator over one call of each variant above what was allocated before
it.  Bytes are the algorithm's, per example: forward 4 (S + P + K) D of rows + 8 (S + 1 + P + K) of ids + 4 S of logits + 4 (1 + 2 (P + K)
+ S) of results; one pass adds the S rows read again (4 S D) and 4 (S D + pad4(S) + (P + K) D) of gradient rows; the step adds K4
reading the three buffers and their ids again and reading and writing (S + P + K) table rows and one logit row.  The fraction is a
kernel's traffic over its time, over the traffic per time of the copy."""
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
from bench_sgns import plan_bytes  # noqa: E402

# cell -> (D, S)
CELLS = {"d%d_s%d" % (D, S): (D, S) for D in (64, 128) for S in (1, 4, 8)}
B, K, P, V, SIDE = 65536, 5, 1, 10 ** 6, 1000


def bench_cell(name, rounds, iters):
    import torch
    import torch.nn.functional as F
    from deep_recommenders_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_eges needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    D, S = CELLS[name]
    J, lr, inv, ld_da = P + K, 1e-3, 1.0 / B, (S + 3) // 4 * 4
    with_att = S > 1
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows = V + SIDE * (S - 1)
    side = torch.empty((rows, D), device="cuda").normal_(0, 1.0 / math.sqrt(D), generator=gen)
    tout = torch.empty((V, D), device="cuda").normal_(0, 1.0 / math.sqrt(D), generator=gen)
    att = torch.empty((V, ld_da), device="cuda").normal_(0, 1.0, generator=gen) if with_att else None
    row_base = torch.tensor([0] + [V + SIDE * s for s in range(S - 1)], dtype=torch.int64, device="cuda")
    items = torch.randint(0, V, (B,), device="cuda", generator=gen)
    side_ids = torch.cat([items[:, None], torch.randint(0, SIDE, (B, S - 1), device="cuda", generator=gen)], dim=1)
    contexts = torch.randint(0, V, (B, P), device="cuda", generator=gen)
    negatives = torch.randint(0, V, (B, K), device="cuda", generator=gen)
    att_ids = items if with_att else None
    flat_side = (side_ids + row_base[None, :]).reshape(-1)
    ids_out = torch.cat([contexts, negatives], dim=1)
    flat_out = ids_out.reshape(-1)
    ids_att = items.reshape(B, 1)
    d_side = torch.empty((B, S * D), device="cuda")
    d_att = torch.empty((B, ld_da), device="cuda")
    d_ctx = torch.empty((B, J * D), device="cuda")
    rb1, rbj = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(J, dtype=torch.int64, device="cuda")
    css, cs1, csj = (torch.arange(n + 1, dtype=torch.int32, device="cuda") for n in (S, 1, J))
    plan_side, plan_att, plan_out = ops.SortPlan(B * S, "cuda"), ops.SortPlan(B, "cuda"), ops.SortPlan(B * J, "cuda")
    scratch = torch.empty((B * max(S, J), D), device="cuda")
    scratch_att = torch.empty((B, ld_da), device="cuda")

    def compose(w, logits, v):
        u = w[:, 0] if logits is None else (torch.softmax(logits, dim=1)[:, :, None] * w).sum(1)
        s = torch.bmm(v, u[:, :, None]).squeeze(2)
        return -(F.logsigmoid(s[:, :P]).sum(1) + F.logsigmoid(-s[:, P:]).sum(1))

    def torch_fwd():
        with torch.no_grad():
            return compose(side[flat_side].reshape(B, S, D), att[items][:, :S] if with_att else None, tout[ids_out])

    def torch_step():
        w = side[flat_side].reshape(B, S, D).requires_grad_(True)
        v = tout[ids_out].requires_grad_(True)
        a = att[items].requires_grad_(True) if with_att else None
        compose(w, a[:, :S] if with_att else None, v).mean().backward()
        side.index_add_(0, flat_side, w.grad.reshape(-1, D), alpha=-lr)
        tout.index_add_(0, flat_out, v.grad.reshape(-1, D), alpha=-lr)
        if with_att:
            att.index_add_(0, items, a.grad, alpha=-lr)

    def eges_fwd():
        return ops.eges_fwd(side, row_base, side_ids, att, att_ids, tout, contexts, negatives, None, False)[0]

    def eges_fwd_grad():
        return ops.eges_fwd(side, row_base, side_ids, att, att_ids, tout, contexts, negatives, None, False, row_scale=inv, d_side=d_side,
                            d_att=d_att, d_ctx=d_ctx)[0]

    def eges_step_atomic():
        eges_fwd_grad()
        ops.emb_pool_bwd(side_ids, S, css, row_base, D, d_side, None, None, None, -lr, side, None)
        if with_att:
            ops.emb_pool_bwd(ids_att, 1, cs1, rb1, ld_da, d_att, None, None, None, -lr, att, None)
        ops.emb_pool_bwd(ids_out, J, csj, rbj, D, d_ctx, None, None, None, -lr, tout, None)

    def eges_step_planned():
        eges_fwd_grad()
        ops.emb_sort_slots(side_ids, row_base, rows, plan_side)
        ops.emb_pool_bwd_sorted(side_ids, row_base, plan_side, D, rows, d_side, None, -lr, side, x_sorted=scratch)
        if with_att:
            ops.emb_sort_slots(ids_att, rb1, V, plan_att)
            ops.emb_pool_bwd_sorted(ids_att, rb1, plan_att, ld_da, V, d_att, None, -lr, att, x_sorted=scratch_att)
        ops.emb_sort_slots(ids_out, rbj, V, plan_out)
        ops.emb_pool_bwd_sorted(ids_out, rbj, plan_out, D, V, d_ctx, None, -lr, tout, x_sorted=scratch)

    def sgns_fwd():
        return ops.sgns_fwd(side, tout, items, contexts[:, 0], negatives, None, False)[0]

    def sgns_fwd_grad():
        return ops.sgns_fwd(side, tout, items, contexts[:, 0], negatives, None, False, row_scale=inv, d_center=d_side, d_ctx=d_ctx)[0]

    logit = S if with_att else 0
    bytes_f = 4.0 * B * ((S + J) * D + 2 * (S + 1 + J) + logit + 1 + 2 * J + S)
    bytes_g = bytes_f + 4.0 * B * (S * D + S * D + ld_da + J * D)
    bytes_step = bytes_g + 4.0 * B * ((S + J) * D + 2 * (S + J) + (ld_da + 2 if with_att else 0)) + 8.0 * B * ((S + J) * D + (ld_da if with_att else 0))
    src = torch.empty(int(bytes_f // 8) * 2, device="cuda")                                 # the forward's traffic, as one copy
    dst = torch.empty_like(src)

    def copy():
        return ops.copy_nt(src, dst)

    # faster and different is not faster: the two forwards on these inputs
    want = torch_fwd()
    diffs = {"eges_vs_torch_loss": float((eges_fwd() - want).abs().max() / want.abs().max())}
    del want
    peaks = {"torch_fwd": peak_mb(torch_fwd), "eges_fwd": peak_mb(eges_fwd), "torch_step": peak_mb(torch_step),
             "eges_step_atomic": peak_mb(eges_step_atomic),
             "eges_step_persistent_buffers": round((d_side.numel() + d_att.numel() + d_ctx.numel()) * 4 / 2 ** 20, 1),
             "eges_step_planned_persistent_extra": round(((scratch.numel() + scratch_att.numel()) * 4 + plan_bytes(plan_side) +
                                                          plan_bytes(plan_att) + plan_bytes(plan_out)) / 2 ** 20, 1)}
    variants = {"torch_fwd": torch_fwd, "eges_fwd": eges_fwd, "eges_fwd_grad": eges_fwd_grad, "torch_step": torch_step,
                "eges_step_atomic": eges_step_atomic, "eges_step_planned": eges_step_planned, "copy_nt": copy}
    if S == 1:
        variants.update({"sgns_fwd": sgns_fwd, "sgns_fwd_grad": sgns_fwd_grad})
        diffs["eges_vs_sgns_loss_bits_differ"] = int((eges_fwd().view(torch.int32) != sgns_fwd().view(torch.int32)).sum())
    res, reps = measure(variants, rounds, iters)
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    ceiling = 2.0 * src.numel() * 4 / (med("copy_nt") * 1e-3)
    frac = lambda n, nbytes: round(nbytes / (med(n) * 1e-3) / ceiling, 4)                   # noqa: E731
    out = {"shape": {"B": B, "K": K, "P": P, "S": S, "V": V, "D": D, "attention": with_att, "side_table_MB": round(side.numel() * 4 / 2 ** 20, 1)},
           "iters_per_window": reps, "max_rel_diff": diffs, "peak_MB": peaks, **res,
           "copy_ceiling_GBps": round(ceiling / 1e9, 1),
           "algorithmic_MB": {"fwd": round(bytes_f / 1e6, 1), "fwd_grad": round(bytes_g / 1e6, 1), "step": round(bytes_step / 1e6, 1)},
           "eges_fwd_speedup_vs_torch": round(med("torch_fwd") / med("eges_fwd"), 3),
           "eges_step_atomic_speedup_vs_torch": round(med("torch_step") / med("eges_step_atomic"), 3),
           "eges_step_planned_speedup_vs_torch": round(med("torch_step") / med("eges_step_planned"), 3),
           "eges_fwd_frac_of_copy_ceiling": frac("eges_fwd", bytes_f),
           "eges_fwd_grad_frac_of_copy_ceiling": frac("eges_fwd_grad", bytes_g),
           "eges_step_atomic_frac_of_copy_ceiling": frac("eges_step_atomic", bytes_step)}
    if S == 1:
        out["eges_over_sgns_fwd"] = round(med("eges_fwd") / med("sgns_fwd"), 3)
        out["eges_over_sgns_fwd_grad"] = round(med("eges_fwd_grad") / med("sgns_fwd_grad"), 3)
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
