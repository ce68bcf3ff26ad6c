"""YoutubeNet's sampled softmax, two ways in ONE process per cell, alternating:

  (a) torch   the fp32 composition a user of torch would write on the device: table[labels], table[sampled] (index) -> matmul -> the
              accidental-hit mask -> logsumexp; the step is autograd back to u and the gathered rows plus index_add_ of -lr times them
              into the class table.  It keeps the [B, S] logits, their softmax and their gradient.
  (b) fused   dr_sampled_softmax_fwd (forward only), forward + dr_sampled_softmax_bwd, and the whole class-table step: forward +
              backward + K4 for d_true and d_sampled, K4 in its atomic form (dr_emb_pool_bwd) and in its planned form
              (dr_emb_sort_slots + dr_emb_pool_bwd_sorted).  The tower (layers.mlp, the slab) is the same code either way and is not timed.

  python tools/bench_youtubenet.py [--rounds 7] [--iters 5 (the least per window; raised to fill ~50 ms)] [--cells paper,wide]
                                   [--limit 300 (seconds per cell)] [--log profiles/youtubenet_bench.log]

Cells: `paper`, the paper's scale: V 1 M, D 256, S 8 192, B 8 192; `wide`, a wide batch: B 65 536, S 4 096, D 64 (V 1 M).  Labels and the
shared negatives follow TensorFlow's log-uniform sampler; log Q is given for both; accidental hits are removed; every row is valid
and row_scale = 1 / B is known to the host.

Every cell runs in a fresh child process under its own time limit, and the first failing cell stops the run.  Device events; every
variant is warmed up; the implementations alternate inside every round; median and min over the rounds and the spread (max - min) /
median are printed with every figure, and the peak of torch's allocator over one call of each variant above what was allocated before
it.  FLOP are those of the products really performed: 2 B S D each, one in the forward (S), four in the backward (S and d_u in the
row-owning sweep, S and d_sampled in the column-owning one) -- five where the mathematics has three; the rate is given as a share of
the fp32 matrix peak (157.3 TFLOP/s: 256 CUs x 4 SIMDs x 64 FLOP / clk x 2.4 GHz)."""
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

PEAK_F32_MATRIX = 157.3e12
# cell -> (V, D, S, B)
CELLS = {"paper": (10 ** 6, 256, 8192, 8192), "wide": (10 ** 6, 64, 4096, 65536)}


def bench_cell(name, rounds, iters):
    import torch
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_youtubenet needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    V, D, S, B = CELLS[name]
    lr, inv = 1e-3, 1.0 / B
    gen = torch.Generator(device="cuda").manual_seed(1)
    table = torch.empty((V, D), device="cuda").normal_(0, 1.0 / math.sqrt(D), generator=gen)
    u = torch.empty((B, D), device="cuda").normal_(0, 1.0, generator=gen)

    def draw(n):                                   # log-uniform: floor(exp(r log(V + 1))) - 1
        r = torch.rand(n, device="cuda", generator=gen, dtype=torch.float64)
        return ((r * math.log(V + 1.0)).exp().long() - 1).clamp_(0, V - 1)
    labels, sampled = draw(B), draw(S)
    c = torch.arange(V, device="cuda", dtype=torch.float64)
    log_q = (torch.log((c + 2.0) / (c + 1.0)) / math.log(V + 1.0) * S).log().float()
    lq_t, lq_s = log_q[labels].contiguous(), log_q[sampled].contiguous()
    del c
    ws = ops.sampled_softmax_workspace(B, S, D, "cuda")
    ids_t, ids_s = labels.reshape(B, 1), sampled.reshape(S, 1)
    plan_t, plan_s = ops.SortPlan(B, "cuda"), ops.SortPlan(S, "cuda")
    scratch = torch.empty((max(B, S), D), device="cuda")

    def compose(uu, tl, ts):
        t = (uu * tl).sum(-1) - lq_t
        s = uu @ ts.T - lq_s[None, :]
        s = s.masked_fill(sampled[None, :] == labels[:, None], -math.inf)
        lg = torch.cat([t[:, None], s], dim=1)
        return torch.logsumexp(lg, dim=1) - t

    def torch_fwd():
        with torch.no_grad():
            return compose(u, table[labels], table[sampled])

    def torch_fwd_bwd():
        uu = u.detach().requires_grad_(True)
        tl = table[labels].requires_grad_(True)
        ts = table[sampled].requires_grad_(True)
        (compose(uu, tl, ts).sum() * inv).backward()
        return uu.grad, tl.grad, ts.grad

    def torch_step():
        _, d_t, d_s = torch_fwd_bwd()
        table.index_add_(0, labels, d_t, alpha=-lr)
        table.index_add_(0, sampled, d_s, alpha=-lr)

    def fused_fwd():
        return ops.sampled_softmax_fwd(u, table, labels, sampled, lq_t, lq_s, None, True, workspace=ws)[2]

    def fused_fwd_bwd():
        t, lse, loss, _ = ops.sampled_softmax_fwd(u, table, labels, sampled, lq_t, lq_s, None, True, workspace=ws)
        return ops.sampled_softmax_bwd(u, table, labels, sampled, t, lse, lq_s, None, True, inv, workspace=ws)

    def fused_step_atomic():
        _, d_t, d_s = fused_fwd_bwd()
        L.sgns_apply_rows(table, ids_t, d_t, -lr)
        L.sgns_apply_rows(table, ids_s, d_s, -lr)

    def fused_step_sorted():
        _, d_t, d_s = fused_fwd_bwd()
        L.sgns_apply_rows(table, ids_t, d_t, -lr, plan_t, scratch)
        L.sgns_apply_rows(table, ids_s, d_s, -lr, plan_s, scratch)

    # faster and different is not faster: the two forwards and the two d_u on these inputs
    want = torch_fwd()
    diffs = {"fused_vs_torch_loss": float((fused_fwd() - want).abs().max() / want.abs().max())}
    g_want, g_got = torch_fwd_bwd()[0], fused_fwd_bwd()[0]
    diffs["fused_vs_torch_d_u"] = float((g_got - g_want).abs().max() / g_want.abs().max())
    del want, g_want, g_got
    peaks = {"torch_fwd": peak_mb(torch_fwd), "fused_fwd": peak_mb(fused_fwd), "torch_fwd_bwd": peak_mb(torch_fwd_bwd),
             "fused_fwd_bwd": peak_mb(fused_fwd_bwd), "fused_workspace": round(ws.numel() / 2 ** 20, 1),
             "one_B_by_S_matrix": round(4.0 * B * S / 2 ** 20, 1)}
    variants = {"torch_fwd": torch_fwd, "fused_fwd": fused_fwd, "torch_fwd_bwd": torch_fwd_bwd, "fused_fwd_bwd": fused_fwd_bwd,
                "torch_step": torch_step, "fused_step_atomic": fused_step_atomic, "fused_step_sorted": fused_step_sorted}
    res, reps = measure(variants, rounds, iters)
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    flop = 2.0 * B * S * D
    tf = lambda n, products: round(products * flop / (med(n) * 1e-3) / 1e12, 2)             # noqa: E731
    out = {"shape": {"B": B, "S": S, "V": V, "D": D, "col_groups": ops.sampled_softmax_col_groups(B, S, D),
                     "row_chunks": ops.sampled_softmax_row_chunks(B, S, D)},
           "iters_per_window": reps, "max_rel_diff": diffs, "peak_MB": peaks, **res,
           "GFLOP_per_product": round(flop / 1e9, 2),
           "fused_fwd_TFLOPs": tf("fused_fwd", 1), "fused_fwd_bwd_TFLOPs": tf("fused_fwd_bwd", 5),
           "fused_fwd_frac_of_fp32_matrix_peak": round(tf("fused_fwd", 1) * 1e12 / PEAK_F32_MATRIX, 4),
           "fused_fwd_bwd_frac_of_fp32_matrix_peak": round(tf("fused_fwd_bwd", 5) * 1e12 / PEAK_F32_MATRIX, 4),
           "torch_fwd_TFLOPs": tf("torch_fwd", 1), "torch_fwd_bwd_TFLOPs": tf("torch_fwd_bwd", 3),
           "fused_fwd_speedup_vs_torch": round(med("torch_fwd") / med("fused_fwd"), 3),
           "fused_fwd_bwd_speedup_vs_torch": round(med("torch_fwd_bwd") / med("fused_fwd_bwd"), 3),
           "fused_step_atomic_speedup_vs_torch": round(med("torch_step") / med("fused_step_atomic"), 3),
           "fused_step_sorted_speedup_vs_torch": round(med("torch_step") / med("fused_step_sorted"), 3)}
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
