"""LS-PLM's bag sum + mixture head for single-valued fields, two ways in ONE process per cell, alternating, with the copy ceiling
(dr_copy_nt) measured in the same call:

  (a) k3_torch  K3 (dr_emb_pool_fwd writes concat [B, F * 2 m]), then the head as a user of torch would write it on the device:
                concat.view(B, F, 2 m).sum(1) + bias -> softmax / sigmoid -> p -> log-loss; backward by autograd into d_concat
  (b) fused     dr_lsplm_fwd (forward) and dr_lsplm_loss_fwd (forward + loss + d_rows in one pass)

  python tools/bench_lsplm.py [--rounds 7] [--iters 5 (the least per window; raised to fill ~50 ms)] [--cells b65536_f39_m12,...]
                              [--limit 300 (seconds per cell)] [--log profiles/lsplm_bench.log]

Cells: B 65 536, F 39, m 12;  B 8 192, F 26, m 4; 100 000 rows per field, ids uniform.  Timed: the forward, forward + loss + gradient
of the rows, and with K4 as the fused SGD step on the table plus the bias update.  Every cell runs in a fresh child process under its
own time limit, and the first failing cell stops the run.  Device events; every variant is warmed up; the implementations alternate
inside every round; median, min and the spread (max - min) / median are printed with every figure, and the peak of torch's allocator
over one call of each variant.  Bytes are the algorithm's, with R = 4 B F 2 m (the rows): the fused forward reads R and writes 8 B; the
one-pass training form reads R and writes R (d_rows) + 4 B 2 m (d_z)."""
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

# cell -> (B, F, m)
CELLS = {"b65536_f39_m12": (65536, 39, 12), "b8192_f26_m4": (8192, 26, 4)}
ROWS_PER_FIELD = 100000


def bench_cell(name, rounds, iters):
    import torch
    from deep_recommenders_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_lsplm needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    B, F, m = CELLS[name]
    W, V, lr = 2 * m, ROWS_PER_FIELD, 1e-3
    gen = torch.Generator(device="cuda").manual_seed(1)
    table = torch.empty((F * V, W), device="cuda").normal_(0, 0.5 / math.sqrt(F), generator=gen)
    bias = torch.zeros(W, device="cuda")
    ids = torch.randint(0, V, (B, F), device="cuda", generator=gen)
    row_base = torch.arange(F, device="cuda") * V
    col_start = torch.arange(F + 1, dtype=torch.int32, device="cuda")
    y = (torch.rand(B, device="cuda", generator=gen) < 0.5).float()
    concat = torch.empty((B, F * W), device="cuda")
    d_z = torch.empty((B, W), device="cuda")
    d_rows = torch.empty((B, F * W), device="cuda")

    def k3():
        ops.emb_pool_fwd(ids, F, col_start if F > 64 else None, row_base, table, want_sum_x=False, want_fm=False, concat=concat)

    def head(c):
        z = c.view(B, F, W).sum(1) + bias
        pi = torch.softmax(z[:, :m], 1)
        p = (pi * torch.sigmoid(z[:, m:])).sum(1)
        q = (pi * torch.sigmoid(-z[:, m:])).sum(1)
        return p, q

    def k3_torch_fwd():
        k3()
        with torch.no_grad():
            return head(concat)[0]

    def k3_torch_loss_bwd():
        k3()
        c = concat.detach().requires_grad_(True)
        p, q = head(c)
        loss = -(y * torch.log(p) + (1 - y) * torch.log(q)).mean()
        loss.backward()
        return c.grad

    def fused_fwd():
        return ops.lsplm_fwd(ids, F, None, row_base, table, m, bias, want_z=False)[0]

    def fused_loss_bwd():
        return ops.lsplm_loss_fwd(ids, F, None, row_base, table, m, bias, y, None, 1.0 / B, d_z=d_z, d_rows=d_rows)

    def k4(g):
        ops.emb_pool_bwd(ids, F, col_start, row_base, W, g, None, None, None, -lr, table, None)

    def k3_torch_step():
        k4(k3_torch_loss_bwd())

    def fused_step():
        fused_loss_bwd()
        k4(d_rows)
        ops.axpy(-lr, ops.lsplm_bias_grad(d_z, m), bias)

    R = 4.0 * B * F * W
    bytes_f = R + 8.0 * B
    bytes_l = 2 * R + 4.0 * B * W + 12.0 * B
    src = torch.empty(int(R // 4), device="cuda")                                           # the rows, as one copy
    dst = torch.empty_like(src)

    def copy():
        return ops.copy_nt(src, dst)

    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())                          # noqa: E731
    want = k3_torch_fwd()
    want_g = k3_torch_loss_bwd().clone()
    fused_loss_bwd()
    diffs = {"fused_p_vs_torch": rel(fused_fwd(), want), "fused_d_rows_vs_torch": rel(d_rows, want_g)}
    del want, want_g
    peaks = {"k3_torch_fwd": peak_mb(k3_torch_fwd), "fused_fwd": peak_mb(fused_fwd), "k3_torch_loss_bwd": peak_mb(k3_torch_loss_bwd),
             "fused_loss_bwd": peak_mb(fused_loss_bwd)}
    peaks["k3_torch_persistent_concat"] = round(concat.numel() * 4 / 2 ** 20, 1)
    variants = {"k3_torch_fwd": k3_torch_fwd, "fused_fwd": fused_fwd, "k3_torch_loss_bwd": k3_torch_loss_bwd,
                "fused_loss_bwd": fused_loss_bwd, "k3_torch_step": k3_torch_step, "fused_step": fused_step, "copy_nt": copy}
    res, reps = measure(variants, rounds, iters)
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    wins = lambda a, b: bool(med(a) * (1 + res[a]["spread"]) < med(b) * (1 - res[b]["spread"]))   # noqa: E731
    ceiling = 2.0 * src.numel() * 4 / (med("copy_nt") * 1e-3)
    frac = lambda n, nbytes: round(nbytes / (med(n) * 1e-3) / ceiling, 4)                   # noqa: E731
    line = {"shape": {"B": B, "F": F, "m": m, "row_floats": W, "rows_per_field": V, "table_MB": round(table.numel() * 4 / 2 ** 20, 1),
                      "rows_MB": round(R / 2 ** 20, 1)},
            "iters_per_window": reps, "max_rel_diff": diffs, "peak_MB": peaks, **res,
            "copy_ceiling_GBps": round(ceiling / 1e9, 1),
            "fused_fwd_speedup_vs_k3_torch": round(med("k3_torch_fwd") / med("fused_fwd"), 3),
            "fused_fwd_wins": wins("fused_fwd", "k3_torch_fwd"),
            "fused_loss_bwd_speedup_vs_k3_torch": round(med("k3_torch_loss_bwd") / med("fused_loss_bwd"), 3),
            "fused_loss_bwd_wins": wins("fused_loss_bwd", "k3_torch_loss_bwd"),
            "fused_step_speedup_vs_k3_torch": round(med("k3_torch_step") / med("fused_step"), 3),
            "fused_step_wins": wins("fused_step", "k3_torch_step"),
            "fused_fwd_frac_of_copy_ceiling": frac("fused_fwd", bytes_f),
            "fused_loss_bwd_frac_of_copy_ceiling": frac("fused_loss_bwd", bytes_l)}
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
