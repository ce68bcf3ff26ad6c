"""EBR's in-batch triplet loss, two ways in ONE process per cell, alternating:

  (a) torch   the fp32 composition a user of torch would write on the device: normalise q and d -> matmul -> mask the diagonal ->
              optional topk -> relu(margin - t + s), summed; forward + backward is autograd back to q and d.  It keeps the [B, B]
              scores, their mask and their gradient.  Skipped where those do not fit (the cell says so).
  (b) fused   dr_margin_rank_fwd (forward only) and forward + dr_margin_rank_bwd + the add of d_neg onto d_pos (layers.margin_rank).
              The towers are the same code either way and are not timed.

  python tools/bench_ebr.py [--rounds 7] [--iters 5 (the least per window; raised to fill ~50 ms)] [--cells b8k_d64_h0,...]
                            [--limit 300 (seconds per cell)] [--log profiles/ebr_bench.log]

Cells: B 8 192 and B 65 536 in-batch at D 64 and D 256, with num_hard 0 and 2; cosine, margin 0.2, Gaussian rows, every row valid,
row_scale = 1 / B.  Every cell runs in a fresh child process under its own time limit, and the first failing cell stops the run.
Device events; every variant is warmed up; the implementations alternate inside every round; median and min over the rounds and the
spread (max - min) / median are printed with every figure, and the peak of torch's allocator over one call of each variant above what
was allocated before it.  FLOP are those of the products really performed: 2 B B D each, one in the forward, four in the backward
(the scores and the weighted sum in the row-owning sweep and again in the column-owning one); the rate is given as a share of the fp32
matrix peak (157.3 TFLOP/s: 256 CUs x 4 SIMDs x 64 FLOP / clk x 2.4 GHz)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ffm import measure, peak_mb  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
MARGIN = 0.2
# cell -> (B, D, num_hard)
CELLS = {"b%dk_d%d_h%d" % (B // 1024, D, K): (B, D, K) for B in (8192, 65536) for D in (64, 256) for K in (0, 2)}
TORCH_BUDGET = 0.6          # the share of the device's free memory the torch side's five [B, B] tensors may take


def bench_cell(name, rounds, iters):
    import torch
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_ebr needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    B, D, K = CELLS[name]
    inv = 1.0 / B
    gen = torch.Generator(device="cuda").manual_seed(1)
    q = torch.empty((B, D), device="cuda").normal_(0, 1.0, generator=gen)
    d = torch.empty((B, D), device="cuda").normal_(0, 1.0, generator=gen)
    ws = ops.margin_rank_workspace(B, B, D, K, "cuda")
    free, _ = torch.cuda.mem_get_info()
    with_torch = 5.0 * 4.0 * B * B <= TORCH_BUDGET * free          # scores, mask, masked scores, hinge, gradient

    def compose(qq, dd):
        qh = qq * torch.clamp_min((qq * qq).sum(-1, keepdim=True), 1e-12) ** -0.5
        dh = dd * torch.clamp_min((dd * dd).sum(-1, keepdim=True), 1e-12) ** -0.5
        t = (qh * dh).sum(-1)
        s = (qh @ dh.T).masked_fill(torch.eye(B, dtype=torch.bool, device="cuda"), -float("inf"))
        if K > 0:
            s = torch.topk(s, K, dim=1).values
        return torch.relu((MARGIN - t)[:, None] + s).sum(-1)

    def torch_fwd():
        with torch.no_grad():
            return compose(q, d)

    def torch_fwd_bwd():
        qq, dd = q.detach().requires_grad_(True), d.detach().requires_grad_(True)
        (compose(qq, dd).sum() * inv).backward()
        return qq.grad, dd.grad

    def fused_fwd():
        return ops.margin_rank_fwd(q, d, None, margin=MARGIN, num_hard=K, workspace=ws)[1]

    def fused_fwd_bwd():
        _, _, d_q, d_d, _ = L.margin_rank(q, d, margin=MARGIN, num_hard_negatives=K, row_scale=inv)
        return d_q, d_d

    variants = {"fused_fwd": fused_fwd, "fused_fwd_bwd": fused_fwd_bwd}
    diffs = {}
    peaks = {"fused_fwd": peak_mb(fused_fwd), "fused_fwd_bwd": peak_mb(fused_fwd_bwd), "fused_workspace": round(ws.numel() / 2 ** 20, 1),
             "one_B_by_B_matrix": round(4.0 * B * B / 2 ** 20, 1)}
    if with_torch:
        # faster and different is not faster: the two forwards and the two d_q on these inputs
        want = torch_fwd()
        diffs["fused_vs_torch_loss"] = float((fused_fwd() - want).abs().max() / want.abs().max())
        g_want, g_got = torch_fwd_bwd()[0], fused_fwd_bwd()[0]
        diffs["fused_vs_torch_d_q"] = float((g_got - g_want).abs().max() / g_want.abs().max())
        del want, g_want, g_got
        peaks.update(torch_fwd=peak_mb(torch_fwd), torch_fwd_bwd=peak_mb(torch_fwd_bwd))
        variants = {"torch_fwd": torch_fwd, "fused_fwd": fused_fwd, "torch_fwd_bwd": torch_fwd_bwd, "fused_fwd_bwd": fused_fwd_bwd}
    res, reps = measure(variants, rounds, iters)
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    flop = 2.0 * B * B * D
    tf = lambda n, products: round(products * flop / (med(n) * 1e-3) / 1e12, 2)             # noqa: E731
    out = {"shape": {"B": B, "D": D, "num_hard": K, "col_groups": ops.margin_rank_col_groups(B, B, D),
                     "row_chunks": ops.margin_rank_row_chunks(B, B, D)},
           "torch_side": "measured" if with_torch else "skipped: five [B, B] fp32 tensors do not fit",
           "iters_per_window": reps, "max_rel_diff": diffs, "peak_MB": peaks, **res,
           "GFLOP_per_product": round(flop / 1e9, 2),
           "fused_fwd_TFLOPs": tf("fused_fwd", 1), "fused_fwd_bwd_TFLOPs": tf("fused_fwd_bwd", 5),
           "fused_fwd_frac_of_fp32_matrix_peak": round(tf("fused_fwd", 1) * 1e12 / PEAK_F32_MATRIX, 4),
           "fused_fwd_bwd_frac_of_fp32_matrix_peak": round(tf("fused_fwd_bwd", 5) * 1e12 / PEAK_F32_MATRIX, 4)}
    if with_torch:
        out.update(torch_fwd_TFLOPs=tf("torch_fwd", 1), torch_fwd_bwd_TFLOPs=tf("torch_fwd_bwd", 3),
                   fused_fwd_speedup_vs_torch=round(med("torch_fwd") / med("fused_fwd"), 3),
                   fused_fwd_bwd_speedup_vs_torch=round(med("torch_fwd_bwd") / med("fused_fwd_bwd"), 3))
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
