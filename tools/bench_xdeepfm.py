"""xDeepFM's CIN layer: the fused CIN + sum-pooling kernels (dr_cin_pool_fwd / dr_cin_pool_bwd) against the existing kernels (dr_cin_fwd +
torch.sum, dr_cin_bwd) and against the composition a user of torch would write on the device in fp32 (einsum outer product -> matmul ->
sum, autograd backward), all three in ONE process per cell.

  python tools/bench_xdeepfm.py [--rounds 7] [--iters 5 (the least per window; raised to fill ~50 ms)] [--cells b4096_l1,...]
                                [--limit 300 (seconds per cell)] [--log profiles/xdeepfm_bench.log]

Cells: the distinct layers of two stacks over 39 fields of D 16 -- B 4096 with CIN layers (100, 100): `b4096_l1` (H0 39, Hk 39, Fm 100) and
`b4096_l2` (Hk 100); B 16384 with layers (200, 200, 200): `b16384_l1` (Hk 39, Fm 200) and `b16384_l2` (Hk 200, Fm 200; layers 2 and 3).
Linear activation, no bias.  The backward cells feed d_out and d_pooled to the new kernel, d_out + d_pooled[:, :, None] to the old one.

Every cell runs in a fresh child process under its own time limit, and the first failing cell stops the run.  Device events; every
variant is warmed up; the implementations alternate inside every round; median and min over the rounds and the spread (max - min) /
median are printed with every figure.  A variant whose single call takes more than 200 ms (the old backward at the large shape) gets one
call per window and three rounds instead of a longer limit.
FLOP: the useful ones -- forward 2 B D H0 Hk Fm; backward twice that for T = g W^T and z^T g (the two contractions of T with x0 / x add
4 B D H0 Hk) -- against the 157.3 TF/s fp32 matrix rate; the kernels' padding of Hk and Fm to the MFMA tile is not counted as work."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MATRIX = 157.3e12
FIELDS, DIM = 39, 16
# cell -> (B, H0, Hk, D, Fm)
CELLS = {"b4096_l1": (4096, FIELDS, FIELDS, DIM, 100), "b4096_l2": (4096, FIELDS, 100, DIM, 100),
         "b16384_l1": (16384, FIELDS, FIELDS, DIM, 200), "b16384_l2": (16384, FIELDS, 200, DIM, 200)}
SLOW_MS = 200.0


def stats(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"median_ms": round(med, 4), "min_ms": round(ms[0], 4), "spread": round((ms[-1] - ms[0]) / med, 4), "rounds": len(ms)}


def bench_cell(name, rounds, iters):
    import torch
    from deep_recommenders_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_xdeepfm needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    B, H0, Hk, D, Fm = CELLS[name]
    gen = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)                          # noqa: E731
    x0, x, W = r(B, H0, D), r(B, Hk, D), r(H0 * Hk, Fm) / math.sqrt(H0 * Hk)
    d_out, d_pooled = r(B, Fm, D), r(B, Fm)
    d_sum = d_out + d_pooled[:, :, None]
    out = ops.cin_fwd(x0, x, W, None, 0)
    leaves = [t.clone().requires_grad_(True) for t in (x0, x, W)]

    def window(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    def compose(a0, a, w):
        z = torch.einsum("bid,bjd->bijd", a0, a).reshape(B, H0 * Hk, D)
        o = torch.einsum("bkd,kf->bfd", z, w)
        return o, o.sum(-1)

    def new_fwd():
        return ops.cin_pool_fwd(x0, x, W, None, 0)

    def old_fwd():
        o = ops.cin_fwd(x0, x, W, None, 0)
        return o, o.sum(-1)

    def torch_fwd():
        with torch.no_grad():
            return compose(x0, x, W)

    def new_bwd():
        return ops.cin_pool_bwd(x0, x, W, 0, out, d_out, d_pooled)

    def old_bwd():
        return ops.cin_bwd(x0, x, W, 0, out, d_sum)

    def torch_fwd_bwd():
        for t in leaves:
            t.grad = None
        o, p = compose(*leaves)
        torch.autograd.backward([o, p], [d_out, d_pooled])

    # faster and different is not faster: the three implementations on these inputs
    n_out, n_pooled = new_fwd()
    o_out, o_pooled = old_fwd()
    t_out, t_pooled = torch_fwd()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())                          # noqa: E731
    diffs = {"out_new_vs_old": rel(n_out, o_out), "pooled_new_vs_old": rel(n_pooled, o_pooled), "out_new_vs_torch": rel(n_out, t_out),
             "pooled_new_vs_torch": rel(n_pooled, t_pooled)}
    ng, og = new_bwd(), old_bwd()
    torch_fwd_bwd()
    for k, nm in enumerate(("d_x0", "d_x", "dW")):
        diffs[nm + "_new_vs_old"] = rel(ng[k], og[k])
        diffs[nm + "_new_vs_torch"] = rel(ng[k], leaves[k].grad)
    del n_out, o_out, t_out, ng, og
    variants = {"new_fwd": new_fwd, "old_fwd_plus_sum": old_fwd, "torch_fwd": torch_fwd, "new_bwd": new_bwd, "old_bwd": old_bwd,
                "torch_fwd_bwd": torch_fwd_bwd}
    reps, nround = {}, {}
    for n, fn in variants.items():                           # every variant has run once above: this call is warm
        one = window(fn, 1)
        if one > SLOW_MS:
            reps[n], nround[n] = 1, min(rounds, 3)
            continue
        for _ in range(2):
            fn()
        reps[n], nround[n] = max(iters, int(math.ceil(50.0 / max(window(fn, iters), 1e-3)))), rounds
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for k in range(rounds):
        for n, fn in variants.items():                       # alternating inside every round
            if k < nround[n]:
                times[n].append(window(fn, reps[n]))
    res = {n: stats(t) for n, t in times.items()}
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    flop_f = 2.0 * B * D * H0 * Hk * Fm
    flop_b = 2 * flop_f + 4.0 * B * D * H0 * Hk
    res_out = {"shape": {"B": B, "H0": H0, "Hk": Hk, "D": D, "Fm": Fm, "act": "linear"}, "iters_per_window": reps, "max_rel_diff": diffs, **res,
               "dw_partials": ops.cin_pool_bwd_partials(B, H0, Hk, D, Fm),
               "fwd_speedup_vs_old": round(med("old_fwd_plus_sum") / med("new_fwd"), 3),
               "fwd_speedup_vs_torch": round(med("torch_fwd") / med("new_fwd"), 3),
               "bwd_speedup_vs_old": round(med("old_bwd") / med("new_bwd"), 3),
               "new_fwd_TFLOPs": round(flop_f / med("new_fwd") / 1e9, 2),
               "new_fwd_frac_of_f32_matrix_peak": round(flop_f / (med("new_fwd") * 1e-3) / PEAK_F32_MATRIX, 4),
               "old_fwd_frac_of_f32_matrix_peak": round(flop_f / (med("old_fwd_plus_sum") * 1e-3) / PEAK_F32_MATRIX, 4),
               "new_bwd_TFLOPs": round(flop_b / med("new_bwd") / 1e9, 2),
               "new_bwd_frac_of_f32_matrix_peak": round(flop_b / (med("new_bwd") * 1e-3) / PEAK_F32_MATRIX, 4),
               "torch_fwd_bwd_over_new_fwd_plus_bwd": round(med("torch_fwd_bwd") / (med("new_fwd") + med("new_bwd")), 3)}
    print("%s: %s" % (name, json.dumps(res_out)), flush=True)


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
