"""Fused DIN interest pooling (dr_din_pool_fwd / dr_din_pool_bwd) against the composition a user of torch would write on the device in
fp32 (expand the query -> cat [q, k, q * k] -> matmul -> Dice -> matmul -> mask -> weighted sum, autograd backward), forward and
forward + backward, in ONE process.

  python tools/bench_din.py [--rounds 7] [--iters 10 (the least per window; raised to fill ~50 ms)] [--shapes t50,t200] [--log profiles/din_bench.log]

Shapes: B 8192, D 64, U 80, Multiply interacter, Dice; T 50 (`t50`) and T 200 (`t200`); lengths uniform in [T / 4, T].  Device events;
every variant is warmed up; the two implementations alternate inside every round; median and min over the rounds and the spread
(max - min) / median are printed, one JSON line at the end.
FLOP: the MFMA products the kernels really perform, padding included -- forward: one [16, D16] x [D16, U16] product per 16-key tile
that holds a valid key; backward: three more per such tile (the hidden layer again, dH Weff^T, dH W[2D:3D]^T) and three
[D16, 4] x [4, U16] chains over ALL B * T rows for the weight gradients (K^T G, q^T G, (q * k)^T G) -- against the 157.3 TF/s fp32
matrix rate.  Bytes: the valid keys once (forward), against 8 TB/s."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import ops  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
PEAK_HBM = 8.0e12
SHAPES = {"t50": (8192, 50, 64, 80), "t200": (8192, 200, 64, 80)}
MODE, ACT, EPS = 2, 4, 1e-8


def compose(q, k, valid, W, b, w_out, b_out, alpha):
    B, T, D = k.shape
    qe = q[:, None, :].expand(B, T, D).reshape(B * T, D)
    kf = k.reshape(B * T, D)
    h = torch.cat([qe, kf, qe * kf], dim=1) @ W + b
    m = h.mean(dim=1, keepdim=True)
    s = torch.sqrt(((h - m) ** 2).mean(dim=1, keepdim=True))
    p = torch.sigmoid((h - m) / torch.sqrt(s + EPS))
    pre = torch.relu(h) - alpha * torch.relu(-h)
    a = torch.where(pre > 0, p * pre, (1 - p) * pre)
    scores = torch.where(valid, (a @ w_out + b_out).reshape(B, T), torch.zeros((), device=k.device))
    return (scores[:, :, None] * k).sum(dim=1), scores


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def stats(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"median_ms": round(med, 4), "min_ms": round(ms[0], 4), "spread": round((ms[-1] - ms[0]) / med, 4)}


def bench_shape(name, rounds, iters, log):
    B, T, D, U = SHAPES[name]
    gen = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)                          # noqa: E731
    q, k, d_out = r(B, D), r(B, T, D), r(B, D)
    W, b, w_out, b_out, alpha = r(3 * D, U) / math.sqrt(3 * D), r(U) * 0.1, r(U, 1) / math.sqrt(U), r(1) * 0.1, r(U) * 0.25
    lengths = torch.randint(T // 4, T + 1, (B,), device="cuda", generator=gen)
    valid = torch.arange(T, device="cuda")[None, :] < lengths[:, None]
    leaves = [t.clone().requires_grad_(True) for t in (q, k, W, b, w_out, b_out, alpha)]

    def fused_fwd():
        return ops.din_pool_fwd(q, k, valid, W, b, w_out, b_out, MODE, ACT, alpha, EPS)

    def fused_fwd_bwd():
        fused_fwd()
        return ops.din_pool_bwd(q, k, valid, W, b, w_out, b_out, MODE, ACT, d_out, None, alpha, EPS)

    def torch_fwd():
        with torch.no_grad():
            return compose(q, k, valid, W, b, w_out, b_out, alpha)

    def torch_fwd_bwd():
        for t in leaves:
            t.grad = None
        compose(leaves[0], leaves[1], valid, *leaves[2:])[0].backward(d_out)

    a = fused_fwd()[0]
    c = torch_fwd()[0]
    diff = float((a - c).abs().max() / c.abs().max())
    del a, c
    variants = {"fused_fwd": fused_fwd, "torch_fwd": torch_fwd, "fused_fwd_bwd": fused_fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # a window of at least ~50 ms of device work per variant: a shorter one measures the clock and the launch queue
    reps = {n: max(iters, int(math.ceil(50.0 / max(window(fn, iters), 1e-3)))) for n, fn in variants.items()}
    times = {n: [] for n in variants}
    for _ in range(rounds):
        for n, fn in variants.items():                       # alternating inside every round
            times[n].append(window(fn, reps[n]))
    res = {n: stats(t) for n, t in times.items()}
    D16, U16 = (D + 15) // 16 * 16, (U + 15) // 16 * 16
    tiles = int(((lengths + 15) // 16).sum())
    flop_tile = 2.0 * 16 * D16 * U16
    flop_f = tiles * flop_tile
    flop_fb = 4 * tiles * flop_tile + 3 * 2.0 * B * T * D16 * U16
    key_bytes = float(lengths.sum()) * D * 4
    f, fb = res["fused_fwd"]["median_ms"] * 1e-3, res["fused_fwd_bwd"]["median_ms"] * 1e-3
    out = {"shape": {"B": B, "T": T, "D": D, "U": U, "mode": "multiply", "act": "dice", "mean_length": round(float(lengths.float().mean()), 1)},
           "iters_per_window": reps, "max_rel_diff_fused_vs_torch": diff, **res,
           "speedup_fwd": round(res["torch_fwd"]["median_ms"] / res["fused_fwd"]["median_ms"], 3),
           "speedup_fwd_bwd": round(res["torch_fwd_bwd"]["median_ms"] / res["fused_fwd_bwd"]["median_ms"], 3),
           "fused_fwd_TFLOPs": round(flop_f / f / 1e12, 2), "fused_fwd_frac_of_f32_matrix_peak": round(flop_f / f / PEAK_F32_MATRIX, 4),
           "fused_fwd_bwd_TFLOPs": round(flop_fb / fb / 1e12, 2),
           "fused_fwd_bwd_frac_of_f32_matrix_peak": round(flop_fb / fb / PEAK_F32_MATRIX, 4),
           "fused_fwd_keys_GBps": round(key_bytes / f / 1e9, 1), "fused_fwd_frac_of_hbm_peak": round(key_bytes / f / PEAK_HBM, 4)}
    line = "%s: " % name + json.dumps(out)
    print(line, flush=True)
    if log:
        log.write(line + "\n")
        log.flush()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default="t50,t200")
    ap.add_argument("--log", default=None, help="also append the per-shape lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_din needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    log = open(a.log, "a") if a.log else None
    res = {"bench": "din_interest_pooling", "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        res[name] = bench_shape(name, a.rounds, a.iters, log)
    print(json.dumps(res))
    if log:
        log.close()


if __name__ == "__main__":
    main()
