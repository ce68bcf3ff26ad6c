"""Fused attention (dr_attn_fwd / dr_attn_bwd) against the unfused composition a user of torch would write on the device in fp32
(matmul -> scale / mask -> softmax -> dropout -> matmul, autograd backward), forward and forward + backward, in ONE process.

  python tools/bench_attention.py [--rounds 7] [--iters 20 (the least per window; raised to fill ~50 ms)] [--shapes example,seqrec] [--log profiles/attention_bench.log]

Shapes: `example` (B 128, L 128, H 2, dh 4: the IMDB example's attention; launch- and softmax-bound, reported, not a gate) and
`seqrec` (B 512, L 256, H 8, dh 64: a sequence-recommender shape), each with a pre-padding mask (lengths uniform in [L / 4, L]),
dropout 0.1, future off and on.  Device events; every variant is warmed up; the two implementations alternate inside every round;
median and min over the rounds and the spread (max - min) / median are printed, one JSON line at the end.
FLOP: forward 4 B H Lq Lk dh (two products); forward + backward 22 B H Lq Lk dh -- the eleven products the kernels really perform
(S and P.V forward; S, dP for delta; S, dP, dV, dK in the key-owning sweep; S, dP, dQ in the query-owning sweep), against the 157.3 TF/s fp32 matrix
rate.  Bytes: Q, K, V, O once (forward), against 8 TB/s."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import ops  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
PEAK_HBM = 8.0e12
MASK_NUM = float(np.float32(-2 ** 32 + 1))
SHAPES = {"example": (128, 128, 2, 4), "seqrec": (512, 256, 8, 64)}


def compose(q, k, v, H, mask, future, rate):
    B, L, W = q.shape
    dh = W // H
    qh, kh, vh = (t.view(B, L, H, dh).transpose(1, 2) for t in (q, k, v))
    s = torch.matmul(qh, kh.transpose(-1, -2)) / math.sqrt(dh)
    s = s + mask[:, None, None, :].to(torch.float32) * MASK_NUM
    if future:
        hidden = torch.triu(torch.ones(L, L, dtype=torch.bool, device=q.device), diagonal=1)
        s = torch.where(hidden, torch.full((), MASK_NUM, device=q.device), s)
    p = torch.nn.functional.dropout(torch.softmax(s, dim=-1), rate, training=True)
    return torch.matmul(p, vh).transpose(1, 2).reshape(B, L, W)


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


def bench_shape(name, future, rounds, iters, log):
    B, L, H, dh = SHAPES[name]
    W = H * dh
    gen = torch.Generator(device="cuda").manual_seed(1)
    q, k, v, d_out = (torch.randn(B, L, W, device="cuda", generator=gen) for _ in range(4))
    lengths = torch.randint(L // 4, L + 1, (B,), device="cuda", generator=gen)
    mask = torch.arange(L, device="cuda")[None, :] < (L - lengths)[:, None]            # pre-padding: True at the padded front
    rate = 0.1
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    state = {"seed": 0}

    def fused_fwd():
        state["seed"] += 1
        return ops.attn_fwd(q, k, v, H, mask, future, rate, state["seed"])

    def fused_fwd_bwd():
        out, st = fused_fwd()
        return ops.attn_bwd(q, k, v, H, d_out, st, mask, future, rate, state["seed"])

    def torch_fwd():
        with torch.no_grad():
            return compose(q, k, v, H, mask, future, rate)

    def torch_fwd_bwd():
        qa.grad = ka.grad = va.grad = None
        compose(qa, ka, va, H, mask, future, rate).backward(d_out)

    # the two paths compute the same thing (dropout off: the two streams differ)
    a, st = ops.attn_fwd(q, k, v, H, mask, future, 0.0, 0)
    b = compose(q, k, v, H, mask, future, 0.0)
    diff = float((a - b).abs().max())
    del a, b, st
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
    flop_f = 4.0 * B * H * L * L * dh
    flop_fb = 22.0 * B * H * L * L * dh
    qkvo = 4.0 * B * L * W * 4
    f, fb = res["fused_fwd"]["median_ms"] * 1e-3, res["fused_fwd_bwd"]["median_ms"] * 1e-3
    out = {"shape": {"B": B, "L": L, "H": H, "dh": dh, "future": future, "dropout": rate}, "iters_per_window": reps, "max_abs_diff_fused_vs_torch_no_dropout": diff,
           **res,
           "speedup_fwd": round(res["torch_fwd"]["median_ms"] / res["fused_fwd"]["median_ms"], 3),
           "speedup_fwd_bwd": round(res["torch_fwd_bwd"]["median_ms"] / res["fused_fwd_bwd"]["median_ms"], 3),
           "fused_fwd_TFLOPs": round(flop_f / f / 1e12, 2), "fused_fwd_frac_of_f32_matrix_peak": round(flop_f / f / PEAK_F32_MATRIX, 4),
           "fused_fwd_bwd_TFLOPs": round(flop_fb / fb / 1e12, 2),
           "fused_fwd_bwd_frac_of_f32_matrix_peak": round(flop_fb / fb / PEAK_F32_MATRIX, 4),
           "fused_fwd_qkvo_GBps": round(qkvo / f / 1e9, 1), "fused_fwd_frac_of_hbm_peak": round(qkvo / f / PEAK_HBM, 4)}
    line = "%s future=%d: " % (name, future) + json.dumps(out)
    print(line, flush=True)
    if log:
        log.write(line + "\n")
        log.flush()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="example,seqrec")
    ap.add_argument("--log", default=None, help="also append the per-shape lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    log = open(a.log, "a") if a.log else None
    res = {"bench": "attention", "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        for future in (False, True):
            res["%s_future%d" % (name, future)] = bench_shape(name, future, a.rounds, a.iters, log)
    print(json.dumps(res))
    if log:
        log.close()


if __name__ == "__main__":
    main()
