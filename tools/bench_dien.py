"""The fused GRU / AUGRU sequence kernels (dr_gru_seq_fwd / dr_gru_seq_bwd) against the per-step composition a user of torch would
write on the device in fp32 (matmul, slices, sigmoid, tanh, where; autograd backward), forward and forward + backward, in ONE process.
For the plain full-length GRU the whole layer (input projection + recurrence, from seq [B, T, D]) is also timed against torch.nn.GRU.

  python tools/bench_dien.py [--rounds 5] [--iters 2 (the least per window; raised to fill ~30 ms)] [--shapes t50,t200] [--log profiles/dien_bench.log]

Shapes: B 8192, D = H = 64; T 50 (`t50`) and T 200 (`t200`) -- tools/bench_din.py's.  Two settings per shape: `gru` (no att, every
sequence of full length) and `augru` (att ~ U(0, 1), lengths uniform in [T / 4, T]).  Device events; every variant is warmed up; the
implementations alternate inside every round; median and min over the rounds and the spread (max - min) / median are printed, one JSON
line at the end.
FLOP: the MFMA products the kernels really perform -- forward one [16, 64] x [64, 192] product per step of a 16-example tile up to the
tile's longest example, backward that product again plus [16, 192] x [192, 64] -- against the 157.3 TF/s fp32 matrix rate (the dU
product of the dense path is not counted).  Bytes: xp once and hs once (forward), against 8 TB/s."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import ops  # noqa: E402
from deep_recommenders_amd.keras.models.ranking import GRU  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
PEAK_HBM = 8.0e12
SHAPES = {"t50": (8192, 50, 64, 64), "t200": (8192, 200, 64, 64)}


def compose(xp, U, h0, lengths, att):
    B, T, _ = xp.shape
    H = U.shape[0]
    h, hs = h0, []
    for t in range(T):
        g = h @ U
        u = torch.sigmoid(xp[:, t, :H] + g[:, :H])
        r = torch.sigmoid(xp[:, t, H:2 * H] + g[:, H:2 * H])
        c = torch.tanh(xp[:, t, 2 * H:] + r * g[:, 2 * H:])
        if att is not None:
            u = att[:, t, None] * u
        hn = (1 - u) * h + u * c
        if lengths is not None:
            on = (t < lengths)[:, None]
            h = torch.where(on, hn, h)
            hs.append(torch.where(on, h, torch.zeros((), device=xp.device)))
        else:
            h = hn
            hs.append(h)
    return torch.stack(hs, dim=1), h


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


def measure(variants, rounds, iters):
    for n, fn in variants.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        print("  warmed up %s" % n, flush=True)
    reps = {n: max(iters, int(math.ceil(30.0 / max(window(fn, iters), 1e-3)))) for n, fn in variants.items()}
    times = {n: [] for n in variants}
    for _ in range(rounds):
        for n, fn in variants.items():                       # alternating inside every round
            times[n].append(window(fn, reps[n]))
    return {n: stats(t) for n, t in times.items()}, reps


def bench_setting(name, setting, rounds, iters, log):
    B, T, D, H = SHAPES[name]
    gen = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)                          # noqa: E731
    xp, U, h0, d_hs, d_hl = r(B, T, 3 * H), r(H, 3 * H) / math.sqrt(H), 0.5 * r(B, H), r(B, T, H), r(B, H)
    augru = setting == "augru"
    att = torch.rand((B, T), device="cuda", generator=gen) if augru else None
    lengths = torch.randint(T // 4, T + 1, (B,), device="cuda", generator=gen).to(torch.int32) if augru else None
    leaves = [t.clone().requires_grad_(True) for t in ((xp, U, h0, att) if augru else (xp, U, h0))]
    ws = ops.gru_seq_bwd_workspace(B, T, H, "cuda")
    hs_buf, dxp_buf = torch.empty((B, T, H), device="cuda"), torch.empty((B, T, 3 * H), device="cuda")

    def fused_fwd():
        return ops.gru_seq_fwd(xp, U, h0, lengths, att, hs=hs_buf)

    def fused_fwd_bwd():
        hs, _ = fused_fwd()
        return ops.gru_seq_bwd(xp, U, h0, lengths, att, hs, d_hs, d_hl, d_xp=dxp_buf, workspace=ws)

    def torch_fwd():
        with torch.no_grad():
            return compose(xp, U, h0, lengths, att)

    def torch_fwd_bwd():
        for t in leaves:
            t.grad = None
        hs, hl = compose(leaves[0], leaves[1], leaves[2], lengths, leaves[3] if augru else None)
        torch.autograd.backward([hs, hl], [d_hs, d_hl])

    a, c = fused_fwd()[0], torch_fwd()[0]
    diff = float((a - c).abs().max() / c.abs().max())
    gf = fused_fwd_bwd()
    torch_fwd_bwd()
    diff_dxp = float((gf[0] - leaves[0].grad).abs().max() / leaves[0].grad.abs().max())
    diff_dU = float((gf[1] - leaves[1].grad).abs().max() / leaves[1].grad.abs().max())
    del a, c, gf
    variants = {"fused_fwd": fused_fwd, "torch_fwd": torch_fwd, "fused_fwd_bwd": fused_fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd}
    extra = {}
    if not augru:
        # the whole layer from seq [B, T, D]: input projection + recurrence, through autograd, against torch.nn.GRU (MIOpen)
        seq = r(B, T, D)
        layer = GRU(H)
        layer.build(D)
        seq_l = seq.clone().requires_grad_(True)

        def layer_fwd():
            with torch.no_grad():
                return layer(seq)

        def layer_fwd_bwd():
            seq_l.grad = None
            layer.zero_grad(set_to_none=True)
            hs, hl = layer(seq_l, return_state=True)
            torch.autograd.backward([hs, hl], [d_hs, d_hl])

        variants.update(layer_fwd=layer_fwd, layer_fwd_bwd=layer_fwd_bwd)
        try:
            ref = torch.nn.GRU(D, H, batch_first=True).cuda()
            seq_r = seq.clone().requires_grad_(True)

            def nn_gru_fwd():
                with torch.no_grad():
                    return ref(seq)

            def nn_gru_fwd_bwd():
                seq_r.grad = None
                ref.zero_grad(set_to_none=True)
                hs, hl = ref(seq_r)
                torch.autograd.backward([hs, hl], [d_hs, d_hl[None]])

            nn_gru_fwd()
            nn_gru_fwd_bwd()
            torch.cuda.synchronize()
            variants.update(nn_gru_fwd=nn_gru_fwd, nn_gru_fwd_bwd=nn_gru_fwd_bwd)
        except Exception as e:                                                              # noqa: BLE001 -- reported, not hidden
            extra["nn_gru"] = "NOT MEASURED: torch.nn.GRU failed on this device: %s" % (str(e).splitlines() or [type(e).__name__])[0][:200]
    res, reps = measure(variants, rounds, iters)
    steps = float(((lengths.reshape(-1, 16).max(dim=1).values.sum()) if augru else torch.tensor(B // 16 * T)))
    flop_f = steps * 2.0 * 16 * H * 3 * H
    flop_fb = flop_f + steps * 2 * 2.0 * 16 * H * 3 * H
    n_valid = float(lengths.sum()) if augru else float(B * T)
    f, fb = res["fused_fwd"]["median_ms"] * 1e-3, res["fused_fwd_bwd"]["median_ms"] * 1e-3
    out = {"shape": {"B": B, "T": T, "D": D, "H": H, "setting": setting, "mean_length": round(n_valid / B, 1)},
           "iters_per_window": reps, "max_rel_diff_hs_fused_vs_torch": diff, "max_rel_diff_dxp": diff_dxp, "max_rel_diff_dU": diff_dU, **res,
           "speedup_fwd": round(res["torch_fwd"]["median_ms"] / res["fused_fwd"]["median_ms"], 3),
           "speedup_fwd_bwd": round(res["torch_fwd_bwd"]["median_ms"] / res["fused_fwd_bwd"]["median_ms"], 3),
           "fused_fwd_TFLOPs": round(flop_f / f / 1e12, 2), "fused_fwd_frac_of_f32_matrix_peak": round(flop_f / f / PEAK_F32_MATRIX, 4),
           "fused_fwd_bwd_TFLOPs": round(flop_fb / fb / 1e12, 2),
           "fused_fwd_bwd_frac_of_f32_matrix_peak": round(flop_fb / fb / PEAK_F32_MATRIX, 4),
           "fused_fwd_GBps": round(n_valid * 4 * H * 4 / f / 1e9, 1), "fused_fwd_frac_of_hbm_peak": round(n_valid * 4 * H * 4 / f / PEAK_HBM, 4),
           **extra}
    if "nn_gru_fwd" in res:
        out["layer_vs_nn_gru_fwd"] = round(res["nn_gru_fwd"]["median_ms"] / res["layer_fwd"]["median_ms"], 3)
        out["layer_vs_nn_gru_fwd_bwd"] = round(res["nn_gru_fwd_bwd"]["median_ms"] / res["layer_fwd_bwd"]["median_ms"], 3)
    line = "%s %s: " % (name, setting) + json.dumps(out)
    print(line, flush=True)
    if log:
        log.write(line + "\n")
        log.flush()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--shapes", default="t50,t200")
    ap.add_argument("--log", default=None, help="also append the per-setting lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dien needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    log = open(a.log, "a") if a.log else None
    res = {"bench": "dien_gru_sequence", "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        for setting in ("gru", "augru"):
            res["%s_%s" % (name, setting)] = bench_setting(name, setting, a.rounds, a.iters, log)
    print(json.dumps(res))
    if log:
        log.close()


if __name__ == "__main__":
    main()
