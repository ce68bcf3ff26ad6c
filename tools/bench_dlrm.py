"""DLRM's pairwise dot interaction: the fused kernels (dr_dot_interact_fwd / dr_dot_interact_bwd) against the composition a user of torch
would write on the device in fp32 (torch.bmm -> [B, N, N] -> tril_indices gather -> cat, autograd backward), both in ONE process per
cell, alternating, with the copy ceiling (dr_copy_nt) measured in the same call.

  python tools/bench_dlrm.py [--rounds 7] [--iters 5 (the least per window; raised to fill ~50 ms)] [--cells b65536_d64,...]
                             [--limit 300 (seconds per cell)] [--log profiles/dlrm_bench.log]

Cells: `b65536_d64` (B 65 536, F 26, D 64, dense vector: the workload's input shape) and `b8192_d128` (B 8 192, F 26, D 128, dense), both
without self interaction; `train_step` is one DLRM training step at B 65 536, 26 hashed fields of 100 000 buckets, D 64, 13 dense
features, bottom [512, 256, 64], top [512, 256], BCE on the logits, fused SGD (the slab's rows in the gather's backward, dr_axpy on
the towers).

Every cell runs in a fresh child process under its own time limit, and the first failing cell stops the run.  Device events; every
variant is warmed up; the implementations alternate inside every round; median and min over the rounds and the spread (max - min) /
median are printed with every figure.  `wins` says whether the fused median is below the composition's by more than both spreads.
Bytes are the algorithm's: forward 4 B (N D + c0 + P) (T read once, the output written once), backward 4 B (2 N D + c0 + P) (T and
d_out read, dT written); the fraction is that traffic over the kernel's time, over the traffic per time of the copy (read + write of
a buffer of the forward's size)."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# cell -> (B, F, D)
CELLS = {"b65536_d64": (65536, 26, 64), "b8192_d128": (8192, 26, 128), "train_step": (65536, 26, 64)}


def stats(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"median_ms": round(med, 4), "min_ms": round(ms[0], 4), "spread": round((ms[-1] - ms[0]) / med, 4), "rounds": len(ms)}


def window(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def measure(variants, rounds, iters):
    """every variant warmed up, windows of >= ~50 ms, the variants alternating inside every round"""
    import torch
    reps = {}
    for n, fn in variants.items():
        for _ in range(3):
            fn()
        reps[n] = max(iters, int(math.ceil(50.0 / max(window(fn, iters), 1e-3))))
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(rounds):
        for n, fn in variants.items():
            times[n].append(window(fn, reps[n]))
    return {n: stats(t) for n, t in times.items()}, reps


def bench_interaction(name, rounds, iters):
    import torch
    from deep_recommenders_amd import ops
    B, F, D = CELLS[name]
    N = F + 1
    gen = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)                          # noqa: E731
    dense, emb = r(B, D), r(B, F * D)
    width = ops.dot_interact_width(F, D)
    d_out = torch.zeros((B, (width + 3) // 4 * 4), device="cuda")[:, :width]
    d_out.copy_(r(B, width))
    li, lj = torch.tril_indices(N, N, -1, device="cuda")
    leaves = [dense.clone().requires_grad_(True), emb.clone().requires_grad_(True)]

    def compose(a, e):
        T = torch.cat([a[:, None, :], e.reshape(B, F, D)], dim=1)
        Z = torch.bmm(T, T.transpose(1, 2))
        return torch.cat([a, Z[:, li, lj]], dim=1)

    def fused_fwd():
        return ops.dot_interact_fwd(dense, emb, F, D)

    def torch_fwd():
        with torch.no_grad():
            return compose(dense, emb)

    def fused_bwd():
        return ops.dot_interact_bwd(dense, emb, F, D, d_out)

    def fused_fwd_bwd():
        fused_fwd()
        return fused_bwd()

    def torch_fwd_bwd():
        for t in leaves:
            t.grad = None
        torch.autograd.backward([compose(*leaves)], [d_out])

    src = torch.empty(B * (N * D + width), device="cuda")                                   # the forward's traffic, as one copy
    dst = torch.empty_like(src)

    def copy():
        return ops.copy_nt(src, dst)

    # faster and different is not faster: both implementations on these inputs
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())                          # noqa: E731
    diffs = {"out_fused_vs_torch": rel(fused_fwd(), torch_fwd())}
    gd, ge = fused_bwd()
    torch_fwd_bwd()
    diffs["d_dense_fused_vs_torch"] = rel(gd, leaves[0].grad)
    diffs["d_emb_fused_vs_torch"] = rel(ge, leaves[1].grad)
    del gd, ge
    variants = {"fused_fwd": fused_fwd, "torch_fwd": torch_fwd, "fused_bwd": fused_bwd, "fused_fwd_bwd": fused_fwd_bwd,
                "torch_fwd_bwd": torch_fwd_bwd, "copy_nt": copy}
    res, reps = measure(variants, rounds, iters)
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    wins = lambda a, b: bool(med(a) * (1 + res[a]["spread"]) < med(b) * (1 - res[b]["spread"]))   # noqa: E731
    bytes_f = 4.0 * B * (N * D + width)
    bytes_b = 4.0 * B * (2 * N * D + width)
    ceiling = 2.0 * src.numel() * 4 / (med("copy_nt") * 1e-3)
    out = {"shape": {"B": B, "F": F, "D": D, "N": N, "dense": True, "self_interaction": False, "width": width},
           "iters_per_window": reps, "max_rel_diff": diffs, **res,
           "copy_ceiling_GBps": round(ceiling / 1e9, 1),
           "fwd_speedup_vs_torch": round(med("torch_fwd") / med("fused_fwd"), 3), "fwd_wins": wins("fused_fwd", "torch_fwd"),
           "fwd_bwd_speedup_vs_torch": round(med("torch_fwd_bwd") / med("fused_fwd_bwd"), 3),
           "fwd_bwd_wins": wins("fused_fwd_bwd", "torch_fwd_bwd"),
           "fused_fwd_GBps": round(bytes_f / (med("fused_fwd") * 1e-3) / 1e9, 1),
           "fused_fwd_frac_of_copy_ceiling": round(bytes_f / (med("fused_fwd") * 1e-3) / ceiling, 4),
           "fused_bwd_GBps": round(bytes_b / (med("fused_bwd") * 1e-3) / 1e9, 1),
           "fused_bwd_frac_of_copy_ceiling": round(bytes_b / (med("fused_bwd") * 1e-3) / ceiling, 4)}
    print("%s: %s" % (name, json.dumps(out)), flush=True)


def bench_train_step(name, rounds, iters):
    import torch
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd import losses, ops
    from deep_recommenders_amd.keras.models.ranking import DLRM
    B, F, D = CELLS[name]
    Nd, V, lr = 13, 100000, 0.05
    torch.manual_seed(42)
    cols = [fc.embedding_column(fc.categorical_column_with_hash_bucket("c%d" % i, V, dtype=int), D) for i in range(F)]
    model = DLRM(cols, bottom_units_size=[512, 256, D], top_units_size=[512, 256], dense_features_key="dense")
    model.slab.sparse_lr = lr
    gen = torch.Generator(device="cuda").manual_seed(42)
    inputs = {"c%d" % i: torch.randint(0, 10 ** 15, (B, 1), device="cuda", generator=gen) for i in range(F)}
    inputs["dense"] = torch.log1p(torch.randn((B, Nd), device="cuda", generator=gen).abs())
    labels = (torch.rand((B, 1), device="cuda", generator=gen) < 0.25).float()
    seen = []

    def step():
        loss = losses.sigmoid_cross_entropy(labels, model.logits(inputs))
        loss.backward()
        for p in model.parameters():
            if p.grad is not None:                                   # the towers; the slab's rows were updated in the backward
                ops.axpy(-lr, p.grad, p.data)
                p.grad = None
        seen.append(loss.detach())

    res, reps = measure({"train_step": step}, rounds, max(iters, 3))
    first, last = float(seen[0]), float(seen[-1])
    out = {"shape": {"B": B, "F": F, "D": D, "num_dense": Nd, "buckets_per_field": V, "bottom": [512, 256, D], "top": [512, 256]},
           "iters_per_window": reps, **res, "examples_per_s": round(B / (res["train_step"]["median_ms"] * 1e-3)),
           "loss_first": round(first, 5), "loss_last": round(last, 5), "steps_run": len(seen)}
    print("%s: %s" % (name, json.dumps(out)), flush=True)


def bench_cell(name, rounds, iters):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dlrm needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    (bench_train_step if name == "train_step" else bench_interaction)(name, rounds, iters)


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
