"""Mini-batch GraphSAGE on the scaled power-law graph of tools/bench_gcn.py (N = 2^20 nodes, ~34.6 M nonzeros): what a sampled step
costs against the full-graph GCN step, and the device sampling chain against a torch composition of it.  ONE process, alternating.

  python tools/bench_sage.py [--rounds 7] [--iters 3 (the least per window; raised to fill ~50 ms)] [--variants a,b,...]
                             [--log profiles/sage_bench.log]

B = 1024 seeds, fanouts (25, 10), features D = 256, GraphSAGE(256, 256) + a 47-class head.  Variants:
  sample_chain    layers.sample_blocks alone: per layer dr_neighbor_sample, dr_frontier_build, dr_block_csr, then the one read-back
  train_step      one training step: sample_blocks, dr_rows_gather of the input rows, forward, backward, Adam
  torch_sampling  the same chain written with torch on the device: per node `fanout` draws floor(rand * deg) into its row (WITH
                  replacement -- without it torch needs a dense [n, max degree] argsort, 10^5 wide here -- so this side does less
                  work than the kernels do), torch.unique of dst ++ nbr, searchsorted for the local indices, and the mean of the
                  indexed rows in place of the block CSR; one read-back (unique's) per layer
  gcn_full_step   tools/bench_gcn.py's `scaled` training step (GCN(256) -> GCN(256) -> GCN(47, softmax) on D_in = 128, full graph)
Device events; every variant is warmed up; the variants alternate inside every round; median and min over the rounds and the spread
(max - min) / median are printed with every figure, one JSON line at the end (appended to --log).  The seeds and the sampling seed
change every call, so no call reuses another's blocks."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_gcn  # noqa: E402
from deep_recommenders_amd import layers as L  # noqa: E402
from deep_recommenders_amd import losses, optim  # noqa: E402
from deep_recommenders_amd.keras.models.retrieval import GCN, GraphSAGE  # noqa: E402

N, PER_NODE, B, FANOUTS, D, C = 1 << 20, 16, 1024, (25, 10), 256, 47


def stats(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"median_ms": round(med, 4), "min_ms": round(ms[0], 4), "spread": round((ms[-1] - ms[0]) / med, 4), "rounds": len(ms)}


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def measure(variants, rounds, iters):
    """every variant warmed up, windows of >= ~50 ms, the variants alternating inside every round"""
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


def torch_sampling(row_ptr, col, feats, seeds, fanouts, gen):
    """the chain in torch, innermost layer first; returns the outermost layer's mean-aggregated input rows"""
    dst = seeds
    layers = []
    for f in reversed(fanouts):
        lo = row_ptr[dst]
        deg = row_ptr[dst + 1] - lo
        pick = (torch.rand((dst.numel(), f), device=dst.device, generator=gen) * deg[:, None]).long()
        nbr = torch.where(deg[:, None] > 0, col[(lo[:, None] + pick).clamp_(max=col.numel() - 1)].long(), torch.full_like(pick, -1))
        ids = torch.unique(torch.cat((dst, nbr.reshape(-1))))
        ids = ids[ids >= 0]
        layers.append((torch.searchsorted(ids, nbr.clamp(min=0)), nbr >= 0))
        dst = ids
    local, ok = layers[-1]
    h = feats[dst]
    return (h[local] * ok[..., None]).sum(1) / ok.sum(1).clamp(min=1)[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--variants", default="sample_chain,train_step,torch_sampling,gcn_full_step")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    want = a.variants.split(",")
    g = bench_gcn.power_law_graph(N, PER_NODE)
    adj = L.SparseAdjacency(g)
    gen = torch.Generator(device="cuda").manual_seed(0)
    feats = torch.randn(N, D, device="cuda", generator=gen)
    labels = torch.nn.functional.one_hot(torch.randint(0, C, (N,), device="cuda", generator=gen), C).float()
    state = {"step": 0}

    def next_seeds():
        state["step"] += 1
        return torch.randint(0, N, (B,), device="cuda", generator=gen), state["step"]

    torch.manual_seed(0)
    sage = GraphSAGE([256, 256], list(FANOUTS), num_classes=C)
    sage(feats, adj, next_seeds()[0], 0)
    sage_opt = optim.Adam(sage.parameters(), lr=0.01)

    def sample_chain():
        seeds, s = next_seeds()
        return L.sample_blocks(adj, seeds, FANOUTS, s)

    def train_step():
        seeds, s = next_seeds()
        sage_opt.zero_grad(set_to_none=True)
        losses.categorical_crossentropy(labels[seeds], sage(feats, adj, seeds, s)).backward()
        sage_opt.step()

    col64 = adj.col

    def torch_chain():
        return torch_sampling(adj.row_ptr, col64, feats, next_seeds()[0], FANOUTS, gen)

    variants = {"sample_chain": sample_chain, "train_step": train_step, "torch_sampling": torch_chain}
    if "gcn_full_step" in want:
        feats128 = torch.randn(N, 128, device="cuda", generator=gen)
        torch.manual_seed(0)
        gcn = bench_gcn.Stack([GCN(256), GCN(256), GCN(C, activation="softmax")])
        gcn(adj, feats128)
        variants["gcn_full_step"] = bench_gcn.train_step_fn(gcn, adj, feats128, labels, None, optim.Adam(gcn.parameters(), lr=0.01))
    variants = {k: v for k, v in variants.items() if k in want}
    res, reps = measure(variants, a.rounds, a.iters)
    blocks = L.sample_blocks(adj, next_seeds()[0], FANOUTS, 1)
    out = {"bench": "sage", "nodes": N, "nnz": adj.nnz, "max_row": int(np.diff(g.indptr).max()), "seeds": B, "fanouts": list(FANOUTS),
           "D": D, "rounds": a.rounds, "iters_per_window": reps,
           "blocks_of_one_call": [{"n_dst": b.n_dst, "n_src": b.n_src, "nnz": b.adj.nnz} for b in blocks], **res}
    line = json.dumps(out)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
