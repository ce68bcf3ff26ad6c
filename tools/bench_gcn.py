"""Training-step and SpMM kernel times of the GCN layer (keras/models/retrieval/gcn.py on dr_csr_spmm).

  python tools/bench_gcn.py [--steps 20] [--warmup 5] [--configs cora,scaled]

Prints one JSON line.  Device events in one process, after warm-up.
  cora    the example's model (GCN(32) -> GCN(7, softmax), Adam(0.01)) on the synthetic Cora-shaped graph: 2708 nodes, so this
          measures launch overhead, not the kernels
  scaled  a seeded power-law graph, N = 2^20 nodes, 16 edges per node before symmetrisation, self loops, D^-1/2 (A+I) D^-1/2;
          features D_in = 128; GCN(256) -> GCN(256) -> GCN(47, softmax).  Reports ms per training step (forward, backward, Adam),
          each SpMM's kernel time (forward on A, backward on the device-built A^T), its bytes over time against the lower bound
          8 nnz + 8 N D and the no-reuse bound 8 nnz + 4 nnz D + 4 N D, the lower bound's fraction of 8 TB/s, and torch.sparse.mm on
          the same CSR as the baseline."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import layers as L  # noqa: E402
from deep_recommenders_amd import losses, optim  # noqa: E402
from deep_recommenders_amd.datasets import Cora, synthetic_cora  # noqa: E402
from deep_recommenders_amd.keras.models.retrieval import GCN  # noqa: E402

PEAK = 8.0e12


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def power_law_graph(N, per_node, seed=0):
    r = np.random.RandomState(seed)
    E = N * per_node
    src = np.repeat(np.arange(N, dtype=np.int64), per_node)
    dst = np.minimum((N * r.random_sample(E) ** 3).astype(np.int64), N - 1)   # in-degree of rank i ~ i^(-2/3): a few large hubs
    perm = r.permutation(N)
    dst = perm[dst]
    a = sp.coo_matrix((np.ones(E, dtype=np.float32), (src, dst)), shape=(N, N)).tocsr()
    a = a + a.T
    a.data[:] = 1.0
    return Cora.spectral_graph(a).astype(np.float32)


def train_step_fn(model, adj, feats, labels, mask, opt):
    def step():
        opt.zero_grad(set_to_none=True)
        loss = losses.categorical_crossentropy(labels, model(adj, feats), sample_weight=mask)
        loss.backward()
        opt.step()
    return step


class Stack(torch.nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.layers = torch.nn.ModuleList(layers)

    def forward(self, adj, x):
        for g in self.layers:
            x = g(x, adj)
        return x


def bench_cora(steps, warmup):
    with tempfile.TemporaryDirectory() as tmp:
        cora = Cora(synthetic_cora(tmp, seed=0))
        ids, features, labels = cora.load_content()
        g = cora.spectral_graph(cora.build_graph(ids))
        np.random.seed(0)
        (yt, mt), _, _ = cora.split_labels(labels)
    adj = L.SparseAdjacency(g)
    feats = torch.from_numpy(features.toarray().astype(np.float32)).cuda()
    torch.manual_seed(0)
    model = Stack([GCN(32), GCN(cora.num_classes, activation="softmax")])
    model(adj, feats)
    opt = optim.Adam(model.parameters(), lr=0.01)
    ms = timed(train_step_fn(model, adj, feats, torch.from_numpy(yt.astype(np.float32)).cuda(), mt, opt), steps, warmup)
    return {"nodes": g.shape[0], "nnz": int(g.nnz), "ms_per_step": round(ms, 4),
            "note": "2708 nodes: the step is launch-bound; this measures launch overhead, not the SpMM"}


def bench_scaled(steps, warmup):
    N, per_node, D_in, C = 1 << 20, 16, 128, 47
    g = power_law_graph(N, per_node)
    deg = np.diff(g.indptr)
    adj = L.SparseAdjacency(g)
    nnz = adj.nnz
    gen = torch.Generator(device="cuda").manual_seed(0)
    feats = torch.randn(N, D_in, device="cuda", generator=gen)
    labels = torch.nn.functional.one_hot(torch.randint(0, C, (N,), device="cuda", generator=gen), C).float()
    torch.manual_seed(0)
    model = Stack([GCN(256), GCN(256), GCN(C, activation="softmax")])
    model(adj, feats)
    opt = optim.Adam(model.parameters(), lr=0.01)
    out = {"nodes": N, "nnz": nnz, "max_row": int(deg.max()), "rows_over_long_threshold": None}
    plan = adj.plan().cpu()
    out["rows_over_long_threshold"] = int(plan[0])
    out["ms_per_step"] = round(timed(train_step_fn(model, adj, feats, labels, None, opt), steps, warmup), 3)
    adjT = adj.transpose()
    spmm = {}
    for name, a, D in (("fwd_D128", adj, 128), ("fwd_D256", adj, 256), ("bwd_D256", adjT, 256)):
        X = torch.randn(N, D, device="cuda", generator=gen)
        o = torch.empty(N, D, device="cuda")
        ms = timed(lambda: a.spmm(X, out=o), steps, warmup)
        lo = 8 * nnz + 8 * N * D
        hi = 8 * nnz + 4 * nnz * D + 4 * N * D
        spmm[name] = {"ms": round(ms, 4), "GBps_lower_bound_bytes": round(lo / ms / 1e6, 1),
                      "GBps_no_reuse_bytes": round(hi / ms / 1e6, 1), "frac_of_8TBps_lower": round(lo / ms / 1e-3 / PEAK, 4)}
    out["spmm"] = spmm
    base = {}
    try:
        At = torch.sparse_csr_tensor(torch.from_numpy(g.indptr.astype(np.int64)), torch.from_numpy(g.indices.astype(np.int64)),
                                     torch.from_numpy(g.data.astype(np.float32)), size=(N, N)).cuda()
        for D in (128, 256):
            X = torch.randn(N, D, device="cuda", generator=gen)
            ref = torch.sparse.mm(At, X)
            err = (ref - adj.spmm(X)).abs().max().item()
            base["torch_sparse_mm_D%d" % D] = {"ms": round(timed(lambda: torch.sparse.mm(At, X), steps, warmup), 4),
                                               "max_abs_diff": err}
    except Exception as e:                                      # noqa: BLE001
        base = {"torch_sparse_mm": "did not run on the device: %s" % str(e).splitlines()[0][:160]}
    out["baseline"] = base
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="cora,scaled")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"bench": "gcn", "steps": a.steps, "warmup": a.warmup}
    for c in a.configs.split(","):
        res[c] = {"cora": bench_cora, "scaled": bench_scaled}[c](a.steps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
