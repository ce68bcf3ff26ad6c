"""IntentGC's vector-wise convolution over a typed block, two ways in ONE process per cell, alternating, with the copy ceiling
(dr_copy_nt) measured in the same call:

  (a) composed  what the package had before: adj.spmm (dr_csr_spmm) for the R aggregates, then the filters as a user of torch would
                write them on the device -- cat to [n, R + 1, D], einsum with W, relu, einsum with theta, relu -- with autograd for the
                backward (layers.aggregate's transposed spmm for the scatter)
  (b) fused     dr_intent_conv_fwd (forward), IntentConv.call(training=True) + backward (dr_intent_conv_bwd + one transposed spmm)

and a whole IntentGC.train_step on a synthetic graph with the model's own IntentConv layers against the same model with every layer
replaced by the composition.

  python tools/bench_intentgc.py [--rounds 7] [--iters 5 (the least per window; raised to fill ~50 ms)] [--cells n65536_r3_f10_d128_l4,...]
                                 [--limit 300 (seconds per cell)] [--log profiles/intentgc_bench.log]

Cells: n_dst 65 536, R 3, fanout 10, D 128, L 4;  n_dst 8 192, R 2, fanout 25, D 64, L 8.  The block has 4 n_dst source rows, every
virtual row `fanout` uniform neighbours.  Every cell runs in a fresh child process under its own time limit, and the first failing cell
stops the run.  Device events; every variant is warmed up; the implementations alternate inside every round; median, min and the spread
(max - min) / median are printed with every figure, and the peak of torch's allocator over one call of each variant.  Bytes are the
algorithm's, with N = 4 n_dst D (one [n_dst, D] matrix): the fused forward reads (1 + R fanout) N of rows and writes N; forward +
backward adds the R N aggregates written and read, d_out, d_self and d_agg (R N) written, and the scatter's read of d_agg (R fanout N
gathered) and write of the 4 N source gradient."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ffm import measure, peak_mb                                            # noqa: E402  (the shared measuring loop)

# cell -> (n_dst, R, fanout, D, L)
CELLS = {"n65536_r3_f10_d128_l4": (65536, 3, 10, 128, 4), "n8192_r2_f25_d64_l8": (8192, 2, 25, 64, 8)}
SRC_FACTOR = 4


def _composed_conv_class():
    import torch
    from torch import nn
    from deep_recommenders_amd import layers as L

    class ComposedConv(nn.Module):
        """IntentConv's interface on the kernels the package had before: spmm + torch element-wise ops, backward by autograd"""

        def __init__(self, kernel, theta):
            super().__init__()
            self.kernel, self.theta = nn.Parameter(kernel.detach().clone()), nn.Parameter(theta.detach().clone())
            self._kept = None

        def call(self, h, block, training=False, **kwargs):
            with torch.set_grad_enabled(bool(training)):
                leaf = h.detach().requires_grad_(bool(training))
                agg = L.aggregate(block.adj, leaf).view(block.n_dst, block.R, h.shape[1])
                a = torch.cat([leaf[:block.n_dst, None, :], agg], dim=1)
                p = torch.relu(torch.einsum("ir,nrd->nid", self.kernel, a))
                out = torch.relu(torch.einsum("i,nid->nd", self.theta, p))
            self._kept = (leaf, out) if training else None
            return out.detach()

        def backward(self, d_out, need_input_grad=True):
            leaf, out = self._kept
            self._kept = None
            out.backward(d_out)
            return leaf.grad

    return ComposedConv


def bench_cell(name, rounds, iters):
    import torch
    from torch import nn
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd import ops
    from deep_recommenders_amd.keras.models.retrieval import IntentConv, IntentGC
    if not torch.cuda.is_available():
        raise SystemExit("bench_intentgc needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    n_dst, R, fanout, D, Lf = CELLS[name]
    n_src = SRC_FACTOR * n_dst
    gen = torch.Generator(device="cuda").manual_seed(1)
    nnz = n_dst * R * fanout
    row_ptr = torch.arange(n_dst * R + 1, device="cuda", dtype=torch.int64) * fanout
    col = torch.randint(0, n_src, (nnz,), device="cuda", generator=gen).to(torch.int32)
    val = torch.full((nnz,), 1.0 / fanout, device="cuda")
    adj = L.SparseAdjacency._from_device(row_ptr, col, val, (n_dst * R, n_src))
    block = L.TypedBlock(adj, torch.arange(n_src, device="cuda"), n_dst, R)
    adj.transpose()                                                                          # built once per block, outside the windows
    h = torch.randn((n_src, D), device="cuda", generator=gen)
    d_out = torch.randn((n_dst, D), device="cuda", generator=gen)
    conv = IntentConv(Lf)
    conv.build(R, "cuda")
    composed = _composed_conv_class()(conv.kernel, conv.theta)

    def composed_fwd():
        return composed.call(h, block)

    def fused_fwd():
        return conv.call(h, block)

    def composed_fwd_bwd():
        composed.call(h, block, training=True)
        return composed.backward(d_out)

    def fused_fwd_bwd():
        conv.call(h, block, training=True)
        return conv.backward(d_out)

    N = 4.0 * n_dst * D
    bytes_f = (1 + R * fanout) * N + N
    bytes_fb = bytes_f + R * N + (1 + R) * N + N + N + R * N + R * fanout * N + SRC_FACTOR * N
    src = torch.empty(int(bytes_f // 8), device="cuda")
    dst = torch.empty_like(src)

    def copy():
        return ops.copy_nt(src, dst)

    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())                          # noqa: E731
    want, want_d = composed_fwd(), composed_fwd_bwd().clone()
    want_gw = composed.kernel.grad.clone()
    got, got_d = fused_fwd(), fused_fwd_bwd()
    diffs = {"out": rel(got, want), "d_h": rel(got_d, want_d), "d_W": rel(conv.kernel.grad, want_gw)}
    composed.kernel.grad = composed.theta.grad = None
    del want, want_d, got, got_d
    peaks = {n: peak_mb(f) for n, f in (("composed_fwd", composed_fwd), ("fused_fwd", fused_fwd), ("composed_fwd_bwd", composed_fwd_bwd),
                                        ("fused_fwd_bwd", fused_fwd_bwd))}

    # a whole train step: R uniform relations of degree 2 fanout over 8 n_dst nodes per side, the batch sized so that the input-side
    # block of the user net has in the order of n_dst / 2 destinations
    B = max(256, n_dst // (1 + R * fanout // 2) // 2)
    nodes = 8 * n_dst
    fan = (fanout, max(1, fanout // 2))

    def relations():
        out = []
        for _ in range(R):
            deg = 2 * fanout
            rp = torch.arange(nodes + 1, device="cuda", dtype=torch.int64) * deg
            c = torch.randint(0, nodes, (nodes * deg,), device="cuda", generator=gen).view(nodes, deg).sort(dim=1).values
            out.append(L.SparseAdjacency._from_device(rp, c.reshape(-1).to(torch.int32), torch.ones(nodes * deg, device="cuda"), (nodes, nodes)))
        return out

    feats = torch.randn((nodes, 64), device="cuda", generator=gen)
    rel_u, rel_i = relations(), relations()

    def model():
        return IntentGC(rel_u, rel_i, feats, feats, embedding_dim=D, num_layers=2, num_filters=Lf, fanouts=fan, dnn_units_size=(D, 64), seed=0)

    fused_model, composed_model = model(), model()
    Composed = _composed_conv_class()
    for net in (composed_model.user_net, composed_model.item_net):
        net.convs = nn.ModuleList([Composed(c.kernel, c.theta) for c in net.convs])
    users = torch.randint(0, nodes, (B,), device="cuda", generator=gen)
    pos = torch.randint(0, nodes, (B,), device="cuda", generator=gen)
    neg = torch.randint(0, nodes, (B // 4,), device="cuda", generator=gen)
    opts = {id(m): torch.optim.SGD(m.parameters(), lr=1e-3) for m in (fused_model, composed_model)}

    def fused_step():
        return fused_model.train_step(users, pos, neg, optimizer=opts[id(fused_model)], seed=3)

    def composed_step():
        return composed_model.train_step(users, pos, neg, optimizer=opts[id(composed_model)], seed=3)

    diffs["first_step_loss"] = abs(fused_step().item() - composed_step().item())
    variants = {"composed_fwd": composed_fwd, "fused_fwd": fused_fwd, "composed_fwd_bwd": composed_fwd_bwd, "fused_fwd_bwd": fused_fwd_bwd,
                "composed_train_step": composed_step, "fused_train_step": fused_step, "copy_nt": copy}
    res, reps = measure(variants, rounds, iters)
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    wins = lambda a, b: bool(med(a) * (1 + res[a]["spread"]) < med(b) * (1 - res[b]["spread"]))   # noqa: E731
    ceiling = 2.0 * src.numel() * 4 / (med("copy_nt") * 1e-3)
    frac = lambda n, nbytes: round(nbytes / (med(n) * 1e-3) / ceiling, 4)                   # noqa: E731
    line = {"shape": {"n_dst": n_dst, "n_src": n_src, "R": R, "fanout": fanout, "D": D, "L": Lf, "nnz": nnz,
                      "step": {"B": B, "S": B // 4, "nodes_per_side": nodes, "fanouts": list(fan),
                               "outer_block_rows": [b[0].n_dst for b in fused_model.blocks]}},
            "iters_per_window": reps, "max_rel_diff": diffs, "peak_MB": peaks, **res,
            "copy_ceiling_GBps": round(ceiling / 1e9, 1),
            "fused_fwd_speedup_vs_composed": round(med("composed_fwd") / med("fused_fwd"), 3),
            "fused_fwd_wins": wins("fused_fwd", "composed_fwd"),
            "fused_fwd_bwd_speedup_vs_composed": round(med("composed_fwd_bwd") / med("fused_fwd_bwd"), 3),
            "fused_fwd_bwd_wins": wins("fused_fwd_bwd", "composed_fwd_bwd"),
            "fused_train_step_speedup_vs_composed": round(med("composed_train_step") / med("fused_train_step"), 3),
            "fused_train_step_wins": wins("fused_train_step", "composed_train_step"),
            "fused_fwd_frac_of_copy_ceiling": frac("fused_fwd", bytes_f),
            "fused_fwd_bwd_frac_of_copy_ceiling": frac("fused_fwd_bwd", bytes_fb)}
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
