"""Float64 references and NumPy restatements for skip-gram with negative sampling (csrc/sgns.hip) and the samplers around it
(csrc/sampling.hip).  No GPU and no package kernel is used here: tests/test_sgns_cpu.py checks this file against autograd, a compiled
dr_mix32 and plain Python loops; tests/test_gpu_sgns.py checks the kernels against it."""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24


# ---- SGNS ------------------------------------------------------------------------------------------------------------------------------
def masks(centers, contexts, negatives, skip_equal):
    """keep [B, 1 + K] bool: the slots that are not skipped"""
    ids = torch.cat([contexts[:, None], negatives], dim=1)
    ex_ok = (centers >= 0) & (contexts >= 0)
    keep = ex_ok[:, None] & (ids >= 0)
    if skip_equal:
        eq = ids == contexts[:, None]
        eq[:, 0] = False
        keep = keep & ~eq
    return ids, keep


def gather(in_table, out_table, centers, ids, keep):
    """u [B, D], v [B, 1 + K, D] in float64; masked ids (any int64) address row 0 and are multiplied by nothing that counts"""
    c = torch.where(keep[:, 0], centers, torch.zeros_like(centers))                            # slot 0 is kept iff the example is
    safe = torch.where(keep, ids, torch.zeros_like(ids))
    return in_table.double()[c], out_table.double()[safe]


def loss_expr(in_table, out_table, centers, contexts, negatives, sample_weight=None, skip_equal=True):
    """(loss_rows [B], scores [B, 1 + K], keep) as literal torch indexing in float64; differentiable in the two tables"""
    ids, keep = masks(centers, contexts, negatives, skip_equal)
    u, v = gather(in_table, out_table, centers, ids, keep)
    s = (u[:, None, :] * v).sum(-1)
    sign = torch.ones(ids.shape[1], dtype=torch.float64)
    sign[0] = -1.0
    terms = F.softplus(sign[None, :] * s) * keep.double()
    w = torch.ones(len(centers), dtype=torch.float64) if sample_weight is None else sample_weight.double()
    return w * terms.sum(1), s * keep.double(), keep


def hand_grads(in_table, out_table, centers, contexts, negatives, d_loss, sample_weight=None, skip_equal=True):
    """the closed form the kernels implement, in float64: coeff g [B, 1 + K], d_center [B, D], d_ctx [B, 1 + K, D], and the per-element
    sums of |terms| the error bounds are made of (abs_center [B, D], abs_ctx [B, 1 + K, D])"""
    ids, keep = masks(centers, contexts, negatives, skip_equal)
    u, v = gather(in_table, out_table, centers, ids, keep)
    s = (u[:, None, :] * v).sum(-1)
    z = torch.zeros(ids.shape[1], dtype=torch.float64)
    z[0] = 1.0
    w = torch.ones(len(centers), dtype=torch.float64) if sample_weight is None else sample_weight.double()
    g = w[:, None] * (torch.sigmoid(s) - z[None, :]) * keep.double()
    c = d_loss.double()[:, None] * g
    d_ctx = c[:, :, None] * u[:, None, :]
    d_center = (c[:, :, None] * v).sum(1)
    return g, d_center, d_ctx, (c[:, :, None] * v).abs().sum(1), d_ctx.abs()


def table_grads(num_in, num_out, centers, ids, keep, d_center, d_ctx):
    """float64 index_add_ of the gradient rows into [num_in, D] and [num_out, D]"""
    D = d_center.shape[1]
    g_in = torch.zeros((num_in, D), dtype=torch.float64)
    g_out = torch.zeros((num_out, D), dtype=torch.float64)
    ok = (centers >= 0)
    g_in.index_add_(0, centers[ok], d_center[ok])
    flat_ids, flat_rows = ids.reshape(-1), d_ctx.reshape(-1, D)
    okf = (ids >= 0).reshape(-1)
    g_out.index_add_(0, flat_ids[okf], flat_rows[okf])
    return g_in, g_out


# ---- dr_mix32 and the samplers ---------------------------------------------------------------------------------------------------------
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def mix32(seed, idx):
    """dr_mix32(seed, idx) of csrc/dr_common.h on uint64 arrays (wrap-around arithmetic), uint32 out"""
    with np.errstate(over="ignore"):
        seed = np.asarray(seed).astype(np.uint64)
        z = np.asarray(idx).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + seed
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)


def alias_sample_ref(prob, alias, n, seed, offset=0):
    prob, alias = np.asarray(prob, dtype=np.float32), np.asarray(alias, dtype=np.int32)
    V = np.uint64(prob.size)
    e = np.uint64(offset) + np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h1 = mix32(np.uint64(seed), np.uint64(2) * e).astype(np.uint64)
        h2 = mix32(np.uint64(seed), np.uint64(2) * e + np.uint64(1))
    slot = ((h1 * V) >> np.uint64(32)).astype(np.int64)
    r = (h2 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.where(r < prob[slot], slot, alias[slot].astype(np.int64))


def alias_distribution(prob, alias):
    """the distribution a table implies, float64"""
    prob = np.asarray(prob, dtype=np.float64)
    V = prob.size
    p = prob / V
    np.add.at(p, np.asarray(alias, dtype=np.int64), (1.0 - prob) / V)
    return p


def random_walk_ref(row_ptr, col, n_rows, starts, L, seed):
    row_ptr, col, starts = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(starts, dtype=np.int64)
    W = starts.size
    walks = np.full((W, L), -1, dtype=np.int64)
    walks[:, 0] = starts
    w = np.arange(W, dtype=np.uint64)
    for t in range(1, L):
        v = walks[:, t - 1]
        ok = (v >= 0) & (v < n_rows)
        vs = np.where(ok, v, 0)
        lo, deg = row_ptr[vs], row_ptr[vs + 1] - row_ptr[vs]
        ok &= deg > 0
        h = mix32(np.uint64(seed), w * np.uint64(L) + np.uint64(t)).astype(np.uint64)
        pick = ((h * np.where(ok, deg, 0).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        nxt = col[np.where(ok, lo + pick, 0)] if col.size else np.zeros(W, dtype=np.int64)
        walks[:, t] = np.where(ok, nxt, -1)
    return walks


def six_node_graph():
    """CSR (row_ptr, col) of an undirected 6-node graph: a triangle 0-1-2, a path 2-3-4, node 5 isolated (only a walk that starts there
    meets it)"""
    edges = [(0, 1), (1, 2), (0, 2), (2, 3), (3, 4)]
    nbrs = [[] for _ in range(6)]
    for a, b in edges:
        nbrs[a].append(b)
        nbrs[b].append(a)
    row_ptr = np.zeros(7, dtype=np.int64)
    col = []
    for i, n in enumerate(nbrs):
        col += sorted(n)
        row_ptr[i + 1] = len(col)
    return row_ptr, np.asarray(col, dtype=np.int32)


def dead_end_graph():
    """directed: 0 -> 1 -> 2 (isolated sink), 3 -> 0: every walk runs into node 2 and continues as -1"""
    row_ptr = np.asarray([0, 1, 2, 2, 3], dtype=np.int64)
    col = np.asarray([1, 2, 0], dtype=np.int32)
    return row_ptr, col


def skipgram_pairs_loops(seqs, window):
    """the double Python loop layers.skipgram_pairs must equal: lists of centers and contexts"""
    centers, contexts = [], []
    offs = [o for o in range(-window, window + 1) if o != 0]
    for row in seqs:
        L = len(row)
        for t in range(L):
            for o in offs:
                p = t + o
                if 0 <= p < L and row[t] >= 0 and row[p] >= 0:
                    centers.append(int(row[t]))
                    contexts.append(int(row[p]))
                else:
                    centers.append(-1)
                    contexts.append(-1)
    return centers, contexts
