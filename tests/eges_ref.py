"""Float64 references and NumPy restatements for skip-gram with side information (csrc/eges.hip), the weighted random walk
(csrc/sampling.hip) and graph_from_sessions.  No GPU and no package kernel is used here: tests/test_eges_cpu.py checks this file against
autograd and plain loops; tests/test_gpu_eges.py checks the kernels against it."""
import numpy as np
import torch
import torch.nn.functional as F

from sgns_ref import mix32

DD = torch.float64


# ---- masks -----------------------------------------------------------------------------------------------------------------------------
def presence(side_ids, contexts):
    """present [B, S] bool: the fields an example reads.  None of a skipped example (contexts[b, 0] < 0, or no field >= 0)."""
    contexts = contexts.reshape(len(side_ids), -1)
    return (side_ids >= 0) & (contexts[:, :1] >= 0)


def slot_masks(contexts, negatives, ex_ok, skip_equal):
    """ids [B, P + K] and keep [B, P + K] bool: the slots that are not skipped"""
    contexts = contexts.reshape(len(ex_ok), -1)
    P = contexts.shape[1]
    ids = torch.cat([contexts, negatives], dim=1)
    keep = ex_ok[:, None] & (ids >= 0)
    if skip_equal:
        eq = (negatives[:, :, None] == contexts[:, None, :]) & (contexts[:, None, :] >= 0)
        keep[:, P:] &= ~eq.any(-1)
    return ids, keep


def aggregate(side_table, row_base, side_ids, att, att_ids, present):
    """alpha [B, S], w [B, S, D], u [B, D] in float64 and use_att [B]; missing fields address row 0 and carry weight 0"""
    B, S = side_ids.shape
    rows = torch.where(present, side_ids + row_base[None, :], torch.zeros_like(side_ids))
    w = side_table.double()[rows]
    if att is None:
        use_att = torch.zeros(B, dtype=torch.bool)
        logits = torch.zeros((B, S), dtype=DD)
    else:
        use_att = (att_ids >= 0) & present.any(1)
        a = att.double()[torch.where(use_att, att_ids, torch.zeros_like(att_ids))][:, :S]
        logits = a * use_att.double()[:, None]
    masked = logits.masked_fill(~present, -float("inf"))
    safe = torch.where(present.any(1)[:, None], masked, torch.zeros_like(masked))               # a row of -inf has no softmax
    alpha = torch.softmax(safe, dim=1) * present.double()
    u = (alpha[:, :, None] * w).sum(1)
    return alpha, w, u, use_att


def loss_expr(side_table, row_base, side_ids, att, att_ids, out_table, contexts, negatives, sample_weight=None, skip_equal=True):
    """(loss_rows [B], scores [B, P + K], keep, alpha [B, S], u [B, D]) as literal torch indexing in float64; differentiable in
    side_table, att and out_table"""
    B = len(side_ids)
    contexts = contexts.reshape(B, -1)
    P = contexts.shape[1]
    present = presence(side_ids, contexts)
    alpha, _, u, _ = aggregate(side_table, row_base, side_ids, att, att_ids, present)
    ids, keep = slot_masks(contexts, negatives, present.any(1), skip_equal)
    v = out_table.double()[torch.where(keep, ids, torch.zeros_like(ids))]
    s = (u[:, None, :] * v).sum(-1)
    sign = torch.ones(ids.shape[1], dtype=DD)
    sign[:P] = -1.0
    terms = F.softplus(sign[None, :] * s) * keep.double()
    wgt = torch.ones(B, dtype=DD) if sample_weight is None else sample_weight.double()
    return wgt * terms.sum(1), s * keep.double(), keep, alpha, u


def hand_grads(side_table, row_base, side_ids, att, att_ids, out_table, contexts, negatives, d_loss, sample_weight=None, skip_equal=True):
    """the closed form the kernels implement, in float64, as a dict: coeff g [B, J], c = d_loss g, d_u [B, D], d_side [B, S, D],
    d_att [B, S], d_ctx [B, J, D], q [B, S], r [B], and what the error bounds are made of (alpha, w, u, v, present, keep, use_att,
    abs_du = sum_j |c_j v_j|)"""
    B = len(side_ids)
    contexts = contexts.reshape(B, -1)
    P = contexts.shape[1]
    present = presence(side_ids, contexts)
    alpha, w, u, use_att = aggregate(side_table, row_base, side_ids, att, att_ids, present)
    ids, keep = slot_masks(contexts, negatives, present.any(1), skip_equal)
    v = out_table.double()[torch.where(keep, ids, torch.zeros_like(ids))]
    s = (u[:, None, :] * v).sum(-1)
    z = torch.zeros(ids.shape[1], dtype=DD)
    z[:P] = 1.0
    wgt = torch.ones(B, dtype=DD) if sample_weight is None else sample_weight.double()
    g = wgt[:, None] * (torch.sigmoid(s) - z[None, :]) * keep.double()
    c = d_loss.double()[:, None] * g
    d_u = (c[:, :, None] * v).sum(1)
    d_ctx = c[:, :, None] * u[:, None, :]
    d_side = alpha[:, :, None] * d_u[:, None, :]
    q = (d_u[:, None, :] * w).sum(-1) * present.double()
    r = (alpha * q).sum(1)
    d_att = alpha * (q - r[:, None]) * use_att.double()[:, None]
    return dict(g=g, c=c, d_u=d_u, d_side=d_side, d_att=d_att, d_ctx=d_ctx, q=q, r=r, alpha=alpha, w=w, u=u, v=v, s=s * keep.double(),
                present=present, keep=keep, ids=ids, use_att=use_att, abs_du=(c[:, :, None] * v).abs().sum(1))


def table_grads(num_side, num_att, num_out, row_base, side_ids, att_ids, h):
    """float64 index_add_ of the gradient rows of hand_grads' dict h into [num_side, D], [num_att, S] and [num_out, D]"""
    B, S, D = h["d_side"].shape
    g_side = torch.zeros((num_side, D), dtype=DD)
    g_att = torch.zeros((num_att, S), dtype=DD)
    g_out = torch.zeros((num_out, D), dtype=DD)
    ok = h["present"].reshape(-1)
    g_side.index_add_(0, (side_ids + row_base[None, :]).reshape(-1)[ok], h["d_side"].reshape(-1, D)[ok])
    if att_ids is not None:
        g_att.index_add_(0, att_ids[h["use_att"]], h["d_att"][h["use_att"]])
    okj = h["keep"].reshape(-1)
    g_out.index_add_(0, h["ids"].reshape(-1)[okj], h["d_ctx"].reshape(-1, D)[okj])
    return g_side, g_att, g_out


# ---- the weighted walk -------------------------------------------------------------------------------------------------------------------
def weighted_pick(cum, lo, hi, t):
    """the search rule: the smallest e in [lo, hi) with cum[e] - base > t, base = cum[lo - 1] (0 at lo == 0); a plain scan"""
    base = int(cum[lo - 1]) if lo > 0 else 0
    for e in range(lo, hi):
        if int(cum[e]) - base > t:
            return e
    raise AssertionError("t = %d is not below the row's total" % t)


def random_walk_weighted_ref(row_ptr, col, cum, n_rows, starts, L, seed):
    row_ptr, col, cum = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(cum, dtype=np.int64)
    starts = np.asarray(starts, dtype=np.int64)
    W = starts.size
    walks = np.full((W, L), -1, dtype=np.int64)
    walks[:, 0] = starts
    w = np.arange(W, dtype=np.uint64)
    for t in range(1, L):
        h = mix32(np.uint64(seed), w * np.uint64(L) + np.uint64(t))
        for i in range(W):
            v = int(walks[i, t - 1])
            if v < 0 or v >= n_rows:
                continue
            lo, hi = int(row_ptr[v]), int(row_ptr[v + 1])
            if hi == lo:
                continue
            base = int(cum[lo - 1]) if lo > 0 else 0
            total = int(cum[hi - 1]) - base
            if total == 0:
                continue
            pick = (int(h[i]) * total) >> 32
            walks[i, t] = col[weighted_pick(cum, lo, hi, pick)]
    return walks


def weighted_six_node_graph():
    """directed CSR (row_ptr, col, weights): node 0 -> 1, 2, 3, 4 with weights (3, 0, 1, 5) -- a zero-weight edge in the middle --,
    1 -> 0 (2), 2 -> 0, 3 (0, 0): a row whose total is 0, 3 -> 4, 0 (0, 7): a zero-weight edge first, 4 -> 3 (1), node 5 isolated"""
    row_ptr = np.asarray([0, 4, 5, 7, 9, 10, 10], dtype=np.int64)
    col = np.asarray([1, 2, 3, 4, 0, 0, 3, 4, 0, 3], dtype=np.int32)
    weights = np.asarray([3, 0, 1, 5, 2, 0, 0, 0, 7, 1], dtype=np.int64)
    return row_ptr, col, weights


# ---- sessions ----------------------------------------------------------------------------------------------------------------------------
def graph_from_sessions_loops(sessions, num_items):
    """the co-occurrence counts as a dense [num_items, num_items] int64 matrix, by loops: counts[a, b] = times b follows a"""
    counts = np.zeros((num_items, num_items), dtype=np.int64)
    for s in sessions:
        for a, b in zip(list(s)[:-1], list(s)[1:]):
            counts[int(a), int(b)] += 1
    return counts
