"""Float64 restatement of YoutubeNet's training arithmetic (include/dr_hotpath.h, "Sampled softmax"): tf.nn.sampled_softmax_loss with
num_true = 1 and no bias, written out -- the loss, hand-written gradients, the log-uniform sampler's probabilities and one SGD step of
the class table by index_add_.  Plain torch on the CPU; shared by tests/test_youtubenet_cpu.py and tests/test_gpu_youtubenet.py."""
import math

import torch

DD = torch.float64
FLT_MAX = 3.4028234663852886e38


def keep_mask(labels, sampled, remove_accidental_hits):
    """bool [B, S]: sampled_j >= 0 and not (remove_accidental_hits and sampled_j == labels_i)"""
    keep = (sampled >= 0)[None, :].expand(labels.shape[0], -1).clone()
    if remove_accidental_hits:
        keep &= sampled[None, :] != labels[:, None]
    return keep


def rows(u, table, labels, sampled):
    """(u with the padding rows zeroed, table[labels] with zeros for padding, table[sampled] with zeros for an id < 0)"""
    valid = labels >= 0
    u0 = torch.where(valid[:, None], u, torch.zeros_like(u))
    tl = torch.where(valid[:, None], table[labels.clamp(min=0)], torch.zeros_like(u))
    ts = table[sampled.clamp(min=0)]
    ts = torch.where((sampled >= 0)[:, None], ts, torch.zeros_like(ts))
    return u0, tl, ts


def _vec(v, n, fill, like):
    return torch.full((n,), fill, dtype=like.dtype) if v is None else v.to(like.dtype)


def logits(u, table, labels, sampled, log_q_true=None, log_q_sampled=None, remove_accidental_hits=True):
    """(t [B], s [B, S] with -inf at left-out entries, keep [B, S]); a padding row has u = 0 and t = 0"""
    u0, tl, ts = rows(u, table, labels, sampled)
    B, S = labels.shape[0], sampled.shape[0]
    valid = labels >= 0
    t = (u0 * tl).sum(-1) - torch.where(valid, _vec(log_q_true, B, 0.0, u0), torch.zeros(B, dtype=u0.dtype))
    s = u0 @ ts.T - _vec(log_q_sampled, S, 0.0, u0)[None, :]
    keep = keep_mask(labels, sampled, remove_accidental_hits)
    return t, s.masked_fill(~keep, -math.inf), keep


def forward(u, table, labels, sampled, log_q_true=None, log_q_sampled=None, sample_weight=None, remove_accidental_hits=True):
    """dict(t, s, keep, lse, loss): lse_i = log(exp(t_i) + sum_kept exp(s_ij)), loss_i = w_i (lse_i - t_i); lse = loss = 0 on padding"""
    t, s, keep = logits(u, table, labels, sampled, log_q_true, log_q_sampled, remove_accidental_hits)
    valid = labels >= 0
    w = _vec(sample_weight, labels.shape[0], 1.0, t)
    lse = torch.logsumexp(torch.cat([t[:, None], s], dim=1), dim=1)
    zero = torch.zeros_like(t)
    return dict(t=t, s=s, keep=keep, lse=torch.where(valid, lse, zero), loss=torch.where(valid, w * (lse - t), zero))


def hand_grads(u, table, labels, sampled, log_q_true=None, log_q_sampled=None, sample_weight=None, remove_accidental_hits=True,
               row_scale=1.0):
    """the gradients of row_scale * sum_i loss_i written out: dict(g [B], G [B, S], d_u, d_true [B, D], d_sampled [S, D]) and the sums
    of absolute terms abs_u, abs_sampled the rounding bounds are evaluated on"""
    f = forward(u, table, labels, sampled, log_q_true, log_q_sampled, sample_weight, remove_accidental_hits)
    u0, tl, ts = rows(u, table, labels, sampled)
    valid = labels >= 0
    w = _vec(sample_weight, labels.shape[0], 1.0, u0)
    c = torch.where(valid, row_scale * w, torch.zeros_like(w))
    g = c * (torch.exp(f["t"] - f["lse"]) - 1.0)
    G = c[:, None] * torch.exp(f["s"] - f["lse"][:, None])                 # exp(-inf) = 0 where left out
    G = torch.where(valid[:, None], G, torch.zeros_like(G))
    g = torch.where(valid, g, torch.zeros_like(g))
    out = dict(f)
    out.update(c=c, g=g, G=G, d_u=g[:, None] * tl + G @ ts, d_true=g[:, None] * u0, d_sampled=G.T @ u0,
               abs_u=g.abs()[:, None] * tl.abs() + G.abs() @ ts.abs(), abs_sampled=G.abs().T @ u0.abs())
    return out


def dense_loss(u, table, labels, sampled, log_q_true=None, log_q_sampled=None, sample_weight=None, remove_accidental_hits=True):
    """the same loss as a dense [B, 1 + S] logits formulation for torch autograd: gather, matmul, -inf at left-out entries, logsumexp.
    Valid rows only (labels >= 0, finite u)."""
    B, S = labels.shape[0], sampled.shape[0]
    t = (u * table[labels]).sum(-1) - _vec(log_q_true, B, 0.0, u)
    s = u @ table[sampled.clamp(min=0)].T - _vec(log_q_sampled, S, 0.0, u)[None, :]
    s = s.masked_fill(~keep_mask(labels, sampled, remove_accidental_hits), -math.inf)
    lg = torch.cat([t[:, None], s], dim=1)
    return _vec(sample_weight, B, 1.0, u) * (torch.logsumexp(lg, dim=1) - lg[:, 0])


def log_uniform(V):
    """float64 [V]: p(c) = log((c + 2) / (c + 1)) / log(V + 1), TensorFlow's log_uniform_candidate_sampler"""
    c = torch.arange(V, dtype=DD)
    return torch.log((c + 2.0) / (c + 1.0)) / math.log(V + 1.0)


def sgd_step(table, labels, sampled, d_true, d_sampled, lr):
    """table - lr * (scatter of d_true by labels + scatter of d_sampled by sampled), ids < 0 skipped; both buffers refer to the table
    before the step"""
    out = table.clone()
    vl, vs = labels >= 0, sampled >= 0
    out.index_add_(0, labels[vl], -lr * d_true[vl])
    out.index_add_(0, sampled[vs], -lr * d_sampled[vs])
    return out
