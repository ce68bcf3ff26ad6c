"""Torch restatement of DIN's Dice (keras/models/ranking/din.py:88-130 of the reference) and of the interest pooling in its literal
composed form -- the query expanded over the sequence, the [B * T, 3D] concat, two Dense layers, mask, weighted sum -- as the reference's
ActivationUnit would compute it pair by pair.  Works in whatever dtype its inputs have (float64 is the tests' truth, float32 on the
CPU their yardstick) and under autograd.  Conventions are the ones torch and TensorFlow share: relu'(0) = 0, `where` takes the else
branch at 0.  One rule is this project's: where a Dice row's standard deviation is 0 its gradient through the standard deviation is
taken as zero (TensorFlow: NaN).  Used by the tests only; the package does not import it."""
import torch


def dice_stats(x, eps):
    """(m, s, r) per row, [M, 1] each: the mean, the standard deviation (the reference's "var") and 1 / sqrt(s + eps).  No gradient
    flows through s where s == 0."""
    m = x.mean(dim=1, keepdim=True)
    var = ((x - m) ** 2).mean(dim=1, keepdim=True)
    pos = var > 0
    s = torch.where(pos, torch.sqrt(torch.where(pos, var, torch.ones_like(var))), torch.zeros_like(var))
    return m, s, 1.0 / torch.sqrt(s + eps)


def dice(x, alpha, eps=1e-8):
    """x [M, N], alpha [N] (Keras PReLU's parameter) -> [M, N]"""
    m, s, r = dice_stats(x, eps)
    p = torch.sigmoid((x - m) * r)
    pre = torch.relu(x) - alpha * torch.relu(-x)
    return torch.where(pre > 0, p * pre, (1 - p) * pre)


def dice_backward(x, alpha, dy, eps=1e-8):
    """(dx, dalpha) by the closed form the kernels implement (no autograd)"""
    n = x.shape[1]
    m, s, r = dice_stats(x, eps)
    p = torch.sigmoid((x - m) * r)
    pre = torch.relu(x) - alpha * torch.relu(-x)
    pos = pre > 0
    dpre = dy * torch.where(pos, p, 1 - p)
    c = dy * pre * torch.where(pos, torch.ones_like(p), -torch.ones_like(p)) * p * (1 - p)
    slope = torch.where(x > 0, torch.ones_like(x), torch.where(x < 0, alpha.expand_as(x), torch.zeros_like(x)))
    dx = dpre * slope + r * (c - c.mean(dim=1, keepdim=True))
    cx = (c * (x - m)).sum(dim=1, keepdim=True)
    safe = torch.where(s > 0, s, torch.ones_like(s))
    dx = dx - torch.where(s > 0, 0.5 * r ** 3 * cx * (x - m) / (n * safe), torch.zeros_like(x))
    dalpha = (dpre * torch.clamp(x, max=0)).sum(dim=0)
    return dx, dalpha


def activation(h, act, alpha=None, eps=1e-8):
    """the hidden layer's activation by its code: 0 linear, 1 relu, 2 sigmoid, 3 tanh, 4 Dice over the hidden units"""
    if act == 0:
        return h
    if act == 1:
        return torch.relu(h)
    if act == 2:
        return torch.sigmoid(h)
    if act == 3:
        return torch.tanh(h)
    if act == 4:
        return dice(h, alpha, eps)
    raise ValueError(act)


def _valid(mask, keys):
    B, T, _ = keys.shape
    return torch.ones((B, T), dtype=torch.bool) if mask is None else torch.as_tensor(mask).bool()


def pool(query, keys, mask, W, b, w_out, b_out, mode, act, alpha=None, eps=1e-8):
    """(out [B, D], scores [B, T]) in the composed form.  Masked keys are skipped: they are replaced before anything reads them."""
    B, T, D = keys.shape
    valid = _valid(mask, keys)
    kz = torch.where(valid[:, :, None], keys, torch.zeros_like(keys))
    q = query[:, None, :].expand(B, T, D).reshape(B * T, D)
    k = kz.reshape(B * T, D)
    parts = [q, k] + ([q - k] if mode == 1 else [q * k] if mode == 2 else [])
    h = torch.cat(parts, dim=1) @ W
    if b is not None:
        h = h + b
    s = activation(h, act, alpha, eps) @ w_out.reshape(-1, 1)
    if b_out is not None:
        s = s + b_out
    scores = torch.where(valid, s.reshape(B, T), torch.zeros((B, T), dtype=keys.dtype))
    return (scores[:, :, None] * kz).sum(dim=1), scores


def pool_folded(query, keys, mask, W, b, w_out, b_out, mode, act, alpha=None, eps=1e-8):
    """the same function in the form the kernel uses: the query's share of the hidden layer once per example, the keys against a
    per-example effective weight"""
    B, T, D = keys.shape
    valid = _valid(mask, keys)
    kz = torch.where(valid[:, :, None], keys, torch.zeros_like(keys))
    W0, W1 = W[:D], W[D:2 * D]
    hq = query @ W0
    if mode == 1:
        hq = hq + query @ W[2 * D:]
        weff = (W1 - W[2 * D:])[None].expand(B, D, W.shape[1])
    elif mode == 2:
        weff = W1[None] + query[:, :, None] * W[2 * D:][None]
    else:
        weff = W1[None].expand(B, D, W.shape[1])
    if b is not None:
        hq = hq + b
    h = torch.bmm(kz, weff) + hq[:, None, :]
    s = activation(h.reshape(B * T, -1), act, alpha, eps) @ w_out.reshape(-1, 1)
    if b_out is not None:
        s = s + b_out
    scores = torch.where(valid, s.reshape(B, T), torch.zeros((B, T), dtype=keys.dtype))
    return (scores[:, :, None] * kz).sum(dim=1), scores
