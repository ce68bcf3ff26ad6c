"""Torch restatement of AFM's attention pooling and of the model's logit, written from the definition (Xiao et al., IJCAI 2017; the
reference ships no code for it).  Works in whatever dtype its inputs have (float64 is the tests' truth) and under autograd, and holds
the closed-form backward.  Used by the tests only; the package does not import it.

For one example with rows e_0 .. e_{F-1} [D] the pairs are numbered q = i (i - 1) / 2 + j for 0 <= j < i < F (DotInteraction's order
without the diagonal), P = F (F - 1) / 2, and

    p_q = e_i * e_j    z_q = p_q W + b    s_q = sum_a max(z_qa, 0) h_a    a = softmax over q of s    out = sum_q a_q p_q
    lse = log sum_q exp(s_q)

The module also draws the inputs of the GPU cases (CASES, case()), so that tests/test_afm_cpu.py can assert on the restatement alone
what tests/test_gpu_afm.py relies on: the relu mask z > 0 is beyond the reach of fp32 rounding."""
import functools

import numpy as np
import torch

U = 2.0 ** -24


def pairs(F):
    """(rows, cols) of the pairs in output order: for i ascending, j ascending within i, j < i"""
    ps = [(i, j) for i in range(F) for j in range(i)]
    return [p[0] for p in ps], [p[1] for p in ps]


def pair_products(e):
    """e [B, F, D] -> p [B, P, D]"""
    rows, cols = pairs(e.shape[1])
    return e[:, rows] * e[:, cols]


def forward(e, W, b, h):
    """dict of p [B, P, D], z [B, P, A], s [B, P], lse [B], attn [B, P], out [B, D]"""
    p = pair_products(e)
    z = p @ W + b
    s = torch.relu(z) @ h
    lse = torch.logsumexp(s, dim=1)
    attn = torch.exp(s - lse[:, None])
    out = (attn[:, :, None] * p).sum(1)
    return dict(p=p, z=z, s=s, lse=lse, attn=attn, out=out)


def backward(e, W, b, h, g):
    """(d_emb [B, F, D], dW [D, A], db [A], dh [A]) from g = d_out [B, D] by the closed form; no autograd.  The derivative of
    max(z, 0) at z == 0 is 0."""
    f = forward(e, W, b, h)
    p, z, a = f["p"], f["z"], f["attn"]
    ds = a * ((p * g[:, None, :]).sum(-1) - (f["out"] * g).sum(-1)[:, None])
    mask = (z > 0).to(z.dtype)
    dz = ds[:, :, None] * h * mask
    dh = (ds[:, :, None] * torch.relu(z)).sum((0, 1))
    db = dz.sum((0, 1))
    dW = torch.einsum("bqd,bqa->da", p, dz)
    dp = a[:, :, None] * g[:, None, :] + dz @ W.T
    rows, cols = pairs(e.shape[1])
    d_emb = torch.zeros_like(e)
    d_emb.index_add_(1, torch.tensor(rows), dp * e[:, cols])
    d_emb.index_add_(1, torch.tensor(cols), dp * e[:, rows])
    return d_emb, dW, db, dh


def afm_logits(e, linear, W, b, h, w_out):
    """e [B, F, D] the gathered embeddings, linear [B] the first-order term with its bias -> logits [B, 1] = linear + out w_out"""
    return linear.reshape(-1, 1) + forward(e, W, b, h)["out"] @ w_out


def eps_z(e, W, b):
    """[B, P, A]: a rigorous bound on the fp32 error of z in any order of summation, (D + 2) u (|p| |W| + |b|)"""
    return (e.shape[2] + 2) * U * (pair_products(e).abs() @ W.abs() + b.abs())


def mask_margin(e, W, b):
    """min |z| / (4 eps_z) over the elements with eps_z > 0: at 1 or more no fp32 evaluation of z can land on the other side of 0"""
    z = forward(e, W, b, torch.zeros(W.shape[1], dtype=e.dtype))["z"].abs()
    ez = eps_z(e, W, b)
    return (z / (4 * ez).clamp_min(1e-300)).min().item()


# (B, F, D, A), "normal" | "grid", seed.  The seeds of the random-normal cases were chosen so that mask_margin >= 1 (test_afm_cpu.py
# asserts it); a grid case has z exact in fp32.
CASES = [((3, 2, 4, 1), "normal", 0),        # P = 1, the smallest
         ((4, 3, 8, 4), "normal", 0),
         ((2, 6, 8, 16), "normal", 0),       # P = 15, below a 16-row tile
         ((2, 7, 8, 16), "normal", 0),       # P = 21, crossing a tile
         ((3, 9, 12, 8), "normal", 0),       # D not a multiple of 8
         ((2, 17, 16, 20), "normal", 0),     # A not a multiple of 16
         ((2, 64, 4, 16), "normal", 0),      # P = 2016, the largest F
         ((3, 26, 64, 32), "grid", 0),       # the workload's row
         ((2, 5, 256, 32), "grid", 0),       # the largest D and the largest A that goes with it
         ((2, 5, 64, 128), "grid", 0),       # the largest A and the largest D that goes with it
         ((70, 7, 20, 5), "grid", 0),        # more examples than a block holds, a remainder block, odd A
         ((8200, 3, 4, 2), "grid", 0)]       # more examples than the grid's waves: every wave walks several (forward from 8193 on)


def draw(shape, kind, seed):
    """(e [B, F, D], W [D, A], b [A], h [A], g [B, D]) as float64 tensors that hold float32 values"""
    B, F, D, A = shape
    rng = np.random.default_rng(7000 + 1000 * seed + 31 * F + 7 * D + A)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).double()                 # noqa: E731
    if kind == "grid":
        e = f32(rng.integers(-8, 9, size=(B, F, D)) / 4.0)
        W = f32(rng.integers(-8, 9, size=(D, A)) / 8.0)
        b = f32(rng.integers(-8, 9, size=(A,)) / 8.0)
        h = torch.from_numpy(rng.standard_normal(A))
        smax = forward(e, W, b, h)["s"].abs().max().item()
        h = f32((h * min(1.0, 3.99 / max(smax, 1e-30))).numpy())                               # max |s| <= 4: a well-conditioned softmax
    else:
        e = f32(rng.standard_normal((B, F, D)))
        W = f32(rng.standard_normal((D, A)) / np.sqrt(D))
        b = f32(0.1 * rng.standard_normal(A))
        h = f32(rng.standard_normal(A) / np.sqrt(A))
    g = f32(rng.standard_normal((B, D)))
    return e, W, b, h, g


@functools.lru_cache(maxsize=None)
def case(index):
    """inputs of CASES[index] with the float64 forward and backward; computed once, never modified"""
    shape, kind, seed = CASES[index]
    e, W, b, h, g = draw(shape, kind, seed)
    with torch.no_grad():
        f = forward(e, W, b, h)
        grads = backward(e, W, b, h, g)
    return dict(shape=shape, kind=kind, e=e, W=W, b=b, h=h, g=g, fwd=f, grads=grads)
