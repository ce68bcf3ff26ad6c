"""Torch restatement of PNN's product layer and of the model's logit, written from the definition (Qu et al., ICDM 2016; the reference
ships no code for it).  Works in whatever dtype its inputs have (float64 is the tests' truth) and under autograd, and holds the
closed-form backward.  Used by the tests only; the package does not import it.

For one example with rows e_0 .. e_{F-1} [D]:  u = sum_i e_i,  out[n] = sum_{d,e} u_d u_e W[d D + e, n] (+ addend[n]) -- the outer
product u u^T flattened row-major times W [D * D, N], the full square.

The module also draws the inputs of the GPU cases (CASES, draw(), case()).  A "grid" case is exact in fp32 under the three conditions of
grid_conditions(): every product and every partial sum, in any order, is then representable, so the fp32 result must equal the float64
one bit for bit."""
import functools

import numpy as np
import torch

U = 2.0 ** -24


def forward(e, W, addend=None):
    """dict of u [B, D], outer [B, D * D], out [B, N] from e [B, F, D], W [D * D, N], addend [B, N] | None"""
    u = e.sum(1)
    outer = (u[:, :, None] * u[:, None, :]).reshape(u.shape[0], -1)
    out = outer @ W
    if addend is not None:
        out = out + addend
    return dict(u=u, outer=outer, out=out)


def backward(e, W, g):
    """(d_emb [B, F, D], dW [D * D, N]) from g = d_out [B, N] by the closed form; no autograd.  The addend's gradient is g itself."""
    B, F, D = e.shape
    u = e.sum(1)
    dW = torch.einsum("bd,be,bn->den", u, u, g).reshape(D * D, -1)
    S = torch.einsum("bn,den->bde", g, W.reshape(D, D, -1))
    du = torch.einsum("bde,be->bd", S + S.transpose(1, 2), u)
    return du[:, None, :].expand(B, F, D).contiguous(), dW


def inner(e, self_interaction=False):
    """[B, P]: <e_i, e_j> for i ascending, j ascending within i, j < i (j <= i with self_interaction): DotInteraction's order"""
    F = e.shape[1]
    ps = [(i, j) for i in range(F) for j in range(i + 1 if self_interaction else i)]
    return (e[:, [p[0] for p in ps]] * e[:, [p[1] for p in ps]]).sum(-1)


ACTS = {"relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh, None: lambda x: x, "linear": lambda x: x}


def pnn_logits(e, w_z, b1, w_inner, w_outer, kernels, biases, self_interaction=False, activation="relu"):
    """e [B, F, D] the gathered embeddings -> logits [B, 1].  l1 = act(z w_z + inner w_inner + outer w_outer + b1), a part being left
    out when its weight is None; then Dense(u, act) for all (kernel, bias) but the last, which is the Dense(1)."""
    act = ACTS[activation]
    pre = e.reshape(e.shape[0], -1) @ w_z + b1
    if w_inner is not None:
        pre = pre + inner(e, self_interaction) @ w_inner
    if w_outer is not None:
        pre = pre + forward(e, w_outer)["out"]
    h = act(pre)
    for i, (W, b) in enumerate(zip(kernels, biases)):
        h = h @ W + b
        if i + 1 < len(kernels):
            h = act(h)
    return h


def grid_conditions(shape):
    """the three conditions under which a grid case is exact in fp32: out (quarters up to F^2 D^2, plus the addend), dW (eighths up
    to B F^2) and du (quarters up to 2 N D F)"""
    B, F, D, N = shape
    return 4 * F * F * D * D + 8 <= 2 ** 24 and 8 * B * F * F <= 2 ** 24 and 8 * N * D * F <= 2 ** 24


# (B, F, D, N), "normal" | "grid"
CASES = [((3, 1, 4, 1), "normal"),          # the smallest
         ((4, 3, 8, 5), "normal"),          # odd N
         ((2, 2, 12, 16), "normal"),        # D^2 = 144, not a multiple of 32 (nor of the 128-column chunk of the du pass)
         ((2, 5, 20, 17), "normal"),        # N crosses a k-tile of 16
         ((2, 3, 16, 300), "normal"),       # three column tiles of 128
         ((40, 4, 32, 24), "normal"),
         ((3, 26, 64, 32), "grid"),         # the workload's row
         ((2, 2, 128, 8), "grid"),          # the largest D
         ((70, 7, 20, 5), "grid"),          # a remainder row tile (64-row blocks of the du pass)
         ((8200, 2, 4, 2), "grid"),         # dW over many row tiles: 33 parts of 256 examples; 129 forward tiles of 64 x 64
         ((130, 3, 8, 4), "grid"),          # crosses a 128-row tile, two parts of dW
         ((33000, 2, 4, 2), "grid"),        # more row tiles than CUs (258: the 128 x 128 forward tile); 52 parts of 640 examples
         ((2100, 2, 8, 2048), "grid")]      # the 128 x 128 forward tile at its full width: 17 x 16 tiles (256 or more take it)


def draw(shape, kind, seed=0):
    """(e [B, F, D], W [D * D, N], g [B, N], addend [B, N]) as float64 tensors that hold float32 values"""
    B, F, D, N = shape
    rng = np.random.default_rng(9000 + 1000 * seed + 31 * F + 7 * D + N)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).double()                 # noqa: E731
    if kind == "grid":
        e = f32(rng.integers(-2, 3, size=(B, F, D)) / 2.0)
        W = f32(rng.integers(-1, 2, size=(D * D, N)))
        g = f32(rng.integers(-2, 3, size=(B, N)) / 2.0)
        addend = f32(rng.integers(-8, 9, size=(B, N)) / 4.0)
    else:
        e = f32(rng.standard_normal((B, F, D)) / np.sqrt(F))
        W = f32(rng.standard_normal((D * D, N)) / D)
        g = f32(rng.standard_normal((B, N)))
        addend = f32(rng.standard_normal((B, N)))
    return e, W, g, addend


@functools.lru_cache(maxsize=None)
def case(index):
    """inputs of CASES[index] with the float64 forward and backward; computed once, never modified"""
    shape, kind = CASES[index]
    e, W, g, addend = draw(shape, kind, 0)
    with torch.no_grad():
        f = forward(e, W)
        grads = backward(e, W, g)
    return dict(shape=shape, kind=kind, e=e, W=W, g=g, addend=addend, fwd=f, grads=grads)


@functools.lru_cache(maxsize=None)
def errors32(index):
    """r32 of u, out, d_emb, dW: the error of the float32 run of the restatement, normalised by max |float64 truth|"""
    c = case(index)
    with torch.no_grad():
        f = forward(c["e"].float(), c["W"].float())
        d_emb, dW = backward(c["e"].float(), c["W"].float(), c["g"].float())
    rel = lambda a, w: (a.double() - w).abs().max().item() / max(w.abs().max().item(), 1e-300)    # noqa: E731
    return dict(u=rel(f["u"], c["fwd"]["u"]), out=rel(f["out"], c["fwd"]["out"]), d_emb=rel(d_emb, c["grads"][0]),
                dW=rel(dW, c["grads"][1]))
