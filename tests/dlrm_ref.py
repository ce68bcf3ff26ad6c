"""Torch restatement of DLRM's pairwise dot interaction and of the model's logit, written from the definition (Naumov et al. 2019; the
reference ships no code for it).  Works in whatever dtype its inputs have (float64 is the tests' truth) and under autograd.  Used by the
tests only; the package does not import it.

For one example T [N, D] is the dense vector t_0 (when given) followed by the F field embeddings in field order, Z = T T^T, and

    self_interaction False:  out[b, c0 + i (i - 1) / 2 + j] = Z[i, j]   for 0 <= j <  i < N      P = N (N - 1) / 2
    self_interaction True :  out[b, c0 + i (i + 1) / 2 + j] = Z[i, j]   for 0 <= j <= i < N      P = N (N + 1) / 2
    out[b, 0:D] = t_0, c0 = D   (without a dense vector c0 = 0 and nothing is copied)

the row-major lower triangle."""
import torch

ACT = {0: (lambda v: v), 1: torch.relu, 2: torch.sigmoid, 3: torch.tanh}


def stack(dense, emb):
    """T [B, N, D] from dense [B, D] | None and emb [B, F, D]"""
    return emb if dense is None else torch.cat([dense[:, None, :], emb], dim=1)


def triangle(N, self_interaction):
    """(rows, cols) of the triangle's elements in output order: for i ascending, j ascending within i"""
    pairs = [(i, j) for i in range(N) for j in range(i + 1 if self_interaction else i)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def dot_interaction(dense, emb, self_interaction=False):
    """dense [B, D] | None, emb [B, F, D] -> [B, c0 + P]"""
    T = stack(dense, emb)
    Z = torch.einsum("bid,bjd->bij", T, T)
    rows, cols = triangle(T.shape[1], self_interaction)
    tri = Z[:, rows, cols]
    return tri if dense is None else torch.cat([dense, tri], dim=1)


def symmetric_gradient(d_tri, N, self_interaction):
    """S = G + G^T [B, N, N] with G the lower-triangular matrix holding d_tri [B, P]; the diagonal is thereby doubled"""
    rows, cols = triangle(N, self_interaction)
    G = torch.zeros((d_tri.shape[0], N, N), dtype=d_tri.dtype)
    G[:, rows, cols] = d_tri
    return G + G.transpose(1, 2)


def dot_interaction_backward(dense, emb, d_out, self_interaction=False):
    """(d_dense | None, d_emb [B, F, D]) by the closed form dT = S T, dT_0 += d_out[:, 0:D]; no autograd"""
    T = stack(dense, emb)
    c0 = 0 if dense is None else dense.shape[1]
    dT = torch.einsum("bij,bjd->bid", symmetric_gradient(d_out[:, c0:], T.shape[1], self_interaction), T)
    if dense is None:
        return None, dT
    return dT[:, 0] + d_out[:, :c0], dT[:, 1:]


def tower(x, Ws, bs, act, last_linear):
    for k, (W, b) in enumerate(zip(Ws, bs)):
        x = x @ W + b
        if not (last_linear and k == len(Ws) - 1):
            x = ACT[act](x)
    return x


def dlrm_logits(emb, dense_features, bottom_Ws, bottom_bs, top_Ws, top_bs, act=1, self_interaction=False):
    """emb [B, F, D] the gathered embeddings, dense_features [B, Nd] | None -> logits [B, 1]
    = top(dot_interaction(bottom(dense_features), emb)); every bottom layer is activated, the top's last layer is linear."""
    bottom = None if dense_features is None else tower(dense_features, bottom_Ws, bottom_bs, act, last_linear=False)
    return tower(dot_interaction(bottom, emb, self_interaction), top_Ws, top_bs, act, last_linear=True)
