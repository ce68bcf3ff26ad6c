"""Torch restatement of xDeepFM: the CIN layer with its sum pooling (keras/models/ranking/xdeepfm.py:71-96 of the reference plus the
paper's sum over the embedding axis), the layer's closed-form backward as the kernels implement it, the stack with the direct
connection, and the model's logit.  Works in whatever dtype its inputs have (float64 is the tests' truth) and under autograd.  act codes
are the kernels': 0 linear, 1 relu, 2 sigmoid, 3 tanh; relu'(0) = 0 as in torch and TensorFlow.  Used by the tests only; the package
does not import it."""
import torch

ACT = {0: (lambda v: v), 1: torch.relu, 2: torch.sigmoid, 3: torch.tanh}


def act_grad(out, act):
    """activation'(pre) through out = activation(pre)"""
    if act == 1:
        return (out > 0).to(out.dtype)
    if act == 2:
        return out * (1 - out)
    if act == 3:
        return 1 - out * out
    return torch.ones_like(out)


def cin_pool(x0, x, W, bias=None, act=0):
    """x0 [B, H0, D], x [B, Hk, D], W [H0 * Hk, Fm], bias [Fm] | None -> (out [B, Fm, D], pooled [B, Fm])"""
    B, H0, D = x0.shape
    Hk = x.shape[1]
    z = (x0[:, :, None, :] * x[:, None, :, :]).reshape(B, H0 * Hk, D)          # the outer product per embedding coordinate
    pre = torch.einsum("bkd,kf->bfd", z, W)
    if bias is not None:
        pre = pre + bias[None, :, None]
    out = ACT[act](pre)
    return out, out.sum(-1)


def cin_pool_backward(x0, x, W, act, out, d_out=None, d_pooled=None):
    """(d_x0, d_x, dW, dbias) by the closed form at the top of csrc/cin.hip with g = (d_out + d_pooled[:, :, None]) act'(out); no autograd"""
    B, H0, D = x0.shape
    Hk, Fm = x.shape[1], W.shape[1]
    g = torch.zeros_like(out)
    if d_out is not None:
        g = g + d_out
    if d_pooled is not None:
        g = g + d_pooled[:, :, None]
    g = g * act_grad(out, act)
    W3 = W.reshape(H0, Hk, Fm)
    T = torch.einsum("bfd,ijf->bijd", g, W3)
    d_x0 = torch.einsum("bjd,bijd->bid", x, T)
    d_x = torch.einsum("bid,bijd->bjd", x0, T)
    dW = torch.einsum("bfd,bid,bjd->ijf", g, x0, x).reshape(H0 * Hk, Fm)
    return d_x0, d_x, dW, g.sum(dim=(0, 2))


def cin_network(x0, Ws, biases, act=0):
    """[B, sum Fm_k]: x_k = CIN(x0, x_{k-1}), x_0 = x0; every layer sum-pooled over D and concatenated (direct connection)"""
    x, pooled = x0, []
    for W, b in zip(Ws, biases):
        x, p = cin_pool(x0, x, W, b, act)
        pooled.append(p)
    return torch.cat(pooled, dim=1)


def xdeepfm_logits(emb, linear, cin_Ws, cin_biases, cin_act, w_cin, dnn_Ws, dnn_bs, dnn_act):
    """emb [B, F, D] the gathered embeddings, linear [B] the first-order term with the bias -> logits [B, 1]
    = linear + CINNetwork(emb) w_cin + DNN(flatten(emb)); the DNN's last layer is linear."""
    h = emb.reshape(emb.shape[0], -1)
    for k, (W, b) in enumerate(zip(dnn_Ws, dnn_bs)):
        h = h @ W + b
        if k < len(dnn_Ws) - 1:
            h = ACT[dnn_act](h)
    return linear.reshape(-1, 1) + cin_network(emb, cin_Ws, cin_biases, cin_act) @ w_cin + h
