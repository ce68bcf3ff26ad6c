"""A restatement of the Transformer package's semantics for the tests: torch on the CPU in float64 (the
oracle) or float32 (the yardstick of the tolerances).  It restates what the reference's keras/models/nlp layers compute, it is NOT
recorded TensorFlow output.  Only the additive padding mask is done in fp32 in both precisions, because its saturation
(float32(s) + float32(-2^32 + 1) == -2^32 for |s| < 128) is part of the semantics.

The dropout masks are the documented counter hash (include/dr_hotpath.h, dr_attn_fwd), restated in numpy."""
import math

import numpy as np
import torch

MASK_NUM = np.float32(-2 ** 32 + 1)          # == -2^32 in fp32
M64 = (1 << 64) - 1


def mix32(seed, idx):
    """the kernels' dr_mix32(seed, idx) on uint64 arrays (wrap-around arithmetic)"""
    with np.errstate(over="ignore"):
        z = idx.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(int(seed) & M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)


def drop_threshold(rate):
    return np.uint32(min(np.float32(4294967040.0), np.float32(rate) * np.float32(4294967296.0)))


def keep_mask(seed, rate, shape):
    """bool array of `shape`: element with linear (row-major) index i is kept iff mix32(seed, i) >= rate * 2^32.  For the
    attention the shape is [B, H, Lq, Lk] (index ((b H + h) Lq + i) Lk + j), for the token embedding [B, L, D]."""
    n = int(np.prod(shape))
    if rate == 0:
        return np.ones(shape, dtype=bool)
    return (mix32(seed, np.arange(n, dtype=np.uint64)) >= drop_threshold(rate)).reshape(shape)


def _t(x, dtype):
    return x.to(dtype) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)).to(dtype)


def attention_scores(q, k, n_heads, mask=None, future=False, dtype=torch.float64):
    """the masked logits [B, H, Lq, Lk]: (q . k) / sqrt(dh), + mask * (-2^32 + 1) as an fp32 add, future entries replaced"""
    B, Lq, W = q.shape
    Lk = k.shape[1]
    H = n_heads
    dh = W // H
    qh = q.to(dtype).reshape(B, Lq, H, dh).permute(0, 2, 1, 3)
    kh = k.to(dtype).reshape(B, Lk, H, dh).permute(0, 2, 1, 3)
    s = torch.matmul(qh, kh.transpose(2, 3)) / (dh ** 0.5)
    if mask is not None:
        m = torch.as_tensor(np.asarray(mask)).to(torch.bool)[:, None, None, :].expand(B, H, Lq, Lk)
        added = (s.to(torch.float32) + torch.tensor(MASK_NUM)).to(dtype)          # the fp32 add of the reference
        s = torch.where(m, added, s)
    if future:
        assert Lq == Lk
        hidden = torch.triu(torch.ones(Lq, Lk, dtype=torch.bool), diagonal=1)
        s = torch.where(hidden, torch.tensor(float(MASK_NUM), dtype=dtype), s)
    return s


def attention_probabilities(q, k, n_heads, mask=None, future=False, dtype=torch.float64):
    return torch.softmax(attention_scores(q, k, n_heads, mask, future, dtype), dim=-1)


def attention(q, k, v, n_heads, mask=None, future=False, keep=None, rate=0.0, dtype=torch.float64):
    """q [B, Lq, H dh], k, v [B, Lk, H dh] (torch, may require grad), mask [B, Lk] bool (True = padded), keep [B, H, Lq, Lk] bool.
    Returns [B, Lq, H dh] in `dtype`."""
    B, Lq, W = q.shape
    Lk = k.shape[1]
    H = n_heads
    p = attention_probabilities(q, k, H, mask, future, dtype)
    if keep is not None and rate > 0:
        p = torch.where(torch.as_tensor(keep), p / (1.0 - float(np.float32(rate))), torch.zeros((), dtype=dtype))
    vh = v.to(dtype).reshape(B, Lk, H, W // H).permute(0, 2, 1, 3)
    return torch.matmul(p, vh).permute(0, 2, 1, 3).reshape(B, Lq, W)


def layer_norm(a, b, gamma, beta, eps=1e-8, dtype=torch.float64):
    s = a.to(dtype) + b.to(dtype) if b is not None else a.to(dtype)
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    return gamma.to(dtype) * ((s - mean) / (var + eps) ** 0.5) + beta.to(dtype)


def position_encoding(L, D):
    t = np.zeros((L, D))
    for pos in range(L):
        for i in range(D):
            t[pos, i] = pos / np.power(10000, (i - i % 2) / D)
    t[:, 0::2] = np.sin(t[:, 0::2])
    t[:, 1::2] = np.cos(t[:, 1::2])
    return t.astype(np.float32)


def token_embedding(table, ids, pos=None, keep=None, rate=0.0, dtype=torch.float64):
    """dropout(table[ids] * sqrt(D) + pos); ids [B, L] numpy / torch integers, keep [B, L, D]"""
    D = table.shape[1]
    ids = torch.as_tensor(np.asarray(ids)).to(torch.int64)
    scale = float(np.float32(math.sqrt(D))) if dtype == torch.float32 else math.sqrt(D)
    e = table.to(dtype)[ids] * scale
    if pos is not None:
        e = e + _t(pos, dtype)[None]
    if keep is not None and rate > 0:
        e = torch.where(torch.as_tensor(keep), e / (1.0 - float(np.float32(rate))), torch.zeros((), dtype=dtype))
    return e


def multi_head_attention(queries, keys, values, wq, wk, wv, n_heads, mask=None, future=False, keep=None, rate=0.0,
                         dtype=torch.float64):
    q = queries.to(dtype) @ wq.to(dtype)
    k = keys.to(dtype) @ wk.to(dtype)
    v = values.to(dtype) @ wv.to(dtype)
    return attention(q, k, v, n_heads, mask, future, keep, rate, dtype)


def feed_forward(x, w1, b1, w2, b2, dtype=torch.float64):
    return torch.relu(x.to(dtype) @ w1.to(dtype) + b1.to(dtype)) @ w2.to(dtype) + b2.to(dtype)


def transformer(params, cfg, enc_ids, dec_ids, keeps=None, dtype=torch.float64):
    """params: {name: torch tensor} under the names of Transformer.state_dict(); cfg: get_config(); keeps: None (all rates 0) or
    {"enc_emb", "dec_emb": [B, L, D], "enc.i", "dec0.i", "dec1.i": [B, H, Lq, Lk]} with the attention rate `att_rate` and the
    embedding rate cfg["dropout_rate"].  Returns the vocabulary softmax [B, L, V]."""
    D, H = cfg["model_dim"], cfg["n_heads"]
    keeps = keeps or {}
    att_rate = keeps.get("att_rate", 0.0)
    emb_rate = cfg["dropout_rate"] if keeps else 0.0
    E = params["embeddings"]
    enc_ids = np.asarray(enc_ids)
    dec_ids = np.asarray(dec_ids)
    enc_mask, dec_mask = enc_ids == 0, dec_ids == 0

    def mha(prefix, i, xq, xkv, mask, future, keep):
        p = "%s.%d." % (prefix, i)
        return multi_head_attention(xq, xkv, xkv, params[p + "_weights_queries"], params[p + "_weights_keys"],
                                    params[p + "_weights_values"], H, mask, future, keep, att_rate, dtype)

    def ln(prefix, i, a, b):
        p = "%s.%d." % (prefix, i)
        return layer_norm(a, b, params[p + "gamma"], params[p + "beta"], 1e-8, dtype)

    def ff(prefix, i, x):
        p = "%s.%d." % (prefix, i)
        return feed_forward(x, params[p + "weights_inner"], params[p + "bias_inner"], params[p + "weights_out"], params[p + "bias_out"],
                            dtype)

    x = token_embedding(E, enc_ids, position_encoding(enc_ids.shape[1], D), keeps.get("enc_emb"), emb_rate, dtype)
    for i in range(cfg["encoder_stack"]):
        a = ln("EncoderLayerNorms0", i, mha("EncoderMultiHeadAttentions", i, x, x, enc_mask, False, keeps.get("enc.%d" % i)), x)
        x = ln("EncoderLayerNorms1", i, ff("EncoderPositionWiseFeedForwards", i, a), a)
    enc = x
    y = token_embedding(E, dec_ids, position_encoding(dec_ids.shape[1], D), keeps.get("dec_emb"), emb_rate, dtype)
    for i in range(cfg["decoder_stack"]):
        a = ln("DecoderLayerNorms0", i, mha("DecoderMultiHeadAttentions0", i, y, y, dec_mask, True, keeps.get("dec0.%d" % i)), y)
        c = ln("DecoderLayerNorms1", i, mha("DecoderMultiHeadAttentions1", i, a, enc, enc_mask, False, keeps.get("dec1.%d" % i)), a)
        y = ln("DecoderLayerNorms2", i, ff("DecoderPositionWiseFeedForwards", i, c), c)
    return torch.softmax(y @ E.to(dtype).T, dim=-1)


def noam_lr(model_dim, step, warmup_steps):
    if step == 0:
        return model_dim ** -0.5 * warmup_steps ** -1.5
    return model_dim ** -0.5 * min(step ** -0.5, step * warmup_steps ** -1.5)


def label_smoothing(y, epsilon=0.1):
    y = np.asarray(y, dtype=np.float64)
    return (1 - epsilon) * y + epsilon / y.shape[-1]


# ---- the magnitudes the attention kernels' error bounds are stated on (tests/test_gpu_attention.py, tests/layer_autograd_cases.py)
def _gamma(d):
    u = 2.0 ** -24
    return d * u / (1.0 - d * u)


def dhp(dh):
    return 16 if dh <= 16 else 32 if dh <= 32 else 64 if dh <= 64 else 128


def attention_magnitudes(q, k, v, d_out, H, mask, future, keep, rate):
    """the formulas of out, dq, dk, dv evaluated on absolute values (float64), [B, L, W] each"""
    B, Lq, W = q.shape
    Lk = k.shape[1]
    dh = W // H
    t64 = lambda a: torch.from_numpy(a).to(torch.float64)                                  # noqa: E731
    heads = lambda a: t64(a).reshape(a.shape[0], a.shape[1], H, dh).permute(0, 2, 1, 3)    # noqa: E731
    merge = lambda a: a.permute(0, 2, 1, 3).reshape(a.shape[0], a.shape[2], W).numpy()     # noqa: E731
    P = attention_probabilities(t64(q), t64(k), H, mask, future)
    D = torch.from_numpy(np.asarray(keep)).to(torch.float64) / (1.0 - float(np.float32(rate))) if rate > 0 else torch.ones_like(P)
    qa, ka, va, ga = heads(np.abs(q)), heads(np.abs(k)), heads(np.abs(v)), heads(np.abs(d_out))
    Pd = P * D
    mag_out = Pd @ va
    mag_dv = Pd.transpose(2, 3) @ ga
    mag_dp = D * (ga @ va.transpose(2, 3))
    mag_delta = (P * mag_dp).sum(-1, keepdim=True)
    mag_ds = P * (mag_dp + mag_delta)
    if future:
        mag_ds = torch.where(torch.triu(torch.ones(Lq, Lk, dtype=torch.bool), 1), torch.zeros((), dtype=torch.float64), mag_ds)
    mag_dq = mag_ds @ ka / math.sqrt(dh)
    mag_dk = mag_ds.transpose(2, 3) @ qa / math.sqrt(dh)
    # the score error: gamma(padded dh) max_ij |q_i| . |k_j| / sqrt(dh)
    es = _gamma(dhp(dh) + 2) * float((qa @ ka.transpose(2, 3)).max()) / math.sqrt(dh)
    return [merge(m) for m in (mag_out, mag_dq, mag_dk, mag_dv)], es
