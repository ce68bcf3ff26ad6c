"""Float64 restatements of the BERT kernels (csrc/bert.hip), of the model of keras/models/nlp/bert.py and of its pretrain_step,
written from the contracts in include/dr_hotpath.h "BERT" and from the model's docstrings.  Every function computes in the dtype of
its inputs, so the same code run in float32 is the yardstick r32 of tests/test_gpu_bert.py.  dr_mix32, the dropout rule and
dr_mlm_mask are integer rules and are restated in NumPy.  tests/test_bert_cpu.py pins all of it against independent formulations."""
import math

import numpy as np
import torch

U = 2.0 ** -24
LN_EPS = 1e-12
DENOM_EPS = 1e-5
M64 = (1 << 64) - 1


# ---- the counter hash and the dropout rule ------------------------------------------------------------------------------------------
def mix32(seed, idx):
    """dr_mix32(seed, idx) for an array of indices (uint64 wrap-around arithmetic)"""
    with np.errstate(over="ignore"):
        z = np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(int(seed) & M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)


def mix32_scalar(seed, idx):
    """the same in Python integers: the independent formulation of the CPU test"""
    z = (idx * 0x9E3779B97F4A7C15 + seed) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (z ^ (z >> 31)) >> 32


def drop_thresh(rate):
    return int(min(np.float32(4294967040.0), np.float32(rate) * np.float32(4294967296.0)))


def keep_mask(seed, n, rate):
    """bool [n]: element i is kept iff mix32(seed, i) >= thresh (always when rate == 0)"""
    if rate == 0:
        return np.ones(n, dtype=bool)
    return mix32(seed, np.arange(n, dtype=np.uint64)) >= np.uint32(drop_thresh(rate))


# ---- a. GELU ------------------------------------------------------------------------------------------------------------------------
def gelu(z):
    return 0.5 * z * (1 + torch.special.erf(z / math.sqrt(2.0)))


def gelu_grad(z):
    """Phi(z) + z phi(z)"""
    return 0.5 * (1 + torch.special.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


# ---- b. embedding + LayerNorm + dropout ---------------------------------------------------------------------------------------------
def table_rows(table, ids):
    """table[ids] with a zero row for an id outside [0, rows)"""
    ok = (ids >= 0) & (ids < table.shape[0])
    return table[ids.clamp(0, table.shape[0] - 1)] * ok[..., None].to(table.dtype)


def embed_sum(ids, segment, tok, pos, seg):
    """s [B, L, D] = tok[ids] + pos[l] + seg[segment]"""
    L = ids.shape[1]
    return table_rows(tok, ids) + pos[:L][None, :, :] + table_rows(seg, segment)


def layer_norm(s, gamma, beta, eps=LN_EPS):
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    return gamma * (s - mean) * rstd + beta, mean.squeeze(-1), rstd.squeeze(-1)


def dropout(x, keep, rate):
    """keep: bool array over x's elements in row-major order (keep_mask)"""
    if rate == 0:
        return x
    k = torch.from_numpy(np.asarray(keep, dtype=bool)).reshape(x.shape)
    return torch.where(k, x / (1 - rate), torch.zeros_like(x))


def bert_embed(ids, segment, tok, pos, seg, gamma, beta, rate=0.0, seed=0, eps=LN_EPS):
    s = embed_sum(ids, segment, tok, pos, seg)
    y, mean, rstd = layer_norm(s, gamma, beta, eps)
    return dropout(y, keep_mask(seed, y.numel(), rate), rate), s, mean, rstd


# ---- c. softmax cross-entropy over integer labels -----------------------------------------------------------------------------------
def softmax_ce_ids(logits, bias, labels, weight, smoothing, row_scale, denom, denom_eps):
    """(row_loss [M], g [M, C]) as dr_softmax_ce_ids states them; rows with a negative label: loss 0, gradient 0, logits not read"""
    M, C = logits.shape
    pad = labels < 0
    z = torch.where(pad[:, None], torch.zeros_like(logits), logits)
    if bias is not None:
        z = z + bias
    lse = torch.logsumexp(z, dim=1)
    lab = labels.clamp(min=0)
    w = torch.ones(M, dtype=logits.dtype) if weight is None else weight
    zl = z.gather(1, lab[:, None]).squeeze(1)
    loss = w * ((1 - smoothing) * (lse - zl) + smoothing * (lse - z.mean(1)))
    onehot = torch.zeros_like(z).scatter_(1, lab[:, None], 1.0)
    coef = row_scale * w / ((denom + denom_eps) if denom is not None else 1.0)
    g = coef[:, None] * (torch.exp(z - lse[:, None]) - (1 - smoothing) * onehot - smoothing / C)
    live = (~pad).to(logits.dtype)
    return loss * live, g * live[:, None]


def vocab_cross_entropy(t, table, bias, labels, weight, smoothing, row_scale, denom, denom_eps):
    """(loss_rows, d_t, d_table, d_bias) of layers.vocab_cross_entropy from zero gradient buffers"""
    loss, g = softmax_ce_ids(t @ table.t(), bias, labels, weight, smoothing, row_scale, denom, denom_eps)
    return loss, g @ table, g.t() @ t, g.sum(0)


# ---- d. masking ---------------------------------------------------------------------------------------------------------------------
def mlm_n(n_cand, prob_q16, P):
    return 0 if n_cand == 0 else min(P, max(1, (n_cand * prob_q16 + 32768) >> 16))


def mlm_mask(ids, V, num_special, mask_id, prob, P, seed):
    """(out_ids, positions int32 [B, P], labels int64 [B, P]) of dr_mlm_mask; ids: int64 array [B, L]"""
    ids = np.asarray(ids, dtype=np.int64)
    B, L = ids.shape
    q16 = int(round(float(prob) * 65536))
    out = ids.copy()
    positions = np.full((B, P), -1, dtype=np.int32)
    labels = np.full((B, P), -1, dtype=np.int64)
    e = np.arange(B * L, dtype=np.uint64).reshape(B, L)
    key = (mix32(seed, e).astype(np.uint64) << np.uint64(32)) | np.arange(L, dtype=np.uint64)[None, :]
    r = mix32(seed + 1, e) % np.uint32(10)
    rnd = num_special + (mix32(seed + 2, e).astype(np.int64) % (V - num_special))
    for b in range(B):
        cand = np.nonzero(ids[b] >= num_special)[0]
        n = mlm_n(len(cand), q16, P)
        chosen = np.sort(cand[np.argsort(key[b, cand], kind="stable")[:n]])
        positions[b, :n] = chosen
        labels[b, :n] = ids[b, chosen]
        for l in chosen:
            if r[b, l] < 8:
                out[b, l] = mask_id
            elif r[b, l] == 8:
                out[b, l] = rnd[b, l]
    return out, positions, labels


# ---- the model ----------------------------------------------------------------------------------------------------------------------
MASK_ADD = -4294967296.0            # the additive padding mask of dr_attn_*: float32(-2^32 + 1)


def attention(q, k, v, H, key_mask):
    """softmax(q k^T / sqrt(dh) + key_mask * (-2^32)) v per head; q, k, v [B, L, H * dh], key_mask [B, L] bool (True = padded)"""
    B, L, W = q.shape
    dh = W // H
    qh, kh, vh = (x.reshape(B, L, H, dh).permute(0, 2, 1, 3) for x in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dh)
    if key_mask is not None:
        s = s + key_mask[:, None, None, :].to(s.dtype) * MASK_ADD
    return (torch.softmax(s, dim=-1) @ vh).permute(0, 2, 1, 3).reshape(B, L, W)


def bert_layer(x, key_mask, p, pre, H):
    D = x.shape[-1]
    qkv = x @ p[pre + "qkv_kernel"] + p[pre + "qkv_bias"]
    ctx = attention(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], H, key_mask)
    a = ctx @ p[pre + "attention_output_kernel"] + p[pre + "attention_output_bias"]
    h = layer_norm(a + x, p[pre + "attention_norm_gamma"], p[pre + "attention_norm_beta"])[0]
    f = gelu(h @ p[pre + "intermediate_kernel"] + p[pre + "intermediate_bias"]) @ p[pre + "output_kernel"] + p[pre + "output_bias"]
    return layer_norm(f + h, p[pre + "output_norm_gamma"], p[pre + "output_norm_beta"])[0]


def bert_forward(p, ids, segment, input_mask, num_layers, H, pre="bert."):
    """(sequence_output, pooled_output) without dropout; p: the state_dict of a BertPretraining in one dtype"""
    e = pre + "embeddings."
    x = bert_embed(ids, segment, p[e + "word_embeddings"], p[e + "position_embeddings"], p[e + "token_type_embeddings"], p[e + "gamma"],
                   p[e + "beta"])[0]
    key_mask = (ids == 0) if input_mask is None else ~input_mask
    for i in range(num_layers):
        x = bert_layer(x, key_mask, p, "%slayers.%d." % (pre, i), H)
    return x, torch.tanh(x[:, 0, :] @ p[pre + "pooler_kernel"] + p[pre + "pooler_bias"])


def pretrain_losses(p, ids_masked, segment, positions, labels, nsp_labels, num_layers, H, input_mask=None):
    """(mlm_loss, nsp_loss): sum_r w_r CE_r / (sum_r w_r + 1e-5) over the slots with labels >= 0, and the mean two-way cross-entropy"""
    seq, pooled = bert_forward(p, ids_masked, segment, input_mask, num_layers, H)
    B, L, D = seq.shape
    rows = (torch.arange(B)[:, None] * L + positions.to(torch.int64).clamp(min=0)).reshape(-1)
    t = gelu(seq.reshape(B * L, D)[rows] @ p["transform_kernel"] + p["transform_bias"])
    t = layer_norm(t, p["transform_norm_gamma"], p["transform_norm_beta"])[0]
    y = labels.reshape(-1)
    w = (y >= 0).to(seq.dtype)
    loss_rows, _ = softmax_ce_ids(t @ p["bert.embeddings.word_embeddings"].t(), p["output_bias"], y, w, 0.0, 1.0, None, 0.0)
    mlm = loss_rows.sum() / (w.sum() + DENOM_EPS)
    nsp_logits = pooled @ p["nsp_kernel"] + p["nsp_bias"]
    nsp = (torch.logsumexp(nsp_logits, 1) - nsp_logits.gather(1, nsp_labels[:, None]).squeeze(1)).mean()
    return mlm, nsp


def pretrain_grads(p, *args, **kw):
    """(mlm_loss, nsp_loss, {name: gradient of mlm_loss + nsp_loss}): what one pretrain_step hands its optimizer"""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    mlm, nsp = pretrain_losses(leaves, *args, **kw)
    (mlm + nsp).backward()
    return mlm.detach(), nsp.detach(), {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in leaves.items()}


def adam_step(p, grads, state, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
    """optim.Adam: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); p -= lr_t m / (sqrt(v) + epsilon)"""
    state["t"] = state.get("t", 0) + 1
    t = state["t"]
    lr_t = lr * math.sqrt(1 - beta_2 ** t) / (1 - beta_1 ** t)
    for k, g in grads.items():
        m = state.setdefault("m." + k, torch.zeros_like(g))
        v = state.setdefault("v." + k, torch.zeros_like(g))
        m.mul_(beta_1).add_(g, alpha=1 - beta_1)
        v.mul_(beta_2).addcmul_(g, g, value=1 - beta_2)
        p[k] = p[k] - lr_t * m / (torch.sqrt(v) + epsilon)


# ---- the tiny task of the training tests --------------------------------------------------------------------------------------------
TINY = dict(V=50, D=16, H=2, layers=2, F=32, max_position=16, T=2, num_special=5, mask_id=4, B=16, L=16, steps=60, lr=0.01, P=4, prob=0.25,
            tokens=4)
CLS, SEP = 2, 3


def tiny_batch(step, cfg=TINY):
    """One batch of the tiny corpus: [CLS] A [SEP] B [SEP]; a sentence repeats ONE ordinary token, so a masked token can be read off
    its neighbours; B repeats A's token (nsp label 0) or another one (label 1).  Returns (ids, segment, nsp_labels) as int64 arrays."""
    rng = np.random.RandomState(1000 + step)
    B, L, V, ns = cfg["B"], cfg["L"], cfg["V"], cfg["num_special"]
    la = (L - 3) // 2
    ids = np.zeros((B, L), dtype=np.int64)
    seg = np.zeros((B, L), dtype=np.int64)
    nsp = rng.randint(0, 2, size=B).astype(np.int64)
    K = cfg["tokens"]                      # the corpus uses the first K ordinary tokens of the vocabulary
    assert 2 <= K <= V - ns
    for b in range(B):
        a = ns + rng.randint(0, K)
        other = a if nsp[b] == 0 else ns + (a - ns + 1 + rng.randint(0, K - 1)) % K
        ids[b] = [CLS] + [a] * la + [SEP] + [other] * (L - 3 - la) + [SEP]
        seg[b, la + 2:] = 1
    return ids, seg, nsp


def tiny_masked(step, cfg=TINY):
    """the batch of `step` with the NumPy masking rule applied (seed = step): (masked ids, segment, positions, labels, nsp_labels)"""
    ids, seg, nsp = tiny_batch(step, cfg)
    out, positions, labels = mlm_mask(ids, cfg["V"], cfg["num_special"], cfg["mask_id"], cfg["prob"], cfg["P"], seed=step)
    return out, seg, positions, labels, nsp


def tiny_params(cfg=TINY, seed=0, dtype=torch.float64):
    """a BertPretraining state_dict drawn on the host (normal(0, 0.02) weights, zero biases, unit gammas), the names of the model's"""
    g = torch.Generator().manual_seed(seed)
    D, F, V = cfg["D"], cfg["F"], cfg["V"]

    def w(*shape):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * 0.02).to(dtype)

    def zeros(n):
        return torch.zeros(n, dtype=dtype)

    def ones(n):
        return torch.ones(n, dtype=dtype)
    e = "bert.embeddings."
    p = {e + "word_embeddings": w(V, D), e + "position_embeddings": w(cfg["max_position"], D), e + "token_type_embeddings": w(cfg["T"], D),
         e + "gamma": ones(D), e + "beta": zeros(D)}
    for i in range(cfg["layers"]):
        pre = "bert.layers.%d." % i
        p.update({pre + "qkv_kernel": w(D, 3 * D), pre + "qkv_bias": zeros(3 * D), pre + "attention_output_kernel": w(D, D),
                  pre + "attention_output_bias": zeros(D), pre + "attention_norm_gamma": ones(D), pre + "attention_norm_beta": zeros(D),
                  pre + "intermediate_kernel": w(D, F), pre + "intermediate_bias": zeros(F), pre + "output_kernel": w(F, D),
                  pre + "output_bias": zeros(D), pre + "output_norm_gamma": ones(D), pre + "output_norm_beta": zeros(D)})
    p.update({"bert.pooler_kernel": w(D, D), "bert.pooler_bias": zeros(D), "transform_kernel": w(D, D), "transform_bias": zeros(D),
              "transform_norm_gamma": ones(D), "transform_norm_beta": zeros(D), "output_bias": zeros(V), "nsp_kernel": w(D, 2),
              "nsp_bias": zeros(2)})
    return p


_TRAINED = {}


def tiny_training(cfg=TINY):
    """the restatement's own float64 training run on the tiny task, computed once: the list of per-step (mlm, nsp) losses"""
    key = tuple(sorted(cfg.items()))
    if key not in _TRAINED:
        p, state, hist = tiny_params(cfg), {}, []
        for step in range(cfg["steps"]):
            ids, seg, positions, labels, nsp = (torch.from_numpy(a) for a in tiny_masked(step, cfg))
            mlm, nsp_loss, grads = pretrain_grads(p, ids, seg, positions, labels, nsp, cfg["layers"], cfg["H"])
            adam_step(p, grads, state, cfg["lr"])
            hist.append((float(mlm), float(nsp_loss)))
        _TRAINED[key] = hist
    return _TRAINED[key]


def final_loss(hist, last=10):
    """the mean masked-LM loss of the last steps of a training run"""
    return sum(m for m, _ in hist[-last:]) / last


# ---- the cases tests/test_gpu_bert.py runs (tests/test_bert_cpu.py asserts what that file relies on) ----------------------------------
LDS_COLS = 32768                    # DR_SOFTMAX_CE_IDS_LDS_COLS
CE_COLS = (1, 2, 5, 64, 257, 1000, LDS_COLS, LDS_COLS + 1)
CE_ROWS = (1, 3, 70)
EMBED_SHAPES = ((1, 1, 4, 3, 1), (3, 5, 20, 7, 2), (2, 128, 64, 50, 2), (2, 8, 1024, 11, 2))      # (B, L, D, V, T)
GELU_SHAPES = ((1, 1), (3, 5), (70, 7), (33, 260))
GELU_SPECIAL = (0.0, 1e-30, -1e-30, 1e-42, -1e-42, 10.0, -10.0, 88.0, -88.0)
MASK_LENGTHS, MASK_PS, MASK_PROBS = (1, 2, 7, 128, 512), (1, 20, 128), (0.15, 1.0)
MASK_V, MASK_SPECIAL, MASK_ID = 300, 5, 4


def ce_case(M, C, seed=0):
    """logits, bias, labels (a padding row where M >= 3), weights and a denominator; |logits + bias| stays far below 80"""
    g = torch.Generator().manual_seed(100 * C + M + seed)
    logits = torch.randn(M, C, generator=g, dtype=torch.float64) * 3
    bias = torch.randn(C, generator=g, dtype=torch.float64)
    labels = torch.randint(0, C, (M,), generator=g)
    if M >= 3:
        labels[1] = -1
    weight = torch.rand(M, generator=g, dtype=torch.float64) + 0.5
    denom = torch.tensor(float(M) * 0.75, dtype=torch.float64)
    return dict(logits=logits, bias=bias, labels=labels, weight=weight, denom=denom)


def gelu_case(M, N):
    g = torch.Generator().manual_seed(7 * M + N)
    z = torch.randn(M, N, generator=g, dtype=torch.float64) * 2
    flat = z.reshape(-1)
    n = min(len(GELU_SPECIAL), flat.numel())
    flat[:n] = torch.tensor(GELU_SPECIAL[:n], dtype=torch.float64)
    return z, torch.randn(M, N, generator=g, dtype=torch.float64)


def embed_case(B, L, D, V, T, equal_ids=False, seed=0):
    """tables with an unreferenced token row (the last) for the NaN check, ids / segments with out-of-range entries where B * L >= 4"""
    g = torch.Generator().manual_seed(1000 * D + 10 * L + B + seed)
    c = dict(tok=torch.randn(V, D, generator=g, dtype=torch.float64), pos=torch.randn(L + 2, D, generator=g, dtype=torch.float64),
             seg=torch.randn(T, D, generator=g, dtype=torch.float64), gamma=torch.randn(D, generator=g, dtype=torch.float64) + 1.5,
             beta=torch.randn(D, generator=g, dtype=torch.float64), d_out=torch.randn(B, L, D, generator=g, dtype=torch.float64))
    ids = torch.randint(0, max(1, V - 1), (B, L), generator=g)
    segment = torch.randint(0, T, (B, L), generator=g)
    if equal_ids:
        ids[:] = 1
    elif B * L >= 4:
        ids.view(-1)[1], ids.view(-1)[2] = -3, V + 5
        segment.view(-1)[0], segment.view(-1)[3] = T, -1
    c["ids"], c["segment"] = ids, segment
    return c


def mask_case(L, seed=0):
    """ids int64 [6, L]: a row of special tokens only, a row with one candidate, a row of candidates only, three mixed rows"""
    rng = np.random.RandomState(31 * L + seed)
    ids = rng.randint(MASK_SPECIAL, MASK_V, size=(6, L)).astype(np.int64)
    ids[0] = rng.randint(0, MASK_SPECIAL, size=L)
    ids[1] = 0
    ids[1, L - 1] = MASK_SPECIAL
    special = rng.rand(3, L) < 0.3
    ids[3:][special] = rng.randint(0, MASK_SPECIAL, size=int(special.sum()))
    return ids
