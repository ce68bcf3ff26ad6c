"""What tests/test_gpu_bert.py stands on, proved without a GPU: the float64 restatements of tests/bert_ref.py agree with independent
formulations (torch.nn.functional, an explicit softmax attention, naive Python loops over Python integers), the new entry points are
declared and wrapped, the model imports, and the cases the GPU file runs have the properties it relies on.

Bound: both sides are float64 evaluations of the same expression in another order, at most a few thousand terms each; RTOL64 of
tests/test_layer_autograd_cpu.py relative to the largest magnitude involved (widened by the row length where a row of 32 769 terms is
summed).

The masking cases: every (L, P, prob) has a row without candidates and a row of candidates only; a row with 0 < n_cand < P exists
wherever P > 1, and a row clipped at P wherever L and prob can reach P at all (with L < P no row can)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bert_ref as R

RTOL64 = 1e-13

ENTRY_POINTS = ("dr_gelu_fwd", "dr_gelu_bwd", "dr_bert_embed_fwd", "dr_bert_embed_bwd", "dr_bert_embed_bwd_workspace_bytes",
                "dr_softmax_ce_ids", "dr_softmax_ce_ids_lds_cols", "dr_colsum_add", "dr_colsum_add_workspace_bytes", "dr_mlm_mask")
WRAPPERS = ("gelu_fwd", "gelu_bwd_", "bert_embed_fwd", "bert_embed_bwd", "softmax_ce_ids", "colsum_add", "mlm_mask")


def _close(a, b, n=1):
    scale = max(1.0, float(b.abs().max()))
    assert a.shape == b.shape and float((a - b).abs().max()) <= n * RTOL64 * scale, float((a - b).abs().max())


def test_every_new_entry_point_is_declared_and_wrapped_and_the_model_imports():
    """fails on the parent commit: none of the names exists there"""
    from deep_recommenders_amd import _lib, layers, ops
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
    for name in WRAPPERS:
        assert callable(getattr(ops, name)), name
    assert callable(layers.vocab_cross_entropy)
    assert ops.SOFTMAX_CE_IDS_LDS_COLS == R.LDS_COLS and _lib.lib().dr_softmax_ce_ids_lds_cols() == R.LDS_COLS
    assert R.LDS_COLS >= 30522 + 2 and R.LDS_COLS * 4 <= 160 * 1024       # BERT's vocabulary fits the CU's LDS
    from deep_recommenders_amd.keras.models.nlp import BERT, BertPretraining
    assert BERT.__name__ == "BERT" and BertPretraining.__name__ == "BertPretraining"
    import inspect
    sig = inspect.signature(layers.vocab_cross_entropy)
    assert list(sig.parameters) == ["t", "table", "bias", "labels", "weight", "smoothing", "row_scale", "denom", "denom_eps", "d_table",
                                    "d_bias", "chunk_rows"]


def test_the_hash_and_the_dropout_rule():
    idx = [0, 1, 2, 63, 64, 12345, 2 ** 31, 2 ** 40 + 7]
    for seed in (0, 1, 2 ** 63 + 5, R.M64):
        got = R.mix32(seed, np.array(idx, dtype=np.uint64))
        assert [int(v) for v in got] == [R.mix32_scalar(seed, i) for i in idx]
    assert R.drop_thresh(0.1) == int(np.float32(0.1) * np.float32(2.0 ** 32)) and R.drop_thresh(0.99999999) == 4294967040
    keep = R.keep_mask(7, 4096, 0.1)
    assert [bool(k) for k in keep[:64]] == [R.mix32_scalar(7, i) >= R.drop_thresh(0.1) for i in range(64)]
    assert 0.85 < keep.mean() < 0.95 and R.keep_mask(7, 16, 0.0).all()


@pytest.mark.parametrize("shape", R.GELU_SHAPES, ids=str)
def test_gelu_and_its_derivative(shape):
    z, dy = R.gelu_case(*shape)
    _close(R.gelu(z), F.gelu(z))
    leaf = z.clone().requires_grad_(True)
    (F.gelu(leaf) * dy).sum().backward()
    _close(R.gelu_grad(z) * dy, leaf.grad)
    assert torch.isfinite(R.gelu(z)).all() and torch.isfinite(R.gelu_grad(z)).all()
    big = torch.tensor([-88.0, -10.0, 10.0, 88.0], dtype=torch.float64)
    assert float(R.gelu(big)[0]) == 0.0 and float(R.gelu_grad(big)[0]) == 0.0 and float(R.gelu(big)[3]) == 88.0


@pytest.mark.parametrize("shape", R.EMBED_SHAPES, ids=str)
def test_embedding_layer_norm_and_dropout(shape):
    B, L, D, V, T = shape
    c = R.embed_case(*shape)
    out, s, mean, rstd = R.bert_embed(c["ids"], c["segment"], c["tok"], c["pos"], c["seg"], c["gamma"], c["beta"])
    tok0 = torch.cat([c["tok"], torch.zeros(1, D, dtype=torch.float64)])         # row V: the zero row of an id out of range
    seg0 = torch.cat([c["seg"], torch.zeros(1, D, dtype=torch.float64)])
    ids = torch.where((c["ids"] >= 0) & (c["ids"] < V), c["ids"], torch.full_like(c["ids"], V))
    sg = torch.where((c["segment"] >= 0) & (c["segment"] < T), c["segment"], torch.full_like(c["segment"], T))
    want_s = F.embedding(ids, tok0) + F.embedding(torch.arange(L), c["pos"])[None] + F.embedding(sg, seg0)
    _close(s, want_s)
    _close(out, F.layer_norm(want_s, (D,), c["gamma"], c["beta"], eps=R.LN_EPS), n=D)
    _close(rstd, 1 / torch.sqrt(want_s.var(-1, unbiased=False) + R.LN_EPS), n=D)
    dropped = R.bert_embed(c["ids"], c["segment"], c["tok"], c["pos"], c["seg"], c["gamma"], c["beta"], rate=0.1, seed=5)[0]
    keep = torch.tensor([R.mix32_scalar(5, i) >= R.drop_thresh(0.1) for i in range(min(out.numel(), 512))])
    flat, dflat = out.reshape(-1)[:keep.numel()], dropped.reshape(-1)[:keep.numel()]
    _close(dflat, torch.where(keep, flat / 0.9, torch.zeros_like(flat)))


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("C", [c for c in R.CE_COLS if c <= 1000] + [R.LDS_COLS + 1])
def test_softmax_cross_entropy_over_integer_labels(C, smoothing):
    for M in R.CE_ROWS:
        c = R.ce_case(M, C)
        assert float((c["logits"] + c["bias"]).abs().max()) < 80                     # what the GPU file relies on
        row_scale, eps = 0.25, 1e-5
        loss, g = R.softmax_ce_ids(c["logits"], c["bias"], c["labels"], c["weight"], smoothing, row_scale, c["denom"], eps)
        leaf = torch.nan_to_num(c["logits"]).clone().requires_grad_(True)
        ce = F.cross_entropy(leaf + c["bias"], c["labels"], ignore_index=-1, reduction="none", label_smoothing=smoothing)
        _close(loss, (ce * c["weight"]).detach(), n=max(1, C // 64))
        (row_scale * (ce * c["weight"]).sum() / (c["denom"] + eps)).backward()
        _close(g, leaf.grad, n=max(1, C // 64))
        pad = c["labels"] < 0
        assert float(loss[pad].abs().sum()) == 0 and float(g[pad].abs().sum()) == 0
        poisoned = c["logits"].clone()
        poisoned[pad] = float("nan")                                                 # a padding row's logits reach nothing
        loss2, g2 = R.softmax_ce_ids(poisoned, c["bias"], c["labels"], c["weight"], smoothing, row_scale, c["denom"], eps)
        assert torch.equal(loss2, loss) and torch.equal(g2, g)
        assert float(g.sum(1).abs().max()) <= C * 2.0 ** -53 * 4                     # gradient rows sum to 0


def test_vocab_cross_entropy_is_the_three_products_around_it():
    g = torch.Generator().manual_seed(3)
    t, table = torch.randn(7, 20, generator=g, dtype=torch.float64), torch.randn(33, 20, generator=g, dtype=torch.float64)
    bias, labels = torch.randn(33, generator=g, dtype=torch.float64), torch.randint(0, 33, (7,), generator=g)
    lt, lb, ltab = (x.clone().requires_grad_(True) for x in (t, bias, table))
    ce = F.cross_entropy(lt @ ltab.t() + lb, labels, reduction="none")
    ce.sum().backward()
    loss, d_t, d_table, d_bias = R.vocab_cross_entropy(t, table, bias, labels, None, 0.0, 1.0, None, 0.0)
    _close(loss, ce.detach()), _close(d_t, lt.grad), _close(d_table, ltab.grad), _close(d_bias, lb.grad)


def test_attention_against_an_explicit_softmax():
    g = torch.Generator().manual_seed(4)
    B, L, H, dh = 2, 5, 2, 3
    q, k, v = (torch.randn(B, L, H * dh, generator=g, dtype=torch.float64) for _ in range(3))
    key_mask = torch.tensor([[False, False, True, False, True], [False] * 5])
    got = R.attention(q, k, v, H, key_mask)
    want = torch.zeros_like(got)
    for b in range(B):
        for h in range(H):
            cols = slice(h * dh, (h + 1) * dh)
            for i in range(L):
                s = [float(q[b, i, cols] @ k[b, j, cols]) / math.sqrt(dh) + (R.MASK_ADD if key_mask[b, j] else 0.0) for j in range(L)]
                m = max(s)
                e = [math.exp(x - m) for x in s]
                for j in range(L):
                    want[b, i, cols] += e[j] / sum(e) * v[b, j, cols]
    _close(got, want)


def _naive_mask(ids, V, num_special, mask_id, prob, P, seed):
    B, L = ids.shape
    q16 = int(round(prob * 65536))
    out, positions, labels = ids.copy(), np.full((B, P), -1, np.int32), np.full((B, P), -1, np.int64)
    for b in range(B):
        keys = sorted(((R.mix32_scalar(seed, b * L + l) << 32) | l) for l in range(L) if ids[b, l] >= num_special)
        n = 0 if not keys else min(P, max(1, (len(keys) * q16 + 32768) >> 16))
        for slot, l in enumerate(sorted(key & 0xFFFFFFFF for key in keys[:n])):
            positions[b, slot], labels[b, slot] = l, ids[b, l]
            r = R.mix32_scalar((seed + 1) & R.M64, b * L + l) % 10
            if r < 8:
                out[b, l] = mask_id
            elif r == 8:
                out[b, l] = num_special + R.mix32_scalar((seed + 2) & R.M64, b * L + l) % (V - num_special)
    return out, positions, labels


@pytest.mark.parametrize("L", R.MASK_LENGTHS)
def test_the_masking_rule_and_the_rows_its_cases_hold(L):
    ids = R.mask_case(L)
    n_cand = (ids >= R.MASK_SPECIAL).sum(1)
    assert n_cand[0] == 0 and n_cand[1] == 1 and n_cand[2] == L
    for P in R.MASK_PS:
        for prob in R.MASK_PROBS:
            q16 = int(round(prob * 65536))
            ns = [R.mlm_n(int(c), q16, P) for c in n_cand]
            assert ns[0] == 0 and (P == 1 or any(0 < c < P for c in n_cand))
            if R.mlm_n(L, q16, P) == P:
                assert ns[2] == P                                                    # the clip at P is reached where it can be
            got = R.mlm_mask(ids, R.MASK_V, R.MASK_SPECIAL, R.MASK_ID, prob, P, seed=11)
            if L <= 128:
                want = _naive_mask(ids, R.MASK_V, R.MASK_SPECIAL, R.MASK_ID, prob, P, 11)
                for a, b in zip(got, want):
                    assert a.dtype == b.dtype and np.array_equal(a, b)
            out, positions, labels = got
            for b in range(ids.shape[0]):
                n = ns[b]
                assert (positions[b, n:] == -1).all() and (labels[b, n:] == -1).all() and (np.diff(positions[b, :n]) > 0).all()
                changed = np.nonzero(out[b] != ids[b])[0]
                assert set(changed) <= set(positions[b, :n]) and (ids[b, positions[b, :n]] >= R.MASK_SPECIAL).all()
    assert any(R.mlm_n(L2, int(round(p * 65536)), P2) == P2 for L2 in R.MASK_LENGTHS for P2 in R.MASK_PS for p in R.MASK_PROBS)


def test_the_model_restatement_gradients_against_finite_differences_of_its_loss():
    """pretrain_grads is autograd through pretrain_losses: a central difference along a random direction agrees"""
    cfg = dict(R.TINY, B=2, L=8)
    p = R.tiny_params(cfg, seed=1)
    ids, seg, positions, labels, nsp = (torch.from_numpy(a) for a in R.tiny_masked(0, cfg))
    mlm, nsp_loss, grads = R.pretrain_grads(p, ids, seg, positions, labels, nsp, cfg["layers"], cfg["H"])
    g = torch.Generator().manual_seed(2)
    d = {k: torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in p.items()}
    h = 1e-6
    up = sum(R.pretrain_losses({k: v + h * d[k] for k, v in p.items()}, ids, seg, positions, labels, nsp, cfg["layers"], cfg["H"]))
    dn = sum(R.pretrain_losses({k: v - h * d[k] for k, v in p.items()}, ids, seg, positions, labels, nsp, cfg["layers"], cfg["H"]))
    want = float(sum((grads[k] * d[k]).sum() for k in p))
    assert abs(float(up - dn) / (2 * h) - want) <= 1e-6 * max(1.0, abs(want))
    assert float(grads["bert.embeddings.word_embeddings"].abs().max()) > 0 and abs(float(mlm) - math.log(cfg["V"])) < 0.5


def test_the_restatement_learns_the_tiny_task():
    cfg = R.TINY
    hist = R.tiny_training(cfg)
    uniform = math.log(cfg["V"] - cfg["num_special"])
    final = R.final_loss(hist)
    print("tiny task: masked-LM loss %.4f -> %.4f (mean of the last 10 of %d steps); uniform predictor %.4f, half of it %.4f"
          % (hist[0][0], final, cfg["steps"], uniform, 0.5 * uniform))
    assert final < 0.5 * uniform
