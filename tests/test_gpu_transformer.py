"""MultiHeadAttention and Transformer on the device against the float64 restatement of tests/transformer_ref.py with injected
weights, the reference test's shape, and the example as a subprocess.

Model-level tolerances: a bound through several LayerNormalizations is not derived here; every tensor is compared relative to the
max-norm of its float64 value, with four times the error the fp32 restatement on the CPU (torch, same formulas, same dropout
masks) shows against float64 on the same inputs, plus the fp32 rounding of the stored result itself (2^-23 of the max-norm).
Every element of every tensor is compared."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import transformer_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=["native", "bf16x3"])
def gemm_mode(request):
    """the projections and the feed-forward are the library's dense GEMM, whose product mode is process-wide: both are covered"""
    from deep_recommenders_amd import ops
    old = ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(old)


def _compare(name, got, want, f32):
    got = np.asarray(got, dtype=np.float64)
    scale = float(np.abs(want).max())
    assert got.shape == want.shape and np.isfinite(got).all(), name
    yard = float(np.abs(f32 - want).max())
    err = float(np.abs(got - want).max())
    tol = 4 * yard + 2 * U * scale
    print("%s: max err %.3g, fp32-CPU yardstick %.3g, max-norm %.3g, err / tol %.3g" % (name, err, yard, scale, err / (tol + 1e-300)))
    return None if err <= tol else "%s: err %g tol %g" % (name, err, tol)


def _prepadded_ids(rng, B, L, V, lengths):
    ids = np.zeros((B, L), dtype=np.int64)
    for b, n in enumerate(lengths):
        if n:
            ids[b, L - n:] = rng.integers(1, V, size=n)
    return ids


@pytest.mark.parametrize("masking", [True, False])
@pytest.mark.parametrize("future", [False, True])
@pytest.mark.parametrize("rate", [0.0, 0.1])
def test_multi_head_attention_against_float64(gemm_mode, masking, future, rate):
    from deep_recommenders_amd.keras.models.nlp import MultiHeadAttention
    rng = np.random.default_rng(11 + 2 * masking + future)
    B, L, Din, H, dh = 3, 19, 6, 2, 4
    x = rng.standard_normal((B, L, Din)).astype(np.float32)
    d_out = rng.standard_normal((B, L, H * dh)).astype(np.float32)
    mask = np.zeros((B, L), dtype=bool)
    mask[0, :] = True
    mask[1, :7] = True
    layer = MultiHeadAttention(H, dh, dropout_rate=rate, masking=masking, future=future, seed=5)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    inputs = [xd, xd, xd] + ([torch.from_numpy(mask).cuda()] if masking else [])
    out = layer(inputs)
    names = ("_weights_queries", "_weights_keys", "_weights_values")
    assert [n for n, _ in layer.named_parameters()] == list(names)                      # three bias-free projections, no output projection
    with torch.no_grad():
        for n in names:
            getattr(layer, n).copy_(torch.from_numpy(rng.standard_normal((Din, H * dh)).astype(np.float32) * 0.6))
    first_seed = layer.last_seed
    out = layer(inputs)
    assert layer.last_seed != first_seed                                                # a fresh mask on every call
    out.backward(torch.from_numpy(d_out).cuda())
    keep = R.keep_mask(layer.last_seed, rate, (B, H, L, L)) if rate > 0 else None
    w = {n: getattr(layer, n).detach().cpu().numpy() for n in names}

    def oracle(dtype):
        tx = torch.from_numpy(x).to(dtype).requires_grad_(True)
        tw = [torch.from_numpy(w[n]).to(dtype).requires_grad_(True) for n in names]
        o = R.multi_head_attention(tx, tx, tx, *tw, H, mask if masking else None, future, keep, rate, dtype)
        o.backward(torch.from_numpy(d_out).to(dtype))
        return [t.detach().double().numpy() for t in [o, tx.grad] + [t.grad for t in tw]]
    want, f32 = oracle(torch.float64), oracle(torch.float32)
    got = [out.detach().cpu().numpy(), xd.grad.cpu().numpy()] + [getattr(layer, n).grad.cpu().numpy() for n in names]
    missed = []
    for what, g, wv, f in zip(("out", "d_inputs") + names, got, want, f32):
        missed.append(_compare("mha %s masking=%d future=%d rate=%g %s" % (gemm_mode, masking, future, rate, what), g, wv, f))
    assert not any(missed), [m for m in missed if m]
    frozen = MultiHeadAttention(H, dh, trainable=False)
    frozen(inputs if masking else inputs + [torch.from_numpy(mask).cuda()])
    assert not any(p.requires_grad for p in frozen.parameters())


@pytest.mark.parametrize("with_dropout", [False, True])
def test_transformer_against_float64(gemm_mode, with_dropout):
    """Output and the gradient of EVERY parameter of a 2 + 2-stack Transformer on pre-padded ids against float64, the tied
    embedding as one tensor; once with all rates 0 and once with the restated dropout masks."""
    from deep_recommenders_amd.keras.models.nlp import MultiHeadAttention, Transformer
    rng = np.random.default_rng(21)
    V, D, H, B, L, F = 50, 8, 2, 4, 16, 12
    enc_ids = _prepadded_ids(rng, B, L, V, [L, 9, 0, 3])                 # full, partial, an empty sequence, a short one
    dec_ids = _prepadded_ids(rng, B, L, V, [5, L, 7, 0])
    model = Transformer(V, D, n_heads=H, encoder_stack=2, decoder_stack=2, feed_forward_size=F, dropout_rate=0.1 if with_dropout else 0.0,
                        seed=3)
    model.build("cuda")
    mhas = [m for m in model.modules() if isinstance(m, MultiHeadAttention)]
    assert len(mhas) == 6 and all(m._dropout_rate == 0.1 for m in mhas)   # their own default, whatever the Transformer's rate
    if not with_dropout:
        for m in mhas:
            m._dropout_rate = 0.0
    with torch.no_grad():                                                 # injected weights: nothing at its initial 1 / 0
        for name, p in model.named_parameters():
            base = 1.0 if name.endswith("gamma") else 0.0
            p.copy_(torch.from_numpy((base + 0.4 * rng.standard_normal(tuple(p.shape))).astype(np.float32)))
    d_out = rng.standard_normal((B, L, V)).astype(np.float32)
    out = model(torch.from_numpy(enc_ids).cuda(), torch.from_numpy(dec_ids).cuda())
    out.backward(torch.from_numpy(d_out).cuda())
    params = {n: p.detach().cpu().numpy() for n, p in model.named_parameters()}
    assert "embeddings" in params and len(params) == 1 + 6 * 3 + 10 * 2 + 4 * 4
    keeps = None
    if with_dropout:
        keeps = {"att_rate": 0.1, "enc_emb": R.keep_mask(model.last_seeds[0], 0.1, (B, L, D)),
                 "dec_emb": R.keep_mask(model.last_seeds[1], 0.1, (B, L, D))}
        for key, mods in (("enc", model.EncoderMultiHeadAttentions), ("dec0", model.DecoderMultiHeadAttentions0),
                          ("dec1", model.DecoderMultiHeadAttentions1)):
            for i, m in enumerate(mods):
                keeps["%s.%d" % (key, i)] = R.keep_mask(m.last_seed, 0.1, (B, H, L, L))

    def oracle(dtype):
        P = {n: torch.from_numpy(a).to(dtype).requires_grad_(True) for n, a in params.items()}
        o = R.transformer(P, model.get_config(), enc_ids, dec_ids, keeps, dtype)
        o.backward(torch.from_numpy(d_out).to(dtype))
        return o.detach().double().numpy(), {n: t.grad.double().numpy() for n, t in P.items()}
    (want, gwant), (f32, gf32) = oracle(torch.float64), oracle(torch.float32)
    tag = "transformer %s dropout=%d " % (gemm_mode, with_dropout)
    missed = [_compare(tag + "out", out.detach().cpu().numpy(), want, f32)]
    np.testing.assert_allclose(out.detach().cpu().numpy().sum(-1), 1.0, rtol=0, atol=(V + 8) * U)
    for n, p in model.named_parameters():                                 # every parameter; the tied embedding as ONE tensor
        assert p.grad is not None, n
        missed.append(_compare(tag + n, p.grad.cpu().numpy(), gwant[n], gf32[n]))
    assert not any(missed), [m for m in missed if m]
    # bit-reproducible: the same seeds give the same bits, gradients included
    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    model.reset_calls()
    out2 = model(torch.from_numpy(enc_ids).cuda(), torch.from_numpy(dec_ids).cuda())
    out2.backward(torch.from_numpy(d_out).cuda())
    assert torch.equal(out, out2) and all(torch.equal(grads[n], p.grad) for n, p in model.named_parameters())
    if with_dropout:
        out3 = model(torch.from_numpy(enc_ids).cuda(), torch.from_numpy(dec_ids).cuda())     # the next call draws other masks
        assert not torch.equal(out, out3)


def test_reference_test_shape_and_config_round_trip():
    """the shape of the reference's transformer test: Transformer(5000, 8, n_heads=2, encoder_stack=2, decoder_stack=2,
    feed_forward_size=50) on (10, 256) random ids -> pooling -> Dense(1, sigmoid)"""
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd.keras.models.nlp import Transformer
    rng = np.random.default_rng(4)
    ids = torch.from_numpy(rng.integers(0, 5000, size=(10, 256))).cuda()
    torch.manual_seed(0)
    model = Transformer(5000, 8, n_heads=2, encoder_stack=2, decoder_stack=2, feed_forward_size=50, seed=9)
    out = model(ids, ids).detach()
    assert out.shape == (10, 256, 5000) and torch.isfinite(out).all()
    sums = out.double().sum(-1).cpu().numpy()
    assert np.abs(sums - 1.0).max() <= (5000 / 64 + 16) * U * 4, np.abs(sums - 1.0).max()      # one wave per row: 79 chained adds + butterfly
    kernel = torch.from_numpy(rng.standard_normal((5000, 1)).astype(np.float32)).cuda()
    bias = torch.zeros(1, dtype=torch.float32, device="cuda")
    pooled = L.global_average_pooling_1d(out)
    np.testing.assert_allclose(pooled.cpu().numpy(), out.double().mean(1).cpu().numpy(), rtol=0, atol=300 * U * float(out.max()))
    pred = L.mlp(pooled, [kernel], [bias], [2])
    assert pred.shape == (10, 1) and torch.isfinite(pred).all() and (pred > 0).all() and (pred < 1).all()
    # a model rebuilt from get_config() + state_dict() predicts the same bits under the same seeds
    clone = Transformer(**model.get_config())
    clone.build("cuda")
    clone.load_state_dict(model.state_dict())
    model.reset_calls()
    a = model(ids, ids)
    b = clone(ids, ids)
    assert torch.equal(a, b) and torch.equal(a, out)


def test_example_trains_on_its_synthetic_set():
    """examples/train_transformer_on_imdb_keras.py as a subprocess on its synthetic set (its defaults: 4096 training sequences, 10 epochs): the
    training loss falls and the test accuracy ends above chance.

    Observed on an MI355X (seed 0): training loss 0.6929 (epoch 1) -> 0.5543 (epoch 10), validation accuracy 0.9658, test
    accuracy 0.9326, 0.2 s per epoch.  The margin asked of the test accuracy is half of the way from chance to 1."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_transformer_on_imdb_keras.py"), "--epochs", "10"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=420, cwd=ROOT)
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stderr[-3000:]
    assert "synthetic" in res.stdout
    losses = [float(m) for m in re.findall(r" - loss: ([0-9.]+)", res.stdout)]
    acc = float(re.search(r"accu on Test: ([0-9.]+)", res.stdout).group(1))
    assert 2 <= len(losses) <= 10 and losses[-1] < losses[0], losses
    assert acc > 0.5 + 0.25, acc
