"""CPU checks of YoutubeNet's arithmetic and surface: the float64 restatement (tests/youtubenet_ref.py) against torch autograd, the
sampler's probabilities, the masking arithmetic, the library's symbols and workspace arithmetic, the model's argument errors."""
import ctypes
import math

import numpy as np
import pytest
import torch

import youtubenet_ref as R

DD = torch.float64


def _case(B=9, S=13, V=11, D=8, seed=0):
    rng = np.random.default_rng(seed)
    u = torch.from_numpy(rng.standard_normal((B, D))).to(DD) * 0.7
    table = torch.from_numpy(rng.standard_normal((V, D))).to(DD) * 0.7
    labels = torch.from_numpy(rng.integers(0, V, size=B))
    sampled = torch.from_numpy(rng.integers(0, V, size=S))
    sampled[S - 1] = -1
    lq_t = torch.from_numpy(rng.uniform(-3.0, -0.5, size=B)).to(DD)
    lq_s = torch.from_numpy(rng.uniform(-3.0, -0.5, size=S)).to(DD)
    w = torch.from_numpy(rng.uniform(0.5, 1.5, size=B)).to(DD)
    return u, table, labels, sampled, lq_t, lq_s, w


@pytest.mark.parametrize("rah", [True, False])
@pytest.mark.parametrize("extras", [True, False])
def test_hand_gradients_equal_autograd_of_the_dense_logits(rah, extras):
    u, table, labels, sampled, lq_t, lq_s, w = _case()
    if not extras:
        lq_t = lq_s = w = None
    assert (sampled[None, :] == labels[:, None]).any()                      # accidental hits are present
    scale = 1.0 / 7.0
    ua, ta = u.clone().requires_grad_(True), table.clone().requires_grad_(True)
    rows = R.dense_loss(ua, ta, labels, sampled, lq_t, lq_s, w, rah)
    (scale * rows.sum()).backward()
    h = R.hand_grads(u, table, labels, sampled, lq_t, lq_s, w, rah, scale)
    torch.testing.assert_close(h["loss"], rows.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(h["d_u"], ua.grad, rtol=1e-11, atol=1e-13)
    d_table = torch.zeros_like(table)
    d_table.index_add_(0, labels, h["d_true"])
    d_table.index_add_(0, sampled[sampled >= 0], h["d_sampled"][sampled >= 0])
    torch.testing.assert_close(d_table, ta.grad, rtol=1e-11, atol=1e-13)
    assert (h["d_sampled"][sampled < 0] == 0).all()
    step = R.sgd_step(table, labels, sampled, h["d_true"], h["d_sampled"], 0.5)
    torch.testing.assert_close(step, table - 0.5 * ta.grad, rtol=1e-11, atol=1e-13)


def test_padding_rows_reach_no_output():
    u, table, labels, sampled, lq_t, lq_s, w = _case()
    ref = R.hand_grads(u, table, labels, sampled, lq_t, lq_s, w, True, 1.0)
    labels2, u2 = labels.clone(), u.clone()
    labels2[2] = -1
    u2[2] = math.nan
    h = R.hand_grads(u2, table, labels2, sampled, lq_t, lq_s, w, True, 1.0)
    assert h["loss"][2] == 0 and (h["d_u"][2] == 0).all() and (h["d_true"][2] == 0).all()
    others = torch.arange(labels.shape[0]) != 2
    assert torch.equal(h["loss"][others], ref["loss"][others]) and torch.isfinite(h["d_sampled"]).all()
    torch.testing.assert_close(h["d_sampled"], ref["d_sampled"] - ref["G"][2][:, None] * u[2][None, :], rtol=1e-11, atol=1e-13)


def test_log_uniform_probabilities_sum_to_one_and_q_is_s_times_p():
    from deep_recommenders_amd.keras.models.retrieval import youtubenet as Y
    for V in (1, 37, 1000, 1_000_000):
        p = Y.log_uniform_probabilities(V)
        assert p.shape == (V,) and (p > 0).all() and (np.diff(p) < 0).all()
        assert abs(math.fsum(p.tolist()) - 1.0) <= 1e-12
        np.testing.assert_allclose(p, R.log_uniform(V).numpy(), rtol=1e-14, atol=0)
        for S in (1, 20, 8192):
            assert np.array_equal(Y.expected_counts(p, S), S * p)


def test_a_row_whose_every_sampled_id_is_its_label_has_loss_zero():
    u, table, labels, _, lq_t, lq_s, w = _case()
    labels = torch.full_like(labels, 4)
    sampled = torch.full((13,), 4, dtype=torch.int64)
    h = R.hand_grads(u, table, labels, sampled, lq_t, lq_s, w, True, 1.0)
    assert (h["loss"] == 0).all() and (h["d_u"] == 0).all() and (h["d_true"] == 0).all() and (h["d_sampled"] == 0).all()
    assert torch.equal(h["lse"], h["t"])


def test_leaving_an_entry_out_equals_adding_minus_flt_max_in_fp32():
    """TensorFlow adds -FLT_MAX to an accidental hit; beside the finite true logit its exp is 0 in fp32"""
    u, table, labels, sampled, lq_t, lq_s, w = (None if t is None else (t.float() if t.is_floating_point() else t) for t in _case())
    t, s, keep = R.logits(u, table, labels, sampled, lq_t, lq_s, False)          # the hits kept: finite scores
    hits = (sampled[None, :] == labels[:, None])
    assert hits.any() and s.dtype == torch.float32
    tf = s + torch.where(hits, torch.full_like(s, -R.FLT_MAX), torch.zeros_like(s))
    tf = tf.masked_fill((sampled < 0)[None, :].expand_as(tf), -math.inf)
    left_out = R.logits(u, table, labels, sampled, lq_t, lq_s, True)[1]
    a = torch.logsumexp(torch.cat([t[:, None], tf], 1), 1)
    b = torch.logsumexp(torch.cat([t[:, None], left_out], 1), 1)
    assert torch.equal(a, b)
    assert torch.equal(torch.softmax(torch.cat([t[:, None], tf], 1), 1), torch.softmax(torch.cat([t[:, None], left_out], 1), 1))


def test_library_exports_the_sampled_softmax_symbols():
    from deep_recommenders_amd import build, _lib
    L = ctypes.CDLL(build.build())
    for name in ("dr_sampled_softmax_fwd", "dr_sampled_softmax_bwd", "dr_sampled_softmax_workspace_bytes"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES


def test_workspace_holds_nothing_of_size_b_times_s():
    from deep_recommenders_amd import ops
    assert ops.sampled_softmax_workspace_bytes(65536, 8192, 256) <= 128 * 2 ** 20
    assert ops.sampled_softmax_workspace_bytes(8192, 8192, 256) <= 128 * 2 ** 20
    for B, S, D in ((1, 1, 4), (257, 257, 20), (8192, 8192, 256), (65536, 4096, 64), (65536, 8192, 256), (1 << 20, 1 << 16, 256)):
        groups, chunks = ops.sampled_softmax_col_groups(B, S, D), ops.sampled_softmax_row_chunks(B, S, D)
        assert 1 <= groups <= ops.SAMPLED_SOFTMAX_MAX_GROUPS <= 64 and 1 <= chunks <= ops.SAMPLED_SOFTMAX_MAX_CHUNKS <= 64
        # the (max, sum) pairs, the d_u partials of the split form, the d_sampled partials: linear in B and in S, never their product
        rows = B if groups > 1 else 0
        assert ops.sampled_softmax_workspace_bytes(B, S, D) <= 4 * (2 * 8 * B + 16 + groups * rows * D + chunks * S * D)
    assert ops.sampled_softmax_col_groups(257, 2 * ops.SAMPLED_SOFTMAX_COL_GROUP + 1, 20) == 3
    assert ops.sampled_softmax_row_chunks(2 * ops.SAMPLED_SOFTMAX_ROW_CHUNK + 1, 257, 20) == 3
    assert ops.sampled_softmax_col_groups(64 * ops.SAMPLED_SOFTMAX_SPLIT_TILES + 1, 257, 4) == 1
    for bad in ((8, 8, 6), (8, 8, 260), (8, 0, 8), (-1, 8, 8), (8, 2 ** 31, 8)):
        with pytest.raises(ValueError):
            ops.sampled_softmax_workspace_bytes(*bad)


def test_model_argument_errors_come_before_the_device():
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.keras.models.retrieval import YoutubeNet
    cols = [fc.embedding_column(fc.categorical_column_with_identity("history", 50), 8)]
    good = dict(embedding_columns=cols, num_classes=40, dnn_units_size=[32, 16], num_sampled=8)
    for change, match in ((dict(dnn_units_size=[32, 18]), "multiple of 4"), (dict(dnn_units_size=[32, 260]), r"\[4, 256\]"),
                          (dict(dnn_units_size=[]), "dnn_units_size"), (dict(num_sampled=0), "num_sampled"),
                          (dict(class_counts=np.ones(39)), "class_counts"), (dict(num_classes=0), "num_classes"),
                          (dict(activation="gelu"), "activation")):
        with pytest.raises(ValueError, match=match):
            YoutubeNet(**{**good, **change})
