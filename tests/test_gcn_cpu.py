"""GCN pieces that need no GPU: the Cora loader on a tiny cora-format fixture, the synthetic Cora-shaped graph, GCN.get_config and
the two branches of categorical_crossentropy's formula (restated here in float64)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from deep_recommenders_amd.datasets import Cora, synthetic_cora
from deep_recommenders_amd.datasets.cora import CORA_CLASSES
from deep_recommenders_amd.keras.models.retrieval import GCN

# 8 papers, 5 words, classes cycling through the first four; cites (cited, citing) with one duplicate pair in both directions
_IDS = [31, 7, 1002, 55, 600, 12, 90, 4]
_WORDS = [[1, 0, 1, 0, 0], [0, 1, 0, 0, 1], [1, 1, 1, 0, 0], [0, 0, 0, 1, 0], [1, 0, 0, 0, 1], [0, 1, 1, 1, 0], [1, 1, 0, 0, 0],
          [0, 0, 1, 1, 1]]
_CITES = [(31, 7), (7, 31), (1002, 55), (600, 12), (90, 4), (4, 31), (12, 1002)]


def _fixture(tmp_path):
    d = tmp_path / "cora"
    d.mkdir()
    with open(d / "cora.content", "w") as f:
        for i, (pid, w) in enumerate(zip(_IDS, _WORDS)):
            f.write("%d\t%s\t%s\n" % (pid, "\t".join(map(str, w)), CORA_CLASSES[i % 4]))
    with open(d / "cora.cites", "w") as f:
        for a, b in _CITES:
            f.write("%d\t%d\n" % (a, b))
    return str(tmp_path)


def test_cora_missing_files_raise_without_network(tmp_path, monkeypatch):
    import socket

    def no_net(*a, **k):
        raise AssertionError("Cora must not touch the network")
    monkeypatch.setattr(socket, "socket", no_net)
    with pytest.raises(FileNotFoundError, match="cora.tgz"):
        Cora(str(tmp_path))


def test_cora_load_content_normalises_rows(tmp_path):
    c = Cora(_fixture(tmp_path))
    ids, feats, labels = c.load_content()
    assert list(ids) == [str(i) for i in _IDS] and c.num_classes == 7
    assert sp.isspmatrix_csr(feats) and feats.dtype == np.float32
    w = np.array(_WORDS, dtype=np.float64)
    assert np.allclose(feats.toarray(), w / w.sum(1, keepdims=True), atol=1e-7)
    _, raw, _ = c.load_content(normalize=False)
    assert np.array_equal(raw.toarray(), w)
    assert list(labels) == [CORA_CLASSES[i % 4] for i in range(8)]


def test_cora_graph_is_symmetric_and_spectral_matches_formula(tmp_path):
    c = Cora(_fixture(tmp_path))
    ids, _, _ = c.load_content()
    g = c.build_graph(ids)
    A = g.toarray()
    assert np.array_equal(A, A.T)
    idx = {pid: i for i, pid in enumerate(_IDS)}
    assert A[idx[31], idx[7]] == 2            # cited both ways: graph + graph.T counts it twice, as the reference does
    assert A[idx[90], idx[4]] == 1 and A[idx[4], idx[90]] == 1 and A[idx[12], idx[1002]] == 1
    assert A[idx[31], idx[55]] == 0
    S = c.spectral_graph(g)
    assert sp.isspmatrix_csr(S)
    # the reference's formula on its own graph: (A + I) with the row sums of (A + I) -> D^-1/2 (A + I) D^-1/2
    AI = A.astype(np.float64) + np.eye(8)
    d = AI.sum(1) ** -0.5
    assert np.allclose(S.toarray(), d[:, None] * AI * d[None, :], atol=1e-12)


def test_cora_split_sizes_and_masks(tmp_path):
    # 20 per class needs >= 20 nodes per class: a synthetic graph of the real size
    path = synthetic_cora(str(tmp_path), num_nodes=400, num_features=50, num_edges=800, words_per_node=6, seed=1)
    c = Cora(path)
    ids, feats, labels = c.load_content()
    np.random.seed(3)
    (trl, trm), (val, vam), (tel, tem) = c.split_labels(labels, num_valid_nodes=100)
    assert trm.dtype == bool and trm.sum() == 20 * 7 and vam.sum() == 100 and tem.sum() == 400 - 140 - 100
    assert not (trm & vam).any() and not (trm & tem).any() and not (vam & tem).any()
    enc = c.encode_labels(labels)
    assert enc.dtype == np.int32 and np.array_equal(enc.sum(1), np.ones(400))
    assert np.array_equal(trl[trm], enc[trm]) and not trl[~trm].any()
    for k in range(7):
        assert trl[:, k].sum() == 20


def test_synthetic_cora_is_deterministic_and_cora_shaped(tmp_path):
    a = synthetic_cora(str(tmp_path / "a"), seed=5)
    b = synthetic_cora(str(tmp_path / "b"), seed=5)
    for f in ("cora.content", "cora.cites"):
        assert open(os.path.join(a, "cora", f)).read() == open(os.path.join(b, "cora", f)).read()
    c = Cora(a)
    ids, feats, labels = c.load_content()
    g = c.build_graph(ids)
    assert feats.shape == (2708, 1433) and len(set(labels)) == 7
    und = sp.triu(g, k=1).nnz
    assert 4500 <= und <= 5429, und
    other = synthetic_cora(str(tmp_path / "c"), seed=6)
    assert open(os.path.join(a, "cora", "cora.cites")).read() != open(os.path.join(other, "cora", "cora.cites")).read()


def test_gcn_get_config_keys():
    cfg = GCN(16, residual=True, use_bias=True, activation="softmax").get_config()
    assert set(cfg) == {"units", "use_bias", "activation", "kernel_initializer", "kernel_regularizer", "bias_initializer",
                        "bias_regularizer"}
    assert cfg["units"] == 16 and cfg["use_bias"] is True and cfg["activation"] == "softmax"
    assert cfg["kernel_initializer"] == "truncated_normal" and cfg["bias_initializer"] == "zeros"
    with pytest.raises(NotImplementedError):
        GCN(4, kernel_regularizer="l2")
    with pytest.raises(NotImplementedError):
        GCN(4, activation="elu")


def _cce_logits_f64(y, logits, w):
    z = logits - logits.max(1, keepdims=True)
    lse = np.log(np.exp(z).sum(1))
    ce = (y * (lse[:, None] - z)).sum(1)
    return (w * ce).sum() / len(y)


def _cce_prob_f64(y, p, w):
    q = np.clip(p / p.sum(1, keepdims=True), 1e-7, 1 - 1e-7)
    return (w * -(y * np.log(q)).sum(1)).sum() / len(y)


def test_categorical_crossentropy_formulas_float64():
    """Both branches' restatements against hand-computed values: a softmax output is scored from its logits unclipped (a row whose
    true-class probability underflows keeps a large loss), any other probability tensor is normalised and clipped at 1e-7; the
    weighted sum is divided by every row (SUM_OVER_BATCH_SIZE), weighted or not."""
    logits = np.array([[0.0, 0.0], [40.0, -40.0], [1.0, 2.0]])
    y = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 1.0]])
    w = np.array([1.0, 1.0, 0.0])
    want = (np.log(2.0) + (80.0 + np.log1p(np.exp(-80.0)))) / 3
    assert abs(_cce_logits_f64(y, logits, w) - want) < 1e-12
    p = np.exp(logits - logits.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    want_p = (np.log(2.0) - np.log(1e-7)) / 3
    assert abs(_cce_prob_f64(y, p, w) - want_p) < 1e-9
    # unnormalised probabilities are normalised first
    assert abs(_cce_prob_f64(y, 2 * p, w) - want_p) < 1e-9
