"""Multi-task learning pieces that need no GPU: numeric_column, the input_layer layout, the synthetic multi-task dataset."""
import numpy as np
import pytest
import torch

from deep_recommenders_amd import feature_column as fc
from deep_recommenders_amd.datasets import SyntheticForMultiTask


def test_numeric_column_attributes():
    c = fc.numeric_column("price")
    assert c.name == "price" and c.key == "price" and c.shape == (1,) and c.default_value is None
    assert c.dtype == torch.float32 and c.normalizer_fn is None and c.width == 1
    c2 = fc.numeric_column("v", shape=(2, 3), default_value=0.5, normalizer_fn=lambda x: x * 2)
    assert c2.shape == (2, 3) and c2.width == 6 and c2.variable_shape == (2, 3)
    assert np.array_equal(c2.host_block({"v": np.ones((4, 2, 3))}), np.full((4, 6), 2.0, np.float32))
    assert np.array_equal(c2.host_block({}, batch_size=2), np.full((2, 6), 1.0, np.float32))
    with pytest.raises(ValueError):
        fc.numeric_column("bad", shape=(0,))
    with pytest.raises(KeyError):
        fc.numeric_column("x").host_block({}, batch_size=3)


def test_input_layer_layout_is_name_sorted():
    cols = [fc.numeric_column("C{}".format(i)) for i in range(256)]
    layout, K = fc.input_layer_layout(cols)
    names = [n for n, _, _, _ in layout]
    assert names[:6] == ["C0", "C1", "C10", "C100", "C101", "C102"]
    assert names == sorted("C{}".format(i) for i in range(256))
    assert [off for _, _, off, _ in layout] == list(range(256)) and K == 256


def test_input_layer_layout_interleaves_embedding_and_numeric_by_name():
    e_b = fc.embedding_column(fc.categorical_column_with_identity("b", 10), 8)      # name "b_embedding"
    e_z = fc.embedding_column(fc.categorical_column_with_hash_bucket("z", 100), 4)   # "z_embedding"
    cols = [e_z, fc.numeric_column("c", shape=(3,)), e_b, fc.numeric_column("a"), fc.numeric_column("y")]
    layout, K = fc.input_layer_layout(cols)
    assert [(n, off, w) for n, _, off, w in layout] == [("a", 0, 1), ("b_embedding", 1, 8), ("c", 9, 3), ("y", 12, 1),
                                                        ("z_embedding", 13, 4)]
    assert K == 17


def test_input_layer_layout_rejects_indicator_columns():
    with pytest.raises(NotImplementedError):
        fc.input_layer_layout([fc.indicator_column(fc.categorical_column_with_identity("a", 3))])


@pytest.mark.parametrize("example_dim", [16, 64, 256, 1024])
def test_synthetic_feature_and_label_keys(example_dim):
    feats, labels = next(SyntheticForMultiTask(1000, example_dim=example_dim, seed=0).input_fn())
    assert sorted(feats) == sorted("C{}".format(i) for i in range(example_dim))
    assert sorted(labels) == ["labels0", "labels1"]


@pytest.mark.parametrize("batch_size", [16, 64, 256, 512])
def test_synthetic_batch_shapes(batch_size):
    feats, labels = next(SyntheticForMultiTask(1000, example_dim=100, seed=0).input_fn(batch_size=batch_size))
    assert feats["C0"].shape == (batch_size, 1) and feats["C0"].dtype == np.float32
    assert labels["labels0"].shape == (batch_size,) and labels["labels1"].shape == (batch_size,)


def test_synthetic_keeps_last_partial_batch_and_repeats():
    batches = list(SyntheticForMultiTask(1000, example_dim=8, seed=0).input_fn(epochs=2, batch_size=300))
    assert [b[0]["C0"].shape[0] for b in batches] == [300, 300, 300, 100] * 2


def test_synthetic_same_seed_same_data():
    a = SyntheticForMultiTask(500, example_dim=32, seed=11).data()
    b = SyntheticForMultiTask(500, example_dim=32, seed=11).data()
    c = SyntheticForMultiTask(500, example_dim=32, seed=12).data()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1])
    assert not np.array_equal(a[0], c[0])


def test_synthetic_task_correlation():
    """the two label weight vectors have cosine p (restated generator)"""
    from deep_recommenders_amd.datasets.synthetic_for_multi_task import synthetic_data
    x, (y0, y1) = synthetic_data(20000, 50, c=0.3, p=0.8, m=0, rng=np.random.RandomState(0))
    w0, *_ = np.linalg.lstsq(x, y0, rcond=None)
    w1, *_ = np.linalg.lstsq(x, y1, rcond=None)
    cos = w0 @ w1 / np.linalg.norm(w0) / np.linalg.norm(w1)
    assert abs(cos - 0.8) < 0.02
