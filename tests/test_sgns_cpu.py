"""CPU checks of the skip-gram restatements the GPU tests compare against (tests/sgns_ref.py) and of the host side of the feature:
ops.alias_table, layers.skipgram_pairs, the wrappers' argument checks and the models' configuration surface."""
import json
import os

import numpy as np
import pytest
import torch

import sgns_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHTS = [1, 2, 3, 4, 0, 10, 0.5]


def _case(B=9, K=5, V=13, D=12, seed=0):
    g = torch.Generator().manual_seed(seed)
    tin = torch.randn(V, D, generator=g, dtype=torch.float64)
    tout = torch.randn(V, D, generator=g, dtype=torch.float64)
    centers = torch.randint(0, V, (B,), generator=g)
    contexts = torch.randint(0, V, (B,), generator=g)
    negatives = torch.randint(0, V, (B, K), generator=g)
    centers[1], contexts[2], negatives[3, 1] = -1, -1, -1
    negatives[4, 0] = contexts[4]
    w = torch.rand(B, generator=g, dtype=torch.float64) + 0.5
    return tin, tout, centers, contexts, negatives, w


@pytest.mark.parametrize("skip_equal", [True, False])
def test_hand_written_gradient_equals_autograd(skip_equal):
    tin, tout, centers, contexts, negatives, w = _case()
    tin.requires_grad_(True)
    tout.requires_grad_(True)
    d_loss = torch.rand(len(centers), dtype=torch.float64) + 0.1
    loss, _, keep = R.loss_expr(tin, tout, centers, contexts, negatives, w, skip_equal)
    (loss * d_loss).sum().backward()
    g, d_center, d_ctx, _, _ = R.hand_grads(tin.detach(), tout.detach(), centers, contexts, negatives, d_loss, w, skip_equal)
    ids, keep2 = R.masks(centers, contexts, negatives, skip_equal)
    assert torch.equal(keep, keep2)
    g_in, g_out = R.table_grads(tin.shape[0], tout.shape[0], centers, torch.where(keep, ids, torch.full_like(ids, -1)), keep, d_center, d_ctx)
    for got, want in ((g_in, tin.grad), (g_out, tout.grad)):
        assert (got - want).abs().max() <= 1e-13 * want.abs().max()
    loss = loss.detach()
    assert float(loss[1]) == 0.0 and float(loss[2]) == 0.0 and not keep[1].any() and not keep[2].any()
    assert not keep[3, 2] and bool(keep[4, 1]) != skip_equal
    assert (g[~keep] == 0).all() and (d_ctx[~keep] == 0).all()


def test_mix32_restatement_equals_the_pinned_hash():
    """the values tests/golden/transformer_kats.json fixes for dr_mix32 (the dropout tests' pins), and the dropout reference's own
    restatement on a few hundred (seed, index) pairs"""
    import transformer_ref as T
    kats = json.load(open(os.path.join(HERE, "golden", "transformer_kats.json")))["mix32"]
    assert len(kats) >= 4
    for k in kats:
        assert int(R.mix32(k["seed"], np.asarray([k["idx"]], dtype=np.uint64))[0]) == k["hash"]
    rng = np.random.default_rng(0)
    idx = rng.integers(0, 2 ** 63, size=300, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    for seed in (0, 1, 12345, 2 ** 64 - 1):
        assert np.array_equal(R.mix32(seed, idx), T.mix32(seed, idx).astype(np.uint32))


def test_alias_table_implies_the_distribution():
    from deep_recommenders_amd import ops
    prob, alias = ops.alias_table(WEIGHTS)
    assert prob.dtype == np.float32 and alias.dtype == np.int32 and prob.shape == alias.shape == (7,)
    want = np.asarray(WEIGHTS, dtype=np.float64) / np.sum(WEIGHTS)
    assert np.abs(R.alias_distribution(prob, alias) - want).max() <= 1e-6
    assert prob[4] == 0.0 and 4 not in alias.tolist()
    uniform = ops.alias_table(np.ones(5))
    assert (uniform[0] == 1.0).all()
    for bad in ([], [0.0, 0.0], [1.0, -1.0], [1.0, float("nan")]):
        with pytest.raises(ValueError):
            ops.alias_table(bad)


def test_reference_draws_follow_the_table():
    from deep_recommenders_amd import ops
    prob, alias = ops.alias_table(WEIGHTS)
    n = 2 ** 20
    draws = R.alias_sample_ref(prob, alias, n, seed=7)
    counts = np.bincount(draws, minlength=7)
    p = np.asarray(WEIGHTS, dtype=np.float64) / np.sum(WEIGHTS)
    sd = np.sqrt(n * p * (1 - p))
    assert counts[4] == 0
    assert (np.abs(counts - n * p) <= 5 * sd).all(), (counts, n * p, sd)
    both = R.alias_sample_ref(prob, alias, 2000, seed=7)
    assert np.array_equal(both[1000:], R.alias_sample_ref(prob, alias, 1000, seed=7, offset=1000))


def test_skipgram_pairs_equals_the_double_loop():
    from deep_recommenders_amd import layers as L
    seqs = torch.tensor([[3, 1, 4, 1, 5], [9, 2, -1, -1, -1], [6, -1, 5, 3, -1]], dtype=torch.int64)
    for window in (1, 2, 6):
        centers, contexts = L.skipgram_pairs(seqs, window)
        want_c, want_o = R.skipgram_pairs_loops(seqs.tolist(), window)
        assert centers.shape == contexts.shape == (3 * 5 * 2 * window,)
        assert centers.tolist() == want_c and contexts.tolist() == want_o
    with pytest.raises(ValueError):
        L.skipgram_pairs(seqs, 0)
    with pytest.raises(ValueError):
        L.skipgram_pairs(seqs.float(), 1)


def test_random_walk_ref_walks_along_edges():
    row_ptr, col = R.six_node_graph()
    edges = {(i, int(j)) for i in range(6) for j in col[row_ptr[i]:row_ptr[i + 1]]}
    starts = np.asarray([0, 1, 2, 3, 4, 5, -1, 6] * 8, dtype=np.int64)
    walks = R.random_walk_ref(row_ptr, col, 6, starts, 12, seed=3)
    assert np.array_equal(walks[:, 0], starts)
    for w in walks:
        if w[0] in (5, -1, 6):                                 # the isolated node, a missing start, a start outside the graph
            assert (w[1:] == -1).all()
            continue
        assert all((int(a), int(b)) in edges for a, b in zip(w[:-1], w[1:]))
    assert len({tuple(w) for w in walks[starts == 2]}) > 1       # walks from one start differ: the hash is per walk
    row_ptr, col = R.dead_end_graph()
    walks = R.random_walk_ref(row_ptr, col, 4, np.asarray([3, 0, 1, 2]), 6, seed=1)
    assert walks.tolist() == [[3, 0, 1, 2, -1, -1], [0, 1, 2, -1, -1, -1], [1, 2, -1, -1, -1, -1], [2, -1, -1, -1, -1, -1]]


def test_no_cpu_fallback():
    from deep_recommenders_amd import ops
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    z = torch.zeros(5, 8)
    i = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ops.sgns_fwd(z, z, i, i, torch.zeros((2, 3), dtype=torch.int64))
    with pytest.raises(RuntimeError):
        ops.sgns_bwd(z, z, i, i, torch.zeros((2, 3), dtype=torch.int64), torch.zeros(2, 4), torch.zeros(2))
    with pytest.raises(RuntimeError):
        ops.alias_sample(torch.ones(4), torch.arange(4, dtype=torch.int32), 8, 0)
    with pytest.raises(RuntimeError):
        ops.random_walk(torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 2, i, 3, 0)


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from deep_recommenders_amd import ops
    i = torch.zeros(2, dtype=torch.int64)
    neg = torch.zeros((2, 3), dtype=torch.int64)

    def z(*shape):
        return torch.zeros(shape)
    for bad in (lambda: ops.sgns_fwd(z(5, 6), z(5, 6), i, i, neg),                              # D % 4
                lambda: ops.sgns_fwd(z(5, 260), z(5, 260), i, i, neg),                          # D > 256
                lambda: ops.sgns_fwd(z(5, 8), z(5, 12), i, i, neg),                             # two widths
                lambda: ops.sgns_fwd(z(5, 8), z(5, 8), i, i, torch.zeros((2, 64), dtype=torch.int64)),   # K > 63
                lambda: ops.sgns_fwd(z(5, 8), z(5, 8), i, i.int(), neg),
                lambda: ops.sgns_fwd(z(5, 8), z(5, 8), i, i, neg[:1]),
                lambda: ops.sgns_fwd(z(5, 16)[:, :8], z(5, 8), i, i, neg),                      # a table that is a view
                lambda: ops.sgns_fwd(z(5, 8), z(5, 8), i, i, neg, sample_weight=z(3)),
                lambda: ops.sgns_fwd(z(5, 8), z(5, 8), i, i, neg, d_center=z(2, 8)),            # buffers without row_scale
                lambda: ops.sgns_fwd(z(5, 8), z(5, 8), i, i, neg, row_scale=1.0, d_ctx=z(2, 40)[:, :32:1][:, :30]),
                lambda: ops.sgns_fwd(z(5, 8), z(5, 8), i, i, neg, row_scale=1.0, d_ctx=z(4, 32)[::2, :].t().contiguous().t()),
                lambda: ops.sgns_fwd(z(5, 8), z(5, 8), i, i, neg, row_scale=1.0, d_center=z(2, 6, 2)[:, :, 0].expand(2, 6)),
                lambda: ops.sgns_bwd(z(5, 8), z(5, 8), i, i, neg, z(2, 3), z(2)),               # coeff is [B, 1 + K]
                lambda: ops.sgns_bwd(z(5, 8), z(5, 8), i, i, neg, z(2, 4), z(3)),
                lambda: ops.sgns_bwd(z(5, 8), z(5, 8), i, i, neg, z(2, 4), z(2), d_ctx=z(2, 64)[:, ::2]),   # a leading dimension < width
                lambda: ops.alias_sample(torch.ones(4), torch.arange(3, dtype=torch.int32), 8, 0),
                lambda: ops.alias_sample(torch.ones(4), torch.arange(4), 8, 0),
                lambda: ops.alias_sample(torch.ones(4), torch.arange(4, dtype=torch.int32), -1, 0),
                lambda: ops.random_walk(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 2, i, 3, 0),
                lambda: ops.random_walk(torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 2, i, 0, 0),
                lambda: ops.random_walk(torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 2, i, 3, 0)):
        with pytest.raises(ValueError):
            bad()


def test_header_declares_the_four_entry_points():
    from deep_recommenders_amd import _lib
    sig = _lib.SIGNATURES
    assert [len(sig[n][1]) for n in ("dr_sgns_fwd", "dr_sgns_bwd", "dr_alias_sample", "dr_random_walk")] == [19, 16, 8, 9]
    import ctypes
    assert sig["dr_sgns_fwd"][1][10] == ctypes.c_float and sig["dr_alias_sample"][1][4] == ctypes.c_uint64


def test_model_configuration_surface():
    from deep_recommenders_amd.keras.models.nlp import Word2Vec
    from deep_recommenders_amd.keras.models.retrieval import DeepWalk, Item2Vec, SkipGram
    assert Item2Vec is SkipGram and issubclass(Word2Vec, SkipGram) and issubclass(DeepWalk, SkipGram)
    torch.manual_seed(0)
    m = SkipGram(50, 16, num_negatives=3, counts=np.arange(50), device="cpu")
    assert m.in_table.shape == m.out_table.shape == (50, 16) and m.embeddings() is m.in_table
    t = m.in_table.detach()
    assert float(t.abs().max()) <= 2.0 / 4.0 + 1e-6 and 0.15 < float(t.std()) < 0.3                        # truncated at 2 sigma, sigma 1/4
    assert float(m.alias_prob[0]) == 0.0                           # count 0: never drawn
    assert (SkipGram(5, 8, device="cpu").alias_prob == 1).all()
    for bad in (lambda: SkipGram(5, 6, device="cpu"), lambda: SkipGram(5, 260, device="cpu"), lambda: SkipGram(5, 8, 64, device="cpu"),
                lambda: SkipGram(5, 8, counts=[1, 2], device="cpu"), lambda: SkipGram(0, 8, device="cpu")):
        with pytest.raises(ValueError):
            bad()
    row_ptr, col = R.six_node_graph()
    idx = [(i, int(j)) for i in range(6) for j in col[row_ptr[i]:row_ptr[i + 1]]]
    dw = DeepWalk((idx, np.ones(len(idx)), (6, 6)), 8, walk_length=4, window=2, num_negatives=2, device="cpu")
    assert dw.num_items == 6 and float(dw.alias_prob[5]) == 0.0    # the isolated node is no negative
    with pytest.raises(ValueError):
        DeepWalk((idx, np.ones(len(idx)), (6, 6)), 8, walk_length=1, window=2, device="cpu")
    with pytest.raises(TypeError):
        DeepWalk(np.eye(6), 8, walk_length=4, window=2, device="cpu")
