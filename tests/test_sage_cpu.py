"""CPU checks of GraphSAGE / PinSage: the surface imports, the header and the built library name the entry points, the wrappers
refuse what the kernels cannot take, and the NumPy restatements the GPU tests compare against (tests/sage_ref.py) have the properties
the specification promises -- among them that the specified key construction samples uniformly."""
import itertools

import numpy as np
import pytest
import torch

import sage_ref as R
from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.retrieval import GraphSAGE, PinSage, SAGEConv
from deep_recommenders_amd.layers import sample_blocks
from deep_recommenders_amd.ops import block_csr, frontier_build, neighbor_sample, walk_neighbors

ENTRY_POINTS = ("dr_neighbor_sample", "dr_walk_neighbors", "dr_frontier_build", "dr_block_csr")


def _graph(n=60, seed=0, hub=40):
    r = np.random.RandomState(seed)
    deg = r.randint(0, 12, size=n)
    deg[3], deg[7] = 0, hub
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate([np.sort(r.choice(n, size=d, replace=False)) for d in deg]).astype(np.int32)
    return row_ptr, col


def test_header_declares_and_library_exports_the_entry_points():
    import ctypes
    from deep_recommenders_amd import _lib
    sig = _lib.SIGNATURES
    assert [len(sig[n][1]) for n in ENTRY_POINTS] == [10, 9, 11, 13]
    assert sig["dr_neighbor_sample"][1][6] == ctypes.c_uint64 and sig["dr_frontier_workspace_bytes"][0] == ctypes.c_int64
    lib = _lib.lib()
    for name in ENTRY_POINTS + ("dr_frontier_workspace_bytes", "dr_block_csr_workspace_bytes"):
        assert getattr(lib, name) is not None
    assert lib.dr_frontier_workspace_bytes(-1, 0) == 0 and lib.dr_frontier_workspace_bytes(10, 100) >= 110 * (3 * 8 + 2 * 4)
    assert ops.SAMPLE_LONG_ROW == 512 and ops.SAMPLE_MAX_FANOUT == 64


def test_wrappers_refuse_what_the_kernels_cannot_take():
    rp, col = torch.zeros(5, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    nodes = torch.zeros(2, dtype=torch.int64)
    walks = torch.zeros((2, 3, 4), dtype=torch.int64)
    cnt, local = torch.zeros(2, dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int32)
    for bad in (lambda: neighbor_sample(rp, col, 4, nodes, 0, 0),                               # fanout out of range
                lambda: neighbor_sample(rp, col, 4, nodes, 65, 0),
                lambda: neighbor_sample(rp.int(), col, 4, nodes, 3, 0),                         # dtypes
                lambda: neighbor_sample(rp, col.long(), 4, nodes, 3, 0),
                lambda: neighbor_sample(rp, col, 4, nodes.int(), 3, 0),
                lambda: neighbor_sample(rp, col, 3, nodes, 3, 0),                               # row_ptr is [n_rows + 1]
                lambda: neighbor_sample(rp, col, 4, nodes.view(1, 2), 3, 0),                    # shapes
                lambda: walk_neighbors(walks, 0),
                lambda: walk_neighbors(walks, 65),
                lambda: walk_neighbors(walks.int(), 3),
                lambda: walk_neighbors(walks[0], 3),
                lambda: walk_neighbors(torch.zeros((1, 64, 18), dtype=torch.int64), 3),         # R (L - 1) = 1088
                lambda: frontier_build(nodes.int(), nodes),
                lambda: frontier_build(nodes, nodes.int()),
                lambda: frontier_build(nodes.view(2, 1), nodes),
                lambda: block_csr(cnt, local.long()),
                lambda: block_csr(cnt.long(), local),
                lambda: block_csr(cnt[:1], local),
                lambda: block_csr(cnt, local[0]),
                lambda: block_csr(cnt, torch.zeros((2, 65), dtype=torch.int32)),                # fanout out of range
                lambda: block_csr(cnt, local, weight=torch.zeros((2, 2))),
                lambda: block_csr(cnt, local, weight=torch.zeros((2, 3), dtype=torch.float64)),
                lambda: block_csr(cnt, local, n_valid=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            bad()


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rp, col = torch.zeros(5, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    nodes = torch.zeros(2, dtype=torch.int64)
    for call in (lambda: neighbor_sample(rp, col, 4, nodes, 3, 0),
                 lambda: walk_neighbors(torch.zeros((2, 3, 4), dtype=torch.int64), 2),
                 lambda: frontier_build(nodes, nodes),
                 lambda: block_csr(torch.zeros(2, dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int32))):
        with pytest.raises(RuntimeError):
            call()


def test_model_surface():
    conv = SAGEConv(8, aggregator="gcn", neighbor_units=4, activation="tanh", use_bias=False, name="c")
    assert conv.get_config() == {"name": "c", "units": 8, "aggregator": "gcn", "neighbor_units": 4, "use_bias": False, "activation": "tanh",
                                 "kernel_initializer": "truncated_normal", "bias_initializer": "zeros"}
    conv.build(6, device="cpu")
    assert conv.kernel.shape == (4, 8) and conv.neighbor_kernel.shape == (6, 4) and conv.self_kernel is None and conv.bias is None
    mean = SAGEConv(8)
    mean.build(6, device="cpu")
    assert mean.kernel.shape == mean.self_kernel.shape == (6, 8) and mean.bias.shape == (8,)
    m = GraphSAGE([16, 8], [5, 3], num_classes=7)
    assert len(m.convs) == 2 and m.get_config()["fanouts"] == [5, 3] and m.get_config()["importance"] is None
    p = PinSage([16, 8], [5, 3], num_walks=10, walk_length=4)
    assert isinstance(p, GraphSAGE) and p.get_config()["importance"] == {"num_walks": 10, "walk_length": 4}
    assert p.get_config()["neighbor_units"] == 16
    for bad in (lambda: SAGEConv(8, aggregator="lstm"), lambda: SAGEConv(8, activation="gelu")):
        with pytest.raises(NotImplementedError):
            bad()
    for bad in (lambda: GraphSAGE([16, 8], [5]), lambda: GraphSAGE([16], [65]), lambda: GraphSAGE([], []), lambda: SAGEConv(8, neighbor_units=0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        sample_blocks(np.eye(3), torch.zeros(2, dtype=torch.int64), [2], 0)
    assert L.sample_blocks is sample_blocks


def test_sample_ref_returns_short_rows_verbatim_and_subsets_of_long_ones():
    row_ptr, col = _graph()
    n_rows = row_ptr.size - 1
    nodes = np.asarray(list(range(n_rows)) + [-1, n_rows, 7, 7], dtype=np.int64)
    for fanout in (1, 5, 11, 64):
        nbr, cnt = R.neighbor_sample_ref(row_ptr, col, n_rows, nodes, fanout, seed=9)
        for i, v in enumerate(nodes.tolist()):
            if v < 0 or v >= n_rows:
                assert cnt[i] == 0 and (nbr[i] == -1).all()
                continue
            row = col[row_ptr[v]:row_ptr[v + 1]]
            assert cnt[i] == min(len(row), fanout) and (nbr[i, cnt[i]:] == -1).all()
            got = nbr[i, :cnt[i]]
            if len(row) <= fanout:
                assert np.array_equal(got, row)                            # verbatim, CSR order
            else:
                assert (np.diff(got) > 0).all() and set(got.tolist()) <= set(row.tolist())   # ascending (sorted rows), no repeats
        assert np.array_equal(nbr[-1], nbr[-2]) and np.array_equal(nbr[-1], nbr[7])   # a node's sample does not depend on its place
    a, _ = R.neighbor_sample_ref(row_ptr, col, n_rows, nodes, 5, seed=1)
    b, _ = R.neighbor_sample_ref(row_ptr, col, n_rows, nodes, 5, seed=2)
    assert not np.array_equal(a[7], b[7])


def test_specified_hash_samples_uniformly():
    """one row of degree 8, fanout 3, seeds 0 .. 4095: every edge is taken 1536 +- 155 times (5 binomial standard deviations of
    sqrt(4096 * 3/8 * 5/8) = 31) and all 56 subsets occur"""
    row_ptr, col = np.asarray([0, 8], np.int64), np.arange(8, dtype=np.int32)
    taken = np.zeros(8, dtype=np.int64)
    subsets = set()
    for seed in range(4096):
        nbr, cnt = R.neighbor_sample_ref(row_ptr, col, 1, np.zeros(1, np.int64), 3, seed)
        assert cnt[0] == 3
        taken[nbr[0]] += 1
        subsets.add(tuple(nbr[0].tolist()))
    assert (np.abs(taken - 1536) <= 155).all(), taken
    assert subsets == set(itertools.combinations(range(8), 3))


def test_walk_neighbors_ref_orders_by_count_then_id():
    walks = np.asarray([[[5, 2, 9, 5], [5, 9, 2, -1], [5, 7, 7, 7]],          # 7 x3, 2 x2, 9 x2 (the tie goes to the smaller id), 5 is the start
                        [[1, -1, -1, -1], [1, 1, 1, 1], [1, -1, -1, -1]]])       # only itself and dead ends
    nbr, weight, cnt = R.walk_neighbors_ref(walks, 4)
    assert nbr.tolist() == [[7, 2, 9, -1], [-1, -1, -1, -1]] and weight.tolist() == [[3, 2, 2, 0], [0, 0, 0, 0]] and cnt.tolist() == [3, 0]
    nbr, weight, cnt = R.walk_neighbors_ref(walks, 2)
    assert nbr.tolist() == [[7, 2], [-1, -1]] and cnt.tolist() == [2, 0]


def test_frontier_ref_round_trip():
    r = np.random.RandomState(3)
    dst = np.asarray([12, 40, 12, 7, 2 ** 40 + 5, -1, -1], dtype=np.int64)
    nbr = r.randint(0, 60, size=(5, 9)).astype(np.int64)
    nbr[r.rand(5, 9) < 0.2] = -1
    nbr[0, 0], nbr[1, 1], nbr[2, 2] = 12, 2 ** 40 + 5, 2 ** 40 + 1
    src, counts, local = R.frontier_build_ref(dst, nbr)
    assert counts[0] == 5 and np.array_equal(src[:5], dst[:5]) and (src[counts[1]:] == -1).all() and src.size == 7 + 45
    new = src[counts[0]:counts[1]]
    assert (np.diff(new) > 0).all() and not set(new.tolist()) & set(dst.tolist()) and new[-1] == 2 ** 40 + 1
    ok = nbr >= 0
    assert np.array_equal(src[local[ok]], nbr[ok]) and (local[~ok] == -1).all()
    assert local[0, 0] == 0 and local[1, 1] == 4                              # a repeated dst id: its lowest index
    assert set(new.tolist()) == set(nbr[ok].tolist()) - set(dst.tolist())
    # the output of one layer is a valid input of the next
    src2, counts2, _ = R.frontier_build_ref(src, np.full(3, -1, np.int64))
    assert counts2.tolist() == [counts[1], counts[1]] and np.array_equal(src2[:src.size], src)


def test_block_csr_ref_rows_sum_to_one():
    r = np.random.RandomState(4)
    n_dst, fanout = 40, 7
    cnt = r.randint(0, fanout + 1, size=n_dst).astype(np.int32)
    local = r.randint(0, 100, size=(n_dst, fanout)).astype(np.int32)
    weight = r.randint(1, 30, size=(n_dst, fanout)).astype(np.float32)
    for w, add_self in ((None, False), (None, True), (weight, False), (weight, True)):
        row_ptr, col, val = R.block_csr_ref(cnt, local, w, add_self, n_valid=35)
        assert row_ptr[0] == 0 and row_ptr[-1] == col.size == val.size
        for i in range(n_dst):
            a, b = row_ptr[i], row_ptr[i + 1]
            k = (cnt[i] + (1 if add_self else 0)) if i < 35 else 0
            assert b - a == k
            if k:
                assert abs(float(val[a:b].astype(np.float64).sum()) - 1.0) <= k * 2.0 ** -23        # 1 ulp of 1 per entry
                assert np.array_equal(col[a:b], ([i] if add_self else []) + local[i, :cnt[i]].tolist())
        if w is None and not add_self:
            i = int(np.flatnonzero(cnt[:35] > 0)[0])
            assert (val[row_ptr[i]:row_ptr[i + 1]] == np.float32(1.0) / np.float32(cnt[i])).all()
