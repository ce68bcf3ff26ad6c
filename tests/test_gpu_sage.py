"""GraphSAGE / PinSage on the GPU: the four sampled-block kernels bit for bit against their NumPy restatements (tests/sage_ref.py),
the layers against a float64 torch composition on the densified blocks (bounds: those of tests/test_gpu_gcn.py's layer test), and
the example's model for 20 steps."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import sage_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FANOUTS = [1, 5, 25, 64]


@pytest.fixture(scope="module", autouse=True)
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------------------------
# dr_neighbor_sample
# ------------------------------------------------------------------------------------------------------------------------------
def _special_degrees():
    from deep_recommenders_amd import ops
    S = ops.SAMPLE_LONG_ROW
    deg = [20000, 0, 1, 63, 64, 65, 513, S - 1, S, S + 1]
    for f in FANOUTS:
        deg += [max(f - 1, 0), f, f + 1]
    return deg


@pytest.fixture(scope="module")
def sample_graph():
    """a few hundred short rows and, in front, the degrees at which the kernel changes its path; neighbour ids up to 50 000"""
    r = np.random.RandomState(0)
    deg = np.asarray(_special_degrees() + r.randint(0, 40, size=300).tolist(), dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate([np.sort(r.choice(50_000, size=d, replace=False)) for d in deg]).astype(np.int32)
    n_rows = deg.size
    nodes = np.concatenate([np.arange(n_rows), [-1, n_rows, 0, 0, 5, n_rows + 7, -1], r.randint(0, n_rows, size=1000)])[:1000].astype(np.int64)
    assert n_rows + 7 <= 1000
    return row_ptr, col, n_rows, nodes, {}


def _sample_ref(g, fanout, seed):
    row_ptr, col, n_rows, nodes, cache = g
    if (fanout, seed) not in cache:
        cache[(fanout, seed)] = R.neighbor_sample_ref(row_ptr, col, n_rows, nodes, fanout, seed)
    return cache[(fanout, seed)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("fanout", FANOUTS)
def test_neighbor_sample_equals_the_reference(sample_graph, fanout, n):
    from deep_recommenders_amd import ops
    row_ptr, col, n_rows, nodes, _ = sample_graph
    want_nbr, want_cnt = _sample_ref(sample_graph, fanout, 11)
    nbr, cnt = ops.neighbor_sample(_d(row_ptr), _d(col), n_rows, _d(nodes[:n]), fanout, 11)
    assert nbr.shape == (n, fanout) and cnt.shape == (n,)
    assert np.array_equal(cnt.cpu().numpy(), want_cnt[:n])
    assert np.array_equal(nbr.cpu().numpy(), want_nbr[:n])
    again, cnt2 = ops.neighbor_sample(_d(row_ptr), _d(col), n_rows, _d(nodes[:n]), fanout, 11)
    assert torch.equal(again, nbr) and torch.equal(cnt2, cnt)


def test_neighbor_sample_seeds_differ_on_a_long_row_and_edgeless_graph(sample_graph):
    from deep_recommenders_amd import ops
    row_ptr, col, n_rows, nodes, _ = sample_graph
    a, _ = ops.neighbor_sample(_d(row_ptr), _d(col), n_rows, _d(nodes[:1]), 25, 1)
    b, _ = ops.neighbor_sample(_d(row_ptr), _d(col), n_rows, _d(nodes[:1]), 25, 2)
    assert not torch.equal(a, b)
    want, _ = R.neighbor_sample_ref(row_ptr, col, n_rows, nodes[:1], 25, 2)
    assert np.array_equal(b.cpu().numpy(), want)
    nbr, cnt = ops.neighbor_sample(torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), 3,
                                   _d(np.asarray([0, 2, -1], np.int64)), 4, 0)
    assert (nbr == -1).all() and (cnt == 0).all()
    nbr, cnt = ops.neighbor_sample(_d(row_ptr), _d(col), n_rows, torch.zeros(0, dtype=torch.int64, device="cuda"), 4, 0)
    assert nbr.shape == (0, 4) and cnt.shape == (0,)


# ------------------------------------------------------------------------------------------------------------------------------
# dr_walk_neighbors
# ------------------------------------------------------------------------------------------------------------------------------
def _walks(n, Rw, Lw, id_range, seed):
    """walks with few distinct ids (ties in the counts), -1 tails, and walks that come back to their start"""
    r = np.random.RandomState(seed)
    w = r.randint(0, id_range, size=(n, Rw, Lw)).astype(np.int64)
    w[:, :, 0] = r.randint(0, id_range, size=(n, 1))
    cut = r.randint(1, Lw + 1, size=(n, Rw))
    for t in range(1, Lw):
        w[:, :, t] = np.where(t >= cut, -1, w[:, :, t])                     # a walk that ended stays -1
    if Lw > 1:
        w[::3, 0, 1] = w[::3, 0, 0]                                         # back onto the start
    w[n // 2, :, 1:] = -1                                                   # a start without any visit
    return w


@pytest.mark.parametrize("Rw,Lw,T,id_range", [(1, 2, 1, 5), (8, 3, 4, 6), (64, 17, 64, 90), (64, 17, 64, 3000), (10, 5, 50, 12)])
def test_walk_neighbors_equals_the_reference(Rw, Lw, T, id_range):
    from deep_recommenders_amd import ops
    walks = _walks(70, Rw, Lw, id_range, seed=Rw)
    want = R.walk_neighbors_ref(walks, T)
    got = ops.walk_neighbors(_d(walks), T)
    for g, w in zip(got, want):
        assert g.dtype == torch.from_numpy(w).dtype and np.array_equal(g.cpu().numpy(), w)
    if (Rw, Lw, T) == (10, 5, 50):
        assert (want[2] < T).all() and (want[0][:, -1] == -1).all()         # fewer than T distinct ids: a -1 tail
    if id_range <= 12 and Rw >= 8:
        c = want[1]
        assert ((c[:, :-1] == c[:, 1:]) & (c[:, 1:] > 0)).any()             # ties in count, resolved by id


def test_walk_neighbors_on_random_walks():
    from deep_recommenders_amd import ops
    r = np.random.RandomState(1)
    n_rows = 50
    deg = r.randint(0, 6, size=n_rows)
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate([np.sort(r.choice(n_rows, size=d, replace=False)) for d in deg]).astype(np.int32)
    nodes = torch.arange(n_rows, device="cuda").repeat_interleave(12)
    walks = ops.random_walk(_d(row_ptr), _d(col), n_rows, nodes, 4, 5).view(n_rows, 12, 4)
    want = R.walk_neighbors_ref(walks.cpu().numpy(), 6)
    for g, w in zip(ops.walk_neighbors(walks, 6), want):
        assert np.array_equal(g.cpu().numpy(), w)


# ------------------------------------------------------------------------------------------------------------------------------
# dr_frontier_build
# ------------------------------------------------------------------------------------------------------------------------------
def _check_frontier(dst, nbr, id_bound=0):
    from deep_recommenders_amd import ops
    want_src, want_counts, want_local = R.frontier_build_ref(dst, nbr)
    src, counts, local = ops.frontier_build(_d(dst), _d(nbr), id_bound)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert np.array_equal(src.cpu().numpy(), want_src)
    assert local.dtype == torch.int32 and np.array_equal(local.cpu().numpy(), want_local)
    return src, counts, local


BIG = 2 ** 40
DST = {"plain": [12, 40, 12, 7, BIG + 5, 3], "padded": [12, 40, 12, 7, BIG + 5, 3, -1, -1, -1]}


@pytest.mark.parametrize("m", [1, 64, 65, 60_000])
@pytest.mark.parametrize("dst_kind", ["plain", "padded"])
@pytest.mark.parametrize("nbr_kind", ["none", "in_dst", "new_distinct", "one_id", "mixed"])
def test_frontier_build_equals_the_reference(nbr_kind, dst_kind, m):
    dst = np.asarray(DST[dst_kind], dtype=np.int64)
    r = np.random.RandomState(m)
    if nbr_kind == "none":
        nbr = np.full(m, -1, np.int64)
    elif nbr_kind == "in_dst":
        nbr = r.choice(dst[dst >= 0], size=m)
    elif nbr_kind == "new_distinct":
        nbr = BIG + 100 + r.permutation(m).astype(np.int64) * 3
    elif nbr_kind == "one_id":
        nbr = np.full(m, BIG + 77, np.int64)
    else:
        nbr = np.where(r.rand(m) < 0.5, r.randint(0, 50, size=m), BIG + r.randint(0, 3000, size=m)).astype(np.int64)
        nbr[r.rand(m) < 0.1] = -1
    _, counts, _ = _check_frontier(dst, nbr)
    if nbr_kind in ("none", "in_dst"):
        assert counts[1].item() == counts[0].item() == 6
    if nbr_kind == "one_id":
        assert counts[1].item() == 7


@pytest.mark.parametrize("N", [16_383, 16_384, 16_385])
def test_frontier_build_around_the_one_launch_scan_limit(N):
    """the scans of up to 16 384 entries are one launch, longer ones three: dst ++ nbr of exactly that many entries and one more"""
    r = np.random.RandomState(N)
    dst = np.asarray(DST["padded"], dtype=np.int64)
    nbr = r.randint(0, 9000, size=N - dst.size).astype(np.int64)
    nbr[r.rand(nbr.size) < 0.1] = -1
    _check_frontier(dst, nbr, id_bound=9000)


def test_frontier_build_with_an_id_bound_and_two_chained_layers():
    r = np.random.RandomState(5)
    n_rows = 1000
    seeds = np.asarray([5, 999, 5, 0, 300], dtype=np.int64)
    nbr1 = r.randint(0, n_rows, size=(5, 7)).astype(np.int64)
    nbr1[r.rand(5, 7) < 0.2] = -1
    src1, counts1, _ = _check_frontier(seeds, nbr1, id_bound=n_rows)
    # the first layer's src, padding included, is the second layer's dst -- on the device, nothing read in between
    nbr2 = r.randint(0, n_rows, size=(src1.numel(), 4)).astype(np.int64)
    nbr2[src1.cpu().numpy() < 0] = -1
    src2, counts2, local2 = _check_frontier(src1.cpu().numpy(), nbr2, id_bound=n_rows)
    assert counts2[0].item() == counts1[1].item() and torch.equal(src2[:counts1[1].item()], src1[:counts1[1].item()])
    # an empty nbr still yields src and counts; an empty call yields empty outputs
    _check_frontier(seeds, np.zeros(0, np.int64), id_bound=n_rows)
    _check_frontier(np.zeros(0, np.int64), nbr1, id_bound=n_rows)
    _check_frontier(np.full(3, -1, np.int64), nbr1)


# ------------------------------------------------------------------------------------------------------------------------------
# dr_block_csr
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dst,fanout", [(1, 1), (300, 7), (5000, 25), (70, 64), (20_000, 3)])
@pytest.mark.parametrize("add_self", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_block_csr_equals_the_reference(weighted, add_self, n_dst, fanout):
    from deep_recommenders_amd import ops
    r = np.random.RandomState(n_dst + fanout)
    cnt = r.randint(0, fanout + 1, size=n_dst).astype(np.int32)
    cnt[0] = 0                                                              # an empty row: nothing, or the self entry alone
    local = r.randint(0, 3 * n_dst, size=(n_dst, fanout)).astype(np.int32)
    weight = r.randint(1, 65, size=(n_dst, fanout)).astype(np.float32) if weighted else None
    for n_valid in (None, max(n_dst - 3, 0)):
        want_rp, want_col, want_val = R.block_csr_ref(cnt, local, weight, add_self, n_valid)
        nv = None if n_valid is None else torch.tensor([7, n_valid], dtype=torch.int64, device="cuda")[1:]
        row_ptr, col, val = ops.block_csr(_d(cnt), _d(local), None if weight is None else _d(weight), add_self=add_self, n_valid=nv)
        assert np.array_equal(row_ptr.cpu().numpy(), want_rp)
        nnz = int(want_rp[-1])
        assert np.array_equal(col[:nnz].cpu().numpy(), want_col)
        assert np.array_equal(val[:nnz].cpu().numpy(), want_val)           # a sequential fp32 sum and one division: reproducible
        assert want_rp[1] == (1 if add_self and (n_valid is None or n_valid > 0) else 0)


# ------------------------------------------------------------------------------------------------------------------------------
# the layers against float64 on the densified blocks
# ------------------------------------------------------------------------------------------------------------------------------
WORST = {"ratio": 0.0}


def _close(got, want, rtol, atol, what):
    """np.allclose's test, with the largest err / bound printed (the PR summary quotes it)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ratio = float((np.abs(got - want) / (atol + rtol * np.abs(want))).max()) if got.size else 0.0
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print("%s: largest err / bound %.3g (worst so far %.3g)" % (what, ratio, WORST["ratio"]))
    assert ratio <= 1.0, what


def _power_graph(n=300, seed=0):
    """a few hundred nodes, two hubs over the sampler's long-row threshold is not possible at n = 300: hubs of degree 250 instead"""
    import scipy.sparse as sp
    r = np.random.RandomState(seed)
    rows, cols = [], []
    for v in range(n):
        d = 250 if v in (3, 150) else (0 if v == 9 else r.randint(1, 12))
        nb = r.choice(n, size=d, replace=False)
        rows += [v] * d
        cols += nb.tolist()
    return sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n, n))


_ACT64 = {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "linear": lambda t: t}


def _conv64(conv, h, A, n_dst, act):
    """SAGEConv restated in float64 on the dense block; returns (out, [parameters in conv.parameters() order as float64 leaves])"""
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.named_parameters()}
    q = torch.relu(h @ P["neighbor_kernel"] + P["neighbor_bias"]) if "neighbor_kernel" in P else h
    agg = A @ q
    if "self_kernel" in P:
        z = h[:n_dst] @ P["self_kernel"] + agg @ P["kernel"]
    else:
        z = agg @ P["kernel"]
    if "bias" in P:
        z = z + P["bias"]
    return _ACT64[act](z), P


@pytest.mark.parametrize("aggregator,neighbor_units,importance,act", [("mean", None, None, "relu"), ("gcn", None, None, "tanh"),
                                                                     ("mean", 12, dict(num_walks=8, walk_length=3), "relu"),
                                                                     ("gcn", 12, None, "sigmoid")])
def test_sageconv_fwd_bwd_matches_float64(aggregator, neighbor_units, importance, act):
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd.keras.models.retrieval import SAGEConv
    torch.manual_seed(0)
    adj = L.SparseAdjacency(_power_graph())
    seeds = torch.tensor([3, 9, 17, 3, 150, 42, 299], dtype=torch.int64)
    (block,) = L.sample_blocks(adj, seeds, [5], seed=4, importance=importance, add_self=aggregator == "gcn")
    assert block.n_dst == 7 and block.adj.shape == (7, block.n_src) and torch.equal(block.src_ids[:7].cpu(), seeds)
    A = torch.from_numpy(block.adj.to_dense().astype(np.float64))
    assert np.allclose(A.sum(1).numpy()[[0, 2, 3, 4, 5, 6]], 1.0, atol=1e-6)
    assert A[1].sum().item() == (1.0 if aggregator == "gcn" else 0.0)      # node 9 has no neighbours
    r = np.random.RandomState(1)
    h = r.standard_normal((block.n_src, 16)).astype(np.float32)
    Rw = r.standard_normal((7, 10)).astype(np.float32)
    # the aggregation alone, forward and backward, at test_gpu_gcn.py's spmm bound: |err| <= 1e-5 (|A| |X|)_ij + 1e-30
    ha = _d(h).requires_grad_(True)
    agg = L.aggregate(block.adj, ha)
    agg.backward(_d(Rw[:, :1].repeat(16, 1)))
    A64, h64n, d64 = A.numpy(), h.astype(np.float64), np.repeat(Rw[:, :1].astype(np.float64), 16, 1)
    for got, want, bound in ((agg.detach().cpu().numpy(), A64 @ h64n, np.abs(A64) @ np.abs(h64n)),
                             (ha.grad.cpu().numpy(), A64.T @ d64, np.abs(A64.T) @ np.abs(d64))):
        err = np.abs(got.astype(np.float64) - want)
        print("aggregate on a block: largest err / bound %.3g" % float((err / (1e-5 * bound + 1e-30)).max()))
        assert (err <= 1e-5 * bound + 1e-30).all()
    conv = SAGEConv(10, aggregator=aggregator, neighbor_units=neighbor_units, activation=act, bias_initializer="ones")
    hd = _d(h).requires_grad_(True)
    out = conv(hd, block)
    (out * _d(Rw)).sum().backward()
    h64 = torch.from_numpy(h.astype(np.float64)).requires_grad_(True)
    o64, P = _conv64(conv, h64, A, 7, act)
    (o64 * torch.from_numpy(Rw.astype(np.float64))).sum().backward()
    tag = "SAGEConv(%s, Q=%s, %s)" % (aggregator, neighbor_units, "walks" if importance else "uniform")
    _close(out.detach().cpu().numpy(), o64.detach().numpy(), 1e-4, 1e-5, tag + " out")
    _close(hd.grad.cpu().numpy(), h64.grad.numpy(), 1e-4, 1e-4, tag + " d h")
    for name, p in conv.named_parameters():
        assert p.grad is not None and p.grad.abs().sum().item() > 0, name
        _close(p.grad.cpu().numpy(), P[name].grad.numpy(), 1e-4, 1e-4, tag + " d " + name)
    if importance is not None:
        assert len(set(block.adj.val.cpu().numpy().tolist())) > 2            # visit-count weights, not a plain mean


@pytest.mark.parametrize("kind", ["sage_mean", "sage_gcn", "pinsage"])
def test_two_layer_model_fwd_bwd_matches_float64(kind):
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd import losses
    from deep_recommenders_amd.keras.models.retrieval import GraphSAGE, PinSage
    torch.manual_seed(1)
    n, D, C = 300, 24, 5
    adj = L.SparseAdjacency(_power_graph(n, seed=2))
    r = np.random.RandomState(3)
    feats = _d(r.standard_normal((n, D)).astype(np.float32)).requires_grad_(True)
    seeds = torch.from_numpy(r.choice(n, size=33, replace=False).astype(np.int64))
    y = np.eye(C, dtype=np.float32)[r.randint(0, C, 33)]
    if kind == "pinsage":
        model = PinSage([16, 12], [6, 4], num_walks=8, walk_length=3, num_classes=C)
    else:
        model = GraphSAGE([16, 12], [6, 4], aggregator=kind[5:], num_classes=C)
    pred = model(feats, adj, seeds, seed=7)
    loss = losses.categorical_crossentropy(y, pred)
    loss.backward()
    assert feats.grad is None                                               # features are inputs: read with dr_rows_gather
    blocks = model.blocks
    assert len(blocks) == 2 and blocks[1].n_dst == 33 and blocks[0].n_dst == blocks[1].n_src and blocks[0].n_src <= n
    assert torch.equal(blocks[1].src_ids[:33].cpu(), seeds) and torch.equal(blocks[0].src_ids[:blocks[0].n_dst], blocks[1].src_ids)
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert all(g.abs().sum().item() > 0 for g in grads.values()) and len(grads) == len(list(model.parameters()))
    # float64 on the dense blocks
    h = feats.detach().cpu().double()[blocks[0].src_ids.cpu()]
    P64 = {}
    for i, (conv, b) in enumerate(zip(model.convs, blocks)):
        h, P = _conv64(conv, h, torch.from_numpy(b.adj.to_dense().astype(np.float64)), b.n_dst, "relu")
        P64.update({"convs.%d.%s" % (i, k): v for k, v in P.items()})
    Wh = model.head_kernel.detach().cpu().double().requires_grad_(True)
    bh = model.head_bias.detach().cpu().double().requires_grad_(True)
    P64.update({"head_kernel": Wh, "head_bias": bh})
    logits = h @ Wh + bh
    l64 = -(torch.from_numpy(y.astype(np.float64)) * torch.log_softmax(logits, 1)).sum(1).mean()
    l64.backward()
    _close(pred.detach().cpu().numpy(), torch.softmax(logits, 1).detach().numpy(), 1e-4, 1e-5, kind + " out")
    assert abs(loss.item() - l64.item()) <= 1e-5 * max(1.0, abs(l64.item()))
    for k, g in grads.items():
        _close(g.cpu().numpy(), P64[k].grad.numpy(), 1e-4, 1e-4, kind + " d " + k)
    # a second run: the same blocks, the same bits
    for p in model.parameters():
        p.grad = None
    pred2 = model(feats, adj, seeds, seed=7)
    losses.categorical_crossentropy(y, pred2).backward()
    assert torch.equal(pred2, pred) and all(torch.equal(p.grad, grads[k]) for k, p in model.named_parameters())
    for a, b in zip(model.blocks, blocks):
        assert torch.equal(a.src_ids, b.src_ids) and torch.equal(a.adj.col, b.adj.col) and torch.equal(a.adj.val, b.adj.val)
    # another seed samples other blocks
    model(feats, adj, seeds, seed=8)
    assert any(a.adj.col.shape != b.adj.col.shape or not torch.equal(a.adj.col, b.adj.col) for a, b in zip(model.blocks, blocks))


@pytest.mark.parametrize("D", [4, 24, 256, 260, 1433])
def test_feature_rows_of_any_width(D):
    from deep_recommenders_amd.keras.models.retrieval.graphsage import gather_feature_rows, pad_feature_columns
    r = np.random.RandomState(D)
    x = torch.from_numpy(r.standard_normal((500, D)).astype(np.float32))
    xp = pad_feature_columns(x).cuda()
    assert xp.shape[1] % 4 == 0 and xp.shape[1] - D < (4 if D <= 256 else 256) and torch.equal(xp[:, :D].cpu(), x) and not xp[:, D:].any()
    ids = _d(r.randint(0, 500, size=77).astype(np.int64))
    assert torch.equal(gather_feature_rows(xp, ids), xp[ids])
    if D % 4:
        with pytest.raises(ValueError):
            gather_feature_rows(x.cuda(), ids)


def test_sample_blocks_against_the_reference_chain():
    """two layers with a hub over the long-row threshold: every array of every block equals the NumPy chain"""
    import scipy.sparse as sp
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd import ops
    r = np.random.RandomState(6)
    n = 1500
    deg = r.randint(0, 9, size=n)
    deg[4] = ops.SAMPLE_LONG_ROW + 200
    rows = np.repeat(np.arange(n), deg)
    cols = np.concatenate([np.sort(r.choice(n, size=d, replace=False)) for d in deg])
    adj = L.SparseAdjacency(sp.csr_matrix((np.ones(rows.size, np.float32), (rows, cols)), shape=(n, n)))
    row_ptr, col = adj.row_ptr.cpu().numpy(), adj.col.cpu().numpy()
    seeds = np.asarray([4, 7, 7, 1200, 33], dtype=np.int64)
    fanouts = [3, 10]
    blocks = L.sample_blocks(adj, torch.from_numpy(seeds), fanouts, seed=21, add_self=True)
    dst = seeds
    for k in (1, 0):
        nbr, cnt = R.neighbor_sample_ref(row_ptr, col, n, dst, fanouts[k], L._layer_seed(21, k))
        src, counts, local = R.frontier_build_ref(dst, nbr)
        rp, c, v = R.block_csr_ref(cnt, local, None, True, counts[0])
        b = blocks[k]
        assert (b.n_dst, b.n_src) == (counts[0], counts[1]) and np.array_equal(b.src_ids.cpu().numpy(), src[:counts[1]])
        assert np.array_equal(b.adj.row_ptr.cpu().numpy(), rp[:counts[0] + 1])
        assert np.array_equal(b.adj.col.cpu().numpy(), c) and np.array_equal(b.adj.val.cpu().numpy(), v)
        dst = src


def test_example_model_trains_for_20_steps(tmp_path):
    from deep_recommenders_amd.datasets import synthetic_cora
    spec = importlib.util.spec_from_file_location("train_graphsage_example", os.path.join(ROOT, "examples", "train_graphsage_on_cora_keras.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    data = synthetic_cora(str(tmp_path), num_nodes=300, num_features=64, num_edges=700, words_per_node=10, seed=0)
    _, _, history = ex.train_model(data, steps=20, batch=140, fanouts=(5, 5), seed=0, verbose=False)    # every step sees the whole training set
    assert len(history) == 20 and all(np.isfinite(history))
    assert history[-1] < history[0], history
