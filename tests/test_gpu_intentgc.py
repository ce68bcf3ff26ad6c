"""IntentGC on the GPU: dr_intent_conv_fwd / dr_intent_mix_fwd / dr_intent_conv_bwd against the float64 restatements of
tests/intentgc_ref.py within the bounds derived there (u = 2^-24; nothing is fitted to the kernel's output), exactly on the integer
grid, the bit equalities the header promises, the typed sampling chain against its NumPy restatement, the layer and one train step
under the project's step rule (error over the largest float64 magnitude <= 16 max(r32, 8 u), tests/test_gpu_afm.py), and the example."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import intentgc_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = R.U
_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(shape, grid=False, act=1):
    """the case with its float64 references, computed once and shared (never written to)"""
    key = (tuple(shape), grid, act)
    if key not in _CASES:
        c = R.make_case(shape, grid=grid, act=act)
        c["agg64"], c["A"], c["n"] = R.typed_aggregate(c["row_ptr"], c["col"], c["val"], c["h"], c["n_dst"], c["R"])
        _CASES[key] = c
    return _CASES[key]


def _h_dev(c, pitched=None):
    """h on the device; pitched: a view of a wider buffer whose padding is NaN"""
    pitched = c["pitched"] if pitched is None else pitched
    if not pitched:
        return _d(c["h"])
    buf = torch.full((c["h"].shape[0], c["D"] + 8), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :c["D"]] = _d(c["h"])
    return buf[:, :c["D"]]


def _fwd(c, want_agg=True, pitched=None, h=None):
    from deep_recommenders_amd import ops
    h = _h_dev(c, pitched) if h is None else h
    return ops.intent_conv_fwd(_d(c["row_ptr"]), _d(c["col"]), _d(c["val"]), c["n_dst"], c["R"], h, _d(c["W"]), _d(c["theta"]), c["act"],
                               want_agg=want_agg)


def _bwd(c, agg, out=None, pitched=None):
    from deep_recommenders_amd import ops
    h = _h_dev(c, pitched)
    return ops.intent_conv_bwd(h[:c["n_dst"]], agg, _d(c["d_out"]), _d(c["W"]), _d(c["theta"]), c["act"], out=out)


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1 / 2: derived bounds, kinks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [1, 0])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_forward_and_backward_within_the_derived_bounds(shape, act):
    c = _case(shape, act=act)
    n_dst, Rr, D = c["n_dst"], c["R"], c["D"]
    W, theta = c["W"].astype(np.float64), c["theta"].astype(np.float64)
    h_self = c["h"][:n_dst].astype(np.float64)
    out, agg = _fwd(c)
    torch.cuda.synchronize()
    out_g, agg_g = _np(out).astype(np.float64), _np(agg).astype(np.float64)
    assert out_g.shape == (n_dst, D) and agg_g.shape == (n_dst, Rr, D)
    assert not np.isnan(out_g).any() and not np.isnan(agg_g).any()
    p, s, want = R.conv_forward(h_self, c["agg64"], W, theta, act)
    b_agg, b_p, b_out, _ = R.forward_bounds(c, h_self, c["agg64"], c["A"], c["n"])
    e_agg, e_out = np.abs(agg_g - c["agg64"]), np.abs(out_g - want)
    tiny = np.finfo(np.float64).tiny
    print("%s act %d: agg error / bound %.3f, out error / bound %.3f" % (shape, act, (e_agg / (b_agg + tiny)).max(), (e_out / (b_out + tiny)).max()))
    assert (e_agg <= b_agg).all() and (e_out <= b_out).all()
    assert (agg_g[c["n"] == 0] == 0).all()                                 # an empty virtual row aggregates to exactly 0

    # the backward is a function of (h_self, agg, d_out, W, theta): the reference takes the agg the kernel stored
    kink = R.kinks(c, p, s, b_p, b_out)
    assert kink.mean() <= R.KINK_LIMIT
    d_out = c["d_out"].astype(np.float64)
    want_b = R.conv_backward(h_self, agg_g, W, theta, act, d_out)
    bounds = R.backward_bounds(c, h_self, agg_g, d_out, kink, b_p)
    for with_out in (True, False):
        got = [_np(x).astype(np.float64) for x in _bwd(c, agg, out=out if with_out else None)]
        for name, x, w, b in zip(("d_self", "d_agg", "d_W", "d_theta"), got, want_b, bounds):
            assert not np.isnan(x).any(), name
            err = np.abs(x - w)
            if name == "d_self":
                err = err * ~kink
            elif name == "d_agg":
                err = err * ~kink[:, None, :]
            print("  %s (out %s): error / bound %.3f" % (name, "given" if with_out else "recomputed", (err / (b + tiny)).max()))
            assert (err <= b).all(), (name, shape, (err / (b + tiny)).max())


# ---- 3: the integer grid --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [1, 0])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_integer_grid_is_exact(shape, act):
    """every product and sum is exact in fp32, so every output equals the float64 value (compared as values: the comparison is exact, a
    signed zero equals a zero)"""
    from deep_recommenders_amd import layers as L
    c = _case(shape, grid=True, act=act)
    n_dst, Rr, D = c["n_dst"], c["R"], c["D"]
    W, theta, h_self, d_out = (c["W"].astype(np.float64), c["theta"].astype(np.float64), c["h"][:n_dst].astype(np.float64),
                               c["d_out"].astype(np.float64))
    out, agg = _fwd(c)
    _, _, want = R.conv_forward(h_self, c["agg64"], W, theta, act)
    assert np.array_equal(_np(agg).astype(np.float64), c["agg64"]) and np.array_equal(_np(out).astype(np.float64), want)
    got = _bwd(c, agg, out=out)
    want_b = R.conv_backward(h_self, c["agg64"], W, theta, act, d_out)
    for name, x, w in zip(("d_self", "d_agg", "d_W", "d_theta"), got, want_b):
        assert np.array_equal(_np(x).astype(np.float64), w), name
    # the whole input gradient through the transposed block
    adj = L.SparseAdjacency._from_device(_d(c["row_ptr"]), _d(c["col"]), _d(c["val"]), (n_dst * Rr, c["n_src"]))
    d_h = torch.zeros((c["n_src"], D), device="cuda")
    d_h[:n_dst] = got[0]
    adj.transpose().spmm(got[1].view(n_dst * Rr, D), accumulate=True, out=d_h)
    want_h = np.zeros((c["n_src"], D))
    want_h[:n_dst] = want_b[0]
    for q in range(n_dst * Rr):
        for k in range(int(c["row_ptr"][q]), int(c["row_ptr"][q + 1])):
            want_h[c["col"][k]] += float(c["val"][k]) * want_b[1][q // Rr, q % Rr]
    assert np.array_equal(_np(d_h).astype(np.float64), want_h)


# ---- 4: bit equalities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES)
def test_bit_equalities(shape):
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd import ops
    c = _case(shape)
    n_dst, Rr, D = c["n_dst"], c["R"], c["D"]
    h = _h_dev(c)
    out, agg = _fwd(c, h=h)
    # agg is adj.spmm(h) on every row that kernel does not split
    adj = L.SparseAdjacency._from_device(_d(c["row_ptr"]), _d(c["col"]), _d(c["val"]), (n_dst * Rr, c["n_src"]))
    spmm = adj.spmm(h).contiguous().view(n_dst, Rr, D)
    short = torch.from_numpy(np.diff(c["row_ptr"]).reshape(n_dst, Rr) <= R.LONG_ROW).cuda()
    assert _same_bits(agg[short], spmm[short])
    if shape == R.SHAPES[4]:
        assert not bool(short.all())
    # the pre-aggregated form gives the same out from the same agg; storing agg or not changes nothing; nor does the pitch of h
    assert _same_bits(out, ops.intent_mix_fwd(h[:n_dst], agg, _d(c["W"]), _d(c["theta"]), c["act"]))
    out2, none = _fwd(c, want_agg=False, h=h)
    assert none is None and _same_bits(out, out2)
    out3, agg3 = _fwd(c, pitched=not c["pitched"])
    assert _same_bits(out, out3) and _same_bits(agg, agg3)
    # run to run, d_W and d_theta included
    a = _bwd(c, agg, out=out)
    b = _bwd(c, agg, out=out)
    r = _bwd(c, agg, out=None)
    for x, y, z in zip(a, b, r):
        assert _same_bits(x, y) and _same_bits(x, z)
    # a destination's bits do not depend on the block around it
    keep = list(range(0, n_dst, 3))
    sub = R.subset_case(c, keep)
    out_s, agg_s = _fwd(sub, pitched=False)
    idx = torch.tensor(keep, device="cuda")
    assert _same_bits(out_s, out[idx]) and _same_bits(agg_s, agg[idx])


# ---- 5: nothing to do, nothing to gather ------------------------------------------------------------------------------------------------
def test_no_destinations_and_a_block_of_empty_rows():
    from deep_recommenders_amd import ops
    W, theta = _d(np.asarray([[0.5, 2.0, -1.0], [-1.5, 1.0, 1.0]], np.float32)), _d(np.asarray([1.25, -0.75], np.float32))
    h = torch.randn((7, 8), device="cuda")
    e_i, e_f = torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, device="cuda")
    out, agg = ops.intent_conv_fwd(torch.zeros(1, dtype=torch.int64, device="cuda"), e_i, e_f, 0, 2, h, W, theta, 1, want_agg=True)
    assert tuple(out.shape) == (0, 8) and tuple(agg.shape) == (0, 2, 8)
    got = ops.intent_conv_bwd(h[:0], agg, out, W, theta, 1)
    assert tuple(got[1].shape) == (0, 2, 8) and (got[2] == 0).all() and (got[3] == 0).all()
    assert tuple(ops.intent_mix_fwd(h[:0], agg, W, theta, 1).shape) == (0, 8)
    for act in (0, 1):
        out, agg = ops.intent_conv_fwd(torch.zeros(4 * 2 + 1, dtype=torch.int64, device="cuda"), e_i, e_f, 4, 2, h, W, theta, act, want_agg=True)
        assert (agg == 0).all()
        hv = h[:4].double().cpu()
        s = 1.25 * torch.relu(0.5 * hv) - 0.75 * torch.relu(-1.5 * hv)
        want = torch.relu(s) if act == 1 else s
        assert (out.double().cpu() - want).abs().max() <= 4 * U * want.abs().max()


# ---- 6: the typed sampling chain ----------------------------------------------------------------------------------------------------------
def _relations(n, Rr, seed):
    import scipy.sparse as sp
    from deep_recommenders_amd import layers as L
    r = np.random.RandomState(seed)
    out = []
    for _ in range(Rr):
        deg = r.randint(0, 9, size=n)
        rows = np.repeat(np.arange(n), deg)
        cols = np.concatenate([np.sort(r.choice(n, size=d, replace=False)) for d in deg])
        out.append(L.SparseAdjacency(sp.csr_matrix((np.ones(rows.size, np.float32), (rows, cols)), shape=(n, n))))
    return out


@pytest.mark.parametrize("Rr", [1, 3])
def test_sample_typed_blocks_against_the_reference_chain(Rr):
    from deep_recommenders_amd import layers as L
    n = 400
    rel = _relations(n, Rr, seed=Rr)
    graphs = [(a.row_ptr.cpu().numpy(), a.col.cpu().numpy()) for a in rel]
    seeds = np.asarray([4, 7, 7, 399, 33, 4], dtype=np.int64)
    fanouts = [3, 5]
    blocks = L.sample_typed_blocks(rel, torch.from_numpy(seeds), fanouts, seed=21)
    want = R.sample_typed_blocks_ref(graphs, n, seeds, fanouts, 21)
    for b, w in zip(blocks, want):
        assert (b.n_dst, b.n_src, b.R) == (w["n_dst"], w["n_src"], Rr) and b.adj.shape == (w["n_dst"] * Rr, w["n_src"])
        assert np.array_equal(_np(b.src_ids), w["src"]) and np.array_equal(_np(b.adj.row_ptr), w["row_ptr"])
        assert np.array_equal(_np(b.adj.col), w["col"]) and np.array_equal(_np(b.adj.val).view(np.int32), w["val"].view(np.int32))
    assert blocks[1].n_dst == 6 and blocks[0].n_dst == blocks[1].n_src
    again = L.sample_typed_blocks(rel, torch.from_numpy(seeds), fanouts, seed=21)
    other = L.sample_typed_blocks(rel, torch.from_numpy(seeds), fanouts, seed=22)
    for b, a in zip(blocks, again):
        assert torch.equal(b.src_ids, a.src_ids) and torch.equal(b.adj.row_ptr, a.adj.row_ptr) and torch.equal(b.adj.col, a.adj.col)
        assert _same_bits(b.adj.val, a.adj.val)
    assert any(b.src_ids.shape != o.src_ids.shape or not torch.equal(b.src_ids, o.src_ids) or not torch.equal(b.adj.col, o.adj.col)
               for b, o in zip(blocks, other))


# ---- 7: the layer and one train step under the step rule -----------------------------------------------------------------------------------
def _step_rule(name, got, want64, want32):
    scale = want64.abs().max().item()
    assert scale > 0, name
    r32 = (want32.double() - want64).abs().max().item() / scale
    err = (got.double().cpu() - want64).abs().max().item() / scale
    limit = 16 * max(r32, 8 * U)
    print("%s: error %.3g = %.2f max(r32, 8u), %.3f of the limit" % (name, err, err / max(r32, 8 * U), err / limit))
    assert err <= limit, (name, err, limit)


@pytest.mark.parametrize("shape", R.SHAPES[:4])
def test_intentconv_call_and_backward_match_float64(shape):
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd.keras.models.retrieval import IntentConv
    c = _case(shape)
    n_dst, Rr, D, n_src = c["n_dst"], c["R"], c["D"], c["n_src"]
    hh = np.nan_to_num(c["h"], nan=0.25)                                  # the layer's d_h covers every source row
    adj = L.SparseAdjacency._from_device(_d(c["row_ptr"]), _d(c["col"]), _d(c["val"]), (n_dst * Rr, n_src))
    block = L.TypedBlock(adj, torch.arange(n_src, device="cuda"), n_dst, Rr)
    conv = IntentConv(c["L"], activation="relu")
    conv.build(Rr, "cuda")
    conv.kernel.data.copy_(_d(c["W"]))
    conv.theta.data.copy_(_d(c["theta"]))
    out = conv.call(_d(hh), block, training=True)
    d_h = conv.backward(_d(c["d_out"]))
    assert conv._kept is None and tuple(d_h.shape) == (n_src, D)
    A = torch.tensor(adj.to_dense().reshape(n_dst, Rr, n_src))
    res = {}
    for dt in (torch.float64, torch.float32):
        h, W, th = (torch.tensor(x, dtype=dt, requires_grad=True) for x in (hh, c["W"], c["theta"]))
        o = R.conv_torch(h[:n_dst], torch.einsum("vrs,sd->vrd", A.to(dt), h), W, th, 1)
        o.backward(torch.tensor(c["d_out"], dtype=dt))
        res[dt] = (o.detach(), h.grad, W.grad, th.grad)
    for name, got, w64, w32 in zip(("out", "d_h", "kernel.grad", "theta.grad"), (out, d_h, conv.kernel.grad, conv.theta.grad),
                                   res[torch.float64], res[torch.float32]):
        _step_rule("%s %s" % (name, shape), got, w64, w32)
    assert conv.call(_d(hh), block) is not None and conv._kept is None     # inference keeps nothing


def _load(net, params):
    with torch.no_grad():
        net.proj_kernel.copy_(_d(params["proj_kernel"]))
        net.proj_bias.copy_(_d(params["proj_bias"]))
        for conv, (W, th) in zip(net.convs, params["convs"]):
            conv.kernel.copy_(_d(W))
            conv.theta.copy_(_d(th))
        for K, b, (Kn, bn) in zip(net.dnn_kernels, net.dnn_biases, params["dnn"]):
            K.copy_(_d(Kn))
            b.copy_(_d(bn))


def _grads(net):
    ps = [net.proj_kernel, net.proj_bias] + [x for conv in net.convs for x in (conv.kernel, conv.theta)] + \
         [x for K, b in zip(net.dnn_kernels, net.dnn_biases) for x in (K, b)]
    return [p.grad for p in ps]


def test_train_step_matches_float64():
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd.keras.models.retrieval import IntentGC
    c = R.make_model_case()
    model = IntentGC([L.SparseAdjacency(m) for m in c["rel_u"]], [L.SparseAdjacency(m) for m in c["rel_i"]], _d(c["feat_u"]), _d(c["feat_i"]),
                     embedding_dim=c["D"], num_layers=2, num_filters=c["L"], fanouts=c["fanouts"], dnn_units_size=c["units"],
                     margin=c["margin"])
    _load(model.user_net, c["user_params"])
    _load(model.item_net, c["item_params"])
    loss = model.train_step(_d(c["users"]), _d(c["pos_items"]), _d(c["neg_items"]), optimizer=None, seed=c["sample_seed"])
    # the step ran on the blocks the restated chain gives: densified, they are the reference's operands
    for blocks, side in zip(model.blocks, ("user", "item")):
        for b, w, dense in zip(blocks, c[side + "_blocks"], c[side + "_dense"]):
            assert np.array_equal(_np(b.src_ids), w["src"])
            assert np.array_equal(b.adj.to_dense().reshape(b.n_dst, 2, b.n_src), dense)
    r64, r32 = R.train_step_ref(c, torch.float64), R.train_step_ref(c, torch.float32)
    assert np.abs(r64[5].numpy()).min() >= 1e-3
    _step_rule("loss", loss.reshape(1), r64[0].reshape(1), r32[0].reshape(1))
    names = ["proj_kernel", "proj_bias", "conv0.kernel", "conv0.theta", "conv1.kernel", "conv1.theta", "dnn0.kernel", "dnn0.bias",
             "dnn1.kernel", "dnn1.bias"]
    for side, net, j in (("user", model.user_net, 1), ("item", model.item_net, 2)):
        for name, g, w64, w32 in zip(names, _grads(net), r64[j], r32[j]):
            _step_rule("%s %s.grad" % (side, name), g, w64, w32)
        _step_rule("%s d_h0" % side, net.d_h0, r64[j + 2], r32[j + 2])
    n_active = float((r64[5] > 0).sum()) / (6 * 5)
    assert abs(model.active_fraction.item() - n_active) < 1e-6
    # forward only: the same vectors as the step's forward, no aggregates kept
    z = model.user_vectors(_d(c["users"]), seed=c["sample_seed"])
    assert tuple(z.shape) == (6, c["units"][-1]) and all(conv._kept is None for conv in model.user_net.convs)
    idx = model.index(torch.arange(c["Ni"]), k=5, seed=c["sample_seed"])
    scores, ids = model.top_k(_d(c["users"]), k=5, seed=c["sample_seed"])
    assert idx is not None and tuple(ids.shape) == (6, 5) and (scores[:, :-1] >= scores[:, 1:]).all()


# ---- 8: the example ------------------------------------------------------------------------------------------------------------------------
def test_example_model_trains_for_20_steps():
    spec = importlib.util.spec_from_file_location("train_intentgc_example", os.path.join(ROOT, "examples", "train_intentgc_on_synthetic_keras.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    runs = [ex.train_model(ex.make_data(num_users=120, num_items=150, seed=0), steps=20, batch=32, num_negatives=16, seed=0, verbose=False)
            for _ in range(2)]
    (_, before, after, history), (_, before2, after2, history2) = runs
    assert len(history) == 20 and all(np.isfinite(history))
    assert after["loss"] < before["loss"], (before, after)
    assert history == history2 and before == before2 and after == after2      # bit-identical from the same seeds
