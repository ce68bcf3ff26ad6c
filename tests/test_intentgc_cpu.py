"""IntentGC without a GPU: the restatements of tests/intentgc_ref.py against torch's float64 autograd and a brute-force loop, the
header / ctypes / library surface of the new entry points, the wrappers' argument checks (all made before any kernel is touched), and
the conditions the GPU cases rely on (kink fraction, hinge room)."""
import os

import numpy as np
import pytest
import torch

import intentgc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["dr_intent_conv_fwd", "dr_intent_mix_fwd", "dr_intent_conv_bwd", "dr_intent_conv_bwd_workspace_bytes"]


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("act", [0, 1])
def test_explicit_backward_equals_float64_autograd(shape, act):
    c = R.make_case(shape, act=act)
    agg, _, _ = R.typed_aggregate(c["row_ptr"], c["col"], c["val"], c["h"], c["n_dst"], c["R"])
    h_self = c["h"][:c["n_dst"]].astype(np.float64)
    W, theta, d_out = c["W"].astype(np.float64), c["theta"].astype(np.float64), c["d_out"].astype(np.float64)
    got = R.conv_backward(h_self, agg, W, theta, act, d_out)
    t = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (h_self, agg, W, theta)]
    out = R.conv_torch(*t, act)
    assert np.array_equal(out.detach().numpy() > 0, R.conv_forward(h_self, agg, W, theta, act)[2] > 0)
    out.backward(torch.tensor(d_out))
    for name, x, want in zip(("d_self", "d_agg", "d_W", "d_theta"), got, (y.grad.numpy() for y in t)):
        scale = np.abs(want).max()
        assert scale > 0 and np.abs(x - want).max() <= 1e-12 * scale, (name, shape)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_cases_have_what_the_gpu_tests_rely_on(shape):
    """empty virtual rows, a destination without neighbours, unreferenced (NaN) rows unless every row is referenced, a full-length row;
    the kink condition is asserted inside make_case; the integer grid is dyadic"""
    for grid in (False, True):
        c = R.make_case(shape, grid=grid)
        lens = np.diff(c["row_ptr"]).reshape(c["n_dst"], c["R"])
        assert (lens == 0).any() and (lens.sum(axis=1) == 0).any()
        assert np.isnan(c["h"]).any() == (c["unused"] > 0) and not np.isnan(c["h"][:c["n_dst"]]).any()
        assert not np.isnan(c["h"][c["col"]]).any()
        if grid:
            assert set(np.unique(lens)) <= {0, 1, 2, 4, 8} and set(np.unique(c["W"] * 2)) <= {-2, -1, 0, 1, 2}
        else:
            assert lens.max() == shape[3] and c["kink_fraction"] <= R.KINK_LIMIT
    assert R.make_case(R.SHAPES[4])["row_ptr"][1] > R.LONG_ROW


def test_translate_relations_equals_the_double_loop():
    from deep_recommenders_amd.keras.models.retrieval import translate_relations
    r = np.random.RandomState(0)
    for N, A, k, weighted in ((30, 12, 3, False), (25, 6, 5, False), (17, 9, 1, True), (8, 3, 20, False)):
        B = (r.rand(N, A) < 0.3).astype(np.float64)                      # 0 / 1 incidences: many equal weights, so the tie rule decides
        if weighted:
            B *= r.randint(1, 4, size=B.shape)
        got = translate_relations(B, k, device="cpu")
        want = R.translate_relations_ref(B, k)
        assert got.shape == (N, N) and np.array_equal(got.to_dense(), want)
        assert (np.count_nonzero(want, axis=1) <= k).all() and np.trace(want) == 0
    with pytest.raises(ValueError, match="top_k"):
        translate_relations(B, 0, device="cpu")


def test_header_declares_and_library_exports_the_entry_points():
    from deep_recommenders_amd import _cabi, _lib
    protos = _cabi.prototypes(os.path.join(ROOT, "include", "dr_hotpath.h"))
    lib = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in protos, name
        assert getattr(lib, name).argtypes == protos[name][1]
    assert len(protos["dr_intent_conv_fwd"][1]) == 16 and len(protos["dr_intent_conv_bwd"][1]) == 22
    # the workspace size is host arithmetic: blocks x L (R + 2) floats, -1 outside the domain
    for n_dst, D, Rr, Lf in ((65536, 128, 3, 4), (8192, 64, 2, 8), (5, 4, 1, 1), (100000, 256, 7, 16)):
        _, parts = R.bwd_grid(n_dst, D)
        assert lib.dr_intent_conv_bwd_workspace_bytes(n_dst, D, Rr, Lf) == parts * Lf * (Rr + 2) * 4
    for bad in ((5, 6, 1, 1), (5, 260, 1, 1), (5, 8, 0, 1), (5, 8, 8, 1), (5, 8, 1, 0), (5, 8, 1, 17), (-1, 8, 1, 1)):
        assert lib.dr_intent_conv_bwd_workspace_bytes(*bad) == -1


def _args(n_dst=6, n_src=10, Rr=2, D=8, Lf=3):
    z = torch.zeros
    return dict(row_ptr=z(n_dst * Rr + 1, dtype=torch.int64), col=z(0, dtype=torch.int32), val=z(0), h=z(n_src, D), W=z(Lf, Rr + 1),
                theta=z(Lf), agg=z(n_dst, Rr, D), d_out=z(n_dst, D), n_dst=n_dst, R=Rr, D=D)


def _fwd(a, **kw):
    from deep_recommenders_amd import ops
    a = {**a, **kw}
    return ops.intent_conv_fwd(a["row_ptr"], a["col"], a["val"], a["n_dst"], a["R"], a["h"], a["W"], a["theta"], a.get("act", 1))


def _mix(a, **kw):
    from deep_recommenders_amd import ops
    a = {**a, **kw}
    return ops.intent_mix_fwd(a["h"][:a["n_dst"]] if "h_self" not in a else a["h_self"], a["agg"], a["W"], a["theta"], a.get("act", 1))


def _bwd(a, **kw):
    from deep_recommenders_amd import ops
    a = {**a, **kw}
    return ops.intent_conv_bwd(a["h"][:a["n_dst"]] if "h_self" not in a else a["h_self"], a["agg"], a["d_out"], a["W"], a["theta"],
                               a.get("act", 1), out=a.get("out"), d_self=a.get("d_self"))


def _misaligned(rows, D):
    return torch.zeros(rows * D + 1)[1:].view(rows, D)


def test_wrappers_refuse_what_the_kernels_cannot_take():
    """every ValueError names the argument and comes before a kernel (or a device) is needed: these run on host tensors"""
    for D in (2, 6, 0, 260, 258):
        a = _args(D=D)
        for f in (_fwd, _mix, _bwd):
            with pytest.raises(ValueError, match="D"):
                f(a)
    for Rr in (0, 8):
        a = _args(Rr=Rr)
        for f in (_fwd, _mix, _bwd):
            with pytest.raises(ValueError, match="R"):
                f(a)
    for Lf in (0, 17):
        a = _args(Lf=Lf)
        for f in (_fwd, _mix, _bwd):
            with pytest.raises(ValueError, match="L = %d|theta|W" % Lf):
                f(a)
    a = _args()
    for f in (_fwd, _mix, _bwd):
        with pytest.raises(ValueError, match="act"):
            f(a, act=2)
        with pytest.raises(ValueError, match="theta"):
            f(a, theta=torch.zeros(4))
        with pytest.raises(ValueError, match="W"):
            f(a, W=torch.zeros(3))
    # pitches: a multiple of 4 and >= D; bases: 16-byte aligned
    with pytest.raises(ValueError, match="h needs"):
        _fwd(a, h=torch.zeros(10, 10)[:, :8])
    with pytest.raises(ValueError, match="h needs"):
        _fwd(a, h=torch.zeros(8, 10).t())
    with pytest.raises(ValueError, match="h must start at a 16-byte"):
        _fwd(a, h=_misaligned(10, 8))
    with pytest.raises(ValueError, match="h must be fp32"):
        _fwd(a, h=torch.zeros(5, 8))                                     # fewer source rows than destinations
    with pytest.raises(ValueError, match="h must be fp32"):
        _fwd(a, h=torch.zeros(10, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="row_ptr"):
        _fwd(a, row_ptr=torch.zeros(12, dtype=torch.int64))
    with pytest.raises(ValueError, match="row_ptr"):
        _fwd(a, row_ptr=torch.zeros(13, dtype=torch.int32))
    with pytest.raises(ValueError, match="val"):
        _fwd(a, val=torch.zeros(3))
    for f in (_mix, _bwd):
        with pytest.raises(ValueError, match="h_self needs"):
            f(a, h_self=torch.zeros(6, 10)[:, :8])
        with pytest.raises(ValueError, match="h_self must start"):
            f(a, h_self=_misaligned(6, 8))
        with pytest.raises(ValueError, match="agg must be fp32"):
            f(a, agg=torch.zeros(6, 3, 8))
        with pytest.raises(ValueError, match="agg must be contiguous"):
            f(a, agg=torch.zeros(6, 2, 12)[:, :, :8])
    with pytest.raises(ValueError, match="d_out needs"):
        _bwd(a, d_out=torch.zeros(6, 10)[:, :8])
    with pytest.raises(ValueError, match="d_out must start"):
        _bwd(a, d_out=_misaligned(6, 8))
    with pytest.raises(ValueError, match="out needs"):
        _bwd(a, out=torch.zeros(6, 9)[:, :8])
    with pytest.raises(ValueError, match="d_self must be fp32"):
        _bwd(a, d_self=torch.zeros(7, 8))
    # a pitched view that IS legal reaches the kernel call, which has no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _fwd(a, h=torch.zeros(10, 12)[:, :8])


def test_model_surface_and_typed_block_checks():
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd.keras.models.retrieval import IntentConv, IntentGC, IntentNet
    conv = IntentConv(4, activation="linear")
    assert conv.get_config() == {"num_filters": 4, "activation": "linear"}
    conv.build(3, device="cpu")
    assert tuple(conv.kernel.shape) == (4, 4) and tuple(conv.theta.shape) == (4,)
    assert (conv.kernel[:, 0] > conv.kernel[:, 1:].abs().max(dim=1).values - 0.25).all() and len(set(conv.kernel[:, 0].tolist())) == 4
    with pytest.raises(ValueError):
        IntentConv(17)
    with pytest.raises(NotImplementedError):
        IntentConv(2, activation="tanh")
    with pytest.raises(RuntimeError, match="training=True"):
        conv.backward(torch.zeros(2, 4))
    with pytest.raises(ValueError, match="embedding_dim"):
        IntentNet(6, 1, 2, (8,))
    import scipy.sparse as sp
    A = L.SparseAdjacency(sp.identity(5, format="csr", dtype=np.float32), device="cpu")
    f = torch.zeros(5, 4)
    with pytest.raises(ValueError, match="fanout"):
        IntentGC([A], [A], f, f, num_layers=2, fanouts=(3,))
    with pytest.raises(ValueError, match="dnn_units_size"):
        IntentGC([A], [A], f, f, dnn_units_size=(8, 6))
    with pytest.raises(TypeError):
        L.sample_typed_blocks([], torch.zeros(2, dtype=torch.int64), [2], 0)
    with pytest.raises(ValueError, match="same nodes"):
        L.sample_typed_blocks([A, L.SparseAdjacency(sp.identity(6, format="csr", dtype=np.float32), device="cpu")],
                              torch.zeros(2, dtype=torch.int64), [2], 0)
    with pytest.raises(ValueError, match="seeds"):
        L.sample_typed_blocks([A], torch.zeros(2, dtype=torch.int32), [2], 0)
    # no autograd Function was added for the layer: it is driven by an explicit backward
    from deep_recommenders_amd.keras.models.retrieval import intentgc
    assert not [v for v in vars(intentgc).values() if isinstance(v, type) and issubclass(v, torch.autograd.Function)]


def test_model_case_hinges_have_room():
    """float64 decides every hinge of the GPU test's train step by at least 1e-3, some on each side; the restated chain gives blocks
    with repeated destinations and both relations present"""
    c = R.make_model_case()
    loss, gu, gi, dhu, dhi, arg = R.train_step_ref(c)
    arg = arg.numpy()
    assert np.abs(arg).min() >= 1e-3, np.abs(arg).min()
    assert (arg > 0).any() and (arg < 0).any() and loss.item() > 0
    assert arg.size == 6 * 5 - 3                                          # three (row, negative) pairs carry the row's own positive
    assert all(g.abs().max() > 0 for g in gu + gi) and dhu.abs().max() > 0 and dhi.abs().max() > 0
    for side in ("user", "item"):
        b1, b0 = c[side + "_blocks"][1], c[side + "_blocks"][0]
        assert b1["n_dst"] == (6 if side == "user" else 11) and b0["n_dst"] == b1["n_src"]
        assert np.allclose(R.block_dense(b1, 2).sum(axis=2)[np.diff(b1["row_ptr"]).reshape(-1, 2) > 0], 1.0)
