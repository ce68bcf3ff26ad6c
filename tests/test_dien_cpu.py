"""CPU checks of the DIEN restatement the GPU tests compare against (tests/dien_ref.py), of the inputs those tests use, of the C
interface of csrc/dien.hip and of the configuration surface of the DIEN classes."""
import numpy as np
import pytest
import torch

import dien_ref as R

DD = torch.float64
ENTRY_POINTS = ("dr_gru_seq_fwd", "dr_gru_seq_bwd", "dr_gru_seq_bwd_workspace_bytes", "dr_seq_attn_fwd", "dr_seq_attn_bwd")


def _close(got, want, tol=1e-12):
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("B,T,D,H", [(3, 5, 6, 4), (2, 9, 3, 8)])
def test_forward_equals_torch_gru_under_the_sign_mapping(B, T, D, H):
    """torch.nn.GRU: z = sigmoid(.), h' = (1 - z) n + z h, so z = 1 - u: the u columns change sign (sigmoid(-x) = 1 - sigmoid(x)); its
    gate order is r, z, n; its reset gate multiplies (h W_hn + b_hn) like the paper's form when bias_hh = 0."""
    rng = np.random.default_rng(B * 100 + T)
    t = lambda *s: torch.from_numpy(rng.normal(size=s))                                       # noqa: E731
    seq, W, b, U, h0 = t(B, T, D), t(D, 3 * H), t(3 * H), t(H, 3 * H) / np.sqrt(H), t(B, H)
    hs, h_last = R.gru_layer(seq, W, b, U, h0=h0)
    gru = torch.nn.GRU(D, H, batch_first=True).double()
    u, r, c = slice(0, H), slice(H, 2 * H), slice(2 * H, 3 * H)
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.cat([W[:, r], -W[:, u], W[:, c]], dim=1).t())
        gru.weight_hh_l0.copy_(torch.cat([U[:, r], -U[:, u], U[:, c]], dim=1).t())
        gru.bias_ih_l0.copy_(torch.cat([b[r], -b[u], b[c]]))
        gru.bias_hh_l0.zero_()
        want, hn = gru(seq, h0[None])
    _close(hs, want)
    _close(h_last, hn[0])


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_hand_written_backward_equals_autograd(index):
    shape, with_att, seed = R.CASES[index]
    c = R.draw(shape, with_att, seed)
    names = [k for k in ("xp", "U", "h0", "att") if c[k] is not None]
    leaves = {k: c[k].clone().requires_grad_(True) for k in names}
    hs, h_last = R.forward(leaves["xp"], leaves["U"], leaves["h0"], c["lengths"], leaves.get("att"))
    want = torch.autograd.grad((hs * c["d_hs"]).sum() + (h_last * c["d_h_last"]).sum(), [leaves[k] for k in names])
    with torch.no_grad():
        d_xp, dU, d_h0, d_att = R.backward(c["xp"], c["U"], c["h0"], c["lengths"], c["att"], c["d_hs"], c["d_h_last"])
    got = dict(xp=d_xp, U=dU, h0=d_h0, att=d_att)
    for k, w in zip(names, want):
        _close(got[k], w)
    # masked steps: exact zeros, and the state is carried
    lens = c["lengths"].long()
    on = torch.arange(shape[1])[None, :] < lens[:, None]
    assert (hs.detach()[~on] == 0).all() and (d_xp[~on] == 0).all() and (d_att is None or (d_att[~on] == 0).all())
    empty = lens == 0
    assert torch.equal(h_last.detach()[empty], c["h0"][empty]) and torch.equal(d_h0[empty], c["d_h_last"][empty])


def test_the_cases_hold_the_forced_lengths_and_float32_values():
    assert [s for s, w, _ in R.CASES if w == 0] == R.SHAPES and [s for s, w, _ in R.CASES if w == 1] == R.SHAPES
    for shape, with_att, seed in R.CASES:
        B, T, H = shape
        c = R.draw(shape, with_att, seed)
        for k in ("xp", "U", "h0", "d_hs", "d_h_last", "q", "d_a") + (("att",) if with_att else ()):
            assert torch.equal(c[k], c[k].float().double())
        assert (c["att"] is not None) == bool(with_att)
        lens = c["lengths"]
        assert lens.dtype == torch.int32 and 0 <= int(lens.min()) and int(lens.max()) <= T
        if B >= 3:
            assert lens[:3].tolist() == [T, 1, 0]
        if shape == (70, 33, 32):
            assert set(lens.tolist()) == set(range(T + 1))


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_another_fp32_association_stays_within_the_limit(index):
    """what tests/test_gpu_dien.py allows the kernel: 16 max(r32, 8u) holds a deliberately different fp32 evaluation (k-chunks of 4
    added last chunk first, exp2-based gates, reversed row sums) with room to spare"""
    shape, with_att, seed = R.CASES[index]
    c = R.draw(shape, with_att, seed)
    want, ref32, alt = R.run(c, DD), R.run(c, torch.float32), R.run(c, torch.float32, R.ALT)
    for name, w, r, a in zip(R.NAMES, want, ref32, alt):
        if w is None:
            continue
        r32, err = R.rel_err(r, w), R.rel_err(a, w)
        print("%s %s: r32 = %.2f u, other association %.2f u, %.3f of the limit" % (name, shape, r32 / R.U24, err / R.U24, err / R.limit(r32)))
        assert err <= R.limit(r32), (name, err, R.limit(r32))


def test_attention_restatement():
    rng = np.random.default_rng(5)
    t = lambda *s: torch.from_numpy(rng.normal(size=s))                                       # noqa: E731
    hs, q, d_a = t(4, 6, 8).requires_grad_(True), t(4, 8).requires_grad_(True), t(4, 6)
    lens = torch.tensor([6, 1, 0, 3], dtype=torch.int32)
    a = R.attention(hs, q, lens)
    _close(a.detach().sum(1), torch.tensor([1.0, 1.0, 0.0, 1.0], dtype=DD))
    assert (a.detach()[1, 1:] == 0).all() and (a.detach()[2] == 0).all() and (a.detach()[3, 3:] == 0).all()
    _close(a.detach()[3, :3], torch.softmax((hs.detach()[3, :3] * q.detach()[3]).sum(-1), dim=0))
    a32 = R.attention(hs.detach().float(), q.detach().float(), lens)                           # the float32 run has no 0 / 0 either
    assert torch.isfinite(a32).all() and (a32[2] == 0).all() and (a32.double() - a.detach()).abs().max() < 1e-6
    want = torch.autograd.grad((a * d_a).sum(), [hs, q])
    with torch.no_grad():
        got = R.attention_backward(hs.detach(), q.detach(), lens, d_a)
    _close(got[0], want[0])
    _close(got[1], want[1])


def test_header_declares_and_the_library_exports_the_entry_points():
    import ctypes
    from deep_recommenders_amd import _lib
    sigs = _lib.SIGNATURES
    for name in ENTRY_POINTS:
        assert name in sigs, name
    assert sigs["dr_gru_seq_bwd_workspace_bytes"][0] is ctypes.c_int64 and len(sigs["dr_gru_seq_bwd_workspace_bytes"][1]) == 3
    assert len(sigs["dr_gru_seq_fwd"][1]) == 13 and len(sigs["dr_gru_seq_bwd"][1]) == 22
    assert len(sigs["dr_seq_attn_fwd"][1]) == 9 and len(sigs["dr_seq_attn_bwd"][1]) == 13
    lib = _lib.lib()
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
    # the domain answers need no device
    assert lib.dr_gru_seq_bwd_workspace_bytes(0, 3, 8) == 0
    assert lib.dr_gru_seq_bwd_workspace_bytes(2, 3, 8) >= 4 * 2 * 4 * 24
    for B, T, H, want in ((2, 3, 6, _lib.DR_EINVAL), (2, 0, 8, _lib.DR_EINVAL), (-1, 3, 8, _lib.DR_EINVAL), (2, 3, 0, _lib.DR_EINVAL),
                          (2, 3, 132, _lib.DR_ESHAPE)):
        assert lib.dr_gru_seq_bwd_workspace_bytes(B, T, H) == want, (B, T, H)
    assert lib.dr_gru_seq_fwd(None, 24, None, None, None, None, 0, 3, 8, None, 8, None, None) == _lib.DR_OK       # B = 0 launches nothing
    assert lib.dr_gru_seq_fwd(None, 24, None, None, None, None, 0, 3, 6, None, 8, None, None) == _lib.DR_EINVAL
    assert lib.dr_gru_seq_fwd(None, 24, None, None, None, None, 0, 3, 132, None, 132, None, None) == _lib.DR_ESHAPE
    assert lib.dr_seq_attn_fwd(None, 8, None, None, 0, 3, 8, None, None) == _lib.DR_OK
    assert lib.dr_seq_attn_fwd(None, 6, None, None, 0, 3, 8, None, None) == _lib.DR_EINVAL


def test_classes_are_exported_and_get_config_round_trips():
    from deep_recommenders_amd.keras.models import ranking
    from deep_recommenders_amd.keras.models.ranking import AUGRU, DIEN, GRU, InterestEvolution, InterestExtractor
    from deep_recommenders_amd.keras.models.ranking.din import Dice
    for cls in (AUGRU, DIEN, GRU, InterestEvolution, InterestExtractor):
        assert getattr(ranking, cls.__name__) is cls
    for cls in (GRU, AUGRU):
        cfg = dict(units=12, use_bias=False, kernel_init="truncated_normal", recurrent_init="glorot_uniform", bias_init="ones")
        assert cls(**cfg).get_config() == cfg and cls(**cls(**cfg).get_config()).get_config() == cfg
        assert cls(8).get_config() == dict(units=8, use_bias=True, kernel_init="glorot_uniform", recurrent_init="glorot_uniform",
                                           bias_init="zeros")
        for units in (6, 132, 0):
            with pytest.raises(ValueError, match="units"):
                cls(units)
    for cls in (InterestExtractor, InterestEvolution):
        assert cls(16).get_config() == {"units": 16} and cls(**cls(16, name="x").get_config()).get_config() == {"name": "x", "units": 16}
    cfg = dict(num_items=50, embedding_dim=8, gru_units=8, dnn_units_size=(20, 10), activation="relu", use_auxiliary_loss=False)
    model = DIEN(device="cpu", **cfg)
    assert model.get_config() == cfg and DIEN(device="cpu", **model.get_config()).get_config() == cfg
    assert tuple(model.item_table.shape) == (50, 8)
    assert DIEN(50, 8, 8, device="cpu").get_config() == dict(num_items=50, embedding_dim=8, gru_units=8, dnn_units_size=(200, 80),
                                                            activation=Dice, use_auxiliary_loss=True)
    with pytest.raises(ValueError, match="gru_units == embedding_dim"):
        DIEN(50, 8, 12, device="cpu")
    with pytest.raises(ValueError, match="embedding_dim"):
        DIEN(50, 6, 6, device="cpu")
    layer = GRU(8)
    layer.build(5, device="cpu")
    assert tuple(layer.kernel.shape) == (5, 24) and tuple(layer.recurrent_kernel.shape) == (8, 24) and tuple(layer.bias.shape) == (24,)


def test_argument_errors_need_no_device_and_there_is_no_fallback():
    from deep_recommenders_amd import layers, ops
    from deep_recommenders_amd.keras.models.ranking import DIEN, GRU
    z = torch.zeros
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.gru_seq_fwd(z(2, 3, 18), z(6, 18))
    with pytest.raises(ValueError, match=r"\[4, 128\]"):
        ops.gru_seq_fwd(z(2, 3, 396), z(132, 396))
    with pytest.raises(ValueError, match="T >= 1"):
        ops.gru_seq_fwd(z(2, 0, 24), z(8, 24))
    with pytest.raises(ValueError, match="xp"):
        ops.gru_seq_fwd(z(2, 3, 20), z(8, 24))
    with pytest.raises(ValueError, match="h0"):
        ops.gru_seq_fwd(z(2, 3, 24), z(8, 24), h0=z(3, 8))
    with pytest.raises(ValueError, match="lengths"):
        ops.gru_seq_fwd(z(2, 3, 24), z(8, 24), lengths=z(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="att"):
        ops.gru_seq_fwd(z(2, 3, 24), z(8, 24), att=z(2, 4))
    with pytest.raises(ValueError, match="hs"):
        ops.gru_seq_fwd(z(2, 3, 24), z(8, 24), hs=z(2, 3, 9)[:, :, :8])
    with pytest.raises(ValueError, match="d_hs"):
        ops.gru_seq_bwd(z(2, 3, 24), z(8, 24), None, None, None, z(2, 3, 8), d_hs=z(2, 3, 4))
    with pytest.raises(ValueError, match="seq_attn"):
        ops.seq_attn_fwd(z(2, 3, 8), z(2, 4))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.seq_attn_fwd(z(2, 3, 6), z(2, 6))
    if not torch.cuda.is_available():
        # in-domain calls on host tensors: the package's RuntimeError, nothing is computed in torch
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.gru_seq_fwd(z(2, 3, 24), z(8, 24))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            layers.gru_sequence(z(2, 3, 24), z(8, 24))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            layers.sequence_attention(z(2, 3, 8), z(2, 8))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            GRU(8)(np.zeros((2, 3, 5), np.float32))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            DIEN(50, 8, 8, device="cpu")(np.zeros((2, 3), np.int64), np.array([3, 1]), np.zeros(2, np.int64))


def test_kernel_source_has_no_atomics_and_no_allocation():
    import os
    import re
    from deep_recommenders_amd import build
    src = open(os.path.join(build.CSRC, "dien.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in code
    for word in ("atomic", "hipMalloc", "hipMemcpy", "getenv"):
        assert word not in code, word
