"""CPU checks of the FFM restatement the GPU tests compare against (tests/ffm_ref.py) and of the configuration surface of
FieldAwareInteraction, FFM and ops.ffm_*."""
import numpy as np
import pytest
import torch

import ffm_ref as R

DD = torch.float64
NAN = float("nan")


def _hand(diagonal):
    """F = 3, k = 1: A[0,1] = 1, A[0,2] = 2, A[1,0] = 3, A[1,2] = 4, A[2,0] = 5, A[2,1] = 6"""
    return torch.tensor([[[diagonal, 1.0, 2.0], [3.0, diagonal, 4.0], [5.0, 6.0, diagonal]]], dtype=DD)[..., None]


def test_hand_written_case():
    """the pairs that meet are (A[1,0], A[0,1]), (A[2,0], A[0,2]), (A[2,1], A[1,2]): 3 * 1 + 5 * 2 + 6 * 4 = 37; NaN on the diagonal
    reaches neither direction"""
    A = _hand(NAN)
    assert A.shape == (1, 3, 3, 1)
    assert R.interaction(A).tolist() == [37.0]
    d = R.interaction_backward(A, torch.tensor([2.0], dtype=DD))
    assert d[0, :, :, 0].tolist() == [[0, 6, 10], [2, 0, 12], [4, 8, 0]]
    assert R.abs_sum(A).tolist() == [37.0]


def test_swapping_two_fields_changes_which_blocks_meet():
    """block j of a row means "towards field j": renumbering the fields consistently (rows and blocks) keeps the sum, handing field 0's
    row to field 1 and back without renumbering the blocks pairs other blocks: 7 * 7 + 5 * 4 + 6 * 2 = 81"""
    A = _hand(7.0)
    perm = [1, 0, 2]
    assert R.interaction(A[:, perm][:, :, perm]).tolist() == [37.0]
    assert R.interaction(A[:, perm]).tolist() == [81.0]


def test_equal_blocks_give_the_fm_second_order_term():
    rng = np.random.default_rng(0)
    B, F, k = 5, 7, 6
    e = torch.from_numpy(rng.normal(size=(B, F, k)))
    A = e[:, :, None, :].expand(B, F, F, k).contiguous()                                      # A[i, j, :] = e_i for every j
    fm = 0.5 * ((e.sum(1) ** 2) - (e ** 2).sum(1)).sum(-1)
    assert (R.interaction(A) - fm).abs().max().item() <= 1e-12


@pytest.mark.parametrize("B,F,k", [(3, 2, 4), (4, 5, 3), (2, 16, 8)])
def test_closed_form_backward_equals_autograd(B, F, k):
    rng = np.random.default_rng(100 * F + k)
    A = torch.from_numpy(rng.normal(size=(B, F, F, k))).requires_grad_(True)
    d = torch.from_numpy(rng.normal(size=(B,)))
    want, = torch.autograd.grad((R.interaction(A) * d).sum(), [A])
    with torch.no_grad():
        got = R.interaction_backward(A, d)
    assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    idx = torch.arange(F)
    assert (got[:, idx, idx] == 0).all()


def test_gather_and_first_order_of_the_restatement():
    table = torch.arange(5 * 2 * 2 * 1, dtype=DD).reshape(10, 2)                              # F = 2, k = 1, two fields of 5 rows
    ids = torch.tensor([[1, 2], [-1, 4]])
    base = torch.tensor([0, 5])
    A = R.gather(table, ids, base, 2, 1)
    assert A[0, :, :, 0].tolist() == [[2, 3], [14, 15]] and A[1, :, :, 0].tolist() == [[0, 0], [18, 19]]
    lin = torch.arange(10, dtype=DD)
    assert R.first_order(lin, torch.tensor([0.5], dtype=DD), ids, base).tolist() == [0.5 + 1 + 7, 0.5 + 9]


def _columns(F=4, k=8, dims=None):
    from deep_recommenders_amd import feature_column as fc
    cats = [fc.categorical_column_with_identity("c%d" % i, 50) for i in range(F)]
    dims = dims or [k] * F
    return [fc.indicator_column(c) for c in cats], [fc.embedding_column(c, d) for c, d in zip(cats, dims)]


def test_ffm_config_and_constructor_errors():
    from deep_recommenders_amd.keras.models.ranking import FFM, FieldAwareInteraction
    ind, emb = _columns()
    model = FFM(ind, emb, device="cpu", name="f")
    assert model.get_config() == {"name": "f", "num_fields": 4, "latent_dim": 8}
    assert model.slab.D == 4 * 8 and model.slab.table.shape == (4 * 50, 32) and model.slab.lin_w.shape == (200,)
    assert model.slab.keys == ["c0", "c1", "c2", "c3"]
    assert model.slab.table.abs().max().item() <= 2.0 / np.sqrt(8) + 1e-6                      # truncated at 2 sigma, sigma = 1 / sqrt(k)
    assert 0.2 < model.slab.table.std().item() < 0.4
    with pytest.raises(ValueError, match="at least 2"):
        FFM(*_columns(F=1), device="cpu")
    with pytest.raises(ValueError, match="must be equal"):
        FFM(*_columns(dims=[8, 8, 4, 8]), device="cpu")
    with pytest.raises(ValueError, match=r"F \* k = 33 \* 8 = 264 exceeds the slab's limit of 256"):
        FFM(*_columns(F=33, k=8), device="cpu")
    with pytest.raises(ValueError, match="multiple of 4"):
        FFM(*_columns(k=6), device="cpu")
    with pytest.raises(ValueError, match="indicator columns"):
        FFM(None, emb, device="cpu")
    with pytest.raises(ValueError, match="indicator columns"):
        FFM([], emb, device="cpu")
    assert FieldAwareInteraction().get_config() == {}
    assert FieldAwareInteraction(name="x").get_config() == {"name": "x"}
    with pytest.raises(ValueError, match="dim should be 3 or 4"):
        FieldAwareInteraction()(np.zeros((2, 12), np.float32))
    with pytest.raises(ValueError, match=r"\[B, F, F \* k\]"):
        FieldAwareInteraction()(np.zeros((2, 3, 8), np.float32))
    with pytest.raises(ValueError, match=r"\[B, F, F, k\]"):
        FieldAwareInteraction()(np.zeros((2, 3, 2, 4), np.float32))


def test_a_column_initializer_sees_the_wide_rows():
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.keras.models.ranking import FFM
    seen = []
    cats = [fc.categorical_column_with_identity("c%d" % i, 10 + i) for i in range(3)]
    emb = [fc.embedding_column(c, 4, initializer=(lambda rows: seen.append(tuple(rows.shape)) or rows.fill_(0.5)) if i == 1 else None)
           for i, c in enumerate(cats)]
    model = FFM([fc.indicator_column(c) for c in cats], emb, device="cpu")
    assert seen == [(11, 12)]
    assert (model.slab.embedding_weights("c1") == 0.5).all() and not (model.slab.embedding_weights("c0") == 0.5).any()


def test_field_order_comes_from_the_columns_not_from_the_inputs():
    from deep_recommenders_amd.keras.models.ranking import FFM
    model = FFM(*_columns(), device="cpu")
    rng = np.random.default_rng(1)
    inputs = {"c%d" % i: rng.integers(0, 50, size=(6, 1)) for i in range(4)}
    permuted = {k: inputs[k] for k in ("c2", "c0", "c3", "c1")}
    ids, col_start, row_base = model.slab.transform(inputs, model.slab.keys)
    ids2, col_start2, row_base2 = model.slab.transform(permuted, model.slab.keys)
    assert col_start is None and col_start2 is None
    assert torch.equal(ids, ids2) and torch.equal(row_base, row_base2)
    assert torch.equal(ids, torch.from_numpy(np.concatenate([inputs["c%d" % i] for i in range(4)], axis=1)))
    assert row_base.tolist() == [0, 50, 100, 150]
    del permuted["c3"]
    with pytest.raises(ValueError, match="'c3' is missing"):
        model.logits(permuted)


def test_row_width_and_argument_errors_need_no_device():
    from deep_recommenders_amd import ops
    assert ops.ffm_row_width(26, 4) == 104 and ops.ffm_row_width(64, 4) == 256 and ops.ffm_row_width(2, 128) == 256
    z = torch.zeros
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64)                                         # noqa: E731
    for call in (lambda F, k: ops.ffm_row_width(F, k),
                 lambda F, k: ops.ffm_fwd(z((2, F * F * k)), F, k),
                 lambda F, k: ops.ffm_bwd(z((2, F * F * k)), F, k, z(2)),
                 lambda F, k: ops.ffm_gather_fwd(i64(2, F), i64(F), z((5, F * k)), F, k),
                 lambda F, k: ops.ffm_gather_bwd(i64(2, F), i64(F), z((5, F * k)), F, k, z(2))):
        with pytest.raises(ValueError, match="multiple of 4"):
            call(3, 6)
        with pytest.raises(ValueError, match="2 <= F <= 64"):
            call(1, 8)
        with pytest.raises(ValueError, match="2 <= F <= 64"):
            call(65, 4)
        with pytest.raises(ValueError, match=r"F \* k <= 256"):
            call(65 // 5, 20 + 4)                                                              # 13 * 24 = 312
        with pytest.raises(ValueError, match=r"F \* k <= 256"):
            call(5, 52)                                                                        # 260
    with pytest.raises(ValueError, match="row stride"):                                        # ld = 50 for 48 columns: not a multiple of 4
        ops.ffm_fwd(z((2, 50))[:, :48], 2, 12)
    with pytest.raises(ValueError, match=r"F \* F \* k columns"):
        ops.ffm_fwd(z((2, 40)), 2, 12)
    with pytest.raises(ValueError, match="one value per example"):
        ops.ffm_bwd(z((2, 48)), 2, 12, z(3))
    with pytest.raises(ValueError, match="ids must be int64"):
        ops.ffm_gather_fwd(i64(2, 3), i64(2), z((5, 24)), 2, 12)
    with pytest.raises(ValueError, match="table must be"):
        ops.ffm_gather_fwd(i64(2, 2), i64(2), z((5, 20)), 2, 12)


def test_kernel_source_has_no_atomics_and_no_allocation():
    """the contract's static half: every sum has one owner (no atomic of any kind), the entry points take no workspace and the file
    allocates nothing and reads no environment"""
    import os
    import re
    from deep_recommenders_amd import build
    src = open(os.path.join(build.CSRC, "ffm.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    code = re.sub(r"/\*.*?\*/", "", code, flags=re.S)
    assert "ffm_fwd_kernel" in code and "dr_ffm_gather_bwd" in code
    for word in ("atomic", "hipMalloc", "hipMemcpy", "getenv", "__shared__"):
        assert word not in code, word


def test_header_library_and_signatures_agree_on_the_entry_points():
    from deep_recommenders_amd import _lib
    import ctypes
    sig = _lib.SIGNATURES
    assert [len(sig[n][1]) for n in ("dr_ffm_fwd", "dr_ffm_bwd", "dr_ffm_gather_fwd", "dr_ffm_gather_bwd")] == [7, 9, 11, 10]
    L = _lib.lib()
    for n in ("dr_ffm_fwd", "dr_ffm_bwd", "dr_ffm_gather_fwd", "dr_ffm_gather_bwd"):
        assert getattr(L, n).restype is ctypes.c_int
