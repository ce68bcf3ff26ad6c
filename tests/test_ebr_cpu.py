"""CPU checks of EBR's arithmetic and surface: the float64 restatement (tests/ebr_ref.py) against torch autograd of the plain
composition, the tie rules, the library's symbols, constants and plan arithmetic, the model's argument errors, and the input conditions
that the random cases of tests/test_gpu_ebr.py rely on (this is where "the reference alone stays within it" is checked)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import ebr_ref as R
from deep_recommenders_amd.ops import MARGIN_RANK_EPS, margin_rank_fwd      # noqa: F401  (no test of this file runs without the feature)

DD = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(in_batch, ids, seed=0, B=9, S=13, D=8):
    rng = np.random.default_rng(seed)
    S = B if in_batch else S
    q = torch.from_numpy(rng.standard_normal((B, D))).to(DD)
    pos = torch.from_numpy(rng.standard_normal((B, D))).to(DD)
    neg = pos if in_batch else torch.from_numpy(rng.standard_normal((S, D))).to(DD)
    q[4] = 0.0                                                      # a zero row: cosine 0 with everything, the unprojected gradient
    q[5] *= 1e-8                                                    # 0 < sum x^2 < eps
    pos[6] *= 1e-8
    neg[7] = neg[7] * 1e-8 if not in_batch else neg[7]
    assert 0 < float((q[5] ** 2).sum()) < R.EPS and 0 < float((pos[6] ** 2).sum()) < R.EPS
    w = torch.from_numpy(rng.uniform(0.5, 1.5, size=B)).to(DD)
    pos_ids = neg_ids = None
    if ids:
        pos_ids = torch.arange(B) + 100
        pos_ids[2] = -1                                             # padding, holding NaN
        q = q.clone()
        q[2] = math.nan
        if in_batch:
            pos_ids[8] = pos_ids[0]                                 # the same document twice
            neg_ids = pos_ids
        else:
            neg_ids = torch.arange(S) + 300
            neg_ids[3] = neg_ids[9] = pos_ids[0]                    # a duplicate id that is row 0's positive
            neg_ids[11] = -1
    return q, pos, neg, pos_ids, neg_ids, w


@pytest.mark.parametrize("num_hard", [0, 3, 8])
@pytest.mark.parametrize("ids", [True, False])
@pytest.mark.parametrize("in_batch", [True, False])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_closed_form_gradients_equal_autograd_of_the_composition(metric, in_batch, ids, num_hard):
    q, pos, neg, pos_ids, neg_ids, w = _case(in_batch, ids)
    scale, margin = 1.0 / 7.0, 0.3
    qa = torch.where(torch.isnan(q), torch.zeros_like(q), q).clone().requires_grad_(True)        # the padding row: any finite value
    pa = pos.clone().requires_grad_(True)
    na = pa if in_batch else neg.clone().requires_grad_(True)
    rows = R.composition(qa, pa, na, pos_ids, neg_ids, w, margin, metric, in_batch, num_hard)
    (scale * rows.sum()).backward()
    h = R.hand_grads(q, pos, neg, pos_ids, neg_ids, w, margin, metric, in_batch, num_hard, scale)
    assert int(h["active"].sum()) > 0 and (h["active"] < h["keep"].sum(-1)).any()            # both sides of the hinge occur
    torch.testing.assert_close(h["loss"], rows.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(h["d_q"], qa.grad, rtol=1e-12, atol=1e-12)
    if in_batch:
        torch.testing.assert_close(h["d_pos"] + h["d_neg"], pa.grad, rtol=1e-12, atol=1e-12)
    else:
        torch.testing.assert_close(h["d_pos"], pa.grad, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(h["d_neg"], na.grad, rtol=1e-12, atol=1e-12)
    if ids:
        assert h["loss"][2] == 0 and (h["d_q"][2] == 0).all() and (h["d_pos"][2] == 0).all() and torch.isfinite(h["d_neg"]).all()
        assert not h["keep"][0][(neg_ids == pos_ids[0])].any()
    if num_hard > 0:
        assert (h["member"].sum(-1) <= num_hard).all() and (h["hard_idx"] >= 0).sum() == h["member"].sum()


def test_ties_go_to_the_smaller_column_and_a_zero_hinge_is_inactive():
    s = torch.tensor([[2.0, 5.0, 5.0, 1.0, 5.0, 2.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [1.0, 3.0, 3.0, 3.0, 2.0, 3.0]], dtype=DD)
    keep = torch.ones_like(s, dtype=torch.bool)
    keep[2, 1] = False
    member, idx = R.select(s, keep, 4)
    assert idx.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3], [2, 3, 5, 4]]
    assert member.sum(-1).tolist() == [4, 4, 4]
    _, idx = R.select(s[:, :2], keep[:, :2], 3)                                                # fewer kept than asked for: -1 padded
    assert idx.tolist() == [[1, 0, -1], [0, 1, -1], [0, -1, -1]]
    # integer grid, dot metric, integer margin: h == 0 occurs and is inactive
    rng = np.random.default_rng(3)
    q, pos, neg, _, _ = R.inputs((4, 40, 12), False, False, rng, integer=True)
    f = R.forward(q, pos, neg, None, None, None, 2.0, "dot", False, 0)
    assert (f["h"] == 0).any() and not f["act"][f["h"] == 0].any() and f["act"][f["h"] > 0].all()
    want = torch.clamp_min(f["h"], 0).sum(-1)
    assert torch.equal(f["loss"], want) and torch.equal(f["active"], (f["h"] > 0).sum(-1))
    # the same selection by a plain loop, ties included
    f = R.forward(q, pos, neg, None, None, None, 2.0, "dot", False, 3)
    for i in range(12):
        order = sorted(range(40), key=lambda j: (-float(f["s"][i, j]), j))[:3]
        assert f["hard_idx"][i].tolist() == order
    assert len({float(v) for v in f["s"][0].tolist()}) < 40                                    # ties are present


def test_library_exports_the_margin_rank_symbols_and_the_constants_are_those_of_ops():
    from deep_recommenders_amd import build, _lib, ops
    L = ctypes.CDLL(build.build())
    for name in ("dr_margin_rank_fwd", "dr_margin_rank_bwd", "dr_margin_rank_workspace_bytes"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "dr_hotpath.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define DR_MARGIN_RANK_(\w+) (\d+)", header)}
    assert consts == {"TILE": ops.MARGIN_RANK_TILE, "COL_GROUP": ops.MARGIN_RANK_COL_GROUP, "MAX_GROUPS": ops.MARGIN_RANK_MAX_GROUPS,
                      "SPLIT_TILES": ops.MARGIN_RANK_SPLIT_TILES, "ROW_CHUNK": ops.MARGIN_RANK_ROW_CHUNK,
                      "MAX_CHUNKS": ops.MARGIN_RANK_MAX_CHUNKS, "MAX_HARD": ops.MARGIN_RANK_MAX_HARD}
    assert (R.TILE, R.COL_GROUP, R.ROW_CHUNK, R.SPLIT_TILES, R.MAX_HARD) == (consts["TILE"], consts["COL_GROUP"], consts["ROW_CHUNK"],
                                                                             consts["SPLIT_TILES"], consts["MAX_HARD"])
    assert R.EPS == ops.MARGIN_RANK_EPS


def test_plan_and_workspace_arithmetic():
    from deep_recommenders_amd import ops
    for B, S, D in ((1, 1, 4), (3, 65, 20), (257, 257, 20), (257, 200, 64), (8192, 8192, 256), (65536, 65536, 64), (8193, 257, 4)):
        assert ops.margin_rank_row_chunks(B, S, D) == R.plan_chunks(B, S)
        assert ops.margin_rank_col_segments(B, S, D) == R.plan_segments(S)
        groups = ops.margin_rank_col_groups(B, S, D)
        assert groups == (R.plan_segments(S) if -(-B // R.TILE) <= R.SPLIT_TILES else 1)
        for K in (0, 8):
            # norms, segment partials, lists, d_q and d_neg partials: linear in B and in S, never their product
            rows = B if groups > 1 else 0
            cap = 4 * (4 * B + 2 * S + 2 * 8 * B + 2 * 8 * B * 8 * (K > 0) + 2 * groups * B + groups * rows * D
                       + (R.plan_chunks(B, S) + 1) * (S * D + S) + 64)
            assert 0 < ops.margin_rank_workspace_bytes(B, S, D, K) <= cap
    D, S, B = R.MERGE
    assert ops.margin_rank_col_segments(B, S, D) == 3 and ops.margin_rank_row_chunks(B, S, D) == 3 and ops.margin_rank_col_groups(B, S, D) == 3
    assert ops.margin_rank_col_groups(R.TILE * R.SPLIT_TILES + 1, S, D) == 1
    assert ops.margin_rank_workspace_bytes(65536, 65536, 256, 8) <= 160 * 2 ** 20
    for bad in ((8, 8, 6, 0), (8, 8, 260, 0), (8, 0, 8, 0), (-1, 8, 8, 0), (8, 2 ** 31, 8, 0), (8, 8, 8, 9), (8, 8, 8, -1)):
        with pytest.raises(ValueError):
            ops.margin_rank_workspace_bytes(*bad)


def test_model_argument_errors_come_before_the_device():
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.keras.models.retrieval import EBR
    qc = [fc.embedding_column(fc.categorical_column_with_identity("query_tokens", 50), 8)]
    dc = [fc.embedding_column(fc.categorical_column_with_identity("title_tokens", 50), 8)]
    good = dict(query_columns=qc, document_columns=dc, dnn_units_size=[32, 16], device="no-such-device")
    for change, match in ((dict(dnn_units_size=[32, 18]), "multiple of 4"), (dict(dnn_units_size=[32, 260]), r"\[4, 256\]"),
                          (dict(dnn_units_size=[]), "dnn_units_size"), (dict(num_hard_negatives=9), "num_hard_negatives"),
                          (dict(num_hard_negatives=-1), "num_hard_negatives"), (dict(num_hard_negatives=1.5), "num_hard_negatives"),
                          (dict(metric="l2"), "metric"), (dict(activation="gelu"), "activation"), (dict(document_columns=[]), "column")):
        with pytest.raises(ValueError, match=match):
            EBR(**{**good, **change})


def _cases():
    for in_batch, shapes in ((False, R.SHAPES), (True, R.IN_BATCH)):
        for shape in shapes:
            for opt in sorted(R.OPTS):
                for num_hard in R.HARD:
                    yield shape, in_batch, opt, num_hard


def test_the_reference_decides_every_hinge_and_selection_of_the_gpu_cases_with_room():
    """the input conditions of tests/test_gpu_ebr.py's random cases, for the seeds it uses, restated here entry by entry"""
    n = 0
    for shape, in_batch, opt, num_hard in _cases():
        c = R.case(shape, in_batch, opt, num_hard)
        h, b = c["ref"], c["bounds"]
        keep = h["keep"]
        room = (h["h"].abs() / b["b_h"].clamp_min(1e-300))[keep]
        assert room.numel() == 0 or float(room.min()) > 4.0, (shape, in_batch, opt, num_hard)
        if num_hard > 0:
            for i in range(shape[2]):
                kept = torch.nonzero(keep[i]).reshape(-1).tolist()
                ranked = sorted(kept, key=lambda j: (-float(h["s"][i, j]), j))
                for k in range(min(num_hard, len(ranked) - 1)):
                    a, z = ranked[k], ranked[k + 1]
                    assert float(h["s"][i, a] - h["s"][i, z]) > 4.0 * float(b["b_s"][i, a] + b["b_s"][i, z]), (shape, opt, num_hard, i, k)
                assert h["hard_idx"][i].tolist() == (ranked[:num_hard] + [-1] * num_hard)[:num_hard]
        # every earlier seed from the base was refused: the seed is the first
        shapes = R.IN_BATCH if in_batch else R.SHAPES
        base = R.SEED_BASE + 100 * (shapes.index(shape) + (len(R.SHAPES) if in_batch else 0))
        chunks = R.plan_chunks(shape[2], shape[1])
        assert base <= c["seed"] < base + R.SEED_TRIES
        assert not any(R.build(shape, in_batch, opt, num_hard, s, chunks)["ok"] for s in range(base, c["seed"]))
        # both sides of the hinge occur wherever the case is large enough to have them
        if shape[1] >= 63 and shape[2] >= 3:
            act = h["act"]
            assert act.any() and (num_hard > 0 or (h["member"] & ~act).any())          # a short list may hold active columns only
        assert torch.isfinite(h["d_q"]).all() and torch.isfinite(h["d_pos"]).all() and torch.isfinite(h["d_neg"]).all()
        assert float(h["s"][keep].abs().max() if keep.any() else 0.0) <= 1.0 + 1e-6
        n += 1
    assert n == (len(R.SHAPES) + len(R.IN_BATCH)) * 2 * len(R.HARD)


def test_integer_grids_stay_exact_in_fp32():
    """the exact cases: every partial sum of the kernels is an integer below 2^24"""
    assert 9 * max(R.DS) < 2 ** 24
    for in_batch, shapes in ((False, R.SHAPES), (True, R.IN_BATCH)):
        for shape in shapes:
            D, S, B = shape
            worst_s = 9 * D
            worst_h = 2 * worst_s + 4
            assert 2 * S * worst_h < 2 ** 24                         # row_loss with a weight of 2
            assert 2 * B * 3 * 2 + 2 * S * 3 * 2 < 2 ** 24           # the gradient rows: sums of +-3 entries with weights <= 2
            assert 2 * max(B, S) * worst_s < 2 ** 24                 # e_i, f_j, c_i t_i
