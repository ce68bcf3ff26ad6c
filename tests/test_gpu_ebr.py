"""GPU tests of the margin-ranking kernels (csrc/margin_rank.hip), their Python surface (ops.margin_rank_fwd / _bwd, layers.margin_rank)
and the EBR model against the float64 restatement in tests/ebr_ref.py.

Tolerances: U = 2^-24, first order in U, derived in the header of tests/ebr_ref.py from fp32 rounding (the chain of D products, the two
inverse norms with the 1 / sqrt allowance measured on the CPU at import against float64 and the project's margin of 4, the number of
additions a term goes through); none is read off the kernel.  The hinge and the selection are discontinuous, so the random cases use
inputs that the float64 reference decides with room (tests/test_ebr_cpu.py asserts it for the seeds used here): row_active and hard_idx
are compared exactly and no entry is excluded from any bound.
  exact cases   integer grids with 9 D < 2^24, metric dot, integer margin and weights, row_scale 1: every partial sum is an integer below
                2^24, so scores, pos_score, row_loss, row_active, hard_idx and the three gradients equal float64 rounded to fp32 bit for
                bit, exact score ties and h == 0 included.
  the model     the towers' .grad against the float64 composition of the whole step restarted from the device's parameters: the layer
                tolerance of tests/test_gpu_gcn.py (rtol 1e-4 / atol 1e-4)."""
import math

import numpy as np
import pytest
import torch

import ebr_ref as R

pytestmark = pytest.mark.gpu

DD = torch.float64
U = R.U


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _within(got, want, bound, what):
    err = (got.detach().double().cpu().reshape(want.shape) - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print("%s: max |err| / bound = %.3f" % (what, ratio))
    assert (err <= bound).all(), "%s: max |err| / bound = %.3f" % (what, ratio)
    return ratio


def _wide(t, fill=math.nan):
    """t [B, D] fp32 as a view of a wider NaN-filled device buffer (pitch D + 8, starting at column 4)"""
    buf = torch.full((t.shape[0], t.shape[1] + 8), fill, dtype=torch.float32, device="cuda")
    view = buf[:, 4:4 + t.shape[1]]
    view.copy_(t)
    return buf, view


def _slack(t):
    """t [N, D] as the first N rows of a table whose last row is NaN and named by no index"""
    buf = torch.full((t.shape[0] + 1, t.shape[1]), math.nan, dtype=torch.float32, device="cuda")
    buf[:t.shape[0]].copy_(t)
    return buf[:t.shape[0]]


def _f(t):
    return None if t is None else t.float().cuda()


def _run(c, sl=slice(None), num_hard=None, want_scores=True, separate=False):
    """forward and backward of rows `sl` of the case (separate negatives only), q and d_q as views of wider NaN-filled buffers"""
    from deep_recommenders_amd import ops
    K = c["num_hard"] if num_hard is None else num_hard
    _, q = _wide(c["q"][sl].float())
    pos = _slack(c["pos"][sl].float())
    neg = None if c["neg"] is None else _slack(c["neg"].float())
    pos_ids = None if c["pos_ids"] is None else c["pos_ids"][sl].cuda()
    neg_ids = None if c["neg_ids"] is None else c["neg_ids"].cuda()
    w = None if c["w"] is None else _f(c["w"][sl])
    if separate:                                    # the in-batch case as a separate-negative call on the same buffer
        neg, neg_ids = pos, (pos_ids if neg_ids is None else neg_ids)
    kw = dict(pos_ids=pos_ids, neg_ids=neg_ids, sample_weight=w, margin=c["margin"], metric=c["metric"], num_hard=K)
    t, loss, active, hard, scores = ops.margin_rank_fwd(q, pos, neg, want_scores=want_scores, **kw)
    dq_buf, dq = _wide(torch.zeros(q.shape))
    d_q, d_pos, d_neg = ops.margin_rank_bwd(q, pos, neg, t, hard, row_scale=c["scale"], d_q=dq, **kw)
    assert d_q.data_ptr() == dq.data_ptr()
    assert torch.isnan(dq_buf[:, :4]).all() and torch.isnan(dq_buf[:, 4 + q.shape[1]:]).all()       # nothing beyond D columns
    return dict(t=t, loss=loss, active=active, hard=hard, s=scores, d_q=d_q, d_pos=d_pos, d_neg=d_neg)


def _all_shapes():
    return [(s, False) for s in R.SHAPES] + [(s, True) for s in R.IN_BATCH]


def _id(v):
    return "%s%s" % ("x".join(str(x) for x in v[0]), "ib" if v[1] else "")


def test_constants_are_those_of_ops():
    from deep_recommenders_amd import ops
    assert (R.TILE, R.COL_GROUP, R.ROW_CHUNK, R.SPLIT_TILES, R.MAX_HARD) == (ops.MARGIN_RANK_TILE, ops.MARGIN_RANK_COL_GROUP,
                                                                             ops.MARGIN_RANK_ROW_CHUNK, ops.MARGIN_RANK_SPLIT_TILES,
                                                                             ops.MARGIN_RANK_MAX_HARD)
    D, S, B = R.MERGE
    assert ops.margin_rank_col_groups(B, S, D) == 3 and ops.margin_rank_row_chunks(B, S, D) == 3


@pytest.mark.parametrize("shape_ib", _all_shapes(), ids=_id)
def test_integer_grids_are_exact(shape_ib):
    shape, in_batch = shape_ib
    D, S, B = shape
    for use_ids in (True, False):
        rng = np.random.default_rng(20 + 2 * (R.SHAPES + R.IN_BATCH).index(shape) + use_ids)
        q, pos, neg, pos_ids, neg_ids = R.inputs(shape, in_batch, use_ids, rng, integer=True)
        w = torch.from_numpy(rng.integers(1, 3, size=B)).to(DD) if use_ids else None
        for K in R.HARD:
            c = dict(q=q, pos=pos, neg=neg, pos_ids=pos_ids, neg_ids=neg_ids, w=w, scale=1.0, metric="dot", margin=2.0, num_hard=K)
            n_eff, nid_eff = (pos, pos_ids) if in_batch else (neg, neg_ids)
            h = R.hand_grads(q, pos, n_eff, pos_ids, nid_eff, w, 2.0, "dot", in_batch, K, 1.0)
            got = _run(c)
            keep = h["keep"]
            want_s = h["s"].masked_fill(~keep, -math.inf).float()
            tag = (shape, in_batch, use_ids, K)
            assert _bits_equal(got["s"].cpu() + 0.0, want_s + 0.0), tag                         # + 0.0: a zero's sign is no rounding
            t_want = torch.where(h["valid"], h["t"], torch.zeros_like(h["t"])).float()
            assert _bits_equal(got["t"].cpu() + 0.0, t_want + 0.0), tag
            assert _bits_equal(got["loss"].cpu() + 0.0, h["loss"].float() + 0.0), tag
            assert torch.equal(got["active"].cpu().long(), h["active"]), tag
            if K > 0:
                assert torch.equal(got["hard"].cpu().long(), h["hard_idx"]), tag
            for k, r in (("d_q", "d_q"), ("d_pos", "d_pos"), ("d_neg", "d_neg")):
                assert _bits_equal(got[k].cpu() + 0.0, h[r].float() + 0.0), (k,) + tag
    if S >= 63 and B >= 64:
        assert (h["h"][h["keep"]] == 0).any()                                                   # h == 0 occurs, and was decided as inactive


@pytest.mark.parametrize("opt", sorted(R.OPTS))
@pytest.mark.parametrize("shape_ib", _all_shapes(), ids=_id)
def test_random_inputs_within_the_derived_bounds(shape_ib, opt):
    shape, in_batch = shape_ib
    D, S, B = shape
    for K in R.HARD:
        c = R.case(shape, in_batch, opt, K)
        assert c["ok"]
        r, b, got = c["ref"], c["bounds"], _run(c)
        tag = "D %d S %d B %d %s%s hard %d " % (D, S, B, opt, " in-batch" if in_batch else "", K)
        keep, valid = r["keep"], r["valid"]
        s = got["s"].cpu()
        assert (s[~keep] == -math.inf).all()
        _within(torch.where(keep, s, torch.zeros_like(s)), r["s0"], b["b_s"], tag + "scores")
        _within(got["t"], torch.where(valid, r["t"], torch.zeros_like(r["t"])), b["b_t"], tag + "pos_score")
        assert torch.equal(got["active"].cpu().long(), r["active"]), tag + "row_active"
        if K > 0:
            assert torch.equal(got["hard"].cpu().long(), r["hard_idx"]), tag + "hard_idx"
        _within(got["loss"], r["loss"], b["b_loss"], tag + "row_loss")
        _within(got["d_q"], r["d_q"], b["b_dq"], tag + "d_q")
        _within(got["d_pos"], r["d_pos"], b["b_dpos"], tag + "d_pos")
        _within(got["d_neg"], r["d_neg"], b["b_dneg"], tag + "d_neg")
        pad = ~valid
        for k in ("t", "loss", "active", "d_q", "d_pos"):                                       # a padding row: zeros, its NaN reaches nothing
            assert (got[k].cpu()[pad] == 0).all(), k
        if K > 0:
            assert (got["hard"].cpu()[pad] == -1).all()
        assert (got["d_neg"].cpu()[~r["nok"]] == 0).all()
        assert all(torch.isfinite(got[k]).all() for k in ("t", "loss", "d_q", "d_pos", "d_neg"))


ROW_KEYS = ("t", "loss", "active", "hard", "d_q", "d_pos")
BIG = (4, 2 * R.COL_GROUP + 1, R.TILE * R.SPLIT_TILES + 1)          # more row tiles than SPLIT_TILES: one block walks every segment


def _gauss_case(shape, K, seed, metric="cosine"):
    D, S, B = shape
    rng = np.random.default_rng(seed)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DD)          # noqa: E731
    return dict(q=t(B, D), pos=t(B, D), neg=t(S, D), pos_ids=None, neg_ids=None, w=None, scale=1.0 / B, metric=metric, margin=0.25,
                num_hard=K, in_batch=False)


@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("shape", [(64, 65, 257), (256, 65, 257), (64, 200, 257), R.MERGE, BIG])
def test_bit_identical_runs_and_batch_independent_rows(shape, K):
    """reruns give the same bits; a row's outputs are the same bits in a batch of 1, of 3 and of B against the same negatives -- for BIG
    that is also the one-block form (B rows) against the split form (1 and 3 rows)"""
    from deep_recommenders_amd import ops
    D, S, B = shape
    if shape == BIG:
        c = _gauss_case(shape, K, 99)
        assert ops.margin_rank_col_groups(B, S, D) == 1 and ops.margin_rank_col_groups(1, S, D) == 3
    else:
        c = R.case(shape, False, "all", K)
    a, b = _run(c, want_scores=False), _run(c, want_scores=False)
    assert a["s"] is None
    for k in a:
        if a[k] is not None:
            assert _bits_equal(a[k], b[k]), k
    for i in (0, 2, B // 2, B - 2):
        one, three = _run(c, sl=slice(i, i + 1), want_scores=False), _run(c, sl=slice(i - 1 if i else 0, (i - 1 if i else 0) + 3), want_scores=False)
        at = 1 if i else 0
        for k in ROW_KEYS:
            if a[k] is None:
                continue
            assert _bits_equal(one[k].reshape(-1), a[k][i].reshape(-1)), (k, i)
            assert _bits_equal(three[k][at].reshape(-1), a[k][i].reshape(-1)), (k, i)


@pytest.mark.parametrize("K", R.HARD)
@pytest.mark.parametrize("B", [3, 64, 257])
def test_in_batch_equals_the_separate_call_on_the_same_buffer(B, K):
    """in_batch with neg = pos against the separate-negative call with neg_ids = pos_ids = arange(B), bit for bit"""
    for metric in ("cosine", "dot"):
        c = dict(R.case((64, B, B), True, "plain", K))
        c["metric"] = metric
        c["pos_ids"] = torch.arange(B, dtype=torch.int64)
        a = _run(c)                                                 # in-batch: the diagonal by position (and by id)
        b = _run(c, separate=True)                                  # separate: the diagonal by id alone
        c["pos_ids"] = None
        plain = _run(c)                                             # and without ids the position alone masks it
        for k in a:
            if a[k] is not None:
                assert _bits_equal(a[k], b[k]) and _bits_equal(a[k], plain[k]), (k, metric)


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_a_list_as_long_as_the_kept_columns_gives_the_bits_of_no_list(metric):
    """num_hard >= the number of kept columns equals num_hard = 0 bit for bit, in loss and gradients: a few columns in one tile, and six
    kept columns spread over three segments of 300"""
    for shape, kept in (((64, 7, 257), None), ((20, 300, 67), (0, 5, 70, 130, 131, 299))):
        c = _gauss_case(shape, 8, 5 + shape[1], metric)
        if kept is not None:
            c["neg_ids"] = torch.full((shape[1],), -1, dtype=torch.int64)
            c["neg_ids"][list(kept)] = torch.arange(len(kept))
        a, b = _run(c, num_hard=8), _run(c, num_hard=0)
        assert int(a["active"].sum()) > 0 and (a["hard"] >= 0).sum() == shape[2] * (len(kept) if kept else shape[1])
        for k in ("t", "loss", "active", "s", "d_q", "d_pos", "d_neg"):
            assert _bits_equal(a[k], b[k]), (k, shape)


def test_empty_batch_refusals_and_the_layer():
    from deep_recommenders_amd import layers, ops
    q, pos, neg = (torch.randn(n, 8, device="cuda") for n in (4, 4, 5))
    t, loss, active, hard, s = ops.margin_rank_fwd(q[:0], pos[:0], neg, num_hard=2, want_scores=True)
    assert t.shape == loss.shape == active.shape == (0,) and hard.shape == (0, 2) and s.shape == (0, 5)
    d_q, d_pos, d_neg = ops.margin_rank_bwd(q[:0], pos[:0], neg, t, hard, num_hard=2)
    assert d_q.shape == d_pos.shape == (0, 8) and d_neg.shape == (5, 8) and (d_neg == 0).all()
    ids4, ids5 = torch.arange(4, device="cuda"), torch.arange(5, device="cuda")
    bad = [
        dict(q=torch.randn(4, 6, device="cuda"), pos=torch.randn(4, 6, device="cuda"), neg=torch.randn(5, 6, device="cuda")),      # D % 4
        dict(q=torch.randn(4, 260, device="cuda"), pos=torch.randn(4, 260, device="cuda"), neg=torch.randn(5, 260, device="cuda")),
        dict(q=torch.randn(4, 9, device="cuda")[:, :8]),                                           # a pitch that is no multiple of 4
        dict(q=torch.randn(8, 4, device="cuda").T),
        dict(q=q.double()),
        dict(pos=pos[:3]),
        dict(pos=torch.randn(4, 12, device="cuda")),
        dict(neg=neg[:0]),                                                                         # S = 0
        dict(neg=torch.randn(5, 12, device="cuda")),
        dict(neg=neg.cpu()),
        dict(pos_ids=ids4[:3]), dict(pos_ids=ids4.int()), dict(neg_ids=ids4), dict(neg_ids=ids5.cpu()),
        dict(sample_weight=torch.ones(4, dtype=torch.float64, device="cuda")), dict(sample_weight=torch.ones(5, device="cuda")),
        dict(num_hard=9), dict(num_hard=-1), dict(metric="l2"),
    ]
    for change in bad:
        args = dict(q=q, pos=pos, neg=neg)
        args.update(change)
        with pytest.raises(ValueError):
            ops.margin_rank_fwd(**args)
    t, loss, active, hard, _ = ops.margin_rank_fwd(q, pos, neg, num_hard=2)
    for change in (dict(pos_score=t[:3]), dict(pos_score=t.double()), dict(hard_idx=None), dict(hard_idx=hard[:, :1]),
                   dict(hard_idx=hard.long()), dict(d_q=torch.empty(4, 9, device="cuda")[:, :8]), dict(d_q=torch.empty(3, 8, device="cuda"))):
        args = dict(q=q, pos=pos, neg=neg, pos_score=t, hard_idx=hard, num_hard=2)
        args.update(change)
        with pytest.raises(ValueError):
            ops.margin_rank_bwd(**args)
    # the C entry points refuse on their own, before any launch: the outputs keep their sentinel
    L, ptr = ops.lib(), ops.ptr
    ws = ops.margin_rank_workspace(4, 5, 8, 2, q.device)
    outs = [torch.full((4,), 7.0, device="cuda"), torch.full((4,), 7.0, device="cuda"), torch.full((4,), 7, dtype=torch.int32, device="cuda"),
            torch.full((4, 2), 7, dtype=torch.int32, device="cuda")]

    def fwd(q=q, ld_q=8, pos=pos, ld_p=8, neg=neg, ld_n=8, D=8, B=4, S=5, metric=1, in_batch=0, K=2, ws=ws, ws_bytes=None, t_out=outs[0],
            hard=outs[3]):
        return L.dr_margin_rank_fwd(ptr(q), ld_q, ptr(pos), ld_p, ptr(neg), ld_n, D, B, S, None, None, None, 0.2, metric, in_batch, K, 1e-12,
                                    ptr(t_out), ptr(outs[1]), ptr(outs[2]), ptr(hard), None, ptr(ws),
                                    ws.numel() if ws_bytes is None else ws_bytes, ops.stream_ptr())

    from deep_recommenders_amd import _lib
    off = torch.randn(4 * 8 + 4, device="cuda")[1:33].reshape(4, 8)                                 # 4 bytes off a 16-byte boundary
    refused = [fwd(D=6), fwd(D=260), fwd(S=0), fwd(B=-1), fwd(S=2 ** 31), fwd(K=9), fwd(K=-1), fwd(metric=2), fwd(in_batch=1),
               fwd(ld_q=6), fwd(ld_q=9), fwd(ld_p=6), fwd(ld_p=10), fwd(ld_n=4), fwd(ld_n=11), fwd(ws_bytes=16), fwd(q=off), fwd(pos=off),
               fwd(neg=off), fwd(q=None), fwd(pos=None), fwd(neg=None), fwd(t_out=None), fwd(hard=None), fwd(ws=None, ws_bytes=1 << 20)]
    assert all(st in (_lib.DR_EINVAL, _lib.DR_ESHAPE) for st in refused), refused
    assert fwd(D=6) == _lib.DR_ESHAPE and fwd(in_batch=1) == _lib.DR_ESHAPE and fwd(K=9) == _lib.DR_EINVAL
    torch.cuda.synchronize()
    assert all((o == 7).all() for o in outs)
    assert fwd(B=0) == _lib.DR_OK and all((o == 7).all() for o in outs)
    assert fwd() == _lib.DR_OK and not (outs[0] == 7).any()
    # the backward's own refusals: the gradients keep their sentinel
    grads = [torch.full((4, 8), 7.0, device="cuda"), torch.full((4, 8), 7.0, device="cuda"), torch.full((5, 8), 7.0, device="cuda")]

    def bwd(q=q, ld_q=8, pos=pos, ld_p=8, neg=neg, ld_n=8, D=8, B=4, S=5, metric=1, in_batch=0, K=2, ws=ws, ws_bytes=None, t_in=outs[0],
            hard=outs[3], d_q=grads[0], ld_dq=8, d_pos=grads[1], d_neg=grads[2]):
        return L.dr_margin_rank_bwd(ptr(q), ld_q, ptr(pos), ld_p, ptr(neg), ld_n, D, B, S, None, None, None, 0.2, metric, in_batch, K, 1e-12,
                                    0.25, ptr(t_in), ptr(hard), ptr(d_q), ld_dq, ptr(d_pos), ptr(d_neg), ptr(ws),
                                    ws.numel() if ws_bytes is None else ws_bytes, ops.stream_ptr())

    off5 = torch.randn(5 * 8 + 4, device="cuda")[1:41].reshape(5, 8)
    refused = [bwd(D=6), bwd(D=260), bwd(S=0), bwd(B=-1), bwd(S=2 ** 31), bwd(K=9), bwd(K=-1), bwd(metric=2), bwd(in_batch=1),
               bwd(ld_q=6), bwd(ld_p=9), bwd(ld_n=4), bwd(ld_dq=6), bwd(ld_dq=9), bwd(ws_bytes=16), bwd(q=off), bwd(pos=off), bwd(neg=off5),
               bwd(d_q=off), bwd(d_pos=off), bwd(d_neg=off5), bwd(q=None), bwd(t_in=None), bwd(hard=None), bwd(d_q=None), bwd(d_pos=None),
               bwd(d_neg=None), bwd(ws=None, ws_bytes=1 << 20)]
    assert all(st in (_lib.DR_EINVAL, _lib.DR_ESHAPE) for st in refused), refused
    assert bwd(D=260) == _lib.DR_ESHAPE and bwd(in_batch=1) == _lib.DR_ESHAPE and bwd(ld_dq=6) == _lib.DR_EINVAL
    torch.cuda.synchronize()
    assert all((g == 7).all() for g in grads)
    assert bwd(B=0) == _lib.DR_OK and all((g == 7).all() for g in grads)
    assert bwd() == _lib.DR_OK
    want = ops.margin_rank_bwd(q, pos, neg, outs[0], outs[3], num_hard=2, row_scale=0.25)
    assert all(_bits_equal(g, w_) for g, w_ in zip(grads, want))
    with pytest.raises(ValueError):
        ops.margin_rank_fwd(q, pos, neg, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    # the layer: views with a pitch go through with their pitch, the inputs' graphs are not touched, in-batch adds d_neg onto d_pos
    _, qv = _wide(q)
    qv.requires_grad_(True)
    rows, act, d_q, d_pos, d_neg = layers.margin_rank(qv, pos, neg, num_hard_negatives=2, row_scale=0.25)
    want = ops.margin_rank_fwd(q, pos, neg, num_hard=2)
    assert _bits_equal(rows, want[1]) and torch.equal(act, want[2]) and not rows.requires_grad and d_q.shape == (4, 8) and d_neg.shape == (5, 8)
    rows, act, d_q, d_pos, d_neg = layers.margin_rank(qv, pos, row_scale=0.25)
    t, _, _, _, _ = ops.margin_rank_fwd(q, pos)
    _, p0, n0 = ops.margin_rank_bwd(q, pos, None, t, None, row_scale=0.25)
    assert d_neg is None and _bits_equal(d_pos, p0 + n0)
    with pytest.raises(ValueError):
        layers.margin_rank(qv, pos, neg, metric="l2")


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def _columns(prefix, n_tokens, n_places, dim):
    from deep_recommenders_amd import feature_column as fc
    return [fc.embedding_column(fc.categorical_column_with_identity(prefix + "_tokens", n_tokens), dim),
            fc.embedding_column(fc.categorical_column_with_identity(prefix + "_place", n_places), dim)]


def _toy_batch(rng, B, n_tokens=96, n_topics=8, n_places=6, bag=5):
    """queries and documents belong to topics; token bags are drawn from the topic's vocabulary"""
    per = n_tokens // n_topics
    topic = rng.integers(0, n_topics, size=B)

    def side():
        bagv = topic[:, None] * per + rng.integers(0, per, size=(B, bag))
        bagv[rng.random((B, bag)) < 0.2] = -1
        bagv[:, 0] = np.where(bagv[:, 0] < 0, topic * per, bagv[:, 0])                             # no empty bag
        return bagv
    place = rng.integers(0, n_places, size=(B, 1))
    qi = {"query_tokens": torch.from_numpy(side()).cuda(), "query_place": torch.from_numpy(place).cuda()}
    di = {"doc_tokens": torch.from_numpy(side()).cuda(), "doc_place": torch.from_numpy(place.copy()).cuda()}
    return qi, di


def _make(seed=0, dim=8, units=(32, 16), **kw):
    from deep_recommenders_amd.keras.models.retrieval import EBR
    m = EBR(_columns("query", 96, 6, dim), _columns("doc", 96, 6, dim), list(units), seed=seed, **kw)
    return m.build()


def _tower64(tower, inputs):
    """the tower in float64 on the CPU from the device's parameters: (output, [leaves] in the order slab table, kernels, biases)"""
    table = tower.slab.table.detach().double().cpu().requires_grad_(True)
    parts = []
    for key in tower.slab.keys:
        ids = inputs[key].cpu()
        ok = ids >= 0
        rows = table[ids.clamp(min=0) + tower.slab.base[key]] * ok[..., None]
        parts.append(rows.sum(1) / ok.sum(1).clamp(min=1)[:, None])
    Ws = [w.detach().double().cpu().requires_grad_(True) for w in tower.dnn_kernels]
    bs = [b.detach().double().cpu().requires_grad_(True) for b in tower.dnn_biases]
    h = torch.cat(parts, dim=1)
    for W, b in zip(Ws, bs):
        h = torch.relu(h @ W + b)
    return h, [table] + Ws + bs


@pytest.mark.parametrize("K", [0, 2])
def test_three_train_steps_against_the_float64_composition(K):
    m = _make(seed=1, num_hard_negatives=K, margin=0.25)
    params = [p for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=0.5)
    rng = np.random.default_rng(5)
    B = 64
    for step in range(3):
        qi, di = _toy_batch(rng, B)
        ids = torch.arange(B) + 10
        ids[3] = -1
        ids[9] = ids[8]
        q64, ql = _tower64(m.query_tower, qi)                                                    # the state the step starts from
        d64, dl = _tower64(m.document_tower, di)
        n_valid = int((ids >= 0).sum())
        rows = R.composition(q64, d64, d64, ids, ids, None, 0.25, "cosine", True, K)
        want_loss = rows.sum() / n_valid
        want_loss.backward()
        before = float(m.loss(qi, di, document_ids=ids))
        loss = m.train_step(qi, di, optimizer=opt, document_ids=ids)
        print("step %d hard %d: loss %.6f (float64 %.6f), active fraction %.3f" % (step, K, float(loss), float(want_loss.detach()), float(m.active_fraction)))
        assert before == float(loss)                                                             # loss() is train_step's value on the same state
        torch.testing.assert_close(loss.double().cpu(), want_loss.detach(), rtol=1e-4, atol=1e-4)
        assert 0 < float(m.active_fraction) <= 1
        for tower, leaves in ((m.query_tower, ql), (m.document_tower, dl)):
            dev = [tower.slab.table] + list(tower.dnn_kernels) + list(tower.dnn_biases)
            for p, ref in zip(dev, leaves):
                # the optimizer has stepped: p = p0 - lr * grad, so the gradient is recovered from .grad, which SGD leaves in place
                assert p.grad is not None and float(ref.grad.abs().max()) > 0
                torch.testing.assert_close(p.grad.double().cpu(), ref.grad, rtol=1e-4, atol=1e-4)


def test_top_k_through_brute_force_and_faiss_agree():
    m = _make(seed=2)
    rng = np.random.default_rng(8)
    _, docs = _toy_batch(rng, 500)
    queries, _ = _toy_batch(rng, 32)
    idents = torch.arange(500, dtype=torch.int64) * 7 + 1
    m.index(docs, identifiers=idents.cuda(), k=10, kind="brute_force")
    s_a, i_a = m.top_k(queries, 10)
    m.index(docs, identifiers=idents.cuda(), k=10, kind="faiss", nlist=8, nprobe=8)
    s_b, i_b = m.top_k(queries, 10)
    assert i_a.shape == (32, 10) and torch.equal(i_a.cpu(), i_b.cpu())
    torch.testing.assert_close(s_a, s_b, rtol=1e-5, atol=1e-6)
    assert float(s_a.max()) <= 1.0 + 1e-5 and set(i_a.cpu().reshape(-1).tolist()) <= set(idents.tolist())
    with pytest.raises(ValueError):
        m.index(docs, kind="pq")
    cfg = m.get_config()
    assert cfg["metric"] == "cosine" and cfg["query_columns"] == [{"key": "query_tokens", "num_buckets": 96, "dimension": 8},
                                                                  {"key": "query_place", "num_buckets": 6, "dimension": 8}]
    assert [c["key"] for c in cfg["document_columns"]] == ["doc_tokens", "doc_place"]
