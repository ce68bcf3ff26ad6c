"""GPU tests of the sampled-softmax kernels (csrc/sampled_softmax.hip), their Python surface (ops.sampled_softmax_fwd / _bwd,
layers.sampled_softmax) and the YoutubeNet model against the float64 restatement in tests/youtubenet_ref.py.

Tolerances, U = 2^-24, first order in U.  None is read off the kernel.
  scores      integer grids with 9 D < 2^24: every partial sum is exact, bit-equal to float64 rounded to fp32, -inf where left out.
              random inputs: sb_ij = (D + 1) U sum_d |u_d v_jd| + U |s_ij|   (any summation order, fused or not; the subtraction of log Q)
  true_logit  tb_i, the same form.
  row_lse     d lse / d x_k = p_k and sum_k p_k = 1, so the inputs move it by at most xb_i = max(tb_i, max_j kept sb_ij).  Every term of the
              sum is exp(x - m) times at most NF = ceil(S / tile) + 2 rescaling factors exp(m - m') of the online softmax, each with the
              relative error EF = 4 A_exp + 17 U (exp itself; its argument, a difference of magnitude <= 16, rounded once; the multiply);
              the S + 1 terms are added in a chain of length <= S + 3; then log and one add:
                lb_i = xb_i + NF EF + (S + 3) U + 4 A_log + 2 U (|lse_i| + 8)
  row_loss    w_i (lb_i + tb_i) + 2 U |loss_i|
  p = exp(x - lse): |dp| <= p (|dx| + |dlse|) <= 2 p max|ds| is the softmax's sensitivity; with exp's own error and its argument's rounding
              pb_ij = p_ij (sb_ij + lb_i + EF),   Gb_ij = |c_i| pb_ij + 2 U |G_ij|,   gb_i = |c_i| (p_t (tb_i + lb_i + EF) + U) + 2 U |g_i|
  d_u         (S + 3) U (|g_i t_d| + sum_j |G_ij v_jd|) + gb_i |t_d| + sum_j Gb_ij |v_jd|
  d_true      gb_i |u_d| + U |g_i u_d|
  d_sampled   (B + 3) U sum_i |G_ij u_id| + sum_i Gb_ij |u_id|
  A_exp, A_log: the transcendental allowance, MEASURED HERE ON THE CPU at import as fp32 torch against float64 over 2^16 + 1 evenly spaced
              points of [-8, 8]: the largest relative error of exp(x) and the largest absolute error of log(exp(x)).  Each enters with the
              project's margin of 4: the device's expf / logf are other implementations of the same 1 - 2 ulp class.  The random cases
              assert |t|, |s| <= 8 (tables and u are N(0, 1) D^-1/4, log Q in [-2, -0.5]).
  class table after a step, against float64 index_add_ of the float64 gradient rows from the same u and table (tests/test_gpu_sgns.py's
              bound for its tables): (n_slots(row) + 2) U (|row| + lr sum_slots |term|), plus lr times the slots' own d_true / d_sampled
              bounds.  The slab's rows: the same form with the layer tolerance of tests/test_gpu_gcn.py (rtol 1e-4 / atol 1e-4) on the
              gradient rows that reach K4.  The tower's .grad: rtol 1e-4 / atol 1e-4 against the float64 composition."""
import functools
import math

import numpy as np
import pytest
import torch

import youtubenet_ref as R

pytestmark = pytest.mark.gpu

DD = torch.float64
U = 2.0 ** -24
S_MAX = 8.0
NV = 37                     # classes of the kernel cases; row NV of the table is NaN and no id names it
MARGIN = 4.0
TILE, COL_GROUP, ROW_CHUNK, SPLIT_TILES = 64, 128, 128, 128         # checked against ops in test_constants_are_those_of_ops
DS, SS, BS = (4, 20, 64, 100, 256), (1, 63, 64, 200), (1, 3, 257)
MERGE = (20, 2 * COL_GROUP + 1, 2 * ROW_CHUNK + 1)                  # three column groups, three row chunks: crosses both merges
# every D with S 65, every S with D 64, every B in both; (D, S, B)
SHAPES = [(D, 65, B) for D in DS for B in BS] + [(64, S, B) for S in SS for B in BS] + [MERGE]
OPTS = {"all": (True, True, True), "plain": (False, False, False)}      # (sample_weight, log_q, remove_accidental_hits)


def _measure():
    x = torch.linspace(-S_MAX, S_MAX, 2 ** 16 + 1, dtype=torch.float32)
    e32, e64 = torch.exp(x).double(), torch.exp(x.double())
    a_exp = float(((e32 - e64).abs() / e64).max())
    y = torch.exp(x.double()).float()                                   # fp32 points of [e^-8, e^8]
    a_log = float((torch.log(y).double() - torch.log(y.double())).abs().max())
    return a_exp, a_log


A_EXP, A_LOG = _measure()


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _within(got, want, bound, what):
    err = (got.detach().double().cpu().reshape(want.shape) - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print("%s: max |err| / bound = %.3f" % (what, ratio))
    assert (err <= bound).all(), "%s: max |err| / bound = %.3f" % (what, ratio)


def _wide(t, fill=math.nan):
    """t [B, D] fp32 as a view of a wider NaN-filled device buffer (pitch D + 8, starting at column 4)"""
    buf = torch.full((t.shape[0], t.shape[1] + 8), fill, dtype=torch.float32, device="cuda")
    view = buf[:, 4:4 + t.shape[1]]
    view.copy_(t)
    return buf, view


def _inputs(shape, rng, integer=False):
    D, S, B = shape
    if integer:
        t = lambda *s: torch.from_numpy(rng.integers(-3, 4, size=s)).to(DD)                    # noqa: E731
        amp = 1.0
    else:
        t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DD)      # noqa: E731
        amp = float(np.float32(D ** -0.25))
    u, table = (t(B, D) * amp).float().to(DD), (t(NV + 1, D) * amp).float().to(DD)
    table[NV] = math.nan
    labels = torch.from_numpy(rng.integers(0, NV, size=B))
    sampled = torch.from_numpy(rng.integers(0, NV, size=S))
    if B >= 3:
        labels[1] = -1                                                                         # a padding row holding NaN
        u[1] = math.nan
    if S >= 2:
        sampled[S // 2] = -1                                                                   # a padding id among ordinary ones
    return u, table, labels, sampled


def _bounds(h, u0, tl, ts, S, B, D, scale):
    """the header's bounds from the float64 results h"""
    keep, valid = h["keep"], h["valid"]
    kd = keep.double() * valid.double()[:, None]
    s0 = torch.where(keep, h["s"], torch.zeros_like(h["s"]))
    sb = ((D + 1) * U * (u0.abs() @ ts.abs().T) + U * s0.abs()) * kd
    tb = ((D + 1) * U * (u0.abs() * tl.abs()).sum(-1) + U * h["t"].abs()) * valid.double()
    EF = MARGIN * A_EXP + 17 * U
    NF = (S + TILE - 1) // TILE + 2
    xb = torch.maximum(tb, sb.max(dim=1).values)
    lb = (xb + NF * EF + (S + 3) * U + MARGIN * A_LOG + 2 * U * (h["lse"].abs() + S_MAX)) * valid.double()
    w = h["w"]
    loss_b = w * (lb + tb) + 2 * U * h["loss"].abs()
    c = h["c"].abs()
    p = torch.exp(s0 - h["lse"][:, None]) * kd
    Gb = c[:, None] * p * (sb + lb[:, None] + EF) + 2 * U * h["G"].abs()
    pt = torch.exp(h["t"] - h["lse"]) * valid.double()
    gb = c * (pt * (tb + lb + EF) + U) + 2 * U * h["g"].abs()
    du_b = (S + 3) * U * h["abs_u"] + gb[:, None] * tl.abs() + Gb @ ts.abs()
    dtrue_b = gb[:, None] * u0.abs() + U * (h["g"][:, None] * u0).abs()
    dsamp_b = (B + 3) * U * h["abs_sampled"] + Gb.T @ u0.abs()
    return dict(b_s=sb, b_t=tb, b_lse=lb, b_loss=loss_b, b_du=du_b, b_dtrue=dtrue_b, b_dsamp=dsamp_b)


def _reference(u, table, labels, sampled, lq_t, lq_s, w, rah, scale):
    D, S, B = u.shape[1], sampled.shape[0], labels.shape[0]
    h = R.hand_grads(u, table, labels, sampled, lq_t, lq_s, w, rah, scale)
    h["valid"] = labels >= 0
    h["w"] = torch.ones(B, dtype=DD) if w is None else w
    finite = torch.isfinite(h["s"])
    assert float(h["s"][finite].abs().max() if finite.any() else 0.0) <= S_MAX and float(h["t"].abs().max()) <= S_MAX
    u0, tl, ts = R.rows(u, table, labels, sampled)
    h.update(_bounds(h, u0, tl, ts, S, B, D, scale))
    return h


@functools.lru_cache(maxsize=None)
def _case(shape, opt):
    """random inputs (float32 values held in float64), the float64 results and their bounds; computed once, never modified"""
    D, S, B = shape
    use_w, use_lq, rah = OPTS[opt]
    rng = np.random.default_rng(7000 + SHAPES.index(shape))
    u, table, labels, sampled = _inputs(shape, rng)
    lq_t = torch.from_numpy(rng.uniform(-2.0, -0.5, size=B).astype(np.float32)).to(DD) if use_lq else None
    lq_s = torch.from_numpy(rng.uniform(-2.0, -0.5, size=S).astype(np.float32)).to(DD) if use_lq else None
    w = torch.from_numpy((rng.random(B) + 0.5).astype(np.float32)).to(DD) if use_w else None
    scale = float(np.float32(1.0 / B))
    c = dict(u=u, table=table, labels=labels, sampled=sampled, lq_t=lq_t, lq_s=lq_s, w=w, rah=rah, scale=scale)
    c["ref"] = _reference(u, table, labels, sampled, lq_t, lq_s, w, rah, scale)
    return c


def _f(t):
    return None if t is None else t.float().cuda()


def _run(c, sl=slice(None), want_scores=True):
    """forward and backward of rows `sl` of the case, u and d_u as views of wider NaN-filled buffers"""
    from deep_recommenders_amd import ops
    _, u = _wide(c["u"][sl].float())
    labels, sampled = c["labels"][sl].cuda(), c["sampled"].cuda()
    table = _f(c["table"])
    lq_t = _f(c["lq_t"][sl]) if c["lq_t"] is not None else None
    w = _f(c["w"][sl]) if c["w"] is not None else None
    t, lse, loss, scores = ops.sampled_softmax_fwd(u, table, labels, sampled, lq_t, _f(c["lq_s"]), w, c["rah"], want_scores)
    du_buf, du = _wide(torch.zeros(u.shape))
    d_u, d_true, d_samp = ops.sampled_softmax_bwd(u, table, labels, sampled, t, lse, _f(c["lq_s"]), w, c["rah"], c["scale"], d_u=du)
    assert d_u.data_ptr() == du.data_ptr()
    assert torch.isnan(du_buf[:, :4]).all() and torch.isnan(du_buf[:, 4 + u.shape[1]:]).all()       # nothing beyond D columns
    return dict(t=t, lse=lse, loss=loss, s=scores, d_u=d_u, d_true=d_true, d_samp=d_samp)


def test_constants_are_those_of_ops():
    from deep_recommenders_amd import ops
    assert (TILE, COL_GROUP, ROW_CHUNK, SPLIT_TILES) == (ops.SAMPLED_SOFTMAX_TILE, ops.SAMPLED_SOFTMAX_COL_GROUP,
                                                         ops.SAMPLED_SOFTMAX_ROW_CHUNK, ops.SAMPLED_SOFTMAX_SPLIT_TILES)
    D, S, B = MERGE
    assert ops.sampled_softmax_col_groups(B, S, D) == 3 and ops.sampled_softmax_row_chunks(B, S, D) == 3


@pytest.mark.parametrize("shape", SHAPES)
def test_scores_on_integer_grids_are_exact(shape):
    from deep_recommenders_amd import ops
    D, S, B = shape
    u, table, labels, sampled = _inputs(shape, np.random.default_rng(20 + SHAPES.index(shape)), integer=True)
    for rah in (True, False):
        want_t, want_s, keep = R.logits(u, table, labels, sampled, None, None, rah)
        _, uv = _wide(u.float())
        t, _, _, s = ops.sampled_softmax_fwd(uv, _f(table), labels.cuda(), sampled.cuda(), remove_accidental_hits=rah, want_scores=True)
        assert s.shape == (B, S) and t.shape == (B,)
        assert _bits_equal(s.cpu() + 0.0, want_s.float() + 0.0)                        # + 0.0: a zero's sign is no rounding
        assert _bits_equal(t.cpu() + 0.0, want_t.float() + 0.0)
        assert (s.cpu()[~keep] == -math.inf).all() and torch.isfinite(s.cpu()[keep]).all()


@pytest.mark.parametrize("opt", sorted(OPTS))
@pytest.mark.parametrize("shape", SHAPES)
def test_random_inputs_within_the_derived_bounds(shape, opt):
    D, S, B = shape
    c = _case(shape, opt)
    r, got = c["ref"], _run(c)
    tag = "D %d S %d B %d %s " % (D, S, B, opt)
    keep = r["keep"]
    s = got["s"].cpu()
    assert (s[~keep] == -math.inf).all()
    valid = r["valid"]                                  # a padding row's scores are those of u = 0: -log Q exactly, bound 0
    _within(torch.where(keep, s, torch.zeros_like(s)), torch.where(keep, r["s"], torch.zeros_like(r["s"])), r["b_s"], tag + "scores")
    _within(got["t"], r["t"], r["b_t"], tag + "true_logit")
    _within(got["lse"], r["lse"], r["b_lse"], tag + "row_lse")
    _within(got["loss"], r["loss"], r["b_loss"], tag + "row_loss")
    _within(got["d_u"], r["d_u"], r["b_du"], tag + "d_u")
    _within(got["d_true"], r["d_true"], r["b_dtrue"], tag + "d_true")
    _within(got["d_samp"], r["d_sampled"], r["b_dsamp"], tag + "d_sampled")
    pad = ~valid
    for k in ("t", "lse", "loss", "d_u", "d_true"):                                     # a padding row: zeros, its NaN reaches nothing
        assert (got[k].cpu()[pad] == 0).all(), k
    assert (got["d_samp"].cpu()[c["sampled"] < 0] == 0).all()
    assert all(torch.isfinite(got[k]).all() for k in ("t", "lse", "loss", "d_u", "d_true", "d_samp"))


ROW_KEYS = ("t", "lse", "loss", "d_u", "d_true")
BIG = (4, 2 * COL_GROUP + 1, TILE * SPLIT_TILES + 1)            # more row tiles than SPLIT_TILES: one block walks every segment


@pytest.mark.parametrize("shape", [(64, 65, 257), (256, 65, 257), (64, 200, 257), MERGE, BIG])
def test_bit_identical_runs_and_batch_independent_rows(shape):
    from deep_recommenders_amd import ops
    D, S, B = shape
    if shape == BIG:
        rng = np.random.default_rng(99)
        u, table, labels, sampled = _inputs(shape, rng)
        c = dict(u=u, table=table, labels=labels, sampled=sampled, lq_t=None, lq_s=None, w=None, rah=True, scale=1.0 / B)
        assert ops.sampled_softmax_col_groups(B, S, D) == 1 and ops.sampled_softmax_col_groups(1, S, D) == 3
    else:
        c = _case(shape, "all")
    a, b = _run(c, want_scores=False), _run(c, want_scores=False)
    assert a["s"] is None
    for k in a:
        if a[k] is not None:
            assert _bits_equal(a[k], b[k]), k
    for i in (0, 2, B // 2, B - 1):
        one = _run(c, sl=slice(i, i + 1), want_scores=False)
        for k in ROW_KEYS:
            assert _bits_equal(one[k].reshape(-1), a[k][i].reshape(-1)), (k, i)


def test_empty_batch_and_refusals():
    from deep_recommenders_amd import layers, ops
    table = torch.randn(NV, 8, device="cuda")
    sampled = torch.arange(5, device="cuda")
    labels = torch.zeros(4, dtype=torch.int64, device="cuda")
    u = torch.randn(4, 8, device="cuda")
    t, lse, loss, s = ops.sampled_softmax_fwd(u[:0], table, labels[:0], sampled, want_scores=True)
    assert t.shape == lse.shape == loss.shape == (0,) and s.shape == (0, 5)
    d_u, d_true, d_samp = ops.sampled_softmax_bwd(u[:0], table, labels[:0], sampled, t, lse)
    assert d_u.shape == d_true.shape == (0, 8) and d_samp.shape == (5, 8) and (d_samp == 0).all()
    bad = [
        dict(table=torch.randn(NV, 6, device="cuda"), u=torch.randn(4, 6, device="cuda")),           # D % 4
        dict(table=torch.randn(NV, 260, device="cuda"), u=torch.randn(4, 260, device="cuda")),       # D > 256
        dict(table=torch.randn(NV, 16, device="cuda")[:, :8]),                                       # a view of the table
        dict(table=torch.randn(8, NV, device="cuda").T),
        dict(table=table.double()),
        dict(u=torch.randn(4, 9, device="cuda")[:, :8]),                                             # a pitch that is no multiple of 4
        dict(u=torch.randn(8, 4, device="cuda").T),
        dict(u=torch.randn(4, 12, device="cuda")),
        dict(sampled=sampled[:0]),                                                                   # S = 0
        dict(sampled=sampled.int()),
        dict(sampled=sampled.reshape(1, 5)),
        dict(labels=labels[:3]),
        dict(labels=labels.int()),
        dict(log_q_true=torch.zeros(3, device="cuda")),
        dict(log_q_sampled=torch.zeros(4, device="cuda")),
        dict(sample_weight=torch.zeros(4, dtype=torch.float64, device="cuda")),
        dict(sampled=sampled.cpu()),
    ]
    for change in bad:
        args = dict(u=u, table=table, labels=labels, sampled=sampled)
        args.update(change)
        with pytest.raises(ValueError):
            ops.sampled_softmax_fwd(**args)
    t, lse, _, _ = ops.sampled_softmax_fwd(u, table, labels, sampled)
    for change in (dict(true_logit=t[:3]), dict(row_lse=lse.double()), dict(d_u=torch.empty(4, 9, device="cuda")[:, :8]),
                   dict(d_u=torch.empty(3, 8, device="cuda"))):
        args = dict(u=u, table=table, labels=labels, sampled=sampled, true_logit=t, row_lse=lse)
        args.update(change)
        with pytest.raises(ValueError):
            ops.sampled_softmax_bwd(**args)
    # the C entry points refuse on their own: a workspace that is too small, a misaligned base
    with pytest.raises(ValueError):
        ops.sampled_softmax_fwd(u, table, labels, sampled, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.sampled_softmax_fwd(torch.randn(4, 12, device="cuda")[:, 1:9], table, labels, sampled)
    # the layer: a view of u with a pitch goes through with its pitch, and u's graph is not touched
    _, uv = _wide(u)
    uv.requires_grad_(True)
    rows, d_u, d_true, d_samp = layers.sampled_softmax(uv, table, labels, sampled, row_scale=0.25)
    want = ops.sampled_softmax_fwd(u, table, labels, sampled)
    assert _bits_equal(rows, want[2]) and not rows.requires_grad and d_u.shape == (4, 8)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def _columns(n_videos, n_tokens, dim):
    from deep_recommenders_amd import feature_column as fc
    return [fc.embedding_column(fc.categorical_column_with_identity("history", n_videos), dim),
            fc.embedding_column(fc.categorical_column_with_identity("search", n_tokens), dim)]


def _toy_batch(rng, B, n_classes, n_blocks, hist_len=5):
    """users belong to taste blocks; histories and the label (the next watch) are drawn from the user's block"""
    per = n_classes // n_blocks
    block = rng.integers(0, n_blocks, size=B)
    hist = block[:, None] * per + rng.integers(0, per, size=(B, hist_len))
    hist[rng.random((B, hist_len)) < 0.2] = -1
    hist[:, 0] = np.where(hist[:, 0] < 0, block * per, hist[:, 0])                      # no empty bag
    search = block[:, None] + np.zeros((B, 1), dtype=np.int64)
    labels = block * per + rng.integers(0, per, size=B)
    age = rng.random((B, 1)).astype(np.float32)
    inputs = {"history": torch.from_numpy(hist).cuda(), "search": torch.from_numpy(search).cuda(), "age": torch.from_numpy(age).cuda()}
    return inputs, torch.from_numpy(labels).cuda()


def _make(seed=0, n_classes=64, n_blocks=8, dim=8, units=(32, 16), S=16, **kw):
    from deep_recommenders_amd.keras.models.retrieval import YoutubeNet
    torch.manual_seed(seed)
    m = YoutubeNet(_columns(n_classes, n_blocks, dim), n_classes, list(units), S, class_counts=np.ones(n_classes),
                   dense_features_key="age", seed=seed, **kw)
    return m.build(1)


def _tower64(model, inputs, slab):
    """the user tower in float64 on the CPU over the slab rows `slab` (float64): (u, x, slab leaf, [kernels], [biases], the bags)"""
    table = slab.clone().requires_grad_(True)
    parts, slots = [], []
    for key in model.slab.keys:
        ids = inputs[key].cpu()
        valid = ids >= 0
        rows = table[ids.clamp(min=0) + model.slab.base[key]] * valid[..., None]
        cnt = valid.sum(1).clamp(min=1)
        parts.append(rows.sum(1) / cnt[:, None])
        slots.append((ids, valid, cnt, model.slab.base[key]))
    x = torch.cat(parts + [inputs["age"].double().cpu()], dim=1)
    x.retain_grad()
    Ws = [w.detach().double().cpu().requires_grad_(True) for w in model.dnn_kernels]
    bs = [b.detach().double().cpu().requires_grad_(True) for b in model.dnn_biases]
    h = x
    for W, b in zip(Ws, bs):
        h = torch.relu(h @ W + b)
    return h, x, table, Ws, bs, slots


def _full_softmax_loss(model, inputs, labels):
    with torch.no_grad():
        u = model.call(inputs).double().cpu()
    return float(torch.nn.functional.cross_entropy(u @ model.class_table.detach().double().cpu().T, labels.cpu()))


def test_train_step_against_the_float64_step():
    m = _make(seed=1, n_classes=NV, n_blocks=1, dim=8, units=(24, 16), S=20)
    rng = np.random.default_rng(5)
    B, lr = 33, 4.0
    inputs, labels = _toy_batch(rng, B, NV, 1)
    labels[3] = -1
    m.slab.sparse_lr = lr
    sampled = torch.from_numpy(rng.integers(0, NV, size=20)).cuda()
    sampled[7] = -1
    table0 = m.class_table.detach().double().cpu()
    slab0 = m.slab.table.detach().double().cpu()
    with torch.no_grad():
        u_gpu = m.call(inputs).double().cpu()                                       # the state the kernels start from
    loss = m.train_step(inputs, labels, lr, sampled=sampled)
    lab, smp = labels.cpu(), sampled.cpu()
    n_valid = int((lab >= 0).sum())
    scale = 1.0 / n_valid
    lq = m.log_q.double().cpu()
    lq_t, lq_s = lq[lab.clamp(min=0)], lq[smp.clamp(min=0)]
    # the class table, from the same u and table
    r = _reference(u_gpu, table0, lab, smp, lq_t, lq_s, None, True, float(np.float32(scale)))
    _within(loss, r["loss"].sum() * scale, (r["b_loss"].sum() + (B + 3) * U * r["loss"].sum()) * scale, "mean loss")
    want = R.sgd_step(table0, lab, smp, r["d_true"], r["d_sampled"], lr)
    vl, vs = lab >= 0, smp >= 0
    n_slots = torch.zeros(NV, dtype=DD).index_add_(0, lab[vl], torch.ones(int(vl.sum()), dtype=DD))
    n_slots.index_add_(0, smp[vs], torch.ones(int(vs.sum()), dtype=DD))
    terms = torch.zeros_like(table0).index_add_(0, lab[vl], r["d_true"][vl].abs()).index_add_(0, smp[vs], r["d_sampled"][vs].abs())
    own = torch.zeros_like(table0).index_add_(0, lab[vl], r["b_dtrue"][vl]).index_add_(0, smp[vs], r["b_dsamp"][vs])
    bound = (n_slots[:, None] + 2) * U * (table0.abs() + lr * terms) + lr * own
    _within(m.class_table.detach(), want, bound, "class table after the step")
    assert (n_slots > 0).any() and not torch.equal(m.class_table.detach().double().cpu(), table0)
    # the tower and the slab, against the float64 composition of the whole step
    u64, x, slab_leaf, Ws, bs, slots = _tower64(m, inputs, slab0)                # the slab as the step found it
    h = R.hand_grads(u64.detach(), table0, lab, smp, lq_t, lq_s, None, True, scale)
    u64.backward(h["d_u"])
    for got, ref, what in [(p.grad, w.grad, "kernel %d" % i) for i, (p, w) in enumerate(zip(m.dnn_kernels, Ws))] + \
                          [(p.grad, w.grad, "bias %d" % i) for i, (p, w) in enumerate(zip(m.dnn_biases, bs))]:
        print("%s .grad: max |err| = %.3e" % (what, float((got.double().cpu() - ref).abs().max())))
        torch.testing.assert_close(got.double().cpu(), ref, rtol=1e-4, atol=1e-4)
    want_slab = slab0 - lr * slab_leaf.grad
    n_s, t_s = torch.zeros(slab0.shape[0], dtype=DD), torch.zeros_like(slab0)
    FD = 0
    for ids, valid, cnt, base in slots:
        D = slab0.shape[1]
        term = (x.grad[:, FD:FD + D] / cnt[:, None]).abs()
        FD += D
        for col in range(ids.shape[1]):
            ok = valid[:, col]
            n_s.index_add_(0, ids[ok, col] + base, torch.ones(int(ok.sum()), dtype=DD))
            t_s.index_add_(0, ids[ok, col] + base, term[ok])
    bound = (n_s[:, None] + 2) * U * (slab0.abs() + lr * t_s) + lr * (1e-4 * t_s + 1e-4 * n_s[:, None])
    _within(m.slab.table.detach(), want_slab, bound, "slab after the step")
    assert not torch.equal(m.slab.table.detach().double().cpu(), slab0)


def test_deterministic_runs_are_bit_identical():
    """the class table through the sorted K4, the tower through torch SGD; the slab is frozen here: its own K4 is the atomic form (bags
    are multi-valued), whose sums over shared rows have no fixed order"""
    curves, tables = [], []
    for _ in range(2):
        m = _make(seed=3, deterministic=True)
        m.slab.table.requires_grad_(False)
        opt = torch.optim.SGD(list(m.dnn_kernels) + list(m.dnn_biases), lr=0.5)
        rng = np.random.default_rng(11)
        losses = []
        for _step in range(20):
            inputs, labels = _toy_batch(rng, 64, 64, 8)
            losses.append(m.train_step(inputs, labels, 8.0, optimizer=opt))
        curves.append(torch.stack(losses))
        tables.append([m.class_table.detach().clone()] + [p.detach().clone() for p in m.dnn_kernels])
    assert _bits_equal(curves[0], curves[1])
    for a, b in zip(*tables):
        assert _bits_equal(a, b)
    assert m.draw_offset == 20 * m.num_sampled and torch.isfinite(curves[0]).all()


def test_training_lowers_the_held_out_full_softmax_loss():
    m = _make(seed=4)
    m.slab.sparse_lr = 8.0
    opt = torch.optim.SGD(list(m.dnn_kernels) + list(m.dnn_biases), lr=0.5)
    held_in, held_lab = _toy_batch(np.random.default_rng(100), 256, 64, 8)
    before = _full_softmax_loss(m, held_in, held_lab)
    rng = np.random.default_rng(12)
    for _ in range(200):
        inputs, labels = _toy_batch(rng, 64, 64, 8)
        m.train_step(inputs, labels, 8.0, optimizer=opt)
    after = _full_softmax_loss(m, held_in, held_lab)
    print("held-out full-softmax loss: %.4f -> %.4f (log 64 = %.4f, log 8 = %.4f)" % (before, after, math.log(64), math.log(8)))
    assert after < before and after < math.log(64)
    assert float(m.loss(held_in, held_lab)) > 0


def test_top_k_returns_the_label_first_for_a_memorised_batch():
    m = _make(seed=5, S=32)
    m.slab.sparse_lr = 8.0
    opt = torch.optim.SGD(list(m.dnn_kernels) + list(m.dnn_biases), lr=0.5)
    B = 16
    hist = torch.arange(B)[:, None] * 4 + torch.arange(3)[None, :]                         # every user a history of its own
    inputs = {"history": hist.cuda(), "search": (torch.arange(B) % 8)[:, None].cuda(), "age": torch.linspace(0, 1, B)[:, None].cuda()}
    labels = (torch.arange(B) * 3 + 1).cuda()
    for _ in range(400):
        m.train_step(inputs, labels, 8.0, optimizer=opt)
    scores, ids = m.top_k(inputs, k=3)
    assert ids.shape == (B, 3) and torch.equal(ids[:, 0].cpu(), labels.cpu())
    assert m.get_config()["num_sampled"] == 32
