"""GPU tests of skip-gram with side information (csrc/eges.hip), the weighted random walk (csrc/sampling.hip), the autograd glue
(layers.eges_loss) and the models (EGES, Airbnb) against the float64 restatement in tests/eges_ref.py.

Tolerances, u32 = 2^-24.  None is read off the kernel.  The slot bounds are tests/test_gpu_sgns.py's with u's own error carried along.
  alpha     e_s = expf(a_s - m): the subtraction's rounding through exp' = exp, plus the expf allowance:  de_s = u32 |a_s - m| e_s + 4 A_EXP.
            Z >= 1 (the largest term is expf(0) = 1) takes S - 1 adds, the quotient one rounding:
              da_s = de_s / Z + alpha_s (sum_t de_t / Z + S u32).
            A row's sum: the e_s the kernel divides are the e_s it added, so sum_s alpha_s = 1 within (S + 2) u32 whatever expf does.
  u         ub_d = (S + 2) u32 sum_s |alpha_s w_sd| + sum_s da_s |w_sd|
  scores    sb_j = (D + 1) u32 sum_d |u_d v_jd| + sum_d ub_d |v_jd|
  loss      w_b sum_j (sb_j + 4 A_sp) + (P + K + 3) u32 w_b sum_j softplus_j
  coeff     cb_j = w_b (sb_j / 4 + 4 A_sg) + 2 u32 |g_j|
  d_u       dub_d = (P + K + 4) u32 sum_j |c_j v_jd| + |scale| sum_j cb_j |v_jd|                      (test_gpu_sgns.py's d_center)
  d_ctx     3 u32 |c_j u_d| + |scale| cb_j |u_d| + |c_j| ub_d
  d_side    2 u32 |alpha_s d_u_d| + da_s |d_u_d| + alpha_s dub_d
  q_s       qb_s = (D + 1) u32 sum_d |d_u_d w_sd| + sum_d dub_d |w_sd|
  r         rb = (S + 2) u32 sum_s |alpha_s q_s| + sum_s (da_s |q_s| + alpha_s qb_s)
  d_att     3 u32 alpha_s (|q_s| + |r|) + da_s |q_s - r| + alpha_s (qb_s + rb)
  A_sp, A_sg as in test_gpu_sgns.py over [-8, 8]; A_EXP likewise, MEASURED HERE ON THE CPU at import: the largest |fp32 torch - float64|
            of exp over 2^16 + 1 evenly spaced fp32 points of [-R, 0], R = 10 covering every a_s - m of the cases (logits ~ N(0, 1); the
            cases assert it).  Each enters with the margin of 4 of that file, for the reason given there.
  tables    after a step, against float64 index_add_ of the float64 gradient rows: (n_slots(row) + 2) u32 (|row| + lr sum_slots |term|)
            plus lr times the slots' own bounds.    .grad: the same without |row| and lr.
Every GPU result is compared with float64 results of THE SAME fp32 inputs; the model test re-reads the tables before every step, so
that eight steps are eight such comparisons and no drift has to be bounded."""
import functools

import numpy as np
import pytest
import torch

import eges_ref as E
import sgns_ref as R

pytestmark = pytest.mark.gpu

DD = torch.float64
U = 2.0 ** -24
S_MAX, R_LOGIT, MARGIN = 8.0, 10.0, 4.0
NV, NSIDE = 37, 7            # rows of field 0 / out_table / att, rows of every side field
NID, NSID = 30, 5            # ids the cases draw from: rows 30 .. 36 resp. 5, 6 of a field are named only where a test says so
# (D, S, P, K, B): every D, every S and every P with B = 257; K in {0, 5}; P + K = 64; B in {1, 3, 257}
SHAPES = [(4, 1, 1, 5, 257), (20, 3, 2, 5, 257), (64, 8, 2, 5, 257), (256, 16, 4, 0, 257), (64, 3, 2, 62, 3), (20, 16, 4, 5, 1),
          (64, 1, 1, 0, 3), (256, 3, 1, 5, 3), (4, 8, 4, 0, 1)]
BIG = [s for s in SHAPES if s[4] == 257]
# EGES toy (64 items in two blocks, the block as side feature, D 16, K 5, B 256; the two side rows are shared by 128 examples each):
# the learning rate was chosen on the float64 restatement, free-running on the CPU for eight steps from tables drawn by the CPU generator
# with the model's distribution.  These curves served that choice only: the test compares every step of the model with the restatement
# of the model's own tables (drawn on the device, another stream: the trailer of this file has that curve), not with these figures.
#   lr 4: 4.133 4.036 3.930 3.827 3.647 3.368 3.160 2.921     lr 16: 4.133 3.824 3.018 2.829 3.019 2.525 2.654 2.495 (oscillates)
#   lr 64: diverges from the third step on
EGES_LR = 4.0


def _measure(fn, lo, hi):
    x = torch.linspace(lo, hi, 2 ** 16 + 1, dtype=torch.float32)
    return float((fn(x).double() - fn(x.double())).abs().max())


A_SP = _measure(torch.nn.functional.softplus, -S_MAX, S_MAX)
A_SG = _measure(torch.sigmoid, -S_MAX, S_MAX)
A_EXP = _measure(torch.exp, -R_LOGIT, 0.0)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cuda(a):
    if a is None:
        return None
    return a.to(torch.float32).cuda() if a.is_floating_point() else a.cuda()


def _within(got, want, bound, what):
    err = (got.detach().double().cpu().reshape(want.shape) - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print("%s: max |err| / bound = %.3f" % (what, ratio))
    assert (err <= bound).all(), "%s: max |err| / bound = %.3f" % (what, ratio)


def _f32(t):
    """float32 values held in float64"""
    return t.float().to(DD)


def _row_base(S):
    return torch.tensor(np.concatenate([[0], np.cumsum(([NV] + [NSIDE] * (S - 1))[:-1])]).astype(np.int64))


def _pad4(n):
    return (n + 3) // 4 * 4


def _inputs(rng, D, S, P, K, B):
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DD)          # noqa: E731
    amp = float(np.float32(D ** -0.25))
    side_table = _f32(t(NV + NSIDE * (S - 1), D) * amp)
    out_table = _f32(t(NV, D) * amp)
    att_full = t(NV, _pad4(S) + 4)                                                              # the kernel reads it at this pitch
    side_ids = torch.from_numpy(np.stack([rng.integers(0, NID if s == 0 else NSID, size=B) for s in range(S)], axis=1))
    att_ids = side_ids[:, 0].clone()
    contexts = torch.from_numpy(rng.integers(0, NID, size=(B, P)))
    negatives = torch.from_numpy(rng.integers(0, NID, size=(B, K)))
    w = torch.from_numpy((rng.random(B) + 0.5).astype(np.float32)).to(DD)
    return dict(side_table=side_table, row_base=_row_base(S), side_ids=side_ids, att_full=att_full, att=att_full[:, :S], att_ids=att_ids,
                out_table=out_table, contexts=contexts, negatives=negatives, w=w, scale=float(np.float32(1.0 / B)))


@functools.lru_cache(maxsize=None)
def _case(shape):
    """random tables, logits, ids, weights and the float64 results with their bounds; computed once, never modified"""
    D, S, P, K, B = shape
    rng = np.random.default_rng(4000 + SHAPES.index(shape))
    c = _inputs(rng, D, S, P, K, B)
    if B >= 3:
        if K >= 1:
            c["negatives"][1, K - 1] = -1                                                       # masks among ordinary examples
        if S >= 2:
            c["side_ids"][2, S - 1] = -1
        c["att_ids"][0] = -1
    c.update(_reference(c, True))
    return c


def _ref_args(c, att=True):
    return (c["side_table"], c["row_base"], c["side_ids"], c["att"] if att else None, c["att_ids"] if att else None, c["out_table"],
            c["contexts"], c["negatives"])


def _reference(c, skip_equal, att=True, d_loss=None, weights=True):
    """the float64 results of the case's inputs and the bounds of the header; d_loss [B] stands for the scalar scale when given"""
    B, S = c["side_ids"].shape
    D, J, P = c["side_table"].shape[1], c["contexts"].shape[1] + c["negatives"].shape[1], c["contexts"].shape[1]
    wgt = c["w"] if weights else torch.ones(B, dtype=DD)
    dl = torch.full((B,), c["scale"], dtype=DD) if d_loss is None else d_loss.double()
    h = E.hand_grads(*_ref_args(c, att), dl, wgt, skip_equal)
    loss = E.loss_expr(*_ref_args(c, att), wgt, skip_equal)[0]
    present, keep, alpha, w, u, v, g, cc = (h[k] for k in ("present", "keep", "alpha", "w", "u", "v", "g", "c"))
    pd, kd = present.double(), keep.double()
    assert float(h["s"].abs().max()) <= S_MAX
    if att:
        a = c["att"].double()[c["att_ids"].clamp_min(0)] * h["use_att"].double()[:, None]
    else:
        a = torch.zeros((B, S), dtype=DD)
    m = a.masked_fill(~present, -float("inf")).max(1).values
    diff = torch.where(present, a - m[:, None], torch.zeros_like(a))
    assert float(diff.min()) >= -R_LOGIT
    e = torch.exp(diff) * pd
    Z = e.sum(1).clamp_min(1.0)
    de = (U * diff.abs() * e + MARGIN * A_EXP) * pd
    da = de / Z[:, None] + alpha * (de.sum(1) / Z + S * U)[:, None]
    ub = (S + 2) * U * (alpha[:, :, None] * w).abs().sum(1) + (da[:, :, None] * w.abs()).sum(1)
    sb = ((D + 1) * U * (u[:, None, :] * v).abs().sum(-1) + (ub[:, None, :] * v.abs()).sum(-1)) * kd
    sign = torch.ones(J, dtype=DD)
    sign[:P] = -1.0
    sp = torch.nn.functional.softplus(sign[None, :] * h["s"]) * kd
    b_loss = wgt * ((sb + MARGIN * A_SP) * kd).sum(1) + (J + 3) * U * wgt * sp.sum(1)
    cb = (wgt[:, None] * (sb / 4 + MARGIN * A_SG) + 2 * U * g.abs()) * kd
    dla = dl.abs()
    dub = (J + 4) * U * h["abs_du"] + dla[:, None] * (cb[:, :, None] * v.abs()).sum(1)
    b_ctx = 3 * U * h["d_ctx"].abs() + dla[:, None, None] * cb[:, :, None] * u.abs()[:, None, :] + cc.abs()[:, :, None] * ub[:, None, :]
    du = h["d_u"]
    b_side = 2 * U * h["d_side"].abs() + da[:, :, None] * du.abs()[:, None, :] + alpha[:, :, None] * dub[:, None, :]
    qb = ((D + 1) * U * (du[:, None, :] * w).abs().sum(-1) + (dub[:, None, :] * w.abs()).sum(-1)) * pd
    q, r = h["q"], h["r"]
    rb = (S + 2) * U * (alpha * q).abs().sum(1) + (da * q.abs() + alpha * qb).sum(1)
    b_att = (3 * U * alpha * (q.abs() + r.abs()[:, None]) + da * (q - r[:, None]).abs() + alpha * (qb + rb[:, None])) * h["use_att"].double()[:, None]
    return dict(h=h, keep=keep, present=present, loss=loss, scores=h["s"], coeff=g, alpha=alpha, u=u, d_side=h["d_side"], d_att=h["d_att"],
                d_ctx=h["d_ctx"], b_alpha=da * pd, b_u=ub, b_scores=sb, b_loss=b_loss, b_coeff=cb, b_side=b_side, b_att=b_att, b_ctx=b_ctx)


def _run(c, grads=True, want_scores=True, skip_equal=True, weights=True, att=True, sl=slice(None)):
    from deep_recommenders_amd import ops
    return ops.eges_fwd(_cuda(c["side_table"]), c["row_base"].cuda(), c["side_ids"][sl].cuda(), _cuda(c["att_full"])[:, :c["att"].shape[1]] if att else None,
                        c["att_ids"][sl].cuda() if att else None, _cuda(c["out_table"]), c["contexts"][sl].cuda(), c["negatives"][sl].cuda(),
                        _cuda(c["w"][sl]) if weights else None, skip_equal, want_scores, c["scale"] if grads else None)


NAMES = ("loss", "coeff", "alpha", "scores", "d_side", "d_att", "d_ctx")


def _check_all(got, c, tag):
    B, S = c["side_ids"].shape
    D, J = c["side_table"].shape[1], c["contexts"].shape[1] + c["negatives"].shape[1]
    loss, coeff, alpha, scores, d_side, d_att, d_ctx = got
    assert alpha.shape == (B, S) and coeff.shape == (B, J) and d_side.shape == (B, S * D) and d_att.shape == (B, _pad4(S))
    _within(alpha, c["alpha"], c["b_alpha"], tag + "alpha")
    _within(scores, c["scores"], c["b_scores"], tag + "scores")
    _within(loss, c["loss"], c["b_loss"], tag + "loss_rows")
    _within(coeff, c["coeff"], c["b_coeff"], tag + "coeff")
    _within(d_side, c["d_side"], c["b_side"], tag + "d_side")
    _within(d_att[:, :S], c["d_att"], c["b_att"], tag + "d_att")
    _within(d_ctx, c["d_ctx"], c["b_ctx"], tag + "d_ctx")
    for t in got:
        assert torch.isfinite(t).all()
    # +0.0, bit for bit: skipped slots, missing fields, the padding of d_att, examples whose logits were taken as 0
    skipped, missing = ~c["keep"], ~c["present"]
    z = lambda t: (t.cpu().view(torch.int32) == 0).all()                                        # noqa: E731
    assert z(coeff.cpu()[skipped]) and z(scores.cpu()[skipped]) and z(d_ctx.cpu().reshape(B, J, D)[skipped])
    assert z(alpha.cpu()[missing]) and z(d_side.cpu().reshape(B, S, D)[missing]) and z(d_att.cpu()[:, :S][missing]) and z(d_att.cpu()[:, S:])
    assert z(d_att.cpu()[~c["h"]["use_att"]])
    live = c["present"].any(1)
    assert ((alpha.cpu().double().sum(1) - 1).abs()[live] <= (S + 2) * U).all() and z(loss.cpu()[~live])


# ---- 1. the anchor: one field, one positive, no attention is dr_sgns_fwd / dr_sgns_bwd ----------------------------------------------------
@pytest.mark.parametrize("skip_equal", [True, False])
@pytest.mark.parametrize("K", [0, 5])
@pytest.mark.parametrize("D", [4, 12, 64, 256])
def test_single_field_single_positive_equals_sgns_bit_for_bit(D, K, skip_equal):
    from deep_recommenders_amd import ops
    B = 257
    rng = np.random.default_rng(D + K)
    t = lambda *s: torch.from_numpy((rng.standard_normal(s) * D ** -0.25).astype(np.float32)).cuda()     # noqa: E731
    tin, tout = t(NV, D), t(NV, D)
    centers = torch.from_numpy(rng.integers(0, NV, size=B))
    contexts = torch.from_numpy(rng.integers(0, NV, size=B))
    negatives = torch.from_numpy(rng.integers(0, NV, size=(B, K)))
    centers[[3, 256]] = -1
    contexts[[5, 64]] = -1
    if K:
        negatives[7, 1] = -1
        negatives[9, 0] = contexts[9]
        negatives[255, K - 1] = contexts[255]
    centers, contexts, negatives = centers.cuda(), contexts.cuda(), negatives.cuda()
    w = torch.from_numpy((rng.random(B) + 0.5).astype(np.float32)).cuda()
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    for weight in (None, w):
        a_loss, a_coeff, a_scores, a_center, a_ctx = ops.sgns_fwd(tin, tout, centers, contexts, negatives, weight, skip_equal, True, 0.25)
        loss, coeff, alpha, scores, d_side, d_att, d_ctx = ops.eges_fwd(tin, zero, centers[:, None], None, None, tout, contexts[:, None],
                                                                        negatives, weight, skip_equal, True, 0.25)
        assert _bits_equal(loss, a_loss) and _bits_equal(coeff, a_coeff) and _bits_equal(scores, a_scores)
        assert _bits_equal(d_side, a_center) and _bits_equal(d_ctx, a_ctx)
        live = ((centers >= 0) & (contexts >= 0)).float()[:, None]
        assert torch.equal(alpha, live) and (d_att.view(torch.int32) == 0).all()
    d_loss = torch.from_numpy(rng.standard_normal(B).astype(np.float32)).cuda()
    b_center, b_ctx = ops.sgns_bwd(tin, tout, centers, contexts, negatives, a_coeff, d_loss, skip_equal)
    e_side, e_att, e_ctx = ops.eges_bwd(tin, zero, centers[:, None], None, None, tout, contexts[:, None], negatives, coeff, alpha, d_loss, skip_equal)
    assert _bits_equal(e_side, b_center) and _bits_equal(e_ctx, b_ctx) and (e_att.view(torch.int32) == 0).all()


# ---- 2. random tables and logits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_random_tables_within_the_derived_bounds(shape):
    c = _case(shape)
    _check_all(_run(c), c, "D %d S %d P %d K %d B %d " % shape)


@pytest.mark.parametrize("shape", [(20, 3, 2, 5, 257), (64, 8, 2, 5, 257)])
def test_without_attention_and_without_weights(shape):
    c = _case(shape)
    ref = dict(c, **_reference(c, False, att=False, weights=False))
    got = _run(c, skip_equal=False, weights=False, att=False)
    _check_all(got, ref, "no att, D %d S %d " % shape[:2])
    n = c["present"].sum(1, keepdim=True).clamp_min(1).float()
    assert torch.equal(got[2].cpu(), c["present"].float() / n)                                  # uniform over the present fields, rounded once


# ---- 3. masks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip_equal", [True, False])
@pytest.mark.parametrize("shape", [(20, 3, 2, 5, 257), (64, 8, 2, 5, 257)])
def test_masks(shape, skip_equal):
    """every mask of the interface on examples of their own; masked entries are -1 or other negative values, every id >= 0 names a
    row of its table; rows no present id names are NaN, so a read of one would show"""
    D, S, P, K, B = shape
    c = _case(shape)
    base = _run(c, skip_equal=skip_equal)
    m = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in c.items() if k in
         ("side_table", "row_base", "side_ids", "att_full", "att_ids", "out_table", "contexts", "negatives", "w", "scale")}
    sid, aid, ctx, neg = m["side_ids"], m["att_ids"], m["contexts"], m["negatives"]
    changed = [10, 11, 12, 63, 64, 100, 128, 200, 255, 256]
    sid[10, 0] = -1                                             # a missing field: first
    sid[11, S // 2] = -2 ** 62                                  #                  a middle one, far negative
    sid[12, S - 1] = -1                                         #                  last
    sid[63, :] = -1                                             # all fields missing: the example is skipped; its other ids name rows
    ctx[63, :], neg[63, :], aid[63] = 31, 31, 31                #   nobody else names
    aid[64] = -1                                                # uniform over the present fields; d_att row is zero
    ctx[100, 1] = -1                                            # a positive of -1 at j >= 1
    ctx[128, 0] = -1                                            # contexts[b, 0] = -1: skipped; its fields, its logits and its other slots
    sid[128, :], aid[128] = torch.tensor([32] + [NSID] * (S - 1)), 32       #   name rows nobody else names
    ctx[128, 1], neg[128, :] = 33, 33
    neg[200, 2] = ctx[200, 1]                                   # a negative equal to the second positive
    sid[255, 0], aid[255] = -1, -1                              # a cold item
    neg[256, 0], neg[256, K - 1] = -1, -7
    m["att"] = m["att_full"][:, :S]
    m.update(_reference(m, skip_equal))
    # NaN in every row no present id names
    side_named = torch.zeros(m["side_table"].shape[0], dtype=torch.bool)
    side_named[(sid + m["row_base"][None, :])[m["present"]]] = True
    out_named = torch.zeros(NV, dtype=torch.bool)
    out_named[m["h"]["ids"][m["keep"]]] = True
    att_named = torch.zeros(NV, dtype=torch.bool)
    att_named[aid[m["h"]["use_att"]]] = True
    assert not side_named[32] and not side_named[NV + NSID] and not out_named[31] and not out_named[33] and not att_named[31] and not att_named[32]
    poisoned = dict(m)
    for key, named in (("side_table", side_named), ("out_table", out_named), ("att_full", att_named)):
        poisoned[key] = m[key].clone()
        poisoned[key][~named] = float("nan")
    got = _run(poisoned, skip_equal=skip_equal)
    _check_all(got, m, "masks, D %d skip_equal %s: " % (D, skip_equal))                          # finite everywhere, and right
    loss, coeff, alpha, scores, d_side, d_att, d_ctx = [t.cpu() for t in got]
    for b in (63, 128):                                         # whole examples
        for t in (loss[b], coeff[b], alpha[b], scores[b], d_side[b], d_att[b], d_ctx[b]):
            assert (t.view(torch.int32) == 0).all()
    assert (d_att[64].view(torch.int32) == 0).all() and (d_att[255].view(torch.int32) == 0).all()
    n64 = float(m["present"][64].sum())
    assert torch.equal(alpha[64], m["present"][64].float() / torch.tensor(n64, dtype=torch.float32))
    assert alpha[255, 0] == 0 and torch.equal(alpha[255, 1:], torch.full((S - 1,), 1.0) / torch.tensor(float(S - 1)))
    assert coeff[100, 1] == 0 and coeff[100, 0] != 0 and coeff[256, P] == 0 and coeff[256, P + K - 1] == 0
    assert (coeff[200, P + 2] == 0) == skip_equal
    if not skip_equal:
        assert scores[200, P + 2] == scores[200, 1]
    untouched = [b for b in range(B) if b not in changed]
    for a, f in zip(got, base):                                 # examples that were not changed keep their bits
        assert _bits_equal(a[untouched], f[untouched])


# ---- 4. one pass against backward, run to run, alone against in the batch, buffers at a pitch ------------------------------------------------
@pytest.mark.parametrize("shape", BIG)
def test_reproducible_and_independent_of_the_batch(shape):
    from deep_recommenders_amd import ops
    D, S, P, K, B = shape
    c = _case(shape)
    first, again = _run(c), _run(c)
    for a, b in zip(first, again):
        assert _bits_equal(a, b)
    plain = _run(c, grads=False, want_scores=False)                                             # the gradient outputs change nothing else
    assert all(_bits_equal(plain[i], first[i]) for i in (0, 1, 2)) and all(plain[i] is None for i in (3, 4, 5, 6))
    for b in (0, 1, 2, 100, 255, 256):                                                          # an example alone: another block shape
        alone = _run(c, sl=slice(b, b + 1))
        for a, f in zip(alone, first):
            assert _bits_equal(a, f[b:b + 1]), (shape, b)
    d_loss = torch.full((B,), c["scale"], dtype=torch.float32, device="cuda")
    args = (_cuda(c["side_table"]), c["row_base"].cuda(), c["side_ids"].cuda(), _cuda(c["att_full"])[:, :S], c["att_ids"].cuda(),
            _cuda(c["out_table"]), c["contexts"].cuda(), c["negatives"].cuda())
    Ws, Wx = S * D, (P + K) * D
    buf_s = torch.full((B, Ws + 8), 7.0, device="cuda")
    buf_x = torch.full((B, Wx + 4), 7.0, device="cuda")
    d_side, d_att, d_ctx = ops.eges_bwd(*args, first[1], first[2], d_loss, True, d_side=buf_s[:, :Ws], d_ctx=buf_x[:, :Wx])
    assert d_side.data_ptr() == buf_s.data_ptr() and (buf_s[:, Ws:] == 7).all() and (buf_x[:, Wx:] == 7).all()
    assert _bits_equal(d_side, first[4]) and _bits_equal(d_att, first[5]) and _bits_equal(d_ctx, first[6])
    buf_s.fill_(7.0)
    buf_x.fill_(7.0)
    one = ops.eges_fwd(*args, _cuda(c["w"]), True, True, c["scale"], d_side=buf_s[:, :Ws], d_ctx=buf_x[:, :Wx])
    assert (buf_s[:, Ws:] == 7).all() and (buf_x[:, Wx:] == 7).all() and _bits_equal(one[4], first[4]) and _bits_equal(one[6], first[6])


# ---- 5. dr_eges_embed ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BIG)
def test_embed(shape):
    from deep_recommenders_amd import ops
    D, S, P, K, B = shape
    c = _case(shape)
    sid, aid = c["side_ids"].clone(), c["att_ids"].clone()
    sid[5, :] = -1                                              # nothing present: a row of +0.0
    if S > 1:
        sid[6, 0], aid[6] = -1, -1                              # a cold item
    present = sid >= 0
    alpha, w, u, _ = E.aggregate(c["side_table"], c["row_base"], sid, c["att"], aid, present)
    ref = _reference(dict(c, side_ids=sid, att_ids=aid, contexts=torch.zeros_like(c["contexts"])), True)        # every example live: u's bound
    buf = torch.full((B, D + 4), 7.0, device="cuda")
    out = ops.eges_embed(_cuda(c["side_table"]), c["row_base"].cuda(), sid.cuda(), _cuda(c["att_full"])[:, :S], aid.cuda(), out=buf[:, :D])
    assert out.data_ptr() == buf.data_ptr() and (buf[:, D:] == 7).all()
    _within(out, u, ref["b_u"], "embed D %d S %d " % (D, S))
    assert (out[5].view(torch.int32) == 0).all()
    if S > 1:
        rows = (sid[6] + c["row_base"])[1:]
        _within(out[6], c["side_table"][rows].mean(0), ref["b_u"][6], "embed, the cold row against the plain average ")
    again = ops.eges_embed(_cuda(c["side_table"]), c["row_base"].cuda(), sid.cuda(), _cuda(c["att_full"])[:, :S], aid.cuda())
    assert _bits_equal(again, out)
    # the forward's u: with integer tables, one field and d_loss g = 1 forced through the backward, d_ctx is u itself
    if S == 1:
        it = torch.from_numpy(np.random.default_rng(1).integers(-3, 4, size=(NV, D))).float().cuda()
        coeff = torch.ones((B, P + K), device="cuda")
        one = torch.ones(B, device="cuda")
        alpha1 = torch.ones((B, 1), device="cuda")
        ids = c["side_ids"].cuda()
        _, _, d_ctx = ops.eges_bwd(it, c["row_base"].cuda(), ids, None, None, it, c["contexts"].abs().cuda(), c["negatives"].abs().cuda(), coeff,
                                   alpha1, one, False)
        emb = ops.eges_embed(it, c["row_base"].cuda(), ids)
        assert _bits_equal(d_ctx.reshape(B, P + K, D)[:, 0], emb) and torch.equal(emb, it[ids[:, 0]])


# ---- 6. dr_random_walk_weighted ------------------------------------------------------------------------------------------------------------
def _cora_shaped(n=300, seed=0):
    """a planted-partition graph in CSR, undirected, a few nodes left without edges (tests/test_gpu_sgns.py's)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n - 5, size=600)
    b = rng.integers(0, n - 5, size=600)
    nbrs = [set() for _ in range(n)]
    for i, j in zip(a, b):
        if i != j:
            nbrs[i].add(int(j))
            nbrs[j].add(int(i))
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    col = []
    for i, s in enumerate(nbrs):
        col += sorted(s)
        row_ptr[i + 1] = len(col)
    return row_ptr, np.asarray(col, dtype=np.int32)


def _weighted_graph(name):
    if name == "six_nodes":
        return E.weighted_six_node_graph()
    if name == "dead_end":
        return R.dead_end_graph() + (np.asarray([2, 0, 3], dtype=np.int64),)                    # 1 -> 2 has weight 0: the walk ends at 1
    row_ptr, col = _cora_shaped()
    weights = np.random.default_rng(5).integers(0, 5, size=len(col)).astype(np.int64)           # zeros among them
    if name == "cora_shaped":
        weights[row_ptr[7]:row_ptr[8]] = 0                                                      # a row whose total is 0
        weights[3] = 2 ** 31                                                                    # totals up to just under 2^32
    return row_ptr, col, weights


@pytest.mark.parametrize("L", [1, 2, 40])
@pytest.mark.parametrize("graph", ["cora_shaped", "six_nodes", "dead_end"])
def test_weighted_walk_equals_the_restatement(graph, L):
    from deep_recommenders_amd import ops
    row_ptr, col, weights = _weighted_graph(graph)
    cum = np.cumsum(weights)
    n = len(row_ptr) - 1
    rng = np.random.default_rng(L)
    starts = rng.integers(0, n, size=257)
    starts[3], starts[100], starts[256] = -1, n - 1, n
    starts[4:12] = [0, 1, 2, 3, 4, 5, 7, 7][:8] if n > 7 else [0, 1, 2, 3, 0, 1, 2, 3]
    dev = lambda a: torch.from_numpy(a).cuda()                                                  # noqa: E731
    got = ops.random_walk_weighted(dev(row_ptr), dev(col), dev(cum), n, dev(starts), L, seed=99).cpu().numpy()
    want = E.random_walk_weighted_ref(row_ptr, col, cum, n, starts, L, seed=99)
    assert got.shape == (257, L) and np.array_equal(got, want)
    # unit weights: dr_random_walk's walks
    unit = ops.random_walk_weighted(dev(row_ptr), dev(col), dev(np.arange(1, len(col) + 1, dtype=np.int64)), n, dev(starts), L, seed=99)
    assert torch.equal(unit, ops.random_walk(dev(row_ptr), dev(col), n, dev(starts), L, seed=99))
    if L > 1:
        zero = {(i, int(col[e])) for i in range(n) for e in range(row_ptr[i], row_ptr[i + 1]) if weights[e] == 0}
        assert zero and all((int(a), int(b)) not in zero for row in got for a, b in zip(row[:-1], row[1:]) if b >= 0)
        assert (got[3, 1:] == -1).all() and (got[256, 1:] == -1).all() and (got >= 0).sum() > 257
        dead = {"cora_shaped": 7, "six_nodes": 2, "dead_end": 1}[graph]
        assert row_ptr[dead + 1] > row_ptr[dead] and (starts == dead).any()                      # a row with edges whose total is 0
        assert (got[starts == dead][:, 1:] == -1).all()                                         #   ends the walk


# ---- 7. layers.eges_loss -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _update_case():
    """B 40, S 3, P 2, K 5, D 64: side feature 2 of field 1 belongs to every example and id 7 is a negative of every example (40 slots
    of one row each: the sorted K4 cuts them into pieces), item 11 is the centre three times (its att row too), a few masks; rows
    30 .. 36 of every table are named by nobody"""
    B, S, P, K, D = 40, 3, 2, 5, 64
    c = _inputs(np.random.default_rng(78), D, S, P, K, B)
    c["att_full"] = c["att_full"][:, :4].contiguous()           # K4's row: [R, pad4(S)], dense
    c["att"] = c["att_full"][:, :S]
    c["side_ids"][:, 1] = 2
    c["negatives"][:, 0] = 7
    c["side_ids"][:3, 0] = 11
    c["att_ids"] = c["side_ids"][:, 0].clone()
    c["negatives"][5, 1] = c["contexts"][6, 0]
    c["negatives"][9, 3] = -1
    c["side_ids"][12, 2] = -1
    c["side_ids"][13, 0], c["att_ids"][13] = -1, -1
    c["contexts"][14, 1] = -1
    c["negatives"][15, 2] = c["contexts"][15, 1]
    return c


def _table_bounds(c, ref, lr, with_rows):
    """(want, bound) per table for table - lr * gradient (with_rows) or the gradient itself, from the case's float64 rows"""
    h = ref["h"]
    S = c["side_ids"].shape[1]
    nums = (c["side_table"].shape[0], c["att"].shape[0], c["out_table"].shape[0])
    grads = E.table_grads(*nums, c["row_base"], c["side_ids"], c["att_ids"], h)
    absd = dict(h, d_side=h["d_side"].abs(), d_att=h["d_att"].abs(), d_ctx=h["d_ctx"].abs())
    sums = E.table_grads(*nums, c["row_base"], c["side_ids"], c["att_ids"], absd)
    slot = E.table_grads(*nums, c["row_base"], c["side_ids"], c["att_ids"], dict(h, d_side=ref["b_side"], d_att=ref["b_att"], d_ctx=ref["b_ctx"]))
    # K4 sees every id >= 0: a skipped slot adds its zeros and counts
    rows_side = (c["side_ids"] + c["row_base"][None, :])[c["side_ids"] >= 0]
    n_side = torch.bincount(rows_side, minlength=nums[0]).double()
    n_att = torch.bincount(c["att_ids"][c["att_ids"] >= 0], minlength=nums[1]).double()
    n_out = torch.bincount(h["ids"][h["ids"] >= 0], minlength=nums[2]).double()
    olds = (c["side_table"], c["att"].double(), c["out_table"])
    out = []
    for old, g, a, sb, n in zip(olds, grads, sums, slot, (n_side, n_att, n_out)):
        if with_rows:
            out.append((old - lr * g, (n[:, None] + 2) * U * (old.abs() + lr * a) + lr * sb))
        else:
            out.append((g, (n[:, None] + 2) * U * a + sb))
    return out, (n_side, n_att, n_out)


@pytest.mark.parametrize("planned", [False, True])
def test_eges_loss_autograd(planned):
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd import ops
    c = _update_case()
    B, S = c["side_ids"].shape
    J = c["contexts"].shape[1] + c["negatives"].shape[1]
    rng = np.random.default_rng(5)
    up = torch.from_numpy(rng.standard_normal(B).astype(np.float32))
    ids = [t.cuda() for t in (c["row_base"], c["side_ids"], c["att_ids"], c["contexts"], c["negatives"])]
    plans = (lambda: (ops.SortPlan(B * S, "cuda"), ops.SortPlan(B, "cuda"), ops.SortPlan(B * J, "cuda"))) if planned else (lambda: None)
    tag = "planned " if planned else "atomic "

    def tables(frozen=None):
        ts = [_cuda(c["side_table"]), _cuda(c["att_full"]), _cuda(c["out_table"])]
        return [t.requires_grad_(i != frozen) for i, t in enumerate(ts)]

    def run(ts, weight, d_loss, sparse_lr=None):
        rows = L.eges_loss(ts[0], ids[0], ids[1], ts[1], ids[2], ts[2], ids[3], ids[4], None if weight is None else weight.cuda(), True,
                           sparse_lr, plans())
        (rows * d_loss.cuda()).sum().backward()
        return rows

    for what, d_loss, weighted in (("mean", torch.full((B,), 1.0 / B), False), ("weighted sum", up, True)):
        ref = _reference(c, True, d_loss=d_loss, weights=weighted)
        ts = tables()
        rows = run(ts, c["w"].float() if weighted else None, d_loss)
        _within(rows, ref["loss"], ref["b_loss"], tag + what + ": loss_rows")
        # float64 autograd on the literal expression is the reference; the closed form supplies the |terms| of the bounds
        rs = [c["side_table"].clone().requires_grad_(True), c["att"].clone().requires_grad_(True), c["out_table"].clone().requires_grad_(True)]
        expr = E.loss_expr(rs[0], c["row_base"], c["side_ids"], rs[1], c["att_ids"], rs[2], c["contexts"], c["negatives"],
                           c["w"] if weighted else None, True)[0]
        (expr * d_loss.double()).sum().backward()
        wants, counts = _table_bounds(c, ref, 1.0, False)
        assert counts[0][NV + 2] == B and counts[2][7] >= B and counts[1][11] >= 3
        for name, t, r, (want, bound) in zip(("side_table", "att", "out_table"), ts, rs, wants):
            assert (want - r.grad).abs().max() <= 1e-12 * r.grad.abs().max()                    # the closed form is autograd's
            got = t.grad[:, :S] if name == "att" else t.grad
            _within(got, r.grad, bound, tag + what + ": %s.grad" % name)
            assert (t.grad[30:NV] == 0).all()
        assert (ts[1].grad[:, S:] == 0).all()
        if planned:                                                                             # the same inputs, the same bits
            ts2 = tables()
            run(ts2, c["w"].float() if weighted else None, d_loss)
            assert all(_bits_equal(a.grad, b.grad) for a, b in zip(ts, ts2))
    # the sparse_lr form: the step in place, no .grad
    lr = 0.5
    ref = _reference(c, True, d_loss=up, weights=True)
    ts = tables()
    run(ts, c["w"].float(), up, sparse_lr=lr)
    wants, _ = _table_bounds(c, ref, lr, True)
    for name, t, (want, bound) in zip(("side_table", "att", "out_table"), ts, wants):
        assert t.grad is None
        got = t.detach()[:, :S] if name == "att" else t.detach()
        _within(got, want, bound, tag + "sparse_lr: " + name)
    assert _bits_equal(ts[0].detach().cpu()[30:NV], c["side_table"].float()[30:NV]) and _bits_equal(ts[2].detach().cpu()[30:], c["out_table"].float()[30:])
    # each input frozen in turn: None in its slot, the others what they were
    full = tables()
    run(full, c["w"].float(), up)
    wants, _ = _table_bounds(c, ref, 1.0, False)
    for frozen in range(3):
        ts = tables(frozen)
        run(ts, c["w"].float(), up)
        for i in range(3):
            if i == frozen:
                assert ts[i].grad is None
            else:
                _within(ts[i].grad[:, :S] if i == 1 else ts[i].grad, *wants[i], tag + "frozen %d: grad %d" % (frozen, i))
                if planned:
                    assert _bits_equal(ts[i].grad, full[i].grad)
    # no attention table at all
    ts = tables()
    rows = L.eges_loss(ts[0], ids[0], ids[1], None, None, ts[2], ids[3], ids[4], None, True, None, None)
    rows.sum().backward()
    assert ts[1].grad is None and ts[0].grad is not None


# ---- 8. the models -------------------------------------------------------------------------------------------------------------------------
def _toy(seed=3, deterministic=True):
    """64 items in two blocks of 32, the block as side feature, sessions that stay inside a block"""
    from deep_recommenders_amd.keras.models.retrieval import EGES, graph_from_sessions
    rng = np.random.default_rng(0)
    sessions = [(rng.integers(0, 32, size=8) + 32 * (i % 2)).tolist() for i in range(200)]
    block = (np.arange(64) // 32).reshape(64, 1)
    torch.manual_seed(0)
    return EGES(64, [2], block, 16, graph_from_sessions(sessions, 64), walk_length=6, window=2, num_negatives=5, seed=seed,
                deterministic=deterministic)


def _toy_pairs(rng, B=256, V=64):
    centers = rng.integers(0, V, size=B)
    contexts = (centers // 32) * 32 + rng.integers(0, 32, size=B)
    negatives = rng.integers(0, V, size=(B, 5))
    centers[3], contexts[5], negatives[7, 2] = -1, -1, -1
    return torch.from_numpy(centers), torch.from_numpy(contexts), torch.from_numpy(negatives)


def _model_state(m):
    side_ids = lambda centers: torch.where(centers[:, None] >= 0, m.item_fields.cpu()[centers.clamp_min(0)], torch.full((1, 1), -1))     # noqa: E731
    return dict(side_table=m.side_table.detach().cpu().double(), att=m.att.detach().cpu().double()[:, :m.num_fields],
                out_table=m.out_table.detach().cpu().double(), row_base=m.row_base.cpu()), side_ids


def test_eges_train_steps_track_the_restatement():
    m = _toy()
    S = m.num_fields
    assert S == 2 and m.side_table.shape == (66, 16) and m.att.shape == (64, 4) and (m.att == 0).all() and m.row_base.tolist() == [0, 64]
    rng = np.random.default_rng(1)
    curve, want_curve = [], []
    for step in range(8):
        centers, contexts, negatives = _toy_pairs(rng)
        state, side_of = _model_state(m)                        # float64 copies of the fp32 tables this step reads
        side_ids = side_of(centers)
        valid = int(((centers >= 0) & (contexts >= 0)).sum())
        c = dict(state, side_ids=side_ids, att_ids=centers, contexts=contexts[:, None], negatives=negatives, w=torch.ones(256, dtype=DD),
                 scale=float(np.float32(1.0 / valid)))
        ref = _reference(c, True)
        loss = m.train_step(centers.cuda(), contexts.cuda(), EGES_LR, negatives.cuda())
        want = ref["loss"].sum() / valid
        bound = ref["b_loss"].sum() / valid + (256 + 2) * U * want
        print("EGES toy step %d: loss %.6f, float64 %.6f, |err| / bound = %.3f" % (step, float(loss), float(want), abs(float(loss) - float(want)) / float(bound)))
        assert abs(float(loss) - float(want)) <= float(bound)
        curve.append(float(loss))
        wants, counts = _table_bounds(dict(c, att=state["att"]), ref, EGES_LR, True)
        for name, t, (w_t, b_t), n in zip(("side_table", "att", "out_table"), (m.side_table, m.att, m.out_table), wants, counts):
            got = t.detach().cpu()
            got = got[:, :S] if name == "att" else got
            _within(got, w_t, b_t, "EGES toy step %d: %s" % (step, name))
            old = state[name].float()
            assert _bits_equal(got[n == 0], old[n == 0])       # rows the batch does not name keep their bits
        assert (m.att.detach()[:, S:] == 0).all()
    assert np.isfinite(curve).all() and np.mean(curve[-2:]) < 0.95 * np.mean(curve[:2])
    # two runs from one seed: the same bits
    def run():                                                  # noqa: E306
        mm, r = _toy(), np.random.default_rng(1)
        losses = []
        for _ in range(3):
            ce, co, _ = _toy_pairs(r)
            losses.append(mm.train_step(ce.cuda(), co.cuda(), EGES_LR))                         # the model's own negatives
        return mm, torch.stack(losses)
    (m1, l1), (m2, l2) = run(), run()
    assert _bits_equal(l1, l2) and m1.draw_offset == 3 * 256 * 5
    for a, b in ((m1.side_table, m2.side_table), (m1.att, m2.att), (m1.out_table, m2.out_table)):
        assert _bits_equal(a.detach(), b.detach())
    assert float(m1.att.detach().abs().max()) > 0


def test_eges_walks_loss_and_embeddings():
    from deep_recommenders_amd import layers as L
    m = _toy(deterministic=False)
    starts = torch.arange(64, dtype=torch.int64, device="cuda")
    walks = m.walks(starts)
    adj = m.adjacency
    want = E.random_walk_weighted_ref(adj.row_ptr.cpu().numpy(), adj.col.cpu().numpy(), m.cum.cpu().numpy(), 64, starts.cpu().numpy(), 6, seed=3 + 1)
    assert np.array_equal(walks.cpu().numpy(), want)
    w = walks.cpu().numpy()
    assert ((w // 32 == w[:, :1] // 32) | (w < 0)).all()         # sessions stay inside a block, so do the walks
    centers, contexts = m.walk_batch(starts)
    assert centers.shape == (64 * 6 * 4,) and torch.equal(centers >= 0, contexts >= 0)
    loss = m.loss(centers, contexts)
    loss.backward()
    assert torch.isfinite(loss) and m.side_table.grad is not None and m.att.grad is not None and m.out_table.grad is not None
    H = m.embeddings()
    state, _ = _model_state(m)
    fields = m.item_fields.cpu()
    ref = _reference(dict(state, side_ids=fields, att_ids=fields[:, 0].clone(), contexts=torch.zeros((64, 1), dtype=torch.int64),
                          negatives=torch.zeros((64, 0), dtype=torch.int64), w=torch.ones(64, dtype=DD), scale=1.0), True)
    assert H.shape == (64, 16)
    _within(H, ref["u"], ref["b_u"], "EGES.embeddings ")
    cold = torch.tensor([[-1, 0], [-1, 1], [-1, -1]])
    Hc = m.embeddings(cold)
    assert _bits_equal(Hc[:2], m.side_table.detach()[64:66]) and (Hc[2].view(torch.int32) == 0).all()
    with pytest.raises(ValueError):
        from deep_recommenders_amd.keras.models.retrieval import EGES
        EGES(4, [2], np.zeros((4, 1)), 8, ([(0, 1)], [0.5], (4, 4)), walk_length=3, window=1)   # a weight that is no integer


def test_airbnb():
    from deep_recommenders_amd.keras.models.retrieval import Airbnb, SkipGram
    V, D, K, Km, B = 60, 16, 3, 2, 200
    market_of = np.arange(V) % 4
    rng = np.random.default_rng(2)
    centers = torch.from_numpy(rng.integers(0, V, size=B))
    contexts = torch.from_numpy(rng.integers(0, V, size=B))
    negatives = torch.from_numpy(rng.integers(0, V, size=(B, K + Km)))
    centers[3], contexts[5], negatives[7, 1] = -1, -1, -1
    torch.manual_seed(0)
    a = Airbnb(V, D, market_of, num_negatives=K, num_market_negatives=Km, seed=1, deterministic=True)
    s = SkipGram(V, D, num_negatives=K + Km, seed=1, deterministic=True)
    with torch.no_grad():
        s.in_table.copy_(a.in_table)
        s.out_table.copy_(a.out_table)
    tin, tout = a.in_table.detach().cpu().double(), a.out_table.detach().cpu().double()
    # no booking anywhere: SkipGram's step, bit for bit
    none = torch.full((B,), -1, dtype=torch.int64)
    la = a.train_step(centers.cuda(), contexts.cuda(), none.cuda(), 0.5, negatives.cuda())
    ls = s.train_step(centers.cuda(), contexts.cuda(), 0.5, negatives.cuda())
    assert _bits_equal(la, ls) and _bits_equal(a.in_table.detach(), s.in_table.detach()) and _bits_equal(a.out_table.detach(), s.out_table.detach())
    assert not _bits_equal(a.in_table.detach().cpu(), tin.float())
    # with bookings: the P = 2 restatement, from the tables as they are now
    booked = torch.from_numpy(rng.integers(0, V, size=B))
    booked[::3] = -1
    tin, tout = a.in_table.detach().cpu().double(), a.out_table.detach().cpu().double()
    valid = int(((centers >= 0) & (contexts >= 0)).sum())
    c = dict(side_table=tin, row_base=torch.zeros(1, dtype=torch.int64), side_ids=centers[:, None], att=None, att_ids=None, out_table=tout,
             contexts=torch.stack([contexts, booked], 1), negatives=negatives, w=torch.ones(B, dtype=DD), scale=float(np.float32(1.0 / valid)))
    ref = _reference(c, True, att=False)
    loss = a.train_step(centers.cuda(), contexts.cuda(), booked.cuda(), 0.5, negatives.cuda())
    want = ref["loss"].sum() / valid
    assert abs(float(loss) - float(want)) <= float(ref["b_loss"].sum() / valid + (B + 2) * U * want)
    h = ref["h"]
    g_side, _, g_out = E.table_grads(V, 1, V, c["row_base"], c["side_ids"], None, h)
    a_side, _, a_out = E.table_grads(V, 1, V, c["row_base"], c["side_ids"], None, dict(h, d_side=h["d_side"].abs(), d_ctx=h["d_ctx"].abs()))
    s_side, _, s_out = E.table_grads(V, 1, V, c["row_base"], c["side_ids"], None, dict(h, d_side=ref["b_side"], d_ctx=ref["b_ctx"]))
    n_in = torch.bincount(centers[centers >= 0], minlength=V).double()
    n_out = torch.bincount(h["ids"][h["ids"] >= 0], minlength=V).double()
    for name, got, old, g, ab, sb, n in (("in_table", a.in_table, tin, g_side, a_side, s_side, n_in), ("out_table", a.out_table, tout, g_out, a_out, s_out, n_out)):
        _within(got, old - 0.5 * g, (n[:, None] + 2) * U * (old.abs() + 0.5 * ab) + 0.5 * sb, "Airbnb with bookings: " + name)
    # the model's own negatives: K from the alias table, then Km members of the centre's market
    cm = centers.cuda()
    market = a.sample_market_negatives(cm).cpu()
    assert market.shape == (B, Km)
    ok = centers >= 0
    assert (market[~ok] == -1).all() and (market[ok] >= 0).all() and (market[ok] % 4 == (centers[ok] % 4)[:, None]).all()
    assert len(set(market[ok].reshape(-1).tolist())) > 8 and not torch.equal(market, a.sample_market_negatives(cm).cpu())
    before = a.draw_offset
    a.train_step(cm, contexts.cuda(), booked.cuda(), 0.5)
    assert a.draw_offset == before + B * K and torch.isfinite(a.in_table).all() and torch.isfinite(a.out_table).all()
    assert torch.isfinite(a.loss(cm, contexts.cuda(), booked.cuda()))


# ---- 9. the C ABI's domain -------------------------------------------------------------------------------------------------------------------
def test_c_abi_domain():
    from deep_recommenders_amd import _lib
    L = _lib.lib()
    s = _lib.stream_ptr()
    p = _lib.ptr
    t = torch.zeros((8, 8), device="cuda")
    base = torch.zeros(2, dtype=torch.int64, device="cuda")
    sid = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    ids = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    neg = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    aid = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.zeros(64, device="cuda")
    big = torch.zeros(512, device="cuda")

    def fwd(**k):
        return L.dr_eges_fwd(k.get("st", p(t)), k.get("D", 8), k.get("rb", p(base)), k.get("sid", p(sid)), k.get("S", 2), k.get("att", p(t)),
                             k.get("ld_att", 8), k.get("aid", p(aid)), k.get("ot", p(t)), p(ids), k.get("P", 2), k.get("neg", p(neg)),
                             k.get("K", 3), k.get("B", 2), None, k.get("flags", 1), 1.0, k.get("loss", p(out)), p(out[8:]), k.get("alpha", p(out[24:])),
                             None, k.get("ds", p(big)), k.get("ld_ds", 16), k.get("da", p(big[64:])), k.get("ld_da", 4), k.get("dx", p(big[128:])),
                             k.get("ld_dx", 40), s)

    bad_shapes = (dict(D=6), dict(D=260), dict(D=0), dict(S=0), dict(S=17), dict(P=0), dict(P=5), dict(K=-1), dict(K=63), dict(B=-1), dict(flags=2))
    bad_grads = (dict(ld_ds=12), dict(ld_ds=18), dict(ld_da=0), dict(ld_da=6), dict(ld_da=20), dict(ld_dx=36), dict(ld_dx=42), dict(ds=p(big) + 4),
                 dict(da=p(big) + 4), dict(dx=p(big) + 4), dict(ds=None), dict(da=None), dict(dx=None))
    bad_ptrs = (dict(st=None), dict(st=p(t) + 4), dict(rb=None), dict(sid=None), dict(aid=None), dict(ld_att=1), dict(ot=None), dict(ot=p(t) + 4),
                dict(neg=None), dict(loss=None), dict(alpha=None))
    assert fwd() == _lib.DR_OK and fwd(B=0) == _lib.DR_OK and fwd(B=0, st=None, sid=None) == _lib.DR_OK
    for bad in bad_shapes + bad_grads + bad_ptrs:
        assert fwd(**bad) == _lib.DR_EINVAL, bad
    assert fwd(ds=None, da=None, dx=None, ld_ds=0, ld_da=0, ld_dx=0) == _lib.DR_OK              # no gradient rows: pitches ignored
    assert fwd(att=None, aid=None, ld_att=0) == _lib.DR_OK and fwd(K=0, neg=None, ld_dx=16) == _lib.DR_OK
    none = dict(ds=None, da=None, dx=None)
    assert fwd(P=4, K=60, B=0, **none) == _lib.DR_OK and fwd(P=4, K=61, B=0, **none) == _lib.DR_EINVAL

    def bwd(**k):
        return L.dr_eges_bwd(k.get("st", p(t)), k.get("D", 8), p(base), p(sid), k.get("S", 2), k.get("att", p(t)), k.get("aid", p(aid)), p(t),
                             p(ids), k.get("P", 2), p(neg), k.get("K", 3), k.get("B", 2), 1, k.get("coeff", p(out)), k.get("alpha", p(out[24:])),
                             k.get("dl", p(out[32:])), k.get("ds", p(big)), k.get("ld_ds", 16), p(big[64:]), k.get("ld_da", 4), p(big[128:]),
                             k.get("ld_dx", 40), s)

    assert bwd() == _lib.DR_OK and bwd(B=0) == _lib.DR_OK and bwd(att=None, aid=None) == _lib.DR_OK
    for bad in (dict(D=6), dict(S=17), dict(P=5), dict(K=63), dict(ld_ds=12), dict(ld_da=6), dict(ld_dx=36), dict(ds=None), dict(ds=p(big) + 4),
                dict(coeff=None), dict(alpha=None), dict(dl=None), dict(aid=None), dict(st=None)):
        assert bwd(**bad) == _lib.DR_EINVAL, bad

    def emb(**k):
        return L.dr_eges_embed(k.get("st", p(t)), k.get("D", 8), p(base), k.get("sid", p(sid)), k.get("S", 2), k.get("att", p(t)), k.get("ld_att", 8),
                               k.get("aid", p(aid)), k.get("n", 2), k.get("out", p(big)), k.get("ld_out", 8), s)

    assert emb() == _lib.DR_OK and emb(n=0) == _lib.DR_OK and emb(att=None, aid=None) == _lib.DR_OK
    for bad in (dict(D=6), dict(S=0), dict(S=17), dict(n=-1), dict(ld_out=4), dict(ld_out=10), dict(out=None), dict(out=p(big) + 4), dict(st=None),
                dict(sid=None), dict(aid=None), dict(ld_att=1)):
        assert emb(**bad) == _lib.DR_EINVAL, bad
    rp = torch.zeros(3, dtype=torch.int64, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    o64 = torch.zeros(8, dtype=torch.int64, device="cuda")
    col = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.dr_random_walk_weighted(p(rp), None, None, 2, p(st), 2, 4, 1, p(o64), s) == _lib.DR_OK
    assert L.dr_random_walk_weighted(p(rp), None, None, 2, p(st), 0, 4, 1, p(o64), s) == _lib.DR_OK
    assert L.dr_random_walk_weighted(p(rp), None, None, 2, p(st), 2, 0, 1, p(o64), s) == _lib.DR_EINVAL
    assert L.dr_random_walk_weighted(p(rp), p(col), None, 2, p(st), 2, 4, 1, p(o64), s) == _lib.DR_EINVAL
    assert L.dr_random_walk_weighted(None, None, None, 2, p(st), 2, 4, 1, p(o64), s) == _lib.DR_EINVAL
    assert L.dr_random_walk_weighted(p(rp), None, None, -1, p(st), 2, 4, 1, p(o64), s) == _lib.DR_EINVAL
    torch.cuda.synchronize()
    assert o64.tolist() == [0, -1, -1, -1, 0, -1, -1, -1]       # a graph without edges: every walk ends at its start


# Largest |err| / bound read on an MI355X, over all shapes and the mask cases:
#   alpha 0.171  scores 0.124  loss_rows 0.056  coeff 0.154  d_side 0.065  d_att 0.010  d_ctx 0.134  dr_eges_embed 0.177
#   layers.eges_loss: side_table.grad 0.023, att.grad 0.001, out_table.grad 0.056; after the sparse_lr step 0.216 (side_table), 0.034 (att)
#   EGES toy, eight steps at lr 4: loss 4.1296 4.1026 4.0766 4.0358 3.9768 3.8731 3.7152 3.5387, each within 0.004 of its bound;
#     tables after a step 0.236 (side_table), 0.021 (att), 0.054 (out_table)
#   Airbnb with bookings: in_table 0.296, out_table 0.052
