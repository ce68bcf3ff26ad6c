"""GPU tests of skip-gram with negative sampling (csrc/sgns.hip), the alias sampler and the random walk (csrc/sampling.hip), the
autograd glue (layers.sgns_loss) and the models (SkipGram, DeepWalk) against the float64 restatement in tests/sgns_ref.py.

Tolerances, u32 = 2^-24.  None is read off the kernel.
  scores    integer tables with D max^2 < 2^24: every partial sum is exact, bit-equal to float64 rounded to fp32.
            random tables: |s_j - ref| <= sb_j = (D + 1) u32 sum_d |u_d v_jd|   (any summation order, fused or not)
  loss      |softplus'| <= 1:  w_b sum_j (sb_j + 4 A_sp) + (K + 3) u32 w_b sum_j softplus_j   (K adds, one multiply by w_b, one spare)
  coeff     |sigmoid'| <= 1/4: cb_j = w_b (sb_j / 4 + 4 A_sg) + 2 u32 |g_j|                    (the subtraction and the multiply by w_b)
  d_center  (K + 4) u32 sum_j |c_j v_jd| + |scale| sum_j cb_j |v_jd|
  d_ctx     3 u32 |c_j u_d| + |scale| cb_j |u_d|
  A_sp, A_sg: the transcendental allowance, MEASURED HERE ON THE CPU at import as the largest |fp32 torch - float64| of softplus resp.
            sigmoid over 2^16 + 1 evenly spaced fp32 points of [-S, S], S = 8 covering every score of the random cases (tables are
            N(0, 1) D^-1/4, scores ~ N(0, 1); the cases assert |s| <= S).  Measured: A_sp = 3.13e-07 (two thirds of an ulp at
            4 .. 8), A_sg = 8.86e-08 (1.5 ulp below 1); each enters with a margin of 4: the device's expf / log1pf are other
            implementations of the same 1 - 2 ulp class, and a wrong formula is off by orders of magnitude more.
  tables    after a step, against float64 index_add_ of the float64 gradient rows: (n_slots(row) + 2) u32 (|row| + lr sum_slots |term|).
            Rows one slot names: bit-equal to row + fl(scale g) or to fma(scale, g, row) of the fp32 gradient row the kernel wrote.
  .grad     (n_slots(row) + 2) u32 sum_slots |term| for the adds, plus the slots' own d_center / d_ctx bounds."""
import functools

import numpy as np
import pytest
import torch

import sgns_ref as R

pytestmark = pytest.mark.gpu

DD = torch.float64
U = 2.0 ** -24
S_MAX = 8.0
NV = 37                     # table rows of the kernel cases
MARGIN = 4.0
# the mean loss divides every pair's gradient by the valid pairs of the batch: 16 / 256 and 100 / ~5000 per pair, chosen on the float64
# restatement of the step (toy: 4.06 -> 2.22 at 16; DeepWalk: 2.78 -> 2.17 at 50 and -> 1.19 at 200, diverging at 800)
TOY_LR, DEEPWALK_LR = 16.0, 100.0
DS, KS, BS = (4, 20, 64, 100, 256), (0, 1, 5, 63), (1, 3, 257)
# every D with K 5, every K with D 64, every B in both
SHAPES = [(D, 5, B) for D in DS for B in BS] + [(64, K, B) for K in KS if K != 5 for B in BS]


def _measure(fn):
    x = torch.linspace(-S_MAX, S_MAX, 2 ** 16 + 1, dtype=torch.float32)
    return float((fn(x).double() - fn(x.double())).abs().max())


A_SP = _measure(torch.nn.functional.softplus)
A_SG = _measure(torch.sigmoid)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cuda(a):
    return a.to(torch.float32).cuda() if a.is_floating_point() else a.cuda()


def _within(got, want, bound, what):
    err = (got.detach().double().cpu().reshape(want.shape) - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print("%s: max |err| / bound = %.3f" % (what, ratio))
    assert (err <= bound).all(), "%s: max |err| / bound = %.3f" % (what, ratio)


def _ids(rng, B, K, V):
    centers = torch.from_numpy(rng.integers(0, V, size=B))
    contexts = torch.from_numpy(rng.integers(0, V, size=B))
    negatives = torch.from_numpy(rng.integers(0, V, size=(B, K)))
    return centers, contexts, negatives


@functools.lru_cache(maxsize=None)
def _case(shape):
    """random tables (float32 values held in float64), ids, weights and the float64 results with their bounds; computed once, never
    modified.  scale = 1 / B stands for row_scale."""
    D, K, B = shape
    rng = np.random.default_rng(3000 + SHAPES.index(shape))
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DD)         # noqa: E731
    amp = float(np.float32(D ** -0.25))
    tin, tout = (t(NV, D) * amp).float().to(DD), (t(NV, D) * amp).float().to(DD)
    centers, contexts, negatives = _ids(rng, B, K, NV)
    if B >= 3 and K >= 1:
        negatives[1, K - 1] = -1                                                               # a masked slot among ordinary ones
    w = torch.from_numpy((rng.random(B) + 0.5).astype(np.float32)).to(DD)
    scale = float(np.float32(1.0 / B))
    c = dict(tin=tin, tout=tout, centers=centers, contexts=contexts, negatives=negatives, w=w, scale=scale)
    c.update(_reference(c, True))
    return c


def _reference(c, skip_equal):
    """the float64 results of the case's inputs and the bounds of the header"""
    tin, tout, centers, contexts, negatives, w, scale = (c[k] for k in ("tin", "tout", "centers", "contexts", "negatives", "w", "scale"))
    B, K, D = negatives.shape[0], negatives.shape[1], tin.shape[1]
    ids, keep = R.masks(centers, contexts, negatives, skip_equal)
    u, v = R.gather(tin, tout, centers, ids, keep)
    loss, scores, _ = R.loss_expr(tin, tout, centers, contexts, negatives, w, skip_equal)
    assert float(scores.abs().max()) <= S_MAX
    g, d_center, d_ctx, abs_center, abs_ctx = R.hand_grads(tin, tout, centers, contexts, negatives, torch.full((B,), scale, dtype=DD), w,
                                                           skip_equal)
    kd = keep.double()
    sb = (D + 1) * U * (u[:, None, :] * v).abs().sum(-1) * kd
    sign = torch.ones(1 + K, dtype=DD)
    sign[0] = -1.0
    sp = torch.nn.functional.softplus(sign[None, :] * scores) * kd
    loss_b = w * ((sb + MARGIN * A_SP) * kd).sum(1) + (K + 3) * U * w * sp.sum(1)
    cb = (w[:, None] * (sb / 4 + MARGIN * A_SG) + 2 * U * g.abs()) * kd
    center_b = (K + 4) * U * abs_center + abs(scale) * (cb[:, :, None] * v.abs()).sum(1)
    ctx_b = 3 * U * abs_ctx + abs(scale) * cb[:, :, None] * u.abs()[:, None, :]
    return dict(keep=keep, loss=loss, scores=scores, coeff=g, d_center=d_center, d_ctx=d_ctx,
                b_scores=sb, b_loss=loss_b, b_coeff=cb, b_center=center_b, b_ctx=ctx_b)


def _run(c, grads=True, want_scores=True, skip_equal=True, weights=True, sl=slice(None)):
    from deep_recommenders_amd import ops
    return ops.sgns_fwd(_cuda(c["tin"]), _cuda(c["tout"]), c["centers"][sl].cuda(), c["contexts"][sl].cuda(), c["negatives"][sl].cuda(),
                        _cuda(c["w"][sl]) if weights else None, skip_equal, want_scores, c["scale"] if grads else None)


@pytest.mark.parametrize("shape", SHAPES)
def test_scores_on_integer_grids_are_exact(shape):
    from deep_recommenders_amd import ops
    D, K, B = shape
    rng = np.random.default_rng(10 + SHAPES.index(shape))
    tin = torch.from_numpy(rng.integers(-3, 4, size=(NV, D))).to(DD)                           # D max^2 <= 256 * 9 < 2^24
    tout = torch.from_numpy(rng.integers(-3, 4, size=(NV, D))).to(DD)
    centers, contexts, negatives = _ids(rng, B, K, NV)
    _, want, _ = R.loss_expr(tin, tout, centers, contexts, negatives, None, False)
    _, _, scores, _, _ = ops.sgns_fwd(_cuda(tin), _cuda(tout), centers.cuda(), contexts.cuda(), negatives.cuda(), None, False, True)
    assert scores.shape == (B, 1 + K)
    assert _bits_equal(scores.cpu() + 0.0, want.float() + 0.0)                                 # + 0.0: a zero's sign is no rounding


@pytest.mark.parametrize("shape", SHAPES)
def test_random_tables_within_the_derived_bounds(shape):
    D, K, B = shape
    c = _case(shape)
    loss, coeff, scores, d_center, d_ctx = _run(c)
    tag = "D %d K %d B %d " % shape
    _within(scores, c["scores"], c["b_scores"], tag + "scores")
    _within(loss, c["loss"], c["b_loss"], tag + "loss_rows")
    _within(coeff, c["coeff"], c["b_coeff"], tag + "coeff")
    _within(d_center, c["d_center"], c["b_center"], tag + "d_center")
    _within(d_ctx, c["d_ctx"], c["b_ctx"], tag + "d_ctx")
    skipped = ~c["keep"]
    assert (coeff.cpu()[skipped] == 0).all() and (scores.cpu()[skipped] == 0).all()
    assert (d_ctx.cpu().reshape(B, 1 + K, D)[skipped].view(torch.int32) == 0).all()             # +0.0, bit for bit


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2] == 257])
def test_reproducible_and_independent_of_the_batch(shape):
    from deep_recommenders_amd import ops
    D, K, B = shape
    c = _case(shape)
    first, again = _run(c), _run(c)
    for a, b in zip(first, again):                                                             # run to run
        assert _bits_equal(a, b)
    plain = _run(c, grads=False, want_scores=False)                                            # the gradient outputs change nothing else
    assert _bits_equal(plain[0], first[0]) and _bits_equal(plain[1], first[1]) and plain[2] is None and plain[3] is None
    for b in (0, 1, 100, 255, 256):                                                            # an example alone: another block shape
        alone = _run(c, sl=slice(b, b + 1))
        for a, f in zip(alone, first):
            assert _bits_equal(a, f[b:b + 1]), (shape, b)
    # the backward, d_loss == row_scale: the same bits as the one-pass form; padded buffers at a pitch are written in place
    d_loss = torch.full((B,), c["scale"], dtype=torch.float32, device="cuda")
    args = (_cuda(c["tin"]), _cuda(c["tout"]), c["centers"].cuda(), c["contexts"].cuda(), c["negatives"].cuda())
    W = (1 + K) * D
    buf_c = torch.full((B, D + 8), 7.0, device="cuda")
    buf_x = torch.full((B, W + 4), 7.0, device="cuda")
    d_center, d_ctx = ops.sgns_bwd(*args, first[1], d_loss, True, d_center=buf_c[:, :D], d_ctx=buf_x[:, :W])
    assert d_center.data_ptr() == buf_c.data_ptr() and (buf_c[:, D:] == 7).all() and (buf_x[:, W:] == 7).all()
    assert _bits_equal(d_center, first[3]) and _bits_equal(d_ctx, first[4])


@pytest.mark.parametrize("skip_equal", [True, False])
@pytest.mark.parametrize("shape", [(20, 5, 257), (64, 5, 257), (256, 5, 3)])
def test_skip_rules(shape, skip_equal):
    """a center of -1, a context of -1, a negative of -1, a negative equal to the positive; ids of 2^62 in masked slots reach nothing"""
    D, K, B = shape
    c = _case(shape)
    base = _run(c, skip_equal=skip_equal)
    centers, contexts, negatives = c["centers"].clone(), c["contexts"].clone(), c["negatives"].clone()
    big = 2 ** 62
    changed = [0, 1] if B == 3 else [0, 1, 63, 64, 200, 256]
    centers[changed[0]] = -1
    negatives[changed[0], 0] = big                              # the example is skipped: its other ids are never looked at
    contexts[changed[1]] = -1
    centers[changed[1]] = big
    eq = None
    if B > 3:
        negatives[63, 2] = -1
        negatives[64, 1] = contexts[64]                         # equal to the positive
        negatives[200, 0] = -1
        negatives[200, 4] = -1
        negatives[256, K - 1] = contexts[256]
        eq = [(64, 2), (256, K)]                                # (example, slot)
    mod = dict(c, centers=centers, contexts=contexts, negatives=negatives)
    mod.update(_reference(mod, skip_equal))
    got = _run(mod, skip_equal=skip_equal)
    tag = "skips, D %d skip_equal %s: " % (D, skip_equal)
    for name, t in zip(("loss", "coeff", "scores", "d_center", "d_ctx"), got):                  # everything, against the masked reference
        _within(t, mod[name], mod["b_" + {"d_center": "center", "d_ctx": "ctx"}.get(name, name)], tag + name)
    loss, coeff, scores, d_center, d_ctx = [t.cpu() for t in got]
    d_ctx = d_ctx.reshape(B, 1 + K, D)
    for b in changed[:2]:                                       # whole examples
        assert loss[b] == 0 and (coeff[b] == 0).all() and (scores[b] == 0).all()
        assert (d_center[b].view(torch.int32) == 0).all() and (d_ctx[b].view(torch.int32) == 0).all()
    untouched = [b for b in range(B) if b not in changed]
    for a, f in zip(got, base):
        assert _bits_equal(a[untouched], f[untouched])
    if B > 3:
        for b, j in ((63, 3), (200, 1), (200, 5)):              # negatives of -1
            assert coeff[b, j] == 0 and scores[b, j] == 0 and (d_ctx[b, j].view(torch.int32) == 0).all()
        for b, j in eq:
            if skip_equal:
                assert coeff[b, j] == 0 and scores[b, j] == 0 and (d_ctx[b, j].view(torch.int32) == 0).all()
            else:                                               # the same row as the positive: the same score, a negative's coefficient
                assert scores[b, j] == scores[b, 0] and coeff[b, j] != 0
        # the slots those examples keep: unchanged bit for bit
        bs = [63, 64, 200, 256]
        same = mod["keep"][bs].clone()
        same[:, 1:] &= negatives[bs] == c["negatives"][bs]
        assert _bits_equal(got[1].cpu()[bs][same], base[1].cpu()[bs][same]) and _bits_equal(got[2].cpu()[bs][same], base[2].cpu()[bs][same])


@functools.lru_cache(maxsize=None)
def _update_case():
    """B 40, K 5, V 50, D 64: id 7 is a negative of every example (40 slots: the sorted K4 cuts the row into pieces), center 11 is used
    three times, example 6's positive is a negative of example 5, rows 40 .. 49 of both tables are named by nobody"""
    B, K, V, D = 40, 5, 50, 64
    rng = np.random.default_rng(77)
    t = lambda *s: torch.from_numpy((rng.standard_normal(s) * D ** -0.25).astype(np.float32)).to(DD)     # noqa: E731
    tin, tout = t(V, D), t(V, D)
    centers = torch.from_numpy(rng.integers(0, 40, size=B))
    contexts = torch.from_numpy(rng.integers(8, 40, size=B))
    negatives = torch.from_numpy(rng.integers(0, 40, size=(B, K)))
    negatives[:, 0] = 7
    centers[:3] = 11
    negatives[5, 1] = contexts[6]
    negatives[9, 3] = -1
    return dict(B=B, K=K, V=V, D=D, tin=tin, tout=tout, centers=centers, contexts=contexts, negatives=negatives)


def _model_from(c, deterministic, seed=0):
    from deep_recommenders_amd.keras.models.retrieval import SkipGram
    m = SkipGram(c["V"], c["D"], num_negatives=c["K"], deterministic=deterministic, seed=seed)
    with torch.no_grad():
        m.in_table.copy_(_cuda(c["tin"]))
        m.out_table.copy_(_cuda(c["tout"]))
    return m


@pytest.mark.parametrize("deterministic", [False, True])
def test_table_update(deterministic):
    from deep_recommenders_amd import ops
    c = _update_case()
    B, K, V, D = c["B"], c["K"], c["V"], c["D"]
    lr = 0.5
    centers, contexts, negatives = c["centers"], c["contexts"], c["negatives"]
    valid = B
    scale = float(np.float32(1.0 / valid))
    ids, keep = R.masks(centers, contexts, negatives, True)
    named = torch.where(keep, ids, torch.full_like(ids, -1))
    g, d_center, d_ctx, _, _ = R.hand_grads(c["tin"], c["tout"], centers, contexts, negatives, torch.full((B,), scale, dtype=DD), None, True)
    g_in, g_out = R.table_grads(V, V, centers, named, keep, d_center, d_ctx)
    a_in, a_out = R.table_grads(V, V, centers, named, keep, d_center.abs(), d_ctx.abs())
    n_in = torch.bincount(centers, minlength=V).double()
    n_out = torch.bincount(ids[ids >= 0], minlength=V).double()           # K4 sees every id >= 0, a skipped slot adds its zeros
    assert n_out[7] > 32 and n_in[11] >= 3
    m = _model_from(c, deterministic)
    # the fp32 gradient rows the step applies (the same call, hence the same bits: test_reproducible_...)
    _, _, _, k_center, k_ctx = ops.sgns_fwd(m.in_table.data, m.out_table.data, centers.cuda(), contexts.cuda(), negatives.cuda(), None, True,
                                            row_scale=1.0 / valid)
    loss = m.train_step(centers.cuda(), contexts.cuda(), lr, negatives.cuda())
    want_loss = R.loss_expr(c["tin"], c["tout"], centers, contexts, negatives)[0].sum() / valid
    assert abs(float(loss) - float(want_loss)) <= 1e-5 * float(want_loss)
    tag = "deterministic " if deterministic else "atomic "
    for name, got, old, grad, absg, n in (("in_table", m.in_table, c["tin"], g_in, a_in, n_in), ("out_table", m.out_table, c["tout"], g_out, a_out, n_out)):
        bound = (n[:, None] + 2) * U * (old.abs() + lr * absg)
        _within(got, old - lr * grad, bound, tag + name + " after the step")
        assert _bits_equal(got.detach().cpu()[40:], old.float()[40:])                          # rows no id names
    # rows one slot names: exact against the fp32 gradient row
    k_center, k_ctx = k_center.cpu(), k_ctx.cpu().reshape(B, 1 + K, D)
    s32 = torch.tensor(-lr, dtype=torch.float32)
    checked = 0
    for b in range(B):
        for table, old, row, grad, count in ([(m.in_table, c["tin"], int(centers[b]), k_center[b], n_in)] +
                                             [(m.out_table, c["tout"], int(ids[b, j]), k_ctx[b, j], n_out) for j in range(1 + K)]):
            if row < 0 or count[row] != 1:
                continue
            o32 = old[row].float()
            two = o32 + s32 * grad
            fused = (o32.double() + s32.double() * grad.double()).float()
            new = table.detach().cpu()[row]
            assert ((new == two) | (new == fused)).all(), (b, row)
            checked += 1
    assert checked >= 5
    if deterministic:                                                                          # the same state, the same bits
        m2 = _model_from(c, True)
        m2.train_step(centers.cuda(), contexts.cuda(), lr, negatives.cuda())
        assert _bits_equal(m2.in_table.detach(), m.in_table.detach()) and _bits_equal(m2.out_table.detach(), m.out_table.detach())


@pytest.mark.parametrize("planned", [False, True])
def test_sgns_loss_autograd(planned):
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd import ops
    c = _update_case()
    B, K, V, D = c["B"], c["K"], c["V"], c["D"]
    centers, contexts, negatives = c["centers"], c["contexts"], c["negatives"]
    rng = np.random.default_rng(5)
    sw = torch.from_numpy((rng.random(B) + 0.5).astype(np.float32))
    up = torch.from_numpy(rng.standard_normal(B).astype(np.float32))
    ids, keep = R.masks(centers, contexts, negatives, True)
    named = torch.where(keep, ids, torch.full_like(ids, -1))
    n_in = torch.bincount(centers, minlength=V).double()
    n_out = torch.bincount(ids[ids >= 0], minlength=V).double()
    plans = (ops.SortPlan(B, "cuda"), ops.SortPlan(B * (1 + K), "cuda")) if planned else None
    for what, d_loss, weight in (("mean", torch.full((B,), 1.0 / B), None), ("weighted sum", up, sw)):
        tin, tout = _cuda(c["tin"]).requires_grad_(True), _cuda(c["tout"]).requires_grad_(True)
        rows = L.sgns_loss(tin, tout, centers.cuda(), contexts.cuda(), negatives.cuda(), None if weight is None else weight.cuda(), True, None, plans)
        (rows.mean() if what == "mean" else (rows * up.cuda()).sum()).backward()
        want_rows = R.loss_expr(c["tin"], c["tout"], centers, contexts, negatives, weight, True)[0]
        assert (rows.detach().cpu().double() - want_rows).abs().max() <= 1e-5 * want_rows.abs().max()
        # float64 autograd on the literal expression is the reference; the closed form supplies the |terms| of the bounds
        rin, rout = c["tin"].clone().requires_grad_(True), c["tout"].clone().requires_grad_(True)
        (R.loss_expr(rin, rout, centers, contexts, negatives, weight, True)[0] * d_loss.double()).sum().backward()
        g, d_center, d_ctx, abs_center, abs_ctx = R.hand_grads(c["tin"], c["tout"], centers, contexts, negatives, d_loss, weight, True)
        u, v = R.gather(c["tin"], c["tout"], centers, ids, keep)
        w = torch.ones(B, dtype=DD) if weight is None else weight.double()
        kd = keep.double()
        sb = (D + 1) * U * (u[:, None, :] * v).abs().sum(-1) * kd
        cb = (w[:, None] * (sb / 4 + MARGIN * A_SG) + 2 * U * g.abs()) * kd
        dl = d_loss.double().abs()
        center_b = (K + 4) * U * abs_center + dl[:, None] * (cb[:, :, None] * v.abs()).sum(1)
        ctx_b = 3 * U * abs_ctx + dl[:, None, None] * cb[:, :, None] * u.abs()[:, None, :]
        a_in, a_out = R.table_grads(V, V, centers, named, keep, d_center.abs(), d_ctx.abs())
        b_in, b_out = R.table_grads(V, V, centers, named, keep, center_b, ctx_b)
        tag = "%s, %s: " % (what, "planned" if planned else "atomic")
        _within(tin.grad, rin.grad, (n_in[:, None] + 2) * U * a_in + b_in, tag + "in_table.grad")
        _within(tout.grad, rout.grad, (n_out[:, None] + 2) * U * a_out + b_out, tag + "out_table.grad")
        assert (tin.grad[40:] == 0).all() and (tout.grad[40:] == 0).all()
    # in_table frozen: no gradient is returned for it, out_table's is what it was
    fin, fout = _cuda(c["tin"]), _cuda(c["tout"]).requires_grad_(True)
    rows = L.sgns_loss(fin, fout, centers.cuda(), contexts.cuda(), negatives.cuda(), sw.cuda(), True, None, plans)
    (rows * up.cuda()).sum().backward()
    assert fin.grad is None and fout.grad is not None
    _within(fout.grad, rout.grad, (n_out[:, None] + 2) * U * a_out + b_out, "in_table frozen: out_table.grad")
    if planned:
        assert _bits_equal(fout.grad, tout.grad)


@pytest.mark.parametrize("V", [7, 100003])
def test_alias_sample_equals_the_restatement(V):
    from deep_recommenders_amd import ops
    rng = np.random.default_rng(V)
    weights = [1, 2, 3, 4, 0, 10, 0.5] if V == 7 else rng.random(V) ** 4
    prob, alias = ops.alias_table(weights)
    dp, da = torch.from_numpy(prob).cuda(), torch.from_numpy(alias).cuda()
    n, seed = 4099, 0x1234567890ABCDEF
    for offset in (0, n, 2 ** 33 + 5):
        got = ops.alias_sample(dp, da, n, seed, offset)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), R.alias_sample_ref(prob, alias, n, seed, offset))
    both = ops.alias_sample(dp, da, 2 * n, seed, 0)
    assert torch.equal(both, torch.cat([ops.alias_sample(dp, da, n, seed, 0), ops.alias_sample(dp, da, n, seed, n)]))
    assert int(both.min()) >= 0 and int(both.max()) < V
    if V == 7:
        assert not (both == 4).any()


def _cora_shaped(n=300, seed=0):
    """a planted-partition graph in CSR, undirected, a few nodes left without edges"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n - 5, size=600)
    b = rng.integers(0, n - 5, size=600)                        # the last 5 nodes stay isolated
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


@pytest.mark.parametrize("L", [1, 2, 40])
@pytest.mark.parametrize("graph", ["cora_shaped", "six_nodes", "dead_end"])
def test_random_walk_equals_the_restatement(graph, L):
    from deep_recommenders_amd import ops
    row_ptr, col = {"cora_shaped": _cora_shaped, "six_nodes": R.six_node_graph, "dead_end": R.dead_end_graph}[graph]()
    n = len(row_ptr) - 1
    rng = np.random.default_rng(L)
    starts = rng.integers(0, n, size=257)
    starts[3], starts[100], starts[256] = -1, n - 1, n          # a missing start, an isolated node (or a sink), one past the graph
    got = ops.random_walk(torch.from_numpy(row_ptr).cuda(), torch.from_numpy(col).cuda(), n, torch.from_numpy(starts).cuda(), L, seed=99)
    want = R.random_walk_ref(row_ptr, col, n, starts, L, seed=99)
    assert got.shape == (257, L) and np.array_equal(got.cpu().numpy(), want)
    if L > 1:
        assert (want[3, 1:] == -1).all() and (want[256, 1:] == -1).all() and (want >= 0).sum() > 257


def _two_block_pairs(rng, B, V=64):
    centers = rng.integers(0, V, size=B)
    contexts = (centers // 32) * 32 + rng.integers(0, 32, size=B)
    return torch.from_numpy(centers).cuda(), torch.from_numpy(contexts).cuda()


def _train_curve(deterministic, steps=30):
    from deep_recommenders_amd.keras.models.retrieval import SkipGram
    torch.manual_seed(0)
    m = SkipGram(64, 16, num_negatives=5, deterministic=deterministic, seed=3)
    rng = np.random.default_rng(1)
    return m, [m.train_step(*_two_block_pairs(rng, 256), lr=TOY_LR) for _ in range(steps)]


def test_skipgram_train_step_lowers_the_loss():
    m, curve = _train_curve(False)
    curve = [float(x) for x in curve]
    print("SkipGram toy: mean loss %.4f -> %.4f" % (curve[0], curve[-1]))
    assert np.isfinite(curve).all() and np.mean(curve[-5:]) < 0.9 * np.mean(curve[:5])
    assert m.draw_offset == 30 * 256 * 5
    rng = np.random.default_rng(2)
    c, o = _two_block_pairs(rng, 256)
    held_out = float(m.loss(c, o).detach())                                                          # the autograd path agrees on the level
    assert held_out < np.mean(curve[:5])


def test_same_seed_same_loss_curve_with_plans():
    m1, c1 = _train_curve(True, steps=8)
    m2, c2 = _train_curve(True, steps=8)
    assert _bits_equal(torch.stack(c1), torch.stack(c2))
    assert _bits_equal(m1.in_table.detach(), m2.in_table.detach()) and _bits_equal(m1.out_table.detach(), m2.out_table.detach())


def test_deepwalk_walk_batch():
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd import ops
    from deep_recommenders_amd.keras.models.retrieval import DeepWalk
    row_ptr, col = _cora_shaped()
    n = len(row_ptr) - 1
    idx = [(i, int(j)) for i in range(n) for j in col[row_ptr[i]:row_ptr[i + 1]]]
    torch.manual_seed(0)
    dw = DeepWalk((idx, np.ones(len(idx)), (n, n)), 16, walk_length=6, window=2, num_negatives=3, seed=5)
    assert np.array_equal(dw.adjacency.row_ptr.cpu().numpy(), row_ptr) and np.array_equal(dw.adjacency.col.cpu().numpy(), col)
    starts = torch.arange(n, dtype=torch.int64, device="cuda")
    centers, contexts = dw.walk_batch(starts)
    assert centers.shape == contexts.shape == (n * 6 * 2 * 2,)
    walks = ops.random_walk(dw.adjacency.row_ptr, dw.adjacency.col, n, starts, 6, seed=5 + 1)  # the first call's seed
    want_c, want_o = L.skipgram_pairs(walks, 2)
    assert torch.equal(centers, want_c) and torch.equal(contexts, want_o)
    assert np.array_equal(walks.cpu().numpy(), R.random_walk_ref(row_ptr, col, n, starts.cpu().numpy(), 6, seed=6))
    valid = (centers >= 0) & (contexts >= 0)
    assert int(valid.sum()) > 0 and int(centers.max()) < n and torch.equal(centers >= 0, contexts >= 0)
    edges = set(idx)
    w = walks.cpu().numpy()
    assert all((int(a), int(b)) in edges for row in w for a, b in zip(row[:-1], row[1:]) if b >= 0)
    negatives = dw.sample_negatives(centers.shape[0])
    before = float(dw.train_step(centers, contexts, 0.0, negatives))                           # lr 0: the loss of a fixed batch
    for _ in range(20):
        c, o = dw.walk_batch(starts)                                                           # every batch walks with a seed of its own
        dw.train_step(c, o, lr=DEEPWALK_LR)
    after = float(dw.train_step(centers, contexts, 0.0, negatives))
    print("DeepWalk toy: mean loss %.4f -> %.4f" % (before, after))
    assert after < 0.9 * before


def test_c_abi_domain():
    from deep_recommenders_amd import _lib
    L = _lib.lib()
    s = _lib.stream_ptr()
    p = _lib.ptr
    t = torch.zeros((8, 8), device="cuda")
    ids = torch.zeros(2, dtype=torch.int64, device="cuda")
    neg = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    out = torch.zeros(64, device="cuda")
    big = torch.zeros(256, device="cuda")
    ok = lambda **k: L.dr_sgns_fwd(p(t), p(t), k.get("D", 8), p(ids), p(ids), p(neg), k.get("B", 2), k.get("K", 3), None, k.get("flags", 1),   # noqa: E731
                                   1.0, p(out), p(out[8:]), None, k.get("dc", p(big)), k.get("ld_dc", 8), k.get("dx", p(big[64:])),
                                   k.get("ld_dx", 32), s)
    assert ok() == _lib.DR_OK and ok(B=0) == _lib.DR_OK
    for bad in (dict(D=6), dict(D=260), dict(D=0), dict(K=64), dict(K=-1), dict(B=-1), dict(flags=2), dict(ld_dc=4), dict(ld_dc=10),
                dict(ld_dx=28), dict(ld_dx=34), dict(dc=p(big) + 4), dict(dx=p(big) + 4), dict(dx=None)):
        assert ok(**bad) == _lib.DR_EINVAL, bad
    assert L.dr_sgns_fwd(p(t), p(t), 8, p(ids), p(ids), p(neg), 2, 3, None, 1, 1.0, p(out), p(out[8:]), None, None, 0, None, 0, s) == _lib.DR_OK
    assert L.dr_sgns_fwd(p(t) + 4, p(t), 8, p(ids), p(ids), p(neg), 2, 3, None, 1, 1.0, p(out), p(out[8:]), None, None, 0, None, 0, s) == _lib.DR_EINVAL
    assert L.dr_sgns_fwd(p(t), p(t), 8, p(ids), p(ids), None, 2, 0, None, 1, 1.0, p(out), p(out[8:]), None, None, 0, None, 0, s) == _lib.DR_OK
    bwd = lambda **k: L.dr_sgns_bwd(p(t), p(t), k.get("D", 8), p(ids), p(ids), p(neg), 2, k.get("K", 3), 1, p(out), p(out[8:]), k.get("dc", p(big)),   # noqa: E731
                                    k.get("ld_dc", 8), p(big[64:]), k.get("ld_dx", 32), s)
    assert bwd() == _lib.DR_OK
    for bad in (dict(D=6), dict(K=64), dict(ld_dc=4), dict(ld_dx=28), dict(dc=None), dict(dc=p(big) + 4)):
        assert bwd(**bad) == _lib.DR_EINVAL, bad
    pr, al = torch.ones(4, device="cuda"), torch.arange(4, dtype=torch.int32, device="cuda")
    o64 = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert L.dr_alias_sample(p(pr), p(al), 4, 8, 1, 0, p(o64), s) == _lib.DR_OK
    assert L.dr_alias_sample(p(pr), p(al), 0, 8, 1, 0, p(o64), s) == _lib.DR_EINVAL
    assert L.dr_alias_sample(p(pr), p(al), 2 ** 31, 8, 1, 0, p(o64), s) == _lib.DR_EINVAL
    assert L.dr_alias_sample(p(pr), None, 4, 8, 1, 0, p(o64), s) == _lib.DR_EINVAL
    rp = torch.zeros(3, dtype=torch.int64, device="cuda")
    assert L.dr_random_walk(p(rp), None, 2, p(ids), 2, 4, 1, p(o64), s) == _lib.DR_OK
    assert L.dr_random_walk(p(rp), None, 2, p(ids), 2, 0, 1, p(o64), s) == _lib.DR_EINVAL
    assert L.dr_random_walk(None, None, 2, p(ids), 2, 4, 1, p(o64), s) == _lib.DR_EINVAL
    torch.cuda.synchronize()
    assert o64.tolist() == [0, -1, -1, -1, 0, -1, -1, -1]       # a graph without edges: every walk ends at its start


# Largest |err| / bound read on an MI355X (B 257; the smaller batches are subsets in kind):
#   D 4 K 5     scores 0.340  loss_rows 0.063  coeff 0.189  d_center 0.118  d_ctx 0.220
#   D 20 K 5    scores 0.071  loss_rows 0.036  coeff 0.088  d_center 0.085  d_ctx 0.115
#   D 64 K 5    scores 0.011  loss_rows 0.010  coeff 0.024  d_center 0.024  d_ctx 0.034
#   D 100 K 5   scores 0.007  loss_rows 0.003  coeff 0.011  d_center 0.011  d_ctx 0.016
#   D 256 K 5   scores 0.002  loss_rows 0.001  coeff 0.002  d_center 0.003  d_ctx 0.004
#   D 64 K 0    scores 0.013  loss_rows 0.009  coeff 0.018  d_center 0.023  d_ctx 0.024
#   D 64 K 1    scores 0.011  loss_rows 0.010  coeff 0.024  d_center 0.038  d_ctx 0.037
#   D 64 K 63   scores 0.012  loss_rows 0.014  coeff 0.024  d_center 0.022  d_ctx 0.035
#   table update (B 40, K 5, V 50, D 64, lr 0.5): in_table 0.850 (a row one slot names: 3 u32 of it), out_table 0.536 atomic, 0.355 sorted
#   .grad through layers.sgns_loss: at most 0.024 in all four modes
#   SkipGram toy 4.1546 -> 2.2356 in 30 steps; DeepWalk toy 2.7851 -> 1.4320 in 20 batches of 300 walks
