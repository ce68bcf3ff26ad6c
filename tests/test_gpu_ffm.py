"""GPU tests of FFM on the fused field-aware interaction kernels (csrc/ffm.hip): the four entry points against the float64 restatement
(tests/ffm_ref.py), bit-reproducibility, the diagonal blocks, independence of an example from its batch, strides, the gather path
against the rows path, the autograd glue in both `sparse_lr` modes, FieldAwareInteraction and FFM end to end.

Tolerances are derived.  An fp32 sum of n products in any order, fused or not, satisfies |err| <= n u / (1 - n u) sum |a b|, u = 2^-24.
  forward       |inter - ref| <= gamma(P k) sum_{j < i, c} |A[i, j, c]| |A[j, i, c]|,  P = F (F - 1) / 2
  first order   |first_order - ref| <= gamma(F + 1) (|lin_bias| + sum_f |lin_w[row_f]|)
  backward      d_rows is one correctly rounded fp32 multiply per element: bit-equal to torch's, nothing to tolerate
  dense table gradient of a row looked up by `mult` slots: gamma(mult + 1) sum |terms| against float64 (mult - 1 adds of products
                that carry one rounding each)
  model logit   the two forward bounds plus one rounding of their sum, u |logit|."""
import functools

import numpy as np
import pytest
import torch

import ffm_ref as R

pytestmark = pytest.mark.gpu

DD = torch.float64
U = 2.0 ** -24
# (B, F, k)
SHAPES = [(3, 2, 4),         # one pair
          (2, 3, 4),         # odd F
          (4, 5, 8),
          (3, 6, 4),         # the example's
          (5, 26, 4),        # 104-float rows, not a multiple of a wave
          (2, 39, 4),
          (2, 64, 4),        # largest F, 64 KB per example
          (2, 16, 16),       # D = 256
          (2, 2, 128),       # largest k
          (3, 8, 32),
          (70, 7, 12),       # k not a multiple of 8, more examples than a block holds, remainder block
          (1, 4, 4)]
V = 5                        # rows per field of the gather cases' table


def gamma(n):
    return n * U / (1.0 - n * U)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cuda(a):
    return a.to(torch.float32).cuda()


def _diag(A, value):
    A = A.clone()
    idx = torch.arange(A.shape[1])
    A[:, idx, idx] = value
    return A


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs (float32 values held in float64) and the float64 results; computed once, never modified"""
    B, F, k = shape
    rng = np.random.default_rng(2000 + SHAPES.index(shape))
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DD)         # noqa: E731
    A, d = t(B, F, F, k), t(B)
    # the gather case: a table of V rows per field, ids with repeats inside the batch and one missing id
    table, lin_w, lin_bias = t(F * V, F * k), t(F * V), t(1)
    ids = torch.from_numpy(rng.integers(0, V, size=(B, F)))
    if B >= 2:
        ids[1, ::2] = ids[0, ::2]
    ids[0, F - 1] = -1
    row_base = torch.arange(F) * V
    Ag = R.gather(table, ids, row_base, F, k)
    w = lin_w[ids.clamp_min(0) + row_base[None, :]].abs() * (ids >= 0)
    return dict(A=A, d=d, inter=R.interaction(A), bound=gamma(F * (F - 1) // 2 * k) * R.abs_sum(A),
                table=table, lin_w=lin_w, lin_bias=lin_bias, ids=ids, row_base=row_base, Ag=Ag,
                inter_g=R.interaction(Ag), bound_g=gamma(F * (F - 1) // 2 * k) * R.abs_sum(Ag),
                first=R.first_order(lin_w, lin_bias, ids, row_base), bound_first=gamma(F + 1) * (lin_bias.abs() + w.sum(-1)))


def _within(got, want, bound, what):
    err = (got.detach().double().cpu() - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print("%s: max |err| / bound = %.3f" % (what, ratio))
    assert (err <= bound).all(), "%s: max |err| / bound = %.3f" % (what, ratio)


def _torch_bwd(A32, d32):
    """torch's fp32 d[:, None, None, None] * A.transpose(1, 2) with +0.0 on the diagonal, [B, F * F * k]"""
    want = _diag(d32[:, None, None, None] * A32.transpose(1, 2), 0.0)
    return want.reshape(A32.shape[0], -1)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward(shape):
    from deep_recommenders_amd import ops
    c = _case(shape)
    B, F, k = shape
    A = _cuda(c["A"])
    inter = ops.ffm_fwd(A, F, k)
    assert inter.shape == (B,)
    _within(inter, c["inter"], c["bound"], "forward %s" % (shape,))
    assert _bits_equal(inter, ops.ffm_fwd(A, F, k))                                           # run to run
    assert _bits_equal(inter, ops.ffm_fwd(A.reshape(B, F, F * k), F, k))
    assert _bits_equal(inter, ops.ffm_fwd(A.reshape(B, F * F * k), F, k))


@pytest.mark.parametrize("shape", SHAPES)
def test_backward(shape):
    from deep_recommenders_amd import ops
    c = _case(shape)
    B, F, k = shape
    A32, d32 = c["A"].to(torch.float32), c["d"].to(torch.float32)
    w = F * F * k
    buf = torch.full((B + 1, w + 8), -7.0, device="cuda")                                     # sentinel columns and a guard row
    d_rows = ops.ffm_bwd(A32.cuda(), F, k, d32.cuda(), d_rows=buf[:B, :w])
    assert d_rows.data_ptr() == buf.data_ptr()
    assert _bits_equal(d_rows.cpu(), _torch_bwd(A32, d32))
    idx = torch.arange(F)
    assert (d_rows.reshape(B, F, F, k)[:, idx, idx].contiguous().view(torch.int32) == 0).all()   # +0.0, bit for bit
    assert (buf[:B, w:] == -7.0).all() and (buf[B] == -7.0).all()
    assert _bits_equal(d_rows, ops.ffm_bwd(A32.cuda(), F, k, d32.cuda()))                     # a buffer of its own, run to run


@pytest.mark.parametrize("shape", SHAPES)
def test_diagonal_blocks_are_never_read(shape):
    from deep_recommenders_amd import ops
    c = _case(shape)
    B, F, k = shape
    zero, nan, d = _cuda(_diag(c["A"], 0.0)), _cuda(_diag(c["A"], float("nan"))), _cuda(c["d"])
    assert torch.isnan(nan).sum().item() == B * F * k
    inter = ops.ffm_fwd(nan, F, k)
    assert torch.isfinite(inter).all() and _bits_equal(inter, ops.ffm_fwd(zero, F, k))
    assert _bits_equal(inter, ops.ffm_fwd(_cuda(c["A"]), F, k))
    assert _bits_equal(ops.ffm_bwd(nan, F, k, d), ops.ffm_bwd(zero, F, k, d))


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] >= 2])
def test_an_example_does_not_depend_on_its_batch(shape):
    from deep_recommenders_amd import ops
    c = _case(shape)
    B, F, k = shape
    lo, hi = (5, 23) if B >= 23 else (1, B)                                                   # not aligned to a block's examples
    A, d = _cuda(c["A"]), _cuda(c["d"])
    full, gfull = ops.ffm_fwd(A, F, k), ops.ffm_bwd(A, F, k, d)
    assert _bits_equal(full[lo:hi], ops.ffm_fwd(A[lo:hi], F, k))
    assert _bits_equal(gfull[lo:hi], ops.ffm_bwd(A[lo:hi], F, k, d[lo:hi]))
    ids, rb, table = c["ids"].cuda(), c["row_base"].cuda(), _cuda(c["table"])
    gat, ggat = ops.ffm_gather_fwd(ids, rb, table, F, k)[0], ops.ffm_gather_bwd(ids, rb, table, F, k, d)
    assert _bits_equal(gat[lo:hi], ops.ffm_gather_fwd(ids[lo:hi], rb, table, F, k)[0])
    assert _bits_equal(ggat[lo:hi], ops.ffm_gather_bwd(ids[lo:hi], rb, table, F, k, d[lo:hi]))
    # NaN in one off-diagonal block of example 1 changes example 1 only
    A2 = A.clone()
    A2[1, 1, 0] = float("nan")
    got, ggot = ops.ffm_fwd(A2, F, k), ops.ffm_bwd(A2, F, k, d)
    others = [b for b in range(B) if b != 1]
    assert torch.isnan(got[1]) and _bits_equal(got[others], full[others]) and _bits_equal(ggot[others], gfull[others])
    assert torch.isnan(ggot[1].reshape(F, F, k)[0, 1]).all() and torch.isnan(ggot[1]).sum().item() == k


@pytest.mark.parametrize("shape", SHAPES)
def test_strided_rows(shape):
    from deep_recommenders_amd import ops
    c = _case(shape)
    B, F, k = shape
    w = F * F * k
    A, d = _cuda(c["A"]).reshape(B, w), _cuda(c["d"])
    buf = torch.full((B, w + 8), float("nan"), device="cuda")
    rows = buf[:, :w]
    rows.copy_(A)
    assert rows.stride(0) == w + 8
    assert _bits_equal(ops.ffm_fwd(rows, F, k), ops.ffm_fwd(A, F, k))
    assert _bits_equal(ops.ffm_bwd(rows, F, k, d), ops.ffm_bwd(A, F, k, d))


@pytest.mark.parametrize("shape", SHAPES)
def test_gather_equals_the_rows_path_on_k3s_concat(shape):
    from deep_recommenders_amd import ops
    c = _case(shape)
    B, F, k = shape
    ids, rb, table, d = c["ids"].cuda(), c["row_base"].cuda(), _cuda(c["table"]), _cuda(c["d"])
    lin_w, lin_bias = _cuda(c["lin_w"]), _cuda(c["lin_bias"])
    concat, _, _ = ops.emb_pool_fwd(ids, F, None, rb, table, want_sum_x=False, want_fm=False)
    assert concat.shape == (B, F * F * k)
    inter, first = ops.ffm_gather_fwd(ids, rb, table, F, k, lin_w, lin_bias)
    assert _bits_equal(inter, ops.ffm_fwd(concat, F, k))
    _within(inter, c["inter_g"], c["bound_g"], "gather forward %s" % (shape,))
    _within(first, c["first"], c["bound_first"], "first order %s" % (shape,))
    again = ops.ffm_gather_fwd(ids, rb, table, F, k, lin_w, lin_bias)                          # run to run
    assert _bits_equal(inter, again[0]) and _bits_equal(first, again[1])
    alone = ops.ffm_gather_fwd(ids, rb, table, F, k)                                          # without the first-order term
    assert alone[1] is None and _bits_equal(alone[0], inter)
    d_rows = ops.ffm_gather_bwd(ids, rb, table, F, k, d)
    assert _bits_equal(d_rows, ops.ffm_bwd(concat, F, k, d))
    assert _bits_equal(d_rows.cpu(), _torch_bwd(c["Ag"].to(torch.float32), c["d"].to(torch.float32)))
    # the slot with the missing id (example 0, the last field) is a row of zeros: K3 wrote zeros, and what the other rows receive from it
    # is d * 0
    assert (concat[0, (F - 1) * F * k:] == 0).all()
    assert (d_rows[0].reshape(F, F, k)[:F - 1, F - 1] == 0).all()


def _distinct_ids(F, rng, B):
    """[B, F], every field's ids all different within the batch (B <= V)"""
    return torch.from_numpy(np.stack([rng.permutation(V)[:B] for _ in range(F)], axis=1))


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[4], SHAPES[9]])
def test_dense_gradients_with_distinct_ids(shape):
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd import ops
    c = _case(shape)
    B, F, k = shape
    ids = _distinct_ids(F, np.random.default_rng(5), B).cuda()
    rb, d = c["row_base"].cuda(), _cuda(c["d"])
    table, lin_w, lin_bias = (_cuda(c[n]).requires_grad_(True) for n in ("table", "lin_w", "lin_bias"))
    inter, first = L.ffm_gather(table, lin_w, lin_bias, ids, rb, F, k, None)
    want_inter, want_first = ops.ffm_gather_fwd(ids, rb, table.detach(), F, k, lin_w.detach(), lin_bias.detach())
    assert _bits_equal(inter, want_inter) and _bits_equal(first, want_first)
    d1 = torch.flip(d, [0]).contiguous()
    g_table, g_lin, g_bias = torch.autograd.grad([inter, first], [table, lin_w, lin_bias], grad_outputs=[d, d1])
    d_rows = ops.ffm_gather_bwd(ids, rb, table.detach(), F, k, d).reshape(B, F, F * k)
    rows = (ids + rb[None, :]).reshape(-1)
    assert _bits_equal(g_table[rows], d_rows.reshape(B * F, F * k))
    untouched = torch.ones(F * V, dtype=torch.bool, device="cuda")
    untouched[rows] = False
    assert (g_table[untouched] == 0).all() and (g_lin[untouched] == 0).all()
    assert _bits_equal(g_lin[rows].reshape(B, F), d1[:, None].expand(B, F))
    _within(g_bias, c["d"].flip(0).sum().reshape(1), gamma(B) * c["d"].abs().sum().reshape(1), "bias gradient %s" % (shape,))


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4], SHAPES[10]])
def test_dense_gradients_with_repeated_ids(shape):
    from deep_recommenders_amd import layers as L
    c = _case(shape)
    B, F, k = shape
    ids, rb = c["ids"], c["row_base"]
    table = _cuda(c["table"]).requires_grad_(True)
    inter, first = L.ffm_gather(table, None, None, ids.cuda(), rb.cuda(), F, k, None)
    assert first is None
    g_table, = torch.autograd.grad(inter, [table], grad_outputs=_cuda(c["d"]))
    terms = R.interaction_backward(c["Ag"], c["d"]).reshape(B, F, F * k)                      # float64, one row per slot
    valid = (ids >= 0).reshape(-1)
    rows = (ids.clamp_min(0) + rb[None, :]).reshape(-1)[valid]
    want = torch.zeros((F * V, F * k), dtype=DD).index_add_(0, rows, terms.reshape(B * F, -1)[valid])
    mag = torch.zeros((F * V, F * k), dtype=DD).index_add_(0, rows, terms.reshape(B * F, -1)[valid].abs())
    mult = torch.zeros(F * V, dtype=DD).index_add_(0, rows, torch.ones(rows.shape[0], dtype=DD))
    assert mult.max().item() >= 2
    m = mult + 1
    _within(g_table, want, (m * U / (1 - m * U))[:, None] * mag, "table gradient, repeated ids %s" % (shape,))
    assert (g_table[(mult == 0).cuda()] == 0).all()


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[4]])
def test_fused_sgd_step_is_the_same_through_both_paths(shape):
    """one `sparse_lr` step through dr_ffm_gather_* and one through K3 + dr_ffm_* from the same state, driven by the same upstream
    gradients.  Every row is looked up by one slot here: K4 adds the slots of a shared row with atomics, whose order is not fixed, so only
    rows with one slot are reproducible bit for bit by either path."""
    from deep_recommenders_amd import layers as L
    c = _case(shape)
    B, F, k = shape
    ids = _distinct_ids(F, np.random.default_rng(6), B).cuda()
    rb, d = c["row_base"].cuda(), _cuda(c["d"])
    d1 = torch.flip(d, [0]).contiguous()
    state = lambda: [torch.nn.Parameter(_cuda(c[n])) for n in ("table", "lin_w", "lin_bias")]  # noqa: E731
    ta, wa, ba = state()
    inter, first = L.ffm_gather(ta, wa, ba, ids, rb, F, k, 0.25)
    torch.autograd.backward([inter, first], [d, d1])
    tb, wb, bb = state()
    concat, first_b, _ = L._EmbPoolFn.apply(tb, wb, bb, ids, F, None, rb, None, 0.25, False)
    inter_b = L.ffm_interaction(concat, F, k)
    assert _bits_equal(inter_b, inter)
    torch.autograd.backward([inter_b, first_b], [d, d1])
    torch.cuda.synchronize()
    assert ta.grad is None and tb.grad is None
    assert not _bits_equal(ta.detach(), _cuda(c["table"])) and not _bits_equal(wa.detach(), _cuda(c["lin_w"]))
    assert _bits_equal(ta.detach(), tb.detach()) and _bits_equal(wa.detach(), wb.detach()) and _bits_equal(ba.detach(), bb.detach())


def test_autograd_glue_of_the_rows_path_and_the_layer():
    from deep_recommenders_amd import layers as L
    from deep_recommenders_amd import ops
    from deep_recommenders_amd.keras.models.ranking import FieldAwareInteraction
    shape = SHAPES[2]
    c = _case(shape)
    B, F, k = shape
    A = _cuda(c["A"]).requires_grad_(True)
    d = _cuda(c["d"])
    inter = L.ffm_interaction(A, F, k)
    assert _bits_equal(inter, ops.ffm_fwd(A.detach(), F, k))
    g, = torch.autograd.grad(inter, [A], grad_outputs=d)
    assert g.shape == (B, F, F, k) and _bits_equal(g.reshape(B, -1), ops.ffm_bwd(A.detach(), F, k, d))
    layer = FieldAwareInteraction()
    assert _bits_equal(layer(A.detach()), inter) and _bits_equal(layer(A.detach().reshape(B, F, F * k)), inter)
    assert _bits_equal(layer.call(c["A"].to(torch.float32).numpy()), inter)


def _model_reference(model, ids):
    """float64 logits from the model's own parameters; ids [B, F, w], -1 = missing; rows are mean-pooled per field.  Returns
    (logit, bound): the two forward bounds plus one rounding of their sum"""
    F, k = model.F, model.k
    table, lin_w, lin_bias = (p.detach().double().cpu() for p in (model.slab.table, model.slab.lin_w, model.slab.lin_bias))
    base = torch.tensor([model.slab.base[key] for key in model.slab.keys])
    valid = ids >= 0
    rows = ids.clamp_min(0) + base[None, :, None]
    e = (table[rows] * valid[..., None]).sum(2) / valid.sum(2).clamp_min(1)[..., None]         # [B, F, F * k]
    A = e.reshape(ids.shape[0], F, F, k)
    w = lin_w[rows] * valid
    first = lin_bias.reshape(()) + w.sum((1, 2))
    logit = first + R.interaction(A)
    n_first = int(valid.sum((1, 2)).max().item()) + 1
    bound = gamma(F * (F - 1) // 2 * k) * R.abs_sum(A) + gamma(n_first) * (lin_bias.abs() + w.abs().sum((1, 2))) + U * logit.abs()
    return logit, bound


@pytest.mark.parametrize("multi_valued", [False, True])
def test_ffm_model(multi_valued):
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.keras.models.ranking import FFM
    torch.manual_seed(0)
    rng = np.random.default_rng(7)
    B, F, k, Vm = 33, 4, 8, 50
    cats = [fc.categorical_column_with_identity("c%d" % i, Vm) for i in range(F)]
    model = FFM([fc.indicator_column(c) for c in cats], [fc.embedding_column(c, k) for c in cats])
    with torch.no_grad():                                                                     # the linear term starts at zero: give it values
        model.slab.lin_w.normal_(0, 0.3)
        model.slab.lin_bias.fill_(0.2)
    width = 3 if multi_valued else 1
    ids = rng.integers(0, Vm, size=(B, F, width))
    if multi_valued:
        ids[:, 1, 2] = -1                                                                     # bags of 2 in field 1 ...
        ids[3, 2, :] = -1                                                                     # ... and an empty one
        ids[:, 3, 1:] = -1                                                                    # field 3 single-valued inside a wider matrix
    else:
        ids[5, 0, 0] = -1
    inputs = {"c%d" % i: ids[:, i, :] if i != 0 else ids[:, i, :1] for i in range(F)}
    ids_ref = torch.from_numpy(ids.copy())
    ids_ref[:, 0, 1:] = -1
    logits = model.logits(inputs)
    assert logits.shape == (B,)
    want, bound = _model_reference(model, ids_ref)
    _within(logits, want, bound, "FFM logits (multi-valued %s)" % multi_valued)
    labels = torch.from_numpy((rng.random(B) < 0.5).astype(np.float32)).cuda()
    from deep_recommenders_amd import losses
    loss = losses.binary_crossentropy(labels, model(inputs))
    loss.backward()
    for p in (model.slab.table, model.slab.lin_w, model.slab.lin_bias):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0
    prob = model.predict(inputs)
    assert prob.shape == (B,) and ((prob > 0) & (prob < 1)).all()
    # one fused SGD step on this path changes exactly the looked-up rows
    model.zero_grad(set_to_none=True)
    model.slab.sparse_lr = 0.1
    before = model.slab.table.detach().clone()
    losses.binary_crossentropy(labels, model(inputs)).backward()
    torch.cuda.synchronize()
    assert model.slab.table.grad is None
    changed = (model.slab.table.detach() != before).any(dim=1).cpu().numpy()
    looked_up = np.zeros(F * Vm, dtype=bool)
    r = (ids_ref + torch.arange(F)[None, :, None] * Vm)[ids_ref >= 0]
    looked_up[np.unique(r.numpy())] = True
    assert np.array_equal(changed, looked_up)


def test_fused_sgd_training_lowers_the_loss():
    """30 steps of `sparse_lr` SGD on a seeded separable task: the label is decided by the pair (c0, c1), which only the interaction sees"""
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd import losses
    from deep_recommenders_amd.keras.models.ranking import FFM
    torch.manual_seed(1)
    rng = np.random.default_rng(8)
    B, F, k, Vm = 512, 4, 4, 6
    cats = [fc.categorical_column_with_identity("c%d" % i, Vm) for i in range(F)]
    model = FFM([fc.indicator_column(c) for c in cats], [fc.embedding_column(c, k) for c in cats])
    model.slab.sparse_lr = 5.0                                                                # the loss is a mean over B examples
    ids = rng.integers(0, Vm, size=(B, F))
    inputs = {"c%d" % i: ids[:, i:i + 1] for i in range(F)}
    labels = torch.from_numpy((((ids[:, 0] < Vm // 2) ^ (ids[:, 1] < Vm // 2))).astype(np.float32)).cuda()
    history = []
    for _ in range(30):
        loss = losses.binary_crossentropy(labels, model(inputs))
        loss.backward()
        history.append(loss.item())
    print("loss: first %.4f, last %.4f" % (history[0], history[-1]))
    assert np.isfinite(history).all() and history[-1] < 0.5 * history[0]


def test_argument_errors_at_the_c_boundary_and_the_empty_batch():
    from deep_recommenders_amd import _lib, ops
    z = lambda *s: torch.zeros(s, device="cuda")                                              # noqa: E731
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64, device="cuda")                         # noqa: E731
    L, p, s = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    rows, d, out, big = z(2, 1024), z(2), z(2), z(2, 1024)
    ids, rb, table = i64(2, 64), i64(64), z(4, 256)
    assert L.dr_ffm_fwd(p(rows), 48, 2, 2, 12, p(out), s) == _lib.DR_OK
    assert L.dr_ffm_bwd(p(rows), 48, p(d), 2, 2, 12, p(big), 48, s) == _lib.DR_OK
    assert L.dr_ffm_gather_fwd(p(ids), 2, 2, p(rb), p(table), 12, None, None, p(out), None, s) == _lib.DR_OK
    assert L.dr_ffm_gather_bwd(p(ids), 2, 2, p(rb), p(table), 12, p(d), p(big), 48, s) == _lib.DR_OK
    for F, k, ld in ((2, 6, 24), (1, 8, 8), (5, 52, 1300), (2, 12, 44), (2, 12, 50), (65, 4, 16900), (2, 132, 528), (2, 0, 0)):
        assert L.dr_ffm_fwd(p(rows), ld, 2, F, k, p(out), s) == _lib.DR_EINVAL, (F, k, ld)
        assert L.dr_ffm_bwd(p(rows), ld, p(d), 2, F, k, p(big), max(ld, 4 * F * F * k), s) == _lib.DR_EINVAL, (F, k, ld)
        assert L.dr_ffm_gather_bwd(p(ids), 2, F, p(rb), p(table), k, p(d), p(big), ld, s) == _lib.DR_EINVAL, (F, k, ld)
        if ld not in (44, 50):                                                                # the gather forward has no pitch
            assert L.dr_ffm_gather_fwd(p(ids), 2, F, p(rb), p(table), k, None, None, p(out), None, s) == _lib.DR_EINVAL, (F, k)
    assert L.dr_ffm_bwd(p(rows), 48, p(d), 2, 2, 12, p(big), 44, s) == _lib.DR_EINVAL                              # ld_d < F F k
    assert L.dr_ffm_fwd(p(rows), 48, -1, 2, 12, p(out), s) == _lib.DR_EINVAL
    assert L.dr_ffm_fwd(None, 48, 2, 2, 12, p(out), s) == _lib.DR_EINVAL
    assert L.dr_ffm_fwd(p(rows) + 4, 48, 2, 2, 12, p(out), s) == _lib.DR_EINVAL                                   # not 16-byte aligned
    # B = 0: nothing launched, empty results
    assert L.dr_ffm_fwd(None, 48, 0, 2, 12, None, s) == _lib.DR_OK
    assert L.dr_ffm_gather_bwd(None, 0, 2, None, None, 12, None, None, 48, s) == _lib.DR_OK
    assert ops.ffm_fwd(z(0, 48), 2, 12).shape == (0,) and ops.ffm_bwd(z(0, 48), 2, 12, z(0)).shape == (0, 48)
    inter, first = ops.ffm_gather_fwd(i64(0, 2), i64(2), z(4, 24), 2, 12, z(4), z(1))
    assert inter.shape == (0,) and first.shape == (0,)
    assert ops.ffm_gather_bwd(i64(0, 2), i64(2), z(4, 24), 2, 12, z(0)).shape == (0, 48)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.ffm_fwd(z(2, 24), 2, 6)
