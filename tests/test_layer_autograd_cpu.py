"""What tests/test_gpu_layer_autograd.py stands on, proved without a GPU: every gradient-layout recipe delivers the strides it
states, the float64 references written for that table agree with independent formulations, the engine that drives a case
accepts a correct layer (the reference itself, run in float32 in the layer's place) in every layout and way of handing inputs over,
and the table claims every autograd Function of the package (read with `ast`, nothing imported)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_autograd_cases as C

# float64 bound of these comparisons: both sides are float64 evaluations of the same expression in another order, n terms each;
# n u64 sum|terms| with u64 = 2^-53 and n <= 64 here is below 1e-13 relative to the largest magnitude involved, which is what is asked
RTOL64 = 1e-13


def _close(a, b):
    scale = max(1.0, float(b.abs().max()))
    assert a.shape == b.shape and float((a - b).abs().max()) <= RTOL64 * scale


SHAPES = {2: [(70, 7), (1, 7), (70, 1), (1, 1)], 3: [(3, 5, 8), (1, 5, 8), (3, 1, 8), (70, 2, 1)], 1: [(70,), (1,)], 0: [()]}


@pytest.mark.parametrize("dim", [0, 1, 2, 3])
def test_every_recipe_delivers_its_strides(dim):
    for shape in SHAPES[dim]:
        for rec in C.recipes_for(dim) + ([C.TWICE] if dim else []):
            x = torch.randn(shape, requires_grad=True)
            res = C.run_layer(C.Entry("identity", None, lambda a: a["x"] * 1.0, None, ["x"], None, None), dict(x=x.detach()), "cpu", [rec])
            (seen,) = res["seen"][0]
            want = rec[4](shape) if rec[4] is not None else None
            if want is not None:
                assert C.same_layout(shape, seen["strides"], want), (rec[0], shape, seen["strides"], want)
            assert torch.equal(res["grads"]["x"], rec[3](shape, C.make_aux(shape, 0, "cpu")).contiguous()), (rec[0], shape)
            if rec[0] == "hand" and dim == 2:
                assert seen["ptr"] % 16 != 0                                     # the base is not 16-byte aligned


def test_probe_refuses_another_layout():
    x = torch.randn(5, 3, requires_grad=True)
    with pytest.raises(AssertionError, match="delivered strides"):
        C.probe(x * 1.0, (0, 1)).sum().backward()                               # .sum() delivers (0, 0)


def test_references_against_independent_formulations():
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)            # noqa: E731
    x = r(9, 7)
    _close(C.ref_softmax(x), F.softmax(x, dim=-1))
    Ws, bs = [r(7, 5), r(5, 1)], [r(5), r(1)]
    _close(C.ref_mlp(x, Ws, bs, (1, 0)), F.linear(F.relu(F.linear(x, Ws[0].t(), bs[0])), Ws[1].t(), bs[1]))
    _close(C.ref_mlp(x, Ws[:1], bs[:1], (2,)), torch.sigmoid(F.linear(x, Ws[0].t(), bs[0])))
    from oracle import torch_ref as T
    x0, W, b = r(9, 7), r(7, 7), r(7)
    _close(C.ref_cross(x0, x, W, b, 0.3), T.cross(x0, x, W, b, 0.3))
    Uw, Vw = r(7, 3), r(3, 7)
    _close(C.ref_cross_low_rank(x0, x, Uw, Vw, b, 0.3), T.cross(x0, x, Uw @ Vw, b, 0.3))
    e = r(9, 3, 4)
    _close(C.ref_fm2(e)[:, 0], T.fm_second_order(e).reshape(-1))
    F_, V, D = 3, 5, 4
    table, lin_w, bias = r(F_ * V, D), r(F_ * V), r(1)
    ids = torch.randint(0, V, (9, F_), generator=g)
    row_base = torch.arange(F_) * V
    concat, fm = C.ref_emb_pool(table, lin_w, bias, ids, row_base)
    concat_o, _, fm_o = T.emb_fm_forward(table, lin_w, float(bias), ids, list(range(F_ + 1)), row_base.tolist())
    _close(concat, concat_o.reshape(9, -1))
    _close(fm, fm_o.reshape(-1))
    _close(C.ref_lin_fields(lin_w, ids, row_base), F.embedding(ids + row_base[None, :], lin_w[:, None])[:, :, 0])
    keep = torch.rand(9, 7, generator=g) < 0.6
    got, want = C.ref_dropout(x, keep, 0.4), x * keep / 0.6
    assert float((got - want).abs().max()) <= 2 * C.U * float(want.abs().max())   # the kernel's scale is the fp32 1 / (1 - rate)
    # the references of the package-wide entries
    y = torch.eye(7, dtype=torch.float64)[torch.randint(0, 7, (9,), generator=g)]
    w = torch.rand(9, generator=g, dtype=torch.float64)
    _close(C.ref_cce_logits(x, y, w), (w * F.cross_entropy(x, y.argmax(1), reduction="none")).sum() / 9)
    _close(C.ref_cce_logits(x, y, None), F.cross_entropy(x, y.argmax(1)))
    p = x.abs() + 0.05
    _close(C.ref_cce_prob(p, y, w), (w * F.nll_loss(torch.log(p / p.sum(1, keepdim=True)), y.argmax(1), reduction="none")).sum() / 9)
    q, c = r(5, 6), r(8, 6)
    cp, ci, sw = torch.rand(8, generator=g, dtype=torch.float64) * 0.8 + 0.1, torch.randint(0, 3, (8,), generator=g), w[:5]
    eye = torch.eye(5, 8, dtype=torch.float64)
    adj = C.ref_adjust(q @ c.t(), eye, cp, ci)
    for i in range(5):
        for j in range(8):
            want_ij = float(q[i] @ c[j]) - math.log(float(cp[j])) + ((1.0 if int(ci[j]) == int(ci[i]) else 0.0) - float(eye[i, j])) * C.MIN_FLOAT
            assert abs(float(adj[i, j]) - want_ij) <= RTOL64 * max(1.0, abs(want_ij))
    # with every negative kept the hard-negative loss is the explicit softmax loss of the oracle
    _close(C.ref_hard_negative(q, c, sw, cp, ci, 0.7, 7), T.inbatch_softmax_loss(q, c, sw, cp, ci, 0.7))
    _close(C.ref_hard_negative(q, c, None, None, None, None, 7), T.inbatch_softmax_loss(q, c))
    # ... and with h of them, the softmax over the positive and the h largest negatives, picked here by sorting
    s = q @ c.t()
    rows = []
    for i in range(5):
        neg = sorted((float(s[i, j]) for j in range(8) if j != i), reverse=True)[:2]
        rows.append(math.log(sum(math.exp(v) for v in neg + [float(s[i, i])])) - float(s[i, i]))
    assert abs(float(C.ref_hard_negative(q, c, None, None, None, None, 2)) - sum(rows)) <= 1e-12 * sum(rows)
    xs, ys = r(4, 5), r(4, 5)
    _close(C._din_concat_ref(xs, ys, 1)[:, 10:], xs - ys)
    _close(C._din_concat_ref(xs, ys, 2), torch.cat([xs, ys, xs * ys], 1))
    assert C._din_concat_ref(xs, ys, 0).shape == (4, 10)


def test_hard_negative_cases_select_with_a_margin():
    """the hard-negative entries: in every row the lowest kept and the highest dropped negative are HARD_GAP forward bounds of
    scores_nt apart, so the fp32 kernels and the float64 reference keep the same columns"""
    for name in ("hard_negative_softmax", "hard_negative_softmax_all"):
        for B in C.BATCHES:
            case = C.ENTRIES[name].build(B)
            gap, bound = C.hard_negative_gap(case, case["h"])
            assert gap >= C.HARD_GAP * bound, (name, B, gap, bound)


ENGINE = ["mlp", "mlp_transposed_W", "cross_transposed_W", "softmax_rows", "dropout", "embedding_slab", "gather_cols", "din_interest_pooling_T5",
          "gru_sequence_T5", "cin_pool_act2", "l2_penalty", "dot_interaction_F3_dense", "token_embedding", "afm_pooling_with_attention", "add_layer_norm_D5", "aggregate_sparse"]
# ... and every entry of a Function outside layers.py or added to it since (those that name their Functions themselves)
ENGINE += [n for n, e in C.ENTRIES.items() if n not in ENGINE and any(k not in sum(C._CLAIMS.values(), []) for _, k in e.functions)]


@pytest.mark.parametrize("name", ENGINE)
def test_engine_accepts_the_float32_reference_in_every_layout(name):
    """the engine of the GPU file, with the entry's own reference run in float32 on the CPU in the layer's place: every recipe, the
    views of the inputs and a frozen input pass the entry's bounds (a kernel is allowed what fp32 torch needs)"""
    entry = C.ENTRIES[name]
    keep = {}

    def call(a):
        if name == "dropout":
            keep["k"] = torch.rand(a["x"].shape, generator=torch.Generator().manual_seed(3)) < 0.6
            return entry.ref(a, [keep["k"].float()])
        return entry.ref(a, None)
    fake = C.Entry(name, entry.build, call, entry.ref, entry.diff, entry.tol_out, entry.tol_grad, present=entry.present,
                   none_when_unused=entry.none_when_unused)
    for B in C.BATCHES:
        case = entry.build(B)
        outs = call(C.leaves_for(case, entry.diff, torch.float32, "cpu")[1])
        dims = [o.dim() for o in (tuple(outs) if isinstance(outs, (tuple, list)) else (outs,))]
        for rname in C.RECIPE_NAMES:
            res = C.run_layer(fake, case, "cpu", [C.recipe_named(d, rname, default="base") for d in dims], seed=B)
            C.check_against_reference(fake, case, res)
        if entry.present:
            res = C.run_layer(fake, case, "cpu", [C.recipe_named(d, "sum", default="base") for d in dims], present=entry.present, seed=B)
            C.check_against_reference(fake, case, res, present=entry.present)
        res = C.run_layer(fake, case, "cpu", [C.recipe_named(d, "base") for d in dims], frozen=(entry.diff[0],), seed=B)
        C.check_against_reference(fake, case, res)


def _layouts(shape):
    """the same values in every layout the recipes deliver, and a few more"""
    base = torch.randn(shape)
    yield "contiguous", base.clone()
    for rec in C.recipes_for(len(shape)):
        yield rec[0], rec[3](shape, C.make_aux(shape, 1, "cpu"))
    if len(shape) == 2:
        M, N = shape
        yield "pitched, aligned", torch.randn(M, C.pad4(N) + 4)[:, :N]
        yield "overlapping rows", torch.randn(M + N)[:M * 1].as_strided((M, N), (1, 1))
        yield "negative-free step 2", torch.randn(M, 2 * N)[:, ::2]


@pytest.mark.parametrize("shape", [(70, 7), (1, 7), (70, 1), (1, 1), (3, 5, 8), (1, 5, 8), (3, 1, 8), (1, 1, 4), (70,), (1,)])
@pytest.mark.parametrize("pitch4,aligned,dense", [(False, False, False), (True, True, False), (False, False, True), (False, True, True)])
def test_rows_helper_gives_rows_a_kernel_can_address(shape, pitch4, aligned, dense):
    """layers._rows, the one layout normaliser: same values; unit column stride; one pitch >= W for every row, also across the
    leading dimensions; the options hold; and a tensor that already qualifies comes back on the same memory"""
    from deep_recommenders_amd.layers import _rows
    W = shape[-1]
    for what, t in _layouts(shape):
        r = _rows(t, pitch4=pitch4, aligned=aligned, dense=dense)
        assert r.shape == t.shape and torch.equal(r, t), what
        assert r.stride(-1) == 1, what
        if r.dim() > 1:
            pitch = r.stride(-2)
            assert pitch >= W and (not pitch4 or dense or pitch % 4 == 0) and (not dense or pitch == W), (what, r.stride())
            step = pitch
            for d in range(r.dim() - 2, -1, -1):
                assert r.stride(d) == step, (what, r.stride())
                step *= r.shape[d]
        if aligned:
            assert r.data_ptr() % 16 == 0, what
        qualifies = t.is_contiguous() and t.data_ptr() % 16 == 0 and (not pitch4 or dense or W % 4 == 0 or t.numel() == W)
        if qualifies:
            assert r.data_ptr() == t.data_ptr(), "%s: a gradient that qualifies was copied" % what


def test_wrappers_refuse_a_leading_dimension_below_the_row_width():
    """a [M, N] tensor with strides (0, 1) -- what (y.sum(0) * w).sum().backward() delivers -- names the same row for every example.
    The wrappers that hand stride(0) to a kernel as the leading dimension refuse it before anything is launched (dr_gather_cols does
    not check lda itself); layers._rows never lets one through."""
    from deep_recommenders_amd import ops
    M, N = 5, 3
    bad = torch.randn(N)[None, :].expand(M, N)
    good = torch.randn(M, N)
    i32 = torch.zeros(N, dtype=torch.int32)
    ids = torch.zeros((M, N), dtype=torch.int64)
    for call in (lambda: ops.gather_cols(bad, None, i32, torch.empty(M, N)), lambda: ops.gather_cols(good, bad, i32, torch.empty(M, N)),
                 lambda: ops.dropout_fwd(bad, 0.5, 1), lambda: ops.dropout_bwd(bad, None, 0.5), lambda: ops.softmax_rows_fwd(bad),
                 lambda: ops.softmax_rows_bwd(good, bad), lambda: ops.act_fwd_(bad, 2), lambda: ops.act_bwd_(good, bad, 2),
                 lambda: ops.lin_fields_bwd(ids, N, None, None, bad, 1.0, None),
                 lambda: ops.emb_pool_bwd(ids, N, None, None, 1, bad, None, None, None, 1.0, None, None),
                 lambda: ops.softmax_rows_fwd(good.t())):
        with pytest.raises(ValueError, match="row stride >= N"):
            call()


def test_wrappers_refuse_or_copy_what_their_kernels_address_densely():
    """the wrappers whose kernels take no leading dimension: a table, a first-order vector or a destination handed over as a view, or
    with another element count than the kernel will index, is a ValueError naming the argument before anything is launched; a
    read-only operand that is merely a view is copied once"""
    from deep_recommenders_amd import ops
    n, R, D = 5, 7, 4
    rows = torch.zeros(n, dtype=torch.int64)
    table, lin, grads = torch.randn(R, D), torch.randn(R), torch.randn(n, D)
    pitched = torch.randn(R, D + 4)[:, :D]
    a = torch.randn(n, D)
    eye = torch.eye(n, R)
    for what, call in (("table", lambda: ops.rows_gather(rows, table.t().contiguous().t())), ("table", lambda: ops.rows_gather(rows, pitched)),
                       ("table", lambda: ops.rows_gather(rows, table.double())), ("lin_w", lambda: ops.rows_gather(rows, table, lin[:-1])),
                       ("lin_w", lambda: ops.rows_gather(rows, table, torch.randn(2 * R)[::2])),
                       ("out_rows", lambda: ops.rows_gather(rows, table, out_rows=torch.empty(n, D + 4)[:, :D])),
                       ("out_lin", lambda: ops.rows_gather(rows, table, lin, out_lin=torch.empty(n - 1))),
                       ("table", lambda: ops.rows_scatter_add(rows, grads, None, 1.0, pitched, None)),
                       ("grads", lambda: ops.rows_scatter_add(rows, grads[:, :3], None, 1.0, table, None)),
                       ("grads", lambda: ops.rows_scatter_add(rows, grads.double(), None, 1.0, table, None)),
                       ("lin_grads", lambda: ops.rows_scatter_add(rows, grads, torch.randn(n + 1), 1.0, table, lin)),
                       ("lin_w", lambda: ops.rows_scatter_add(rows, grads, torch.randn(n), 1.0, table, torch.randn(2 * R)[::2])),
                       ("rowdot", lambda: ops.rowdot(a, a[:-1])), ("scores_nt", lambda: ops.scores_nt(a, torch.randn(3, D + 1))),
                       ("bias", lambda: ops.cin_fwd(torch.randn(n, 2, D), torch.randn(n, 3, D), torch.randn(6, 3), torch.randn(2))),
                       ("d_out", lambda: ops.cin_bwd(torch.randn(n, 2, D), torch.randn(n, 3, D), torch.randn(6, 3), 0, torch.randn(n, 3, D),
                                                     torch.randn(n, 3, D + 1))),
                       ("out", lambda: ops.rows_scale(a, torch.ones(n), out=torch.empty(n, D + 4)[:, :D])),
                       ("d_out", lambda: ops.din_concat_bwd(a, a, 0, torch.randn(2 * D)[None, :].expand(n, 2 * D))),
                       ("d_out", lambda: ops.din_concat_bwd(a, a, 1, torch.randn(n, 2 * D))),
                       ("cce_prob_rows: p", lambda: ops.cce_prob_rows(torch.rand(D)[None, :].expand(n, D), torch.rand(n, D))),
                       ("sample_weight", lambda: ops.cce_prob_rows(torch.rand(n, D), torch.rand(n, D), torch.rand(n + 1))),
                       ("cand_prob", lambda: ops.logits_adjust(eye, eye, cand_prob=torch.rand(R - 1))),
                       ("cand_ids", lambda: ops.logits_adjust(eye, eye, cand_ids=torch.zeros(R, dtype=torch.int32))),
                       ("labels", lambda: ops.logits_adjust(eye, eye[:, :-1])),
                       ("labels", lambda: ops.softmax_ce_rows(eye, eye[:-1])),
                       ("sample_weight", lambda: ops.softmax_ce_rows(eye, eye, 1.0, torch.rand(n + 1))),
                       ("cols", lambda: ops.softmax_ce_rows_bwd(eye, eye, 1.0, None, 1.0, cols=torch.zeros(n, R - 1, dtype=torch.int64),
                                                                out=torch.zeros(n, R))),
                       ("out", lambda: ops.softmax_ce_rows_bwd(eye, eye, 1.0, None, 1.0, out=torch.zeros(R, n).t())),
                       ("labels", lambda: ops.bce_fwd_bwd(torch.randn(n), torch.rand(n + 1))),
                       ("labels", lambda: ops.bce_prob_fwd_bwd(torch.rand(n), torch.rand(n - 1), 1)),
                       ("dy", lambda: ops.sigmoid_bwd(torch.rand(n), torch.rand(n + 1))),
                       ("scores", lambda: ops.topk_select(torch.randn(R)[None, :].expand(n, R), 2)),
                       ("take_along_rows", lambda: ops.take_along_rows(torch.randn(R)[None, :].expand(n, R), torch.zeros(n, 2, dtype=torch.int64))),
                       ("sample_weight", lambda: ops.inbatch_softmax_fwd(a, a, sample_weight=torch.rand(n + 1))),
                       ("candidate_ids", lambda: ops.inbatch_softmax_fwd(a, a, cand_ids=torch.zeros(n, dtype=torch.int32))),
                       ("x", lambda: ops.reduce_sum(torch.zeros(3, dtype=torch.float64)))):
        with pytest.raises(ValueError, match=what):
            call()
    t = torch.randn(D, n).t()
    got = ops._dense_arg(t, "t", shape=(n, D))
    assert got.is_contiguous() and torch.equal(got, t) and ops._dense_arg(a, "a") is a and ops._dense_arg(None, "none") is None
    with pytest.raises(ValueError, match="t must be contiguous"):
        ops._dense_arg(t, "t", copy=False)


def test_recipe_named_refuses_a_name_the_rank_does_not_have():
    assert C.recipe_named(3, "sum0", default="base")[0] == "base"
    with pytest.raises(KeyError):
        C.recipe_named(3, "sum0")


def test_rows_helper_refuses_another_dtype():
    from deep_recommenders_amd.layers import _rows
    with pytest.raises(TypeError, match="fp32"):
        _rows(torch.zeros(3, 4, dtype=torch.float64))


# A Function that cannot be put in the table: (module, class name) -> the reason.  Empty, and expected to stay so.
NOT_IN_THE_TABLE = {}


def test_every_autograd_function_of_the_package_is_claimed_by_an_entry():
    """every class under deep_recommenders_amd/ whose bases name torch.autograd.Function is run by at least one entry of the table, and
    no entry names a class that is not there"""
    found = set(C.package_functions())
    assert len(found) >= 48, "the scan found %d Functions, fewer than the 48 of the day this test was written: %s" % (len(found), sorted(found))
    claimed = {f for e in C.ENTRIES.values() for f in e.functions}
    assert all(e.functions for e in C.ENTRIES.values()), "entries that name no Function: %s" % [n for n, e in C.ENTRIES.items() if not e.functions]
    orphans = sorted(found - claimed - set(NOT_IN_THE_TABLE))
    assert not orphans, "autograd Functions no entry of tests/layer_autograd_cases.py runs: %s" % orphans
    gone = sorted((claimed | set(NOT_IN_THE_TABLE)) - found)
    assert not gone, "entries (or NOT_IN_THE_TABLE) name Functions the package does not have: %s" % gone
    assert all(isinstance(r, str) and r for r in NOT_IN_THE_TABLE.values())


def test_package_functions_reads_every_way_of_naming_the_base(tmp_path):
    pkg = tmp_path / "pkg" / "sub"
    pkg.mkdir(parents=True)
    (pkg / "m.py").write_text("import torch\nfrom torch.autograd import Function\nclass A(torch.autograd.Function): pass\n"
                              "class B(Function): pass\nclass C(object): pass\n")
    (tmp_path / "pkg" / "__init__.py").write_text("from torch import autograd\nclass D(autograd.Function): pass\n")
    got = C.package_functions(str(tmp_path / "pkg"))
    assert sorted(got) == [(C.PKG, "D"), (C.PKG + ".sub.m", "A"), (C.PKG + ".sub.m", "B")]
