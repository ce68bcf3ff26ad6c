"""What tests/test_gpu_layer_autograd.py and tests/test_layer_autograd_cpu.py share: the pass-through probe, the gradient-layout
recipes, the table of layers (inputs, call, float64 reference, tolerances) and the small engine that drives one case.  Imports
without a GPU: the layer under test is only imported inside an entry's `call`.

A case runs the same computation twice.  The reference side builds float64 leaves on the CPU, calls the entry's `ref` (plain torch
operations) and lets torch's autograd differentiate sum_k <out_k, G_k>; the same on float32 leaves is the yardstick some bounds use.
The device side builds fp32 leaves, calls the layer, puts the probe directly after every output and drives the backward through a
recipe's downstream graph, which delivers the same gradient VALUES G_k in another memory layout.

Strides of a dimension of size 1 carry no meaning (torch leaves them arbitrary); the probe compares the others."""
import math

import numpy as np
import torch

U = 2.0 ** -24


def gamma(n):
    """n roundings: n u / (1 - n u) (tests/test_gpu_ffm.py, tests/test_gpu_helper_kernels.py)"""
    return n * U / (1.0 - n * U)


def pad4(n):
    return (n + 3) // 4 * 4


# --------------------------------------------------------------------------------------------------------------------------------------
# the probe
# --------------------------------------------------------------------------------------------------------------------------------------
def same_layout(shape, got, want):
    return all(n <= 1 or g == w for n, g, w in zip(shape, got, want))


class _Probe(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, expect, seen):
        ctx.expect, ctx.seen = expect, seen
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        if ctx.expect is not None:
            assert same_layout(g.shape, g.stride(), ctx.expect), "the recipe delivered strides %s for shape %s, not %s" % (
                tuple(g.stride()), tuple(g.shape), tuple(ctx.expect))
        if ctx.seen is not None:
            ctx.seen.append(dict(strides=tuple(g.stride()), dtype=g.dtype, ptr=g.data_ptr(), grad=g, before=g.clone()))
        return g, None, None


def probe(y, expect=None, seen=None):
    """y, unchanged; its backward returns the gradient OBJECT it received and asserts that it arrived with the strides `expect`"""
    return _Probe.apply(y, expect, seen)


# --------------------------------------------------------------------------------------------------------------------------------------
# gradient-layout recipes, per number of dimensions of the output.  A recipe is (name, kind, fn, values, strides):
#   kind "graph"         fn(y, aux) is the scalar loss of a downstream graph of the probed output y
#   kind "hand"          fn(aux, shape) is a gradient tensor built by hand for torch.autograd.backward(y, grad_tensors=...)
#   values(shape, aux)   the fp32 gradient values that arrive
#   strides(shape)       the strides they arrive with (observed with CPU torch; asserted by the probe on every run, on the device too)
# make_aux(shape, seed, device) draws the random weights once per output.
# --------------------------------------------------------------------------------------------------------------------------------------
def make_aux(shape, seed, device):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(shape, generator=g)
    aux = dict(r=r)
    if len(shape) == 2:
        M, N = shape
        aux.update(w=torch.randn(N, generator=g), v=torch.randn(M, generator=g), rT=r.t().contiguous(),
                   wide=torch.randn(M * (N + 3) + 1, generator=g))
    elif len(shape) == 3:
        B, L, W = shape
        aux.update(w=torch.randn(B, W, generator=g), rT=r.transpose(0, 1).contiguous(), wide=torch.randn(B * L * (W + 3) + 1, generator=g),
                   big=torch.randn(B, L, W, generator=g))
    elif len(shape) == 1:
        aux.update(wide=torch.randn(2 * shape[0] + 1, generator=g))
    aux["r2"] = torch.randn(shape, generator=g)
    return {k: t.to(device) for k, t in aux.items()}


def _hand2(aux, shape):
    M, N = shape
    return aux["wide"][1:1 + M * (N + 3)].view(M, N + 3)[:, :N]            # pitch N + 3, base 4 bytes past a 16-byte boundary


def _hand3(aux, shape):
    B, L, W = shape
    return aux["wide"][1:1 + B * L * (W + 3)].view(B, L, W + 3)[:, :, :W]


_ONES = lambda s, a: torch.ones(s, device=a["r"].device)      # noqa: E731
# (name, kind, fn, values, strides): kind "graph": fn(y, aux) is the scalar loss of the downstream graph; kind "hand": fn(aux, shape) is
# the gradient tensor handed to torch.autograd.backward(y, grad_tensors=...)
RECIPES = {
    2: [("base", "graph", lambda y, a: (y * a["r"]).sum(), lambda s, a: a["r"], lambda s: (s[1], 1)),
        ("sum", "graph", lambda y, a: y.sum(), _ONES, lambda s: (0, 0)),
        ("sum0", "graph", lambda y, a: (y.sum(0) * a["w"]).sum(), lambda s, a: a["w"][None, :].expand(s), lambda s: (0, 1)),
        ("sum1", "graph", lambda y, a: (y.sum(1) * a["v"]).sum(), lambda s, a: a["v"][:, None].expand(s), lambda s: (1, 0)),
        # the factor is a CONTIGUOUS [N, M] tensor: with r.t() (strides (1, N)) autograd hands back a row-major gradient
        ("t", "graph", lambda y, a: (y.t().contiguous() * a["rT"]).sum(), lambda s, a: a["rT"].t(), lambda s: (1, s[0])),
        ("hand", "hand", _hand2, lambda s, a: _hand2(a, s), lambda s: (s[1] + 3, 1))],
    3: [("base", "graph", lambda y, a: (y * a["r"]).sum(), lambda s, a: a["r"], lambda s: (s[1] * s[2], s[2], 1)),
        ("sum", "graph", lambda y, a: y.sum(), _ONES, lambda s: (0, 0, 0)),
        # y.sum(1) times a weight: torch expands the [B, W] product's gradient, so the examples lie W apart, not L * W
        ("sum1", "graph", lambda y, a: (y.sum(1) * a["w"]).sum(), lambda s, a: a["w"][:, None, :].expand(s), lambda s: (s[2], 0, 1)),
        # the same broadcast over the steps at the pitch of a whole example: the expanded row 0 of a [B, L, W] tensor, by hand
        ("row0", "hand", lambda a, s: a["big"][:, :1, :].expand(s), lambda s, a: a["big"][:, :1, :].expand(s), lambda s: (s[1] * s[2], 0, 1)),
        ("t", "graph", lambda y, a: (y.transpose(0, 1).contiguous() * a["rT"]).sum(), lambda s, a: a["rT"].transpose(0, 1),
         lambda s: (s[2], s[0] * s[2], 1)),
        ("hand", "hand", _hand3, lambda s, a: _hand3(a, s), lambda s: (s[1] * (s[2] + 3), s[2] + 3, 1))],
    1: [("base", "graph", lambda y, a: (y * a["r"]).sum(), lambda s, a: a["r"], lambda s: (1,)),
        ("sum", "graph", lambda y, a: y.sum(), _ONES, lambda s: (0,)),
        ("hand", "hand", lambda a, s: a["wide"][1:1 + 2 * s[0]:2], lambda s, a: a["wide"][1:1 + 2 * s[0]:2], lambda s: (2,))],
    0: [("base", "graph", lambda y, a: y * a["r"], lambda s, a: a["r"], lambda s: ())],
}
# consumed twice: autograd adds the two gradients (one fp32 addition per element) before the layer sees them
TWICE = ("twice", "graph", lambda y, a: (y * a["r"]).sum() + (y * a["r2"]).sum(), lambda s, a: a["r"] + a["r2"], None)
RECIPE_NAMES = ("base", "sum", "sum0", "sum1", "row0", "t", "hand")


def materialised(recipe):
    """the same gradient values as `recipe` delivers, contiguous in a fresh tensor: the baseline of the bit-equality checks"""
    return (recipe[0] + "/dense", "hand", lambda a, s, v=recipe[3]: v(s, a).contiguous().clone(), recipe[3], lambda s: None)


def recipe_named(dim, name, default=None):
    """the recipe `name` for a `dim`-dimensional output.  Where the outputs of one layer differ in rank a layout may not exist for all
    of them: `default` names the recipe the others take then; without it an unknown name is an error, never silently the baseline."""
    for r in RECIPES[dim]:
        if r[0] == name:
            return r
    if default is None:
        raise KeyError("no recipe %r for a %d-dimensional output" % (name, dim))
    return recipe_named(dim, default)


def recipes_for(dim):
    return RECIPES[dim]


# --------------------------------------------------------------------------------------------------------------------------------------
# how an input is handed over.  make(value) -> the leaf that requires grad; show(leaf) -> what the layer receives
# --------------------------------------------------------------------------------------------------------------------------------------
def _pitched_make(v):
    buf = torch.zeros(tuple(v.shape[:-1]) + (pad4(v.shape[-1]) + 4,), dtype=v.dtype, device=v.device)
    buf[..., :v.shape[-1]] = v
    return buf


PRESENT = {
    "plain": (lambda v: v.clone(), lambda leaf, v: leaf),
    # a column slice of a padded buffer (pitch a multiple of 4, base aligned: what EmbeddingSlab's ld_concat produces)
    "pitched": (_pitched_make, lambda leaf, v: leaf[..., :v.shape[-1]]),
    # a weight kept transposed
    "transposed": (lambda v: v.t().contiguous(), lambda leaf, v: leaf.t()),
    # a bias that is one number, expanded (the case's value is replaced by its first element)
    "expanded": (lambda v: v.reshape(-1)[:1].clone(), lambda leaf, v: leaf.expand(v.shape)),
}


# --------------------------------------------------------------------------------------------------------------------------------------
# tolerances: functions (want64, want32) -> a bound broadcastable to want64.  Each names the test file its formula is from.
# --------------------------------------------------------------------------------------------------------------------------------------
def tol_yard(c, floor):
    """max(c * yardstick, floor) * max|ref|, the yardstick being the float32 run of the same reference against float64"""
    def f(w64, w32, ctx=None):
        scale = w64.abs().max().item() if w64.numel() else 0.0
        yard = (w32.double() - w64).abs().max().item() / scale if scale > 0 else 0.0
        return torch.full_like(w64, max(c * yard, floor) * scale)
    return f


def tol_allclose(rtol, atol_of_max, plus=0.0, atol=0.0):
    """numpy.testing.assert_allclose's atol + rtol |ref| with atol = atol_of_max * (max|ref| + plus) + atol"""
    def f(w64, w32, ctx=None):
        m = w64.abs().max().item() if w64.numel() else 0.0
        return atol + atol_of_max * (m + plus) + rtol * w64.abs()
    return f


def tol_rel(c):
    return lambda w64, w32, ctx=None: c * w64.abs()


def tol_abs(c):
    """c times what the reference gives on the absolute values of its inputs (and of the incoming gradient): the sum of the
    magnitudes of the terms, for a reference that is a polynomial with non-negative coefficients"""
    return lambda w64, w32, ctx: c * ctx["abs"]


TOL_DIN = tol_yard(8.0, 2e-6)                      # tests/test_gpu_din.py::_check: max(8 yard, 2e-6) max|ref|
TOL_FP32_16 = tol_yard(16.0, 16 * 8 * U)          #  16 max(r32, 8u) max|ref|: test_gpu_afm / pnn / dien


class Entry:
    """one row of the table"""

    def __init__(self, name, build, call, ref, diff, tol_out, tol_grad, bit_equal=True, present=None, spy=None, functions=(),
                 none_when_unused=False):
        self.name, self.build, self.call, self.ref = name, build, call, ref
        self.functions = tuple(functions)             # (module, class name) of the autograd Functions this entry runs
        # True: an input no USED output depends on gets no gradient at all on the device (the multi-task Functions return None for
        # the parameters of a task nobody consumed); the reference's gradient there must be exactly zero
        self.none_when_unused = none_when_unused
        self.diff = diff                              # names of the differentiable inputs
        self.tol_out, self.tol_grad = tol_out, tol_grad
        self.bit_equal = bit_equal                    # False: the backward combines with fp32 atomics
        self.present = present or {}                  # input name -> another way of handing it over ("pitched", ...)
        self.spy = spy                                # (ops function name, argument index): that argument IS the incoming gradient


def leaves_for(case, diff, dtype, device, present=None, frozen=()):
    present = present or {}
    leaves, shown = {}, {}
    for k, v in case.items():
        if not (isinstance(v, torch.Tensor) and v.is_floating_point()):
            shown[k] = v.to(device) if isinstance(v, torch.Tensor) else v
            continue
        make, show = PRESENT[present.get(k, "plain")]
        val = v.to(device=device, dtype=dtype)
        leaf = make(val)
        if k in diff and k not in frozen:
            leaf.requires_grad_(True)
        leaves[k] = leaf
        shown[k] = show(leaf, val)
    return leaves, shown


def reference(entry, case, Gs, dtype, present=None, got_outs=None):
    """(outputs, {name: gradient}) of the entry's float reference on the CPU for the output gradients Gs (None: output unused)"""
    leaves, shown = leaves_for(case, entry.diff, dtype, "cpu", present)
    outs = entry.ref(shown, got_outs)
    outs = tuple(outs) if isinstance(outs, (tuple, list)) else (outs,)
    loss = 0
    for k, (o, G) in enumerate(zip(outs, Gs)):
        if G is not None and o is not None and o.requires_grad:
            loss = loss + (o * G.detach().to("cpu", dtype)).sum()
    names = [k for k in entry.diff if case.get(k) is not None]
    grads = {}
    if isinstance(loss, torch.Tensor):
        gs = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
        grads = {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(names, gs)}
    return tuple(None if o is None else o.detach() for o in outs), grads


# --------------------------------------------------------------------------------------------------------------------------------------
# float64 references written for this table (the others are tests/*_ref.py); checked against independent formulations by
# tests/test_layer_autograd_cpu.py
# --------------------------------------------------------------------------------------------------------------------------------------
ACT = {0: (lambda v: v), 1: torch.relu, 2: torch.sigmoid, 3: torch.tanh}


def ref_fm2(x):
    """0.5 sum_d ((sum_f x)^2 - sum_f x^2) -> [B, 1]"""
    return 0.5 * (x.sum(1) ** 2 - (x ** 2).sum(1)).sum(1, keepdim=True)


def ref_mlp(x, Ws, bs, acts):
    for W, b, a in zip(Ws, bs, acts):
        x = x @ W
        x = ACT[a](x if b is None else x + b)
    return x


def ref_cross(x0, x, W, b, diag):
    prod = x @ W + diag * x
    return x0 * (prod if b is None else prod + b) + x


def ref_cross_low_rank(x0, x, Uw, Vw, b, diag):
    prod = (x @ Uw) @ Vw + diag * x
    return x0 * (prod if b is None else prod + b) + x


def ref_dropout(x, keep, rate):
    """tf.nn.dropout with the kept set given: x * fp32(1 / (1 - rate)) where kept"""
    scale = float(np.float32(1) / (np.float32(1) - np.float32(rate)))
    return torch.where(keep, x * scale, torch.zeros_like(x))


def ref_softmax(x):
    e = torch.exp(x - x.max(dim=-1, keepdim=True).values)
    return e / e.sum(dim=-1, keepdim=True)


def ref_emb_pool(table, lin_w, lin_bias, ids, row_base, second_order=True):
    """single-valued fields: concat [B, F * D], fm logit [B] = bias + sum_f lin_w[row] + 0.5 sum_d ((sum_f e)^2 - sum_f e^2); an id < 0
    is a missing value (a zero row)"""
    rows = ids.clamp_min(0) + row_base[None, :]
    ok = (ids >= 0)
    e = torch.where(ok[:, :, None], table[rows], torch.zeros((), dtype=table.dtype))
    fm = torch.where(ok, lin_w[rows], torch.zeros((), dtype=table.dtype)).sum(1) + lin_bias.reshape(())
    if second_order:
        fm = fm + ref_fm2(e)[:, 0]
    return e.reshape(ids.shape[0], -1), fm


def ref_lin_fields(lin_w, ids, row_base):
    rows = ids.clamp_min(0) + row_base[None, :]
    return torch.where(ids >= 0, lin_w[rows], torch.zeros((), dtype=lin_w.dtype))


# --------------------------------------------------------------------------------------------------------------------------------------
# the table
# --------------------------------------------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape):
    return torch.randn(*shape, generator=g)


def _L():
    from deep_recommenders_amd import layers
    return layers


BATCHES = (1, 70)            # batch 1, and one that is neither a multiple of 4 nor of a 64-lane wave


# ---- GEMM layers: tests/test_gpu_kernels.py::test_linear_fwd_bwd gives, per GEMM with reduction length R, atol c sqrt(R) (max|ref| + 1)
# with c = 2e-6 (forward, dx) or 4e-6 (dW), and 1e-5 sqrt(M) 4 for a bias gradient.  A layer made of n GEMMs in a chain gets the sum
# of its parts' bounds: the weights here are scaled by 1 / sqrt(K), so a later stage passes an earlier stage's error on with a gain
# of about one, and each part's term is evaluated at the final quantity's magnitude.
def tol_gemm(c, R, n=1):
    return tol_allclose(0.0, n * c * math.sqrt(R), plus=1.0)


def _mlp_build(B, widths, acts, seed):
    g = _g(seed)
    case = dict(x=_rn(g, B, widths[0]), acts=tuple(acts))
    for i in range(len(widths) - 1):
        case["W%d" % i] = _rn(g, widths[i], widths[i + 1]) / math.sqrt(widths[i])
        case["b%d" % i] = _rn(g, widths[i + 1]) * 0.3
    return case


def _mlp_parts(a):
    n = len(a["acts"])
    return [a["W%d" % i] for i in range(n)], [a["b%d" % i] for i in range(n)]


def _mlp_entry(name, widths, acts, present=None):
    n = len(acts)
    diff = ["x"] + ["W%d" % i for i in range(n)] + ["b%d" % i for i in range(n)]

    def tol_grad(case):
        M = case["x"].shape[0]
        t = {"x": tol_gemm(2e-6, max(widths), n)}
        for i in range(n):
            t["W%d" % i] = tol_gemm(4e-6, M, n - i)
            t["b%d" % i] = tol_allclose(0.0, 0.0, atol=(n - i) * 1e-5 * math.sqrt(M) * 4)
        return t
    return Entry(name, lambda B: _mlp_build(B, widths, acts, 11), lambda a: _L().mlp(a["x"], *_mlp_parts(a), a["acts"]),
                 lambda a, _: ref_mlp(a["x"], *_mlp_parts(a), a["acts"]), diff,
                 lambda case: [tol_gemm(2e-6, max(widths), n)], tol_grad, bit_equal=False, present=present,
                 spy=("linear_bwd_dw", 1) if acts[-1] == 0 else None)


def _cross_build(B, D, seed, low_rank=0):
    g = _g(seed)
    case = dict(x0=_rn(g, B, D), x=_rn(g, B, D), b=_rn(g, D) * 0.3, diag=0.3)
    if low_rank:
        case.update(U=_rn(g, D, low_rank) / math.sqrt(D), V=_rn(g, low_rank, D) / math.sqrt(low_rank))
    else:
        case.update(W=_rn(g, D, D) / math.sqrt(D))
    return case


def _cross_tol_grad(D, n):
    # the combine is elementwise (a few roundings, inside test_cross_known_answer_and_random's rtol = atol = 1e-5); the GEMMs as above
    def f(case):
        M = case["x"].shape[0]
        t = {k: tol_allclose(1e-5, n * 2e-6 * math.sqrt(D), plus=1.0, atol=1e-5) for k in ("x0", "x")}
        t.update({k: tol_gemm(4e-6, M, n) for k in ("W", "U", "V")})
        t["b"] = tol_allclose(0.0, 0.0, atol=n * 1e-5 * math.sqrt(M) * 4)
        return t
    return f


def _slab_build(B, F, D, V, seed):
    g = _g(seed)
    ids = torch.randint(0, V, (B, F), generator=g)
    if B > 1:
        ids[1] = ids[0]                                # a repeated row: two examples add into the same table rows
        ids[2, 0] = -1                                 # a missing value
    return dict(table=_rn(g, F * V, D) * 0.5, lin_w=_rn(g, F * V), lin_bias=_rn(g, 1), ids=ids, row_base=torch.arange(F) * V, F=F, V=V, D=D)


def _slab(a, with_linear=True):
    """an EmbeddingSlab whose parameters ARE the case's leaves (sparse_lr None: the gradients materialise)"""
    from deep_recommenders_amd import feature_column as fc
    L = _L()
    cats = [fc.categorical_column_with_identity("f%d" % f, a["V"]) for f in range(a["F"])]
    slab = L.EmbeddingSlab([fc.embedding_column(c, a["D"]) for c in cats], [fc.indicator_column(c) for c in cats] if with_linear else None,
                           device=a["table"].device)
    for k in ("table", "lin_w", "lin_bias"):
        delattr(slab, k)
        setattr(slab, k, a.get(k))
    feats = {"f%d" % f: a["ids"][:, f] for f in range(a["F"])}
    return slab, feats, ["f%d" % f for f in range(a["F"])]


def _slab_call(a):
    slab, feats, keys = _slab(a)
    concat, fm, _ = slab(feats, keys)
    return concat, fm


def _linf_call(a):
    slab, feats, keys = _slab(a)
    return slab.first_order_fields(feats, keys)


def _gather_build(B, seed):
    g = _g(seed)
    return dict(num=_rn(g, B, 3), emb=_rn(g, B, 8), col_map=torch.tensor([0, -1, -2, 1, -3, -4, -5, -6, 2, -7, -8], dtype=torch.int32),
                emb_map=torch.tensor([1, 2, 4, 5, 6, 7, 9, 10], dtype=torch.int32))


def _di_build(B, F, D, dense, seed):
    g = _g(seed)
    return dict(dense=_rn(g, B, D) if dense else None, emb=_rn(g, B, F, D))


def _afm_build(B, F, D, A, seed):
    g = _g(seed)
    return dict(emb=_rn(g, B, F, D), W=_rn(g, D, A) / math.sqrt(D), b=_rn(g, A) * 0.3, h=_rn(g, A) / math.sqrt(A))


def _pnn_build(B, F, D, N, seed):
    g = _g(seed)
    return dict(emb=_rn(g, B, F, D) * 0.5, W=_rn(g, D * D, N) / D, addend=_rn(g, B, N))


def _afm_ref(a, _):
    import afm_ref as R
    return R.forward(a["emb"], a["W"], a["b"], a["h"])["out"]


def _pnn_ref(a, _):
    import pnn_ref as R
    return R.forward(a["emb"], a["W"], a["addend"])["out"]


def _di_ref(a, _):
    import dlrm_ref as R
    return R.dot_interaction(a["dense"], a["emb"])


ENTRIES = {}


def _add(e):
    ENTRIES[e.name] = e


_add(Entry("fm_second_order", lambda B: dict(x=_rn(_g(1), B, 3, 4)), lambda a: _L().fm_second_order(a["x"]), lambda a, _: ref_fm2(a["x"]),
           ["x"],
           lambda case: [tol_allclose(0.0, 1e-5)],                                 # tests/test_gpu_kernels.py::test_fm2_fwd_bwd
           lambda case: {"x": tol_allclose(1e-5, 0.0, atol=1e-5)}))
_add(_mlp_entry("mlp", (7, 5, 1), (1, 0)))                                           # relu below the top (folded into dx), one unit on top
_add(_mlp_entry("mlp_sigmoid_top", (6, 3), (2,)))                                    # act_bwd_ works in place on a clone of dy
_add(_mlp_entry("mlp_transposed_W", (7, 5, 1), (1, 0), present={"W0": "transposed", "W1": "transposed", "x": "pitched", "b0": "expanded"}))
_add(Entry("cross", lambda B: _cross_build(B, 7, 2), lambda a: _L().cross(a["x0"], a["x"], a["W"], a["b"], a["diag"]),
           lambda a, _: ref_cross(a["x0"], a["x"], a["W"], a["b"], a["diag"]), ["x0", "x", "W", "b"],
           lambda case: [tol_allclose(1e-5, 0.0, atol=1e-5)],                      # tests/test_gpu_kernels.py::test_cross_known_answer_and_random
           _cross_tol_grad(7, 2), bit_equal=False))
_add(Entry("cross_transposed_W", lambda B: _cross_build(B, 7, 2), lambda a: _L().cross(a["x0"], a["x"], a["W"], a["b"], a["diag"]),
           lambda a, _: ref_cross(a["x0"], a["x"], a["W"], a["b"], a["diag"]), ["x0", "x", "W", "b"],
           lambda case: [tol_allclose(1e-5, 0.0, atol=1e-5)], _cross_tol_grad(7, 2), bit_equal=False,
           present={"W": "transposed", "b": "expanded", "x0": "pitched"}))
_add(Entry("cross_low_rank", lambda B: _cross_build(B, 7, 3, low_rank=3),
           lambda a: _L().cross_low_rank(a["x0"], a["x"], a["U"], a["V"], a["b"], a["diag"]),
           lambda a, _: ref_cross_low_rank(a["x0"], a["x"], a["U"], a["V"], a["b"], a["diag"]), ["x0", "x", "U", "V", "b"],
           lambda case: [tol_allclose(2e-5, 0.0, atol=2e-5)],                      # two GEMMs and the combine: twice test_cross's
           _cross_tol_grad(7, 3), bit_equal=False))
_add(Entry("cross_low_rank_transposed", lambda B: _cross_build(B, 7, 3, low_rank=3),
           lambda a: _L().cross_low_rank(a["x0"], a["x"], a["U"], a["V"], a["b"], a["diag"]),
           lambda a, _: ref_cross_low_rank(a["x0"], a["x"], a["U"], a["V"], a["b"], a["diag"]), ["x0", "x", "U", "V", "b"],
           lambda case: [tol_allclose(2e-5, 0.0, atol=2e-5)], _cross_tol_grad(7, 3), bit_equal=False,
           present={"U": "transposed", "V": "transposed"}))
# dropout: y = x * fp32(1 / (1 - rate)) where kept, bit for bit (tests/test_gpu_small_kernels.py::test_dropout); against the float64
# product that is one rounding, u |ref|.  The kept set is read off the forward's output (x has no zeros).
_add(Entry("dropout", lambda B: dict(x=_rn(_g(4), B, 7).abs() + 0.1, rate=0.4, seed=77),
           lambda a: _L().dropout(a["x"], a["rate"], a["seed"]),
           lambda a, got: ref_dropout(a["x"], got[0].cpu() != 0, a["rate"]), ["x"],
           lambda case: [tol_rel(U)], lambda case: {"x": tol_rel(U)}, spy=("dropout_bwd", 0), present={"x": "pitched"}))
_add(Entry("tied_projection", lambda B: dict(x=_rn(_g(5), B, 6), table=_rn(_g(6), 9, 6) / math.sqrt(6)),
           lambda a: _L().tied_projection(a["x"], a["table"]), lambda a, _: a["x"] @ a["table"].t(), ["x", "table"],
           # tests/test_gpu_helper_kernels.py::test_scores_nt_direct's 4 sqrt(D) u (|a| |b|^T) is at most this scalar form of it
           lambda case: [tol_gemm(2e-6, 6)],
           lambda case: {"x": tol_gemm(2e-6, 9), "table": tol_gemm(4e-6, case["x"].shape[0])}, spy=("linear_fwd", 0)))
_add(Entry("tied_projection_transposed", lambda B: dict(x=_rn(_g(5), B, 6), table=_rn(_g(6), 9, 6) / math.sqrt(6)),
           lambda a: _L().tied_projection(a["x"], a["table"]), lambda a, _: a["x"] @ a["table"].t(), ["x", "table"],
           lambda case: [tol_gemm(2e-6, 6)],
           lambda case: {"x": tol_gemm(2e-6, 9), "table": tol_gemm(4e-6, case["x"].shape[0])}, present={"table": "transposed", "x": "pitched"}))
# tests/test_gpu_kernels.py::test_emb_pool_fwd_matches_oracle / test_emb_pool_bwd_matches_autograd_oracle: fm atol 2e-5 max|ref|, the
# concat is a copy (exact); g_table rtol 1e-4, atol 1e-5 (max|ref| + 1); g_lin rtol 1e-4, atol 1e-5; the bias gradient is a sum of B
# terms like a Dense bias gradient (1e-5 sqrt(B) 4).  No plan: the rows are combined with fp32 atomics.
_SLAB_TOL = lambda case: {"table": tol_allclose(1e-4, 1e-5, plus=1.0), "lin_w": tol_allclose(1e-4, 0.0, atol=1e-5),      # noqa: E731
                          "lin_bias": tol_allclose(0.0, 0.0, atol=1e-5 * math.sqrt(case["ids"].shape[0]) * 4)}
_add(Entry("embedding_slab", lambda B: _slab_build(max(B, 3) if B > 1 else 1, 3, 4, 5, 7), _slab_call,
           lambda a, _: ref_emb_pool(a["table"], a["lin_w"], a["lin_bias"], a["ids"], a["row_base"]), ["table", "lin_w", "lin_bias"],
           lambda case: [tol_rel(0.0), tol_allclose(0.0, 2e-5)], _SLAB_TOL, bit_equal=False, spy=("emb_pool_bwd", 5)))
_add(Entry("lin_fields", lambda B: _slab_build(max(B, 3) if B > 1 else 1, 3, 4, 5, 8), _linf_call,
           lambda a, _: ref_lin_fields(a["lin_w"], a["ids"], a["row_base"]), ["lin_w"],
           lambda case: [tol_rel(0.0)],                                            # single-valued fields: a copy of one weight
           lambda case: {"lin_w": tol_allclose(1e-4, 0.0, atol=1e-5)}, bit_equal=False, spy=("lin_fields_bwd", 4)))
# _GatherColsFn as InputLayer calls it: a column gather each way, exact (tests/test_gpu_helper_kernels.py::test_gather_cols)
def _il_build(B, seed):
    g = _g(seed)
    V = 5
    return dict(table=_rn(g, 2 * V, 4) * 0.5, num_a=_rn(g, B, 2), num_n=_rn(g, B, 1), ids=torch.randint(0, V, (B, 2), generator=g), V=V)


def _il_call(a):
    """InputLayer over numeric columns "a" (2 wide), "n" and embedding columns "c", "z": sorted by name the blocks interleave, so the
    layer builds col_map / emb_map itself and runs _GatherColsFn; its slab's table IS the case's leaf"""
    from deep_recommenders_amd import feature_column as fc
    emb = [fc.embedding_column(fc.categorical_column_with_identity(k, a["V"]), 4) for k in ("z", "c")]
    layer = _L().InputLayer([fc.numeric_column("n"), emb[0], fc.numeric_column("a", 2), emb[1]], device=a["table"].device)
    delattr(layer.slab, "table")
    setattr(layer.slab, "table", a["table"])
    return layer({"a": a["num_a"], "n": a["num_n"], "c": a["ids"][:, 0], "z": a["ids"][:, 1]})


def _il_ref(a, _):
    e = a["table"][a["ids"] + torch.arange(2)[None, :] * a["V"]]
    return torch.cat([a["num_a"], e[:, 0], a["num_n"], e[:, 1]], dim=1)           # a, c_embedding, n, z_embedding


# _GatherColsFn through InputLayer: a column gather each way, exact; the table's gradient then goes through the slab's backward
# (atomics, the slab's bound below).  The entry after it calls the Function as InputLayer does, with emb a pitched view.
_add(Entry("input_layer", lambda B: _il_build(B, 14), _il_call, _il_ref, ["table"], lambda case: [tol_rel(0.0)],
           lambda case: {"table": tol_allclose(1e-4, 1e-5, plus=1.0)}, bit_equal=False, spy=("gather_cols", 0)))
_add(Entry("gather_cols", lambda B: _gather_build(B, 9),
           lambda a: _L()._GatherColsFn.apply(a["num"], a["emb"], a["col_map"], a["emb_map"], 11),
           lambda a, _: torch.cat([a["num"], a["emb"]], 1)[:, [0, 3, 4, 1, 5, 6, 7, 8, 2, 9, 10]], ["emb"],
           lambda case: [tol_rel(0.0)], lambda case: {"emb": tol_rel(0.0)}, spy=("gather_cols", 0), present={"emb": "pitched"}))
# tests/test_gpu_afm.py::test_backward and test_gpu_pnn.py::test_normal_cases_are_within_the_fp32_limit: 16 max(r32, 8u) max|ref| for
# the gradients and PNN's out; AFM's out against test_gpu_afm's forward bound is elementwise and needs the stage magnitudes -- the
# same 16 max(r32, 8u) form is used for it here, which test_gpu_afm.py's header reports the kernel inside of by a factor of ten
for _F, _D, _A in ((2, 4, 1), (3, 8, 5)):                                            # the smallest F, D, A and one size above
    _add(Entry("afm_pooling_F%d" % _F, lambda B, F=_F, D=_D, A=_A: _afm_build(B, F, D, A, 10 + F),
               lambda a: _L().afm_pooling(a["emb"], a["W"], a["b"], a["h"])[0], _afm_ref, ["emb", "W", "b", "h"],
               lambda case: [TOL_FP32_16], lambda case: {k: TOL_FP32_16 for k in ("emb", "W", "b", "h")}, spy=("afm_pool_bwd", 7),
               present={"W": "transposed", "b": "expanded"}))
_add(Entry("afm_pooling_with_attention", lambda B: _afm_build(B, 3, 8, 5, 13),           # two outputs, the second non-differentiable
           lambda a: _L().afm_pooling(a["emb"], a["W"], a["b"], a["h"], want_attention=True),
           lambda a, _: (_afm_ref(a, _), __import__("afm_ref").forward(a["emb"], a["W"], a["b"], a["h"])["attn"].detach()),
           ["emb", "W", "b", "h"], lambda case: [TOL_FP32_16, tol_rel(1e-4)],      # attn: tests/test_gpu_afm.py's model test, rtol 1e-4
           lambda case: {k: TOL_FP32_16 for k in ("emb", "W", "b", "h")}))
for _F, _D, _N in ((1, 4, 1), (3, 8, 6)):
    _add(Entry("pnn_outer_F%d" % _F, lambda B, F=_F, D=_D, N=_N: _pnn_build(B, F, D, N, 20 + F),
               lambda a: _L().pnn_outer(a["emb"], a["W"], a["addend"]), _pnn_ref, ["emb", "W", "addend"],
               lambda case: [TOL_FP32_16], lambda case: {"emb": TOL_FP32_16, "W": TOL_FP32_16, "addend": tol_rel(0.0)},
               present={"addend": "pitched"}))
# tests/test_gpu_dlrm.py: forward (D + 2) u (|T| |T|^T) per triangle element, backward (N + 3) u sum_j |g_ij| |T_j|_d.  Both are at
# most (D + 2) u resp. (N + 3) u times what the reference itself gives on the absolute values of its inputs, which is how they are
# computed here: ref(|dense|, |emb|) and its gradient under |G|.
def _di_tol_out(case):
    D, c0 = case["emb"].shape[2], 0 if case["dense"] is None else case["emb"].shape[2]

    def f(w64, w32, ctx):
        b = (D + 2) * U * ctx["abs"]
        b[:, :c0] = 0                                      # the dense columns are a copy
        return b
    return [f]


# Inputs as views, where a layer has none in the table: a 3-d or 4-d emb / rows of dot_interaction, afm_pooling, pnn_outer and
# ffm_interaction must be contiguous by the wrappers' contract (ValueError otherwise: tests/test_gpu_dlrm.py, _afm, _pnn, _ffm.py pin
# it), and the tables of EmbeddingSlab and ffm_gather are nn.Parameters, contiguous by construction (ffm_gather refuses another).
for _F, _D, _dense in ((2, 4, False), (1, 4, True), (3, 8, True), (7, 4, True)):      # F = 7: a width (32) that is a multiple of 4
    _add(Entry("dot_interaction_F%d_%s" % (_F, "dense" if _dense else "nodense"), lambda B, F=_F, D=_D, d=_dense: _di_build(B, F, D, d, 30 + F),
               lambda a: _L().dot_interaction(a["dense"], a["emb"]), _di_ref, ["dense", "emb"],
               _di_tol_out, lambda case: {k: tol_abs((case["emb"].shape[1] + (case["dense"] is not None) + 3) * U) for k in ("dense", "emb")},
               spy=("dot_interact_bwd", 4)))
# softmax: tests/test_gpu_helper_kernels.py::test_softmax_rows.  Forward (gamma(d + 3) + 4 yard) max(y, u), d = ceil(C / 64) + 6.
# Backward gamma(d + 3) |y| (|dy| + sum|y dy|) against float64 fed the kernel's own y; the float64 reference here has its own y, so
# the forward's relative error enters once through each of the three factors y: (4 gamma(d + 3) + 12 yard) on the same magnitude,
# which is what the reference gives on |dy| ("abs" below: |y| (|dy| + sum |y| |dy|)).
def _softmax_fwd_tol(case):
    d = math.ceil(case["x"].shape[1] / 64) + 6

    def f(w64, w32, ctx=None):
        mag = w64.clamp_min(U)
        return (gamma(d + 3) + 4 * ((w32.double() - w64).abs() / mag).max().item()) * mag
    return f


def _softmax_bwd_tol(case):
    d = math.ceil(case["x"].shape[1] / 64) + 6

    def f(w64, w32, ctx):
        y, G = ctx["outs64"][0], ctx["G"][0].double().abs()
        yard = ((ctx["outs32"][0].double() - y).abs() / y.clamp_min(U)).max().item()
        return (4 * gamma(d + 3) + 12 * yard) * y * (G + (y * G).sum(1, keepdim=True))
    return f


_add(Entry("softmax_rows", lambda B: dict(x=_rn(_g(40), B, 7) * 2), lambda a: _L().softmax_rows(a["x"]), lambda a, _: ref_softmax(a["x"]),
           ["x"], lambda case: [_softmax_fwd_tol(case)], lambda case: {"x": _softmax_bwd_tol(case)}, spy=("softmax_rows_bwd", 1), present={"x": "transposed"}))
# l2_penalty and the residual add: n-term fp32 sums, n 2^-24 times the float64 sum of magnitudes
_add(Entry("l2_penalty", lambda B: dict(w=_rn(_g(41), 5, 3), coeff=0.01), lambda a: _L().l2_penalty(a["w"], a["coeff"]),
           lambda a, _: a["coeff"] * (a["w"] ** 2).sum(), ["w"],
           lambda case: [lambda w64, w32, ctx=None: torch.full_like(w64, 15 * U * 0.01 * float((case["w"].double() ** 2).sum()))],
           lambda case: {"w": tol_rel(3 * U)}, present={"w": "transposed"}))       # 2 coeff d w: the fp32 coefficient and one product
_add(Entry("add_residual", lambda B: dict(out=_rn(_g(42), B, 5), x=_rn(_g(43), B, 5)), lambda a: _L()._AddFn.apply(a["out"], a["x"]),
           lambda a, _: a["out"] + a["x"], ["out", "x"],
           lambda case: [lambda w64, w32, ctx=None: 2 * U * (case["out"].double().abs() + case["x"].double().abs())],
           lambda case: {"out": tol_rel(0.0), "x": tol_rel(0.0)}, present={"out": "pitched"}))
# activation: tests/test_gpu_small_kernels.py::test_act_bwd: gamma(3) |dy| (1 + |y|)^2 from the saved fp32 y; the forward is libm
# (test_act_fwd: within 4 u of float64 relative to max(|y|, tiny)) and its error reaches the derivative once: (gamma(3) + 8 u)
for _act, _nm in ((1, "relu"), (2, "sigmoid"), (3, "tanh")):
    _add(Entry("activation_" + _nm, lambda B: dict(x=_rn(_g(44), B, 5)), lambda a, act=_act: _L().activation(a["x"], act),
               lambda a, _, act=_act: ACT[act](a["x"]), ["x"], lambda case: [tol_rel(4 * U)],
               lambda case: {"x": lambda w64, w32, ctx: (gamma(3) + 8 * U) * ctx["G"][0].double().abs() * (1 + ctx["outs64"][0].abs()) ** 2},
               present={"x": "pitched"}))


def _ffm_build(B, F, k, seed):
    g = _g(seed)
    V = 4
    ids = torch.randint(0, V, (B, F), generator=g)
    if B > 2:
        ids[1] = ids[0]
        ids[2, 0] = -1
    return dict(rows=_rn(g, B, F, F, k), table=_rn(g, F * V, F * k) * 0.5, lin_w=_rn(g, F * V), lin_bias=_rn(g, 1), ids=ids,
                row_base=torch.arange(F) * V, F=F, k=k)


def _ffm_gather_ref(a, _):
    import ffm_ref as R
    A = R.gather(a["table"], a["ids"], a["row_base"], a["F"], a["k"])
    return R.interaction(A), R.first_order(a["lin_w"], a["lin_bias"], a["ids"], a["row_base"])


# tests/test_gpu_ffm.py: forward gamma(F (F - 1) / 2 k) * abs_sum(A) ("abs" of the reference); d_rows is one correctly rounded
# multiply (u |ref|); first order gamma(F + 1) (|bias| + sum|w|); the gathered table gradient adds at most m slots into a row:
# gamma(m) times the magnitudes, m <= B here; taken as the slab's bound above (rtol 1e-4, atol 1e-5 (max + 1)) for the atomics
for _F, _k in ((2, 4), (3, 8)):
    _add(Entry("ffm_interaction_F%d" % _F, lambda B, F=_F, k=_k: _ffm_build(B, F, k, 50 + F),
               lambda a: _L().ffm_interaction(a["rows"], a["F"], a["k"]),
               lambda a, _: __import__("ffm_ref").interaction(a["rows"]), ["rows"],
               lambda case: [tol_abs(gamma(case["F"] * (case["F"] - 1) // 2 * case["k"]))], lambda case: {"rows": tol_rel(U)}))
    _add(Entry("ffm_gather_F%d" % _F, lambda B, F=_F, k=_k: _ffm_build(B, F, k, 60 + F),
               lambda a: _L().ffm_gather(a["table"], a["lin_w"], a["lin_bias"], a["ids"], a["row_base"], a["F"], a["k"]),
               _ffm_gather_ref, ["table", "lin_w", "lin_bias"],
               lambda case: [tol_abs(gamma(case["F"] * (case["F"] - 1) // 2 * case["k"])), tol_abs(gamma(case["F"] + 1))], _SLAB_TOL,
               bit_equal=False))


def _dice_ref(a, _):
    import din_ref as R
    return R.dice(a["x"], a["alpha"], 1e-8)


# tests/test_gpu_din.py::_check: max(8 yard, 2e-6) max|ref| for Dice and the interest pooling, forward and backward
for _N in (1, 5):
    _add(Entry("dice_N%d" % _N, lambda B, N=_N: dict(x=_rn(_g(70 + N), B, N), alpha=_rn(_g(71), N) * 0.5),
               lambda a: _L().dice(a["x"], a["alpha"]), _dice_ref, ["x", "alpha"], lambda case: [TOL_DIN],
               lambda case: {"x": TOL_DIN, "alpha": TOL_DIN}, spy=("dice_bwd", 2), present={"x": "pitched"}))


def _din_build(B, T, D, Uh, mode, act, seed):
    g = _g(seed)
    n_in = 2 if mode == 0 else 3
    mask = torch.rand(B, T, generator=g) < 0.7
    if B > 1:
        mask[0] = False                                    # an example with no valid key
        mask[1] = True
    return dict(query=_rn(g, B, D), keys=_rn(g, B, T, D), mask=mask, W=_rn(g, n_in * D, Uh) * (1.5 / math.sqrt(n_in * D)), b=_rn(g, Uh) * 0.2,
                w_out=_rn(g, Uh, 1) / math.sqrt(Uh), b_out=_rn(g, 1) * 0.2, alpha=_rn(g, Uh) * 0.5 if act == 4 else None, mode=mode, act=act)


_DIN_ARGS = ("query", "keys", "mask", "W", "b", "w_out", "b_out", "mode", "act", "alpha")
for _T, _D, _Uh, _mode, _act in ((1, 4, 1, 0, 1), (5, 8, 3, 2, 4)):
    _add(Entry("din_interest_pooling_T%d" % _T, lambda B, a=(_T, _D, _Uh, _mode, _act): _din_build(B, *a, 80),
               lambda a: _L().din_interest_pooling(*[a[k] for k in _DIN_ARGS]),
               lambda a, _: __import__("din_ref").pool(*[a[k] for k in _DIN_ARGS]), ["query", "keys", "W", "b", "w_out", "b_out", "alpha"],
               lambda case: [TOL_DIN, TOL_DIN], lambda case: {k: TOL_DIN for k in ("query", "keys", "W", "b", "w_out", "b_out", "alpha")},
               present={"query": "pitched", "keys": "pitched", "W": "transposed", "b": "expanded"}))


def _cin_build(B, H0, Hk, D, Fm, seed):
    g = _g(seed)
    return dict(x0=_rn(g, B, H0, D), x=_rn(g, B, Hk, D), W=_rn(g, H0 * Hk, Fm) / math.sqrt(H0 * Hk), bias=_rn(g, Fm) * 0.2,
                W2=_rn(g, H0 * Fm, 2) / math.sqrt(H0 * Fm), bias2=_rn(g, 2) * 0.2)


def _cin_tol_out(case):
    """tests/test_gpu_xdeepfm.py: out rtol 1e-5, atol 2e-6 scale, scale = max|x0| max|x| max|W| sqrt(H0 Hk); pooled D times that"""
    H0, Hk, D = case["x0"].shape[1], case["x"].shape[1], case["x0"].shape[2]
    scale = (case["x0"].abs().max() * case["x"].abs().max() * case["W"].abs().max()).item() * math.sqrt(H0 * Hk)
    return [tol_allclose(1e-5, 0.0, atol=2e-6 * scale), tol_allclose(1e-5, 0.0, atol=D * 2e-6 * scale)]


_CIN_GRAD = tol_allclose(2e-4, 2e-5)                                                # tests/test_gpu_xdeepfm.py::_check_grads
for _act in (0, 2):
    _add(Entry("cin_pool_act%d" % _act, lambda B: _cin_build(B, 2, 3, 4, 3, 90),
               lambda a, act=_act: _L().cin_pool(a["x0"], a["x"], a["W"], a["bias"], act),
               lambda a, _, act=_act: __import__("xdeepfm_ref").cin_pool(a["x0"], a["x"], a["W"], a["bias"], act), ["x0", "x", "W", "bias"],
               _cin_tol_out, lambda case: {k: _CIN_GRAD for k in ("x0", "x", "W", "bias")},
               present={"x0": "pitched", "x": "pitched", "W": "transposed"}))


def _cin_stack_build(B, seed):
    g = _g(seed)
    H0, D, F1, F2 = 2, 4, 3, 2
    return dict(x0=_rn(g, B, H0, D), W=_rn(g, H0 * H0, F1) / 2, bias=_rn(g, F1) * 0.2, W2=_rn(g, H0 * F1, F2) / math.sqrt(H0 * F1),
                bias2=_rn(g, F2) * 0.2)


def _cin_stack_tol(case):
    # tests/test_gpu_xdeepfm.py's stack test: rtol 1e-5, atol 8 * 2e-6 scale (1 + scale)
    scale = (case["x0"].abs().max() ** 2 * max(case["W"].abs().max(), case["W2"].abs().max())).item() * math.sqrt(6)
    return [tol_allclose(1e-5, 0.0, atol=case["x0"].shape[2] * 8 * 2e-6 * scale * (1 + scale))]


for _act in (0, 1):
    _add(Entry("cin_stack_act%d" % _act, lambda B: _cin_stack_build(B, 91),
               lambda a, act=_act: _L().cin_stack(a["x0"], [a["W"], a["W2"]], [a["bias"], a["bias2"]], act),
               lambda a, _, act=_act: __import__("xdeepfm_ref").cin_network(a["x0"], [a["W"], a["W2"]], [a["bias"], a["bias2"]], act),
               ["x0", "W", "bias", "W2", "bias2"], _cin_stack_tol, lambda case: {k: _CIN_GRAD for k in ("x0", "W", "bias", "W2", "bias2")},
               present={"x0": "pitched", "W2": "transposed"}))


def _gru_build(B, T, H, with_att, seed):
    g = _g(seed)
    lengths = torch.randint(0, T + 1, (B,), generator=g)
    lengths[0] = T
    if B > 1:
        lengths[1] = 0
    return dict(xp=_rn(g, B, T, 3 * H), U=_rn(g, H, 3 * H) / math.sqrt(H), h0=_rn(g, B, H) * 0.5, lengths=lengths,
                att=torch.rand(B, T, generator=g) if with_att else None, q=_rn(g, B, H))


# tests/test_gpu_dien.py::_check with dien_ref.limit: 16 max(r32, 8u) max|ref|
for _T, _att in ((1, False), (5, True)):
    _add(Entry("gru_sequence_T%d" % _T, lambda B, T=_T, att=_att: _gru_build(B, T, 4 if T == 1 else 8, att, 100 + T),
               lambda a: _L().gru_sequence(a["xp"], a["U"], a["h0"], a["lengths"], a["att"]),
               lambda a, _: __import__("dien_ref").forward(a["xp"], a["U"], a["h0"], a["lengths"], a["att"]), ["xp", "U", "h0", "att"],
               lambda case: [TOL_FP32_16, TOL_FP32_16], lambda case: {k: TOL_FP32_16 for k in ("xp", "U", "h0", "att")},
               present={"xp": "pitched", "U": "transposed", "h0": "pitched"}))
    _add(Entry("sequence_attention_T%d" % _T, lambda B, T=_T: dict(hs=_rn(_g(110 + T), B, T, 4), **{k: v for k, v in _gru_build(B, T, 4, False, 111).items()
                                                                                                 if k in ("q", "lengths")}),
               lambda a: _L().sequence_attention(a["hs"], a["q"], a["lengths"]),
               lambda a, _: __import__("dien_ref").attention(a["hs"], a["q"], a["lengths"]), ["hs", "q"],
               lambda case: [TOL_FP32_16], lambda case: {"hs": TOL_FP32_16, "q": TOL_FP32_16}, present={"hs": "pitched", "q": "pitched"}))

FLOOR = 2.0 ** -100                                      # tests/test_gpu_attention.py: magnitudes are floored at fp32 underflow


def tol_abs_yard(n):
    """tests/test_gpu_attention.py's form: (gamma(n) + 4 yard) (mag + FLOOR), mag the reference on absolute values, yard the float32
    run of the reference relative to mag"""
    def f(w64, w32, ctx):
        mag = ctx["abs"] + FLOOR
        return (gamma(n) + 4 * float(((w32.double() - w64).abs() / mag).max())) * mag
    return f


# ---- graph aggregation: tests/test_gpu_gcn.py::_check_spmm, 1e-5 (|A| |X|)_ij + 1e-30 -- the reference on absolute values; the
# backward is the same product with the transpose.  The dense adjacency goes through the GEMM: test_linear_fwd_bwd's forward and dW.
def _agg_build(B, seed):
    g = _g(seed)
    n_rows, n_cols = 9, max(B, 2)
    adj = _rn(g, n_rows, n_cols) * (torch.rand(n_rows, n_cols, generator=g) < 0.4)
    adj[3] = 0                                                                      # an empty row
    return dict(adj=adj, X=_rn(g, n_cols, 5))


_SP_TOL = lambda w64, w32, ctx: 1e-5 * ctx["abs"] + 1e-30      # noqa: E731
_add(Entry("aggregate_sparse", lambda B: _agg_build(B, 120),
           lambda a: _L().aggregate(_L().SparseAdjacency(a["adj"].to_sparse_coo(), device=a["adj"].device), a["X"]),
           lambda a, _: a["adj"] @ a["X"], ["X"], lambda case: [_SP_TOL], lambda case: {"X": _SP_TOL}, present={"X": "pitched"}))
_add(Entry("aggregate_dense", lambda B: _agg_build(B, 121), lambda a: _L().aggregate(a["adj"], a["X"]),
           lambda a, _: a["adj"] @ a["X"], ["X"], lambda case: [tol_gemm(2e-6, case["X"].shape[0])], lambda case: {"X": tol_gemm(4e-6, 9)},
           present={"X": "pitched"}))
_add(Entry("global_average_pooling_1d", lambda B: dict(x=_rn(_g(122), B, 5, 6)), lambda a: _L().global_average_pooling_1d(a["x"]),
           lambda a, _: a["x"].mean(1), ["x"], lambda case: [_SP_TOL], lambda case: {"x": _SP_TOL}))


def _tok_build(B, seed):
    import transformer_ref as R
    g = _g(seed)
    V, D, L = 6, 5, 4
    ids = torch.randint(0, V - 1, (B, L), generator=g)                               # row V - 1 is looked up by nobody
    ids[0] = 2
    return dict(table=_rn(g, V, D), ids=ids, pos=torch.from_numpy(R.position_encoding(L, D)))


def _tok_tol_grad(case):
    counts = int(torch.bincount(case["ids"].reshape(-1), minlength=case["table"].shape[0]).max())
    return {"table": tol_abs_yard(counts + 8)}               # tests/test_gpu_attention.py::test_token_embedding


_add(Entry("token_embedding", lambda B: _tok_build(B, 123), lambda a: _L().token_embedding(a["table"], a["ids"], a["pos"]),
           lambda a, _: __import__("transformer_ref").token_embedding(a["table"], a["ids"], a["pos"], dtype=a["table"].dtype), ["table"],
           lambda case: [tol_abs_yard(6)], _tok_tol_grad, spy=("token_embedding_bwd", 1), present={"table": "transposed"}))


def _tok_drop_ref(a, got):
    import transformer_ref as R
    keep = None if got is None else got[0].cpu() != 0        # the kept set, read off the forward's output (no value is 0 otherwise)
    return R.token_embedding(a["table"], a["ids"], a["pos"], keep=keep, rate=0.3 if keep is not None else 0.0, dtype=a["table"].dtype)


_add(Entry("token_embedding_dropout", lambda B: _tok_build(B, 123),
           lambda a: _L().token_embedding(a["table"], a["ids"], a["pos"], rate=0.3, seed=5), _tok_drop_ref, ["table"],
           lambda case: [tol_abs_yard(6)], _tok_tol_grad))


def _ln_build(B, D, seed, with_b=True):
    g = _g(seed)
    return dict(a=_rn(g, B, 3, D), b=_rn(g, B, 3, D) if with_b else None, gamma=1 + 0.3 * _rn(g, D), beta=0.3 * _rn(g, D))


def _ln_tols(case):
    """tests/test_gpu_attention.py::test_add_layernorm, its magnitudes restated in torch (float64): (gamma(n) + 4 yard) (mag + FLOOR)
    with n = D + 32, 2 D + 48, M + D + 32, M + 8 for y, d_s, d_gamma, d_beta"""
    D = case["a"].shape[-1]
    M = case["a"].numel() // D
    a, g, be = case["a"].double().reshape(M, D), case["gamma"].double()[None], case["beta"].double()[None]
    s = a + (case["b"].double().reshape(M, D) if case["b"] is not None else 0.0)
    mean = s.mean(1, keepdim=True)
    d = s - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-8)
    xh = d * rstd
    spread = s.abs() + mean.abs()
    A = spread * rstd + xh.abs() * (d.abs() * spread).mean(1, keepdim=True) / (var + 1e-8)
    Ar = A.max(1, keepdim=True).values

    def mk(n, mag_of):
        def f(w64, w32, ctx):
            dy = ctx["G"][0].double().reshape(M, D)
            gg = (dy * g).abs()
            m1, m2 = gg.mean(1, keepdim=True), (gg * xh.abs()).mean(1, keepdim=True)
            mag = mag_of(dy, gg, m1, m2, w64).reshape(w64.shape) + FLOOR
            return (gamma(n) + 4 * float(((w32.double() - w64).abs() / mag).max())) * mag
        return f
    y = mk(D + 32, lambda dy, gg, m1, m2, w: g.abs() * (xh.abs() + A) + be.abs())
    ds = mk(2 * D + 48, lambda dy, gg, m1, m2, w: rstd * (gg + m1 + xh.abs() * m2 + Ar * (m2 + m1 + xh.abs() * m1)) + Ar * w.reshape(M, D).abs())
    dg = mk(M + D + 32, lambda dy, gg, m1, m2, w: (dy.abs() * (xh.abs() + A)).sum(0))
    db = mk(M + 8, lambda dy, gg, m1, m2, w: dy.abs().sum(0))
    return y, {"a": ds, "b": ds, "gamma": dg, "beta": db}


def _ln_fwd_tol(case):
    f = _ln_tols(case)[0]
    # the forward's magnitude needs no incoming gradient
    return [lambda w64, w32, ctx: f(w64, w32, dict(ctx, G=[torch.zeros_like(w64)]))]


for _D, _wb in ((1, True), (5, True), (6, False)):
    _add(Entry("add_layer_norm_D%d" % _D, lambda B, D=_D, wb=_wb: _ln_build(B, D, 124 + D, wb),
               lambda a: _L().add_layer_norm(a["a"], a["b"], a["gamma"], a["beta"]),
               lambda a, _: __import__("transformer_ref").layer_norm(a["a"], a["b"], a["gamma"], a["beta"], dtype=a["a"].dtype),
               ["a", "b", "gamma", "beta"], _ln_fwd_tol, lambda case: _ln_tols(case)[1], spy=("add_layernorm_bwd", 4),
               present={"a": "pitched"} if _D == 5 else None))


def _attn_build(B, H, Lq, Lk, dh, seed):
    g = _g(seed)
    mask = torch.zeros(B, Lk, dtype=torch.bool)
    mask[0, Lk - 1:] = Lk > 1                                                      # a padded key
    return dict(q=_rn(g, B, Lq, H * dh), k=_rn(g, B, Lk, H * dh), v=_rn(g, B, Lk, H * dh), mask=mask, H=H)


def _attn_tols(case):
    """tests/test_gpu_attention.py::_check: (gamma(n) + sens es + 4 yard) (mag + FLOOR), the magnitudes being transformer_ref.attention_magnitudes; rate = 0"""
    import transformer_ref as TA
    H, Lq, Lk = case["H"], case["q"].shape[1], case["k"].shape[1]
    dh = case["q"].shape[2] // H
    chains = [Lk + TA.dhp(dh) + 16] + [Lq + Lk + 2 * TA.dhp(dh) + 32] * 3
    sens = [2, 4, 4, 2]

    def mk(i):
        def f(w64, w32, ctx):
            G = ctx["G"][0] if ctx["G"][0] is not None else torch.zeros_like(case["q"])
            mags, es = TA.attention_magnitudes(case["q"].numpy(), case["k"].numpy(), case["v"].numpy(), G.float().contiguous().numpy(), H,
                                      case["mask"].numpy(), False, None, 0.0)
            mag = torch.from_numpy(mags[i]) + FLOOR
            return (gamma(chains[i]) + sens[i] * es + 4 * float(((w32.double() - w64).abs() / mag).max())) * mag
        return f
    return [mk(0)], {"q": mk(1), "k": mk(2), "v": mk(3)}


for _H, _Lq, _Lk, _dh in ((1, 1, 1, 1), (2, 3, 5, 3)):
    _add(Entry("attention_H%d" % _H, lambda B, a=(_H, _Lq, _Lk, _dh): _attn_build(B, *a, 130),
               lambda a: _L().attention(a["q"], a["k"], a["v"], a["H"], a["mask"]),
               lambda a, _: __import__("transformer_ref").attention(a["q"], a["k"], a["v"], a["H"], a["mask"].numpy(), dtype=a["q"].dtype),
               ["q", "k", "v"], lambda case: _attn_tols(case)[0], lambda case: _attn_tols(case)[1], spy=("attn_bwd", 4),
               present={"q": "pitched"}))

# --------------------------------------------------------------------------------------------------------------------------------------
# The Functions of the rest of the package, and the two layers.py gained after the table was first written
# --------------------------------------------------------------------------------------------------------------------------------------
PKG = "deep_recommenders_amd"
_LAYERS, _LOSSES = PKG + ".layers", PKG + ".losses"
_SBCNM, _XDEEPFM = PKG + ".keras.models.retrieval.sbcnm", PKG + ".keras.models.ranking.xdeepfm"
_DIEN, _DIN = PKG + ".keras.models.ranking.dien", PKG + ".keras.models.ranking.din"
_ESMM = PKG + ".estimator.models.multi_task_learning.esmm"
_MMOE = PKG + ".estimator.models.multi_task_learning.mixture_of_experts"


def _mod(name):
    import importlib
    return importlib.import_module(name)


def tol_sum(*tols):
    """a Function made of several kernels: the sum of its parts' bounds"""
    return lambda w64, w32, ctx=None: sum(t(w64, w32, ctx) for t in tols)


def tol_close(c):
    """tests/test_gpu_multitask.py::_close and _check_model_parity: c max(1, max|ref|)"""
    return lambda w64, w32, ctx=None: torch.full_like(w64, c * max(1.0, float(w64.abs().max()) if w64.numel() else 1.0))


def _gmax(ctx):
    return max([float(G.abs().max()) for G in ctx["G"] if G is not None and G.numel()] or [1.0])


def tol_allclose_g(rtol, atol):
    """assert_allclose's rtol |ref| + atol of a test that sent the gradient 1 into a loss: the absolute part scales with the incoming
    gradient (the largest |G|), the relative part does by itself"""
    return lambda w64, w32, ctx: rtol * w64.abs() + atol * _gmax(ctx)


def tol_rel_yard(n, c=4.0):
    """(gamma(n) + c yard) |ref|, yard the largest relative error of the float32 run of the reference"""
    def f(w64, w32, ctx=None):
        nz = w64 != 0
        yard = float(((w32.double() - w64).abs()[nz] / w64.abs()[nz]).max()) if bool(nz.any()) else 0.0
        return (gamma(n) + c * yard) * w64.abs()
    return f


_K4_TOL = tol_allclose(1e-4, 1e-5, plus=1.0)        # K4 into a dense gradient buffer: the slab's bound above (test_emb_pool_bwd_matches_autograd_oracle)


# ---- skip-gram with negative sampling.  tests/test_gpu_sgns.py bounds every stage element by element from intermediate sums of
# magnitudes (scores, coeff, rows) that this table does not have; the yardstick form test_gpu_afm / pnn / dien use is taken for the two
# gather kernels (16 max(r32, 8u) max|ref|), and a table gradient adds K4's bound to it (rows shared by several examples are summed there)
def _sgns_build(B, K, skip_equal, seed):
    g = _g(seed)
    V, D = 9, 4                                              # D % 4 == 0 is the kernels' domain; 9 rows: every row is shared at B = 70
    n = B if B == 1 else max(B, 4)
    centers, contexts = torch.randint(0, V, (n,), generator=g), torch.randint(0, V, (n,), generator=g)
    negatives = torch.randint(0, V, (n, K), generator=g)
    if K:
        negatives[0, 0] = contexts[0]                        # a negative equal to its context: skipped, or not, by skip_equal
    if n > 1:
        centers[1] = -1                                      # a skipped example
        centers[2] = centers[3] = centers[0]                 # one row of in_table shared by three examples
        contexts[2] = contexts[0]
    return dict(in_table=_rn(g, V, D) * D ** -0.25, out_table=_rn(g, V, D) * D ** -0.25, centers=centers, contexts=contexts,
                negatives=negatives if K else None, w=torch.rand(n, generator=g) + 0.5, skip_equal=skip_equal)


def _sgns_call(a, planned):
    from deep_recommenders_amd import ops
    n, K = a["centers"].shape[0], 0 if a["negatives"] is None else a["negatives"].shape[1]
    dev = a["in_table"].device
    plans = (ops.SortPlan(n, dev), ops.SortPlan(n * (1 + K), dev)) if planned else None
    return _L().sgns_loss(a["in_table"], a["out_table"], a["centers"], a["contexts"], a["negatives"], a["w"], a["skip_equal"], None, plans)


def _sgns_ref(a, _):
    import sgns_ref as R
    neg = a["negatives"] if a["negatives"] is not None else torch.empty((a["centers"].shape[0], 0), dtype=torch.int64)
    return R.loss_expr(a["in_table"], a["out_table"], a["centers"], a["contexts"], neg, a["w"], a["skip_equal"])[0].to(a["in_table"].dtype)


_SGNS_GRAD = tol_sum(TOL_FP32_16, _K4_TOL)
for _K, _se, _pl in ((5, True, False), (5, False, True), (0, True, True), (0, False, False)):
    _add(Entry("sgns_loss_K%d_%s_%s" % (_K, "skip" if _se else "keep", "plans" if _pl else "atomics"),
               lambda B, K=_K, se=_se: _sgns_build(B, K, se, 140 + K), lambda a, pl=_pl: _sgns_call(a, pl), _sgns_ref, ["in_table", "out_table"],
               lambda case: [TOL_FP32_16], lambda case: {"in_table": _SGNS_GRAD, "out_table": _SGNS_GRAD},
               bit_equal=_pl,                                # without plans K4 combines with fp32 atomics
               functions=[(_LAYERS, "_SgnsFn")]))


# ---- skip-gram with side information: the same two-kernel-plus-K4 structure and the same bounds (tests/test_gpu_eges.py's are
# element by element as test_gpu_sgns.py's are)
def _eges_build(B, with_att, P, seed):
    g = _g(seed)
    S, D, V, R_att, K = 3, 4, 5, 6, 3                        # S = 3: att is [R_att, pad4(S)] = [6, 4], the last column padding
    n = B if B == 1 else max(B, 4)
    side_ids = torch.randint(0, V, (n, S), generator=g)
    att_ids = torch.randint(0, R_att, (n,), generator=g)
    contexts, negatives = torch.randint(0, 9, (n, P), generator=g), torch.randint(0, 9, (n, K), generator=g)
    negatives[0, 0] = contexts[0, 0]                         # a negative equal to a positive (skip_equal)
    if n > 1:
        side_ids[1, 0] = -1                                  # a missing field
        att_ids[2] = -1                                      # a cold-start example: the plain average
        side_ids[3] = side_ids[0]                            # rows shared by two examples
    return dict(side_table=_rn(g, S * V, D) * D ** -0.25, att=_rn(g, R_att, pad4(S)) if with_att else None, out_table=_rn(g, 9, D) * D ** -0.25,
                row_base=torch.arange(S) * V, side_ids=side_ids, att_ids=att_ids, contexts=contexts, negatives=negatives,
                w=torch.rand(n, generator=g) + 0.5)


def _eges_call(a, planned):
    from deep_recommenders_amd import ops
    n, S = a["side_ids"].shape
    J = a["contexts"].shape[1] + a["negatives"].shape[1]
    dev = a["side_table"].device
    plans = (ops.SortPlan(n * S, dev), ops.SortPlan(n, dev), ops.SortPlan(n * J, dev)) if planned else None
    return _L().eges_loss(a["side_table"], a["row_base"], a["side_ids"], a["att"], a["att_ids"], a["out_table"], a["contexts"], a["negatives"],
                          a["w"], True, None, plans)


def _eges_ref(a, _):
    import eges_ref as R
    return R.loss_expr(a["side_table"], a["row_base"], a["side_ids"], a["att"], a["att_ids"], a["out_table"], a["contexts"], a["negatives"],
                       a["w"], True)[0].to(a["side_table"].dtype)


for _att, _P, _pl in ((True, 1, False), (True, 2, True), (False, 1, True), (False, 2, False)):
    _add(Entry("eges_loss_%s_P%d_%s" % ("att" if _att else "noatt", _P, "plans" if _pl else "atomics"),
               lambda B, att=_att, P=_P: _eges_build(B, att, P, 150 + P), lambda a, pl=_pl: _eges_call(a, pl), _eges_ref,
               ["side_table", "att", "out_table"], lambda case: [TOL_FP32_16],
               lambda case: {k: _SGNS_GRAD for k in ("side_table", "att", "out_table")}, bit_equal=_pl, functions=[(_LAYERS, "_EgesFn")]))


# ---- losses.py.  tests/test_gpu_kernels.py::test_bce_modes: the loss within 1e-5 of its value, d_logit rtol 1e-4, atol 1e-9;
# tests/test_gpu_helper_kernels.py::test_bce_prob_fwd_bwd: d_prob within g(4) + four times the fp32 formula's relative error, one more
# rounding here for the product with d_loss; ::test_sigmoid_fwd_bwd: rtol 2e-5, atol 2e-6 forward, the backward dy y (1 - y) bit for
# bit from the fp32 y -- against float64 that is activation_sigmoid's bound above; tests/test_gpu_multitask.py::test_mse_matches_float64:
# 1e-4 max(1, max|ref|) for the loss and d_pred; tests/test_gpu_gcn.py::test_categorical_crossentropy_both_branches: the loss within
# 1e-5 of its value, the logits' gradient atol 1e-6, the probabilities' rtol 1e-4, atol 1e-6.
def _bin_build(B, prob, seed):
    g = _g(seed)
    x = _rn(g, B, 1) * 2
    return dict(x=torch.sigmoid(x) * 0.9 + 0.05 if prob else x, labels=(torch.rand(B, 1, generator=g) < 0.4).float())


def _T():
    from oracle import torch_ref
    return torch_ref


_add(Entry("sigmoid_cross_entropy", lambda B: _bin_build(B, False, 160), lambda a: _mod(_LOSSES).sigmoid_cross_entropy(a["labels"], a["x"]),
           lambda a, _: _T().sigmoid_cross_entropy(a["labels"], a["x"]), ["x"], lambda case: [tol_rel(1e-5)],
           lambda case: {"x": tol_allclose_g(1e-4, 1e-9)}, present={"x": "pitched"}, functions=[(_LOSSES, "_LogitLossFn")]))
_add(Entry("log_loss", lambda B: _bin_build(B, True, 161), lambda a: _mod(_LOSSES).log_loss(a["labels"], a["x"]),
           lambda a, _: _T().log_loss(a["labels"], a["x"]), ["x"], lambda case: [tol_rel(1e-5)],
           lambda case: {"x": tol_rel_yard(5)}, present={"x": "pitched"}, functions=[(_LOSSES, "_ProbLossFn")]))
_add(Entry("binary_crossentropy", lambda B: _bin_build(B, True, 162), lambda a: _mod(_LOSSES).binary_crossentropy(a["labels"], a["x"]),
           lambda a, _: _T().keras_bce(a["labels"], a["x"]), ["x"], lambda case: [tol_rel(1e-5)],
           lambda case: {"x": tol_rel_yard(5)}, present={"x": "pitched"}, functions=[(_LOSSES, "_ProbLossFn")]))
_add(Entry("losses_sigmoid", lambda B: dict(x=_rn(_g(163), B, 5) * 2), lambda a: _mod(_LOSSES).sigmoid(a["x"]), lambda a, _: torch.sigmoid(a["x"]),
           ["x"], lambda case: [tol_allclose(2e-5, 0.0, atol=2e-6)],
           lambda case: {"x": lambda w64, w32, ctx: (gamma(3) + 8 * U) * ctx["G"][0].double().abs() * (1 + ctx["outs64"][0].abs()) ** 2},
           present={"x": "pitched"}, functions=[(_LOSSES, "_SigmoidFn")]))
for _Tn in (1, 3):
    _add(Entry("mean_squared_error_T%d" % _Tn, lambda B, T=_Tn: dict(p=_rn(_g(164 + T), B, T) * 2, labels=_rn(_g(165 + T), B, T)),
               lambda a: _mod(_LOSSES).mean_squared_error(a["labels"], a["p"]),
               lambda a, _, T=_Tn: ((a["p"] - a["labels"]) ** 2).mean(0).reshape(() if T == 1 else (T,)), ["p"], lambda case: [tol_close(1e-4)],
               lambda case: {"p": tol_close(1e-4)}, present={"p": "pitched"}, functions=[(_LOSSES, "_MseFn")]))


def _cce_build(B, weighted, prob, seed):
    g = _g(seed)
    C = 7
    x = _rn(g, B, C) * 2
    w = (torch.rand(B, generator=g) < 0.5).float()
    w[0] = 1.0                                               # at least one row counts
    return dict(x=x.abs() + 0.05 if prob else x, y=torch.eye(C)[torch.randint(0, C, (B,), generator=g)], w=w if weighted else None)


def ref_cce_logits(x, y, w):
    ce = -(y * torch.log_softmax(x, 1)).sum(1)
    return (ce if w is None else w * ce).sum() / x.shape[0]


def ref_cce_prob(p, y, w):
    ce = -(y * torch.log(torch.clamp(p / p.sum(1, keepdim=True), 1e-7, 1 - 1e-7))).sum(1)
    return (ce if w is None else w * ce).sum() / p.shape[0]


for _wt in (False, True):
    _add(Entry("categorical_crossentropy_logits" + ("_weighted" if _wt else ""), lambda B, wt=_wt: _cce_build(B, wt, False, 170),
               lambda a: _mod(_LOSSES).categorical_crossentropy(a["y"], _L().softmax_rows(a["x"]), a["w"]),
               lambda a, _: ref_cce_logits(a["x"], a["y"], a["w"]), ["x"], lambda case: [tol_rel(1e-5)],
               lambda case: {"x": tol_allclose_g(0.0, 1e-6)}, present={"x": "pitched"},
               functions=[(_LOSSES, "_SoftmaxCEFn"), (_LAYERS, "_SoftmaxRowsFn")]))
    _add(Entry("categorical_crossentropy_prob" + ("_weighted" if _wt else ""), lambda B, wt=_wt: _cce_build(B, wt, True, 171),
               lambda a: _mod(_LOSSES).categorical_crossentropy(a["y"], a["x"], a["w"]),
               lambda a, _: ref_cce_prob(a["x"], a["y"], a["w"]), ["x"], lambda case: [tol_rel(1e-5)],
               lambda case: {"x": tol_allclose_g(1e-4, 1e-6)}, present={"x": "pitched"}, functions=[(_LOSSES, "_CceProbFn")]))


# ---- retrieval (sbcnm.py).  tests/test_gpu_retrieval.py::test_retrieval_loss_and_gradients: the loss 2e-5 |ref| + 1e-4, dq and dc rtol
# 1e-3, atol 2e-5, against oracle.torch_ref.inbatch_softmax_loss; the explicit [Bq, Nc] path is the same call sequence on the row
# kernels and takes the same bound.  ::test_retrieval_hard_negatives_backward_matches_autograd_oracle: the loss 1e-4 |ref|, the gradients
# rtol 1e-3, atol 5e-5.  The score matrix: tests/test_gpu_helper_kernels.py::test_scores_nt_direct, 4 sqrt(D) u (|a| |b|^T), and its two
# gradient GEMMs as tied_projection's above.  dr_logits_adjust: tests/test_gpu_small_kernels.py, min(g(3) + 4 yard, 1e-6) of the sum of
# the terms' magnitudes; its gradient is the incoming one, unchanged.
MIN_FLOAT = float(np.finfo(np.float32).min / 100.0)
MAX_FLOAT = float(np.finfo(np.float32).max / 100.0)
HARD_GAP = 64.0                                              # the selection's margin, in forward bounds of scores_nt


def _ret_build(B, Nc, extras, seed, D=6):
    g = _g(seed)
    case = dict(q=_rn(g, B, D), c=_rn(g, Nc, D), w=None, cp=None, ci=None, temperature=None)
    if extras:
        case.update(w=torch.rand(B, generator=g) + 0.5, cp=torch.rand(Nc, generator=g) * 0.85 + 0.05,
                    ci=torch.randint(0, max(2, Nc // 3), (Nc,), generator=g), temperature=0.7)
    return case


def _ret_args(a):
    return a["q"], a["c"], a["w"], a["cp"], a["ci"], 1.0 if a["temperature"] is None else 1.0 / a["temperature"]


def _ret_ref(a, _):
    return _T().inbatch_softmax_loss(a["q"], a["c"], a["w"], a["cp"], a["ci"], a["temperature"])


def ref_adjust(scores, labels, cp, ci):
    """dr_logits_adjust on eye labels: scores - log p_j + (dup_ij - labels_ij) MIN_FLOAT, dup_ij = [id_j == id_i]"""
    if cp is not None:
        scores = scores - torch.log(cp)
    if ci is not None:
        scores = scores + ((ci[:scores.shape[0], None] == ci[None, :]).to(scores.dtype) - labels) * MIN_FLOAT
    return scores


def ref_hard_negative(q, c, w, cp, ci, temperature, h):
    """sbcnm.py:145-151 restated: scores -> corrections -> the positive and the h highest negatives -> CCE(from_logits, SUM)"""
    labels = torch.eye(q.shape[0], c.shape[0], dtype=q.dtype)
    scores = ref_adjust(q @ c.t(), labels, cp, ci)
    idx = torch.topk(scores.detach() + labels * MAX_FLOAT, min(h + 1, c.shape[0]), dim=1).indices
    s_sel, l_sel = torch.gather(scores, 1, idx), torch.gather(labels, 1, idx)
    if temperature is not None:
        s_sel = s_sel / temperature
    row = torch.logsumexp(s_sel, 1) * l_sel.sum(1) - (s_sel * l_sel).sum(1)
    return (row if w is None else row * w).sum()


def hard_negative_gap(case, h):
    """(the smallest distance, over the rows, between the lowest kept and the highest dropped negative score; the forward bound of
    scores_nt at its largest): the float64 reference and the fp32 kernels select the same columns when the first is a multiple of the
    second"""
    q, c = case["q"].double(), case["c"].double()
    labels = torch.eye(q.shape[0], c.shape[0], dtype=torch.float64)
    s = ref_adjust(q @ c.t(), labels, None if case["cp"] is None else case["cp"].double(), case["ci"])
    neg = torch.sort(s.masked_fill(labels > 0, -float("inf")), dim=1, descending=True).values
    bound = float(4 * math.sqrt(q.shape[1]) * U * (q.abs() @ c.abs().t()).max())
    if neg.shape[1] <= h + 1:                                # every negative is kept (the positive's own slot sorts last)
        return float("inf"), bound
    return float((neg[:, h - 1] - neg[:, h]).min()), bound


def _hard_build(B, extras, h, seed):
    for s in range(seed, seed + 64):                         # the first seed at which every row's selection has the margin
        case = _ret_build(B, B, extras, s)
        gap, bound = hard_negative_gap(case, h)
        if gap >= HARD_GAP * bound:
            break
    assert gap >= HARD_GAP * bound, "no case with a selection margin of %g forward bounds in 64 seeds" % HARD_GAP
    return dict(case, h=h)


_RET_OUT, _RET_GRAD = tol_allclose(2e-5, 0.0, atol=1e-4), tol_allclose_g(1e-3, 2e-5)
for _ex in (False, True):
    _sfx = "_all" if _ex else ""
    _add(Entry("inbatch_softmax" + _sfx, lambda B, ex=_ex: _ret_build(B, B, ex, 180), lambda a: _mod(_SBCNM)._InBatchSoftmaxFn.apply(*_ret_args(a)),
               _ret_ref, ["q", "c"], lambda case: [_RET_OUT], lambda case: {"q": _RET_GRAD, "c": _RET_GRAD}, bit_equal=False,
               present={"q": "pitched", "c": "transposed" if _ex else "pitched"}, functions=[(_SBCNM, "_InBatchSoftmaxFn")]))
    _add(Entry("explicit_softmax" + _sfx, lambda B, ex=_ex: _ret_build(B, B + 3, ex, 181),          # Nc != Bq
               lambda a: _mod(_SBCNM)._ExplicitSoftmaxFn.apply(*_ret_args(a)), _ret_ref, ["q", "c"], lambda case: [_RET_OUT],
               lambda case: {"q": _RET_GRAD, "c": _RET_GRAD}, bit_equal=False,
               present={"q": "pitched", "c": "transposed" if _ex else "pitched"}, functions=[(_SBCNM, "_ExplicitSoftmaxFn")]))
    _add(Entry("hard_negative_softmax" + _sfx, lambda B, ex=_ex: _hard_build(B, ex, 3, 182),
               lambda a: _mod(_SBCNM)._HardNegativeSoftmaxFn.apply(*_ret_args(a), a["h"]),
               lambda a, _: ref_hard_negative(a["q"], a["c"], a["w"], a["cp"], a["ci"], a["temperature"], a["h"]), ["q", "c"],
               lambda case: [tol_rel(1e-4)], lambda case: {"q": tol_allclose_g(1e-3, 5e-5), "c": tol_allclose_g(1e-3, 5e-5)}, bit_equal=False,
               present={"q": "pitched", "c": "transposed" if _ex else "pitched"}, functions=[(_SBCNM, "_HardNegativeSoftmaxFn")]))
for _nm, _pres in (("retrieval_scores", {"q": "pitched", "c": "pitched"}), ("retrieval_scores_transposed", {"c": "transposed"})):
    _add(Entry(_nm, lambda B: _ret_build(B, B + 3, False, 183), lambda a: _mod(_SBCNM)._ScoresFn.apply(a["q"], a["c"]),
               lambda a, _: a["q"] @ a["c"].t(), ["q", "c"], lambda case: [tol_abs(4 * math.sqrt(case["q"].shape[1]) * U)],
               lambda case: {"q": tol_gemm(2e-6, case["c"].shape[0]), "c": tol_gemm(4e-6, case["q"].shape[0])}, bit_equal=False,
               present=_pres, functions=[(_SBCNM, "_ScoresFn")]))


def _adjust_build(B, with_ids, seed):
    g = _g(seed)
    Nc = B + 3
    return dict(scores=_rn(g, B, Nc) * 2, labels=torch.eye(B, Nc), cp=torch.rand(Nc, generator=g) * 0.85 + 0.05,
                ci=torch.randint(0, max(2, Nc // 3), (Nc,), generator=g) if with_ids else None)


def _adjust_tol(case):
    def f(w64, w32, ctx=None):
        mag = case["scores"].double().abs() + torch.log(case["cp"].double()).abs()[None, :]
        if case["ci"] is not None:
            mag = mag + ((case["ci"][:mag.shape[0], None] == case["ci"][None, :]).double() - case["labels"].double()).abs() * abs(MIN_FLOAT)
        return min(gamma(3) + 4 * float(((w32.double() - w64).abs() / mag).max()), 1e-6) * mag
    return [f]


for _ids in (False, True):
    _add(Entry("retrieval_adjust" + ("_ids" if _ids else ""), lambda B, ids=_ids: _adjust_build(B, ids, 184),
               lambda a: _mod(_SBCNM)._AdjustFn.apply(a["scores"], a["labels"], a["cp"], a["ci"]),
               lambda a, _: ref_adjust(a["scores"], a["labels"], a["cp"], a["ci"]), ["scores"], _adjust_tol,
               lambda case: {"scores": tol_rel(0.0)}, present={"scores": "pitched"}, functions=[(_SBCNM, "_AdjustFn")]))

# ---- the CIN layer (xdeepfm.py::_CinFn on dr_cin_fwd / dr_cin_bwd): tests/test_gpu_cin_din.py::test_cin_forward_backward_match_oracle, the
# out bound and the gradients' of cin_pool above
for _act, _bias in ((0, True), (0, False), (2, True), (2, False)):
    _add(Entry("cin_act%d%s" % (_act, "_bias" if _bias else ""),
               lambda B, bias=_bias: {k: v for k, v in _cin_build(B, 2, 3, 4, 3, 190).items() if k in ("x0", "x", "W") or (k == "bias" and bias)},
               lambda a, act=_act: _mod(_XDEEPFM)._CinFn.apply(a["x0"], a["x"], a["W"], a.get("bias"), act),
               lambda a, _, act=_act: __import__("xdeepfm_ref").cin_pool(a["x0"], a["x"], a["W"], a.get("bias"), act)[0], ["x0", "x", "W", "bias"],
               lambda case: _cin_tol_out(case)[:1], lambda case: {k: _CIN_GRAD for k in ("x0", "x", "W", "bias")},
               present={"x0": "pitched", "x": "pitched"}, functions=[(_XDEEPFM, "_CinFn")]))

# ---- DIEN's row dot product and item rows.  tests/test_gpu_small_kernels.py::test_rowdot: g(ceil(D / 64) + 6) sum|a b|; ::test_rows_scale:
# one correctly rounded multiply.  Item rows: a copy forward; backward fp32 atomics into a zeroed table, at most `count` additions into a
# row: g(count) of the summed magnitudes
_add(Entry("row_dot", lambda B: dict(a=_rn(_g(200), B, 5), b=_rn(_g(201), B, 5)), lambda a: _mod(_DIEN)._RowDotFn.apply(a["a"], a["b"]),
           lambda a, _: (a["a"] * a["b"]).sum(1, keepdim=True), ["a", "b"], lambda case: [tol_abs(gamma(7))],
           lambda case: {"a": tol_rel(U), "b": tol_rel(U)}, present={"a": "pitched", "b": "pitched"}, functions=[(_DIEN, "_RowDotFn")]))


def _items_build(B, seed):
    g = _g(seed)
    ids = torch.randint(0, 9, (B,), generator=g)
    if B > 2:
        ids[1] = ids[2] = ids[0]                             # duplicate ids
    return dict(table=_rn(g, 9, 4), ids=ids)


for _how in ("transposed", "pitched"):                       # (never "expanded": a table is no broadcast)
    _add(Entry("item_rows_" + _how, lambda B: _items_build(B, 202), lambda a: _mod(_DIEN)._ItemRowsFn.apply(a["table"], a["ids"]),
               lambda a, _: a["table"][a["ids"]], ["table"], lambda case: [tol_rel(0.0)],
               lambda case: {"table": tol_abs(gamma(int(torch.bincount(case["ids"]).max())))}, bit_equal=False,
               present={"table": _how}, functions=[(_DIEN, "_ItemRowsFn")]))


# ---- DIN's concat: copies and one subtraction or product forward (one rounding); backward a sum of at most two terms, one of them a
# product (g_x + g_int y, g_y - g_int, ...): three roundings of terms each at most sum_blocks |G| times (1 + |x| + |y|).  (The reference
# subtracts, so tol_abs, which needs non-negative coefficients, does not apply.)
def _din_concat_ref(x, y, mode):
    return torch.cat([x, y] + ([x - y] if mode == 1 else [x * y] if mode == 2 else []), dim=1)


def _din_grad_tol(w64, w32, ctx):
    G, D = ctx["G"][0].double().abs(), ctx["case"]["x"].shape[1]
    return gamma(3) * sum(G[:, i:i + D] for i in range(0, G.shape[1], D)) * (1 + ctx["case"]["x"].double().abs() + ctx["case"]["y"].double().abs())


for _mode in (0, 1, 2):
    _add(Entry("din_concat_mode%d" % _mode, lambda B: dict(x=_rn(_g(210), B, 5), y=_rn(_g(211), B, 5)),
               lambda a, mode=_mode: _mod(_DIN)._DinConcatFn.apply(a["x"], a["y"], mode),
               lambda a, _, mode=_mode: _din_concat_ref(a["x"], a["y"], mode), ["x", "y"], lambda case: [tol_rel(U)],
               lambda case: {"x": _din_grad_tol, "y": _din_grad_tol}, present={"x": "pitched", "y": "pitched"},
               functions=[(_DIN, "_DinConcatFn")]))
for _nm, _mode in (("Subtract", 1), ("Multiply", 2)):        # the interacter layers: the sliced third block
    _add(Entry("din_" + _nm.lower(), lambda B: dict(x=_rn(_g(212), B, 5), y=_rn(_g(213), B, 5)),
               lambda a, nm=_nm: getattr(_mod(_DIN), nm)()([a["x"], a["y"]]),
               lambda a, _, mode=_mode: _din_concat_ref(a["x"], a["y"], mode)[:, 10:], ["x", "y"], lambda case: [tol_rel(U)],
               lambda case: {"x": _din_grad_tol, "y": _din_grad_tol}, present={"x": "pitched"}, functions=[(_DIN, "_DinConcatFn")]))


# ---- the multi-task Functions, through a tiny model whose fused parameter storage is loaded from the case's leaves before every call
# (the Function reads the model's buffers; the leaves are the autograd slots, as model.params are).  tests/test_gpu_multitask.py::
# _check_model_parity: outputs 1e-4 max(1, max|ref|), gradients 2e-4 max(1, max|ref|).  Every dW of these models takes a workspace
# (GroupedStack.backward, _MMoEFn.backward), so the partials are combined in a fixed order: bit_equal.
_MT_K, _MT_H, _MT_E, _MT_T, _MT_TU = 3, 4, 3, 2, 3
_MODELS = {}


def _mt_names(kind):
    if kind == "esmm":
        return {"%s/dense%s/%s" % (s, sfx, p): shp for s in ("pCVR", "pCTR")
                for sfx, p, shp in (("", "kernel", (_MT_K, _MT_H)), ("", "bias", (_MT_H,)), ("_1", "kernel", (_MT_H, 1)), ("_1", "bias", (1,)))}
    names = {}
    for e in range(_MT_E):
        sfx = "" if e == 0 else "_%d" % e
        names["mixture_of_experts/dense%s/kernel" % sfx], names["mixture_of_experts/dense%s/bias" % sfx] = (_MT_K, _MT_H), (_MT_H,)
    for t in range(_MT_T):
        names["multi_gate/dense%s/kernel" % ("" if t == 0 else "_%d" % t)] = (_MT_K, _MT_E)
        names.update({"task%d/dense/kernel" % t: (_MT_H, _MT_TU), "task%d/dense/bias" % t: (_MT_TU,),
                      "task%d/dense_1/kernel" % t: (_MT_TU, 1), "task%d/dense_1/bias" % t: (1,)})
    return names


def _mt_build(B, kind, seed):
    g = _g(seed)
    case = dict(x=_rn(g, B, _MT_K))
    for n, shp in _mt_names(kind).items():
        case[n] = _rn(g, *shp) * (0.3 if n.endswith("bias") else 1.0 / math.sqrt(shp[0]))
    return case


def _mt_model(kind, a):
    """the model of `kind` on the leaves' device, built once, its grouped buffers loaded with the case's values"""
    from deep_recommenders_amd import feature_column as fc
    dev = a["x"].device
    if (kind, str(dev)) not in _MODELS:
        mtl = _mod(PKG + ".estimator.models.multi_task_learning")
        cols = [fc.numeric_column("C%d" % i) for i in range(_MT_K)]
        _MODELS[(kind, str(dev))] = mtl.ESMM(cols, [_MT_H], device=dev) if kind == "esmm" else \
            mtl.MMoE(cols, num_tasks=_MT_T, num_experts=_MT_E, expert_hidden_units=[_MT_H], task_hidden_units=[_MT_TU], device=dev)
    model = _MODELS[(kind, str(dev))]
    with torch.no_grad():
        for n in model._order:
            model._views[n].copy_(a[n])
    return model


def _mt_call(kind, a):
    model = _mt_model(kind, a)
    fn = _mod(_ESMM)._ESMMFn if kind == "esmm" else _mod(_MMOE)._MMoEFn
    return tuple(fn.apply(model, a["x"], *[a[n] for n in model._order]))


def _mt_ref(kind, a):
    import multitask_ref as R
    if kind == "esmm":
        return tuple(R._ref_esmm_x(a["x"], a, 2))
    return tuple(R._ref_mmoe_x(a["x"], a, _MT_E, _MT_T, [_MT_H], [_MT_TU]))


for _kind, _fn, _n_out in (("esmm", (_ESMM, "_ESMMFn"), 3), ("mmoe", (_MMOE, "_MMoEFn"), _MT_T)):
    _add(Entry(_kind, lambda B, kind=_kind: _mt_build(B, kind, 220), lambda a, kind=_kind: _mt_call(kind, a),
               lambda a, _, kind=_kind: _mt_ref(kind, a), ["x"] + list(_mt_names(_kind)), lambda case, n=_n_out: [tol_close(1e-4)] * n,
               lambda case, kind=_kind: {k: tol_close(2e-4) for k in ["x"] + list(_mt_names(kind))}, none_when_unused=True, functions=[_fn]))


# which Functions the entries written before the `functions` field run, by the entry's name up to its variant
_CLAIMS = {"fm_second_order": ["_Fm2Fn"], "mlp": ["_MlpFn"], "cross_low_rank": ["_CrossLowRankFn"], "cross": ["_CrossFn"], "dropout": ["_DropoutFn"],
           "tied_projection": ["_TiedProjectionFn"], "embedding_slab": ["_EmbPoolFn"], "lin_fields": ["_LinFieldsFn"],
           "input_layer": ["_GatherColsFn", "_EmbPoolFn"], "gather_cols": ["_GatherColsFn"], "afm_pooling": ["_AfmPoolFn"],
           "pnn_outer": ["_PnnOuterFn"], "dot_interaction": ["_DotInteractFn"], "softmax_rows": ["_SoftmaxRowsFn"], "l2_penalty": ["_L2Fn"],
           "add_residual": ["_AddFn"], "activation": ["_ActFn"], "ffm_interaction": ["_FfmFn"], "ffm_gather": ["_FfmGatherFn"],
           "dice": ["_DiceFn"], "din_interest_pooling": ["_DinPoolFn"], "cin_pool": ["_CinPoolFn"], "cin_stack": ["_CinStackFn"],
           "gru_sequence": ["_GruSeqFn"], "sequence_attention": ["_SeqAttnFn"], "aggregate_sparse": ["_SpmmFn"],
           "aggregate_dense": ["_DenseAggFn"], "global_average_pooling_1d": ["_SpmmFn"], "token_embedding": ["_TokenEmbeddingFn"],
           "add_layer_norm": ["_AddLayerNormFn"], "attention": ["_AttentionFn"]}
for _e in ENTRIES.values():
    if not _e.functions:
        _key = max((k for k in _CLAIMS if _e.name == k or _e.name.startswith(k + "_")), key=len)
        _e.functions = tuple((_LAYERS, c) for c in _CLAIMS[_key])


def package_functions(root=None):
    """[(module, class name)] of every class of the package whose bases name torch.autograd.Function, read with `ast`: nothing is
    imported, so it runs without a GPU"""
    import ast
    import os
    root = root or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), PKG)
    found = []
    for d, _, files in sorted(os.walk(root)):
        for f in sorted(files):
            if not f.endswith(".py"):
                continue
            path = os.path.join(d, f)
            module = ".".join([PKG] + [p for p in os.path.relpath(path, root)[:-3].split(os.sep) if p != "__init__"])
            with open(path) as fh:
                tree = ast.parse(fh.read(), path)
            for node in ast.walk(tree):
                if isinstance(node, ast.ClassDef) and any(ast.unparse(b) in ("torch.autograd.Function", "autograd.Function", "Function")
                                                          for b in node.bases):
                    found.append((module, node.name))
    return found


# The layers whose backward is documented as running in a fixed order are held to bit-equality across layouts (Entry.bit_equal).  The
# others combine partial sums with fp32 atomics, whose order changes from run to run, and are held to the float64 bound only: mlp,
# cross and cross_low_rank (linear_bwd_dw without a workspace) and the embedding backward without a plan (EmbeddingSlab, _LinFieldsFn,
# ffm_gather through K4).


# --------------------------------------------------------------------------------------------------------------------------------------
# the engine
# --------------------------------------------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def abs_case(case):
    return {k: (v.abs() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in case.items()}


def run_layer(entry, case, device, recipes, present=None, frozen=(), seed=0, times=1):
    """The layer on fp32 leaves on `device`, a probe after every output, ONE backward through the recipes' downstream graphs.
    recipes: one recipe per output, None for an output that is not used.  Returns dict(outs, grads, seen, G, leaves); with times > 1
    the same graph is run backward again (retain_graph) and `again` holds the later gradients."""
    leaves, shown = leaves_for(case, entry.diff, torch.float32, device, present, frozen)
    outs = entry.call(shown)
    outs = outs if isinstance(outs, tuple) else (outs,)
    tensors, grads_in, seen, Gs = [], [], [], []
    for k, (o, rec) in enumerate(zip(outs, recipes)):
        if rec is None or o is None or not o.requires_grad:
            Gs.append(None)
            seen.append([])
            continue
        aux = make_aux(tuple(o.shape), 1000 * seed + k, device)
        name, kind, fn, values, strides = rec
        mine = []
        seen.append(mine)
        y = probe(o, None if strides is None else strides(tuple(o.shape)), mine)
        Gs.append(values(tuple(o.shape), aux))
        if kind == "graph":
            tensors.append(fn(y, aux))
            grads_in.append(None)
        else:
            tensors.append(y)
            grads_in.append(fn(aux, tuple(o.shape)))
    result = dict(outs=[None if o is None else o.detach() for o in outs], seen=seen, G=Gs, leaves=leaves, runs=[])
    for _ in range(times):
        for leaf in leaves.values():
            leaf.grad = None
        if tensors:
            torch.autograd.backward(tensors, grads_in, retain_graph=True)
        result["runs"].append({k: (None if leaf.grad is None else leaf.grad.detach().clone()) for k, leaf in leaves.items()})
    result["grads"] = result["runs"][0]
    return result


def _fit(bound, leaf_shape, kind, value):
    """the bound of a gradient, which the tolerance computed in the layer's own layout, in the layout of the leaf it arrives in"""
    if not isinstance(bound, torch.Tensor):
        bound = torch.tensor(float(bound), dtype=torch.float64)
    if kind == "expanded":
        return bound.max() * value.numel()                   # the leaf is one number: its gradient is the sum over the expansion
    if tuple(bound.shape) == tuple(leaf_shape) or bound.dim() == 0:
        return bound
    if kind == "transposed":
        return bound.t()
    if kind == "pitched":
        full = torch.zeros(leaf_shape, dtype=torch.float64)  # beyond the view's columns the gradient is exactly 0
        full[..., :bound.shape[-1]] = bound
        return full
    return bound.expand(leaf_shape)


def check_against_reference(entry, case, res, present=None, forward=True, report=None):
    """forward values and every gradient of `res` (run_layer) within the entry's bounds of the float64 reference; returns the largest
    err / bound per quantity"""
    present = present or {}
    used = [G is not None for G in res["G"]]
    got_outs = [o if o is None else o.cpu() for o in res["outs"]]
    outs64, grads64 = reference(entry, case, res["G"], torch.float64, present, got_outs=got_outs)
    outs32, grads32 = reference(entry, case, res["G"], torch.float32, present, got_outs=got_outs)
    absG = [None if G is None else G.abs() for G in res["G"]]
    outs_abs, grads_abs = reference(entry, abs_case(case), absG, torch.float64, present, got_outs=got_outs)
    ctx = dict(outs64=outs64, outs32=outs32, G=[None if G is None else G.cpu() for G in res["G"]], case=case)
    ratios = {}

    def within(what, got, w64, w32, wabs, tol, kind="plain", value=None):
        if got is None and entry.none_when_unused and not all(used):
            assert float(w64.abs().max()) == 0.0, "%s: %s is missing although a used output depends on it" % (entry.name, what)
            ratios[what] = 0.0
            return
        assert got is not None, "%s: %s is missing" % (entry.name, what)
        got = got.detach().cpu()
        assert tuple(got.shape) == tuple(w64.shape) and got.dtype == torch.float32, "%s: %s is %s %s, expected fp32 %s" % (
            entry.name, what, got.dtype, tuple(got.shape), tuple(w64.shape))
        assert torch.isfinite(got).all(), "%s: %s is not finite" % (entry.name, what)
        view = {"pitched": lambda w: w[..., :value.shape[-1]], "transposed": lambda w: w.t()}.get(kind, lambda w: w)
        bound = tol(view(w64), view(w32), dict(ctx, abs=None if wabs is None else view(wabs)))      # in the layer's own layout
        bound = _fit(bound, w64.shape, kind, value).to(torch.float64)
        err = (got.double() - w64).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
        if float(err.max() if err.numel() else 0.0) == 0.0:
            ratio = 0.0
        ratios[what] = ratio
        assert bool((err <= bound).all()), "%s: %s is off by %.3g of its bound (max |err| %.3g)" % (entry.name, what, ratio, float(err.max()))

    if forward:
        for k, tol in enumerate(entry.tol_out(case)):
            if outs64[k] is not None and res["outs"][k] is not None:
                within("out%d" % k, res["outs"][k], outs64[k], outs32[k], outs_abs[k], tol)
    tols = entry.tol_grad(case)
    for name in entry.diff:
        if case.get(name) is None or name not in grads64:
            continue
        leaf = res["leaves"][name]
        if not leaf.requires_grad:
            assert res["grads"][name] is None, "%s: the frozen %s received a gradient" % (entry.name, name)
            continue
        if not any(used):
            continue
        within("d_" + name, res["grads"][name], grads64[name], grads32[name], grads_abs[name], tols[name], present.get(name, "plain"), case[name])
    if report is not None:
        for k, v in ratios.items():
            report[k] = max(report.get(k, 0.0), v)
    return ratios
