"""BERT on the device: the kernels of csrc/bert.hip, layers.vocab_cross_entropy, the model of keras/models/nlp/bert.py and its
pretrain_step against the float64 restatement of tests/bert_ref.py.

Tolerance (tests/test_gpu_afm.py's rule, as tests/test_gpu_lsplm.py uses it): a tensor's error is normalised by the largest absolute
float64 value, r32 is the same figure for the restatement's own float32 run (the reference is measured, never the kernel) and the
limit is 16 max(r32, 8 u).  Integer results (the dropout mask, dr_mlm_mask) equal the NumPy restatement exactly.  The properties of
the inputs this file relies on are asserted on the CPU in tests/test_bert_cpu.py."""
import math

import numpy as np
import pytest
import torch

import bert_ref as R
import layer_autograd_cases as C
from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops, optim
from deep_recommenders_amd.keras.models.nlp import BERT, BertPretraining      # the feature: without it this file does not import

pytestmark = pytest.mark.gpu
U = R.U
DEV = "cuda"


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def held(name, got, ref64, ref32):
    scale = ref64.abs().max().item()
    got = got.detach().cpu().double()
    assert tuple(got.shape) == tuple(ref64.shape), (name, tuple(got.shape), tuple(ref64.shape))
    assert not torch.isnan(got).any(), name
    if scale == 0:
        assert got.abs().max().item() == 0, name
        return
    r32 = (ref32.double() - ref64).abs().max().item() / scale
    err = (got - ref64).abs().max().item() / scale
    limit = 16 * max(r32, 8 * U)
    print("%s: error %.3g = %.2f max(r32, 8u), %.3f of the limit" % (name, err, err / max(r32, 8 * U), err / limit))
    assert err <= limit, (name, err, limit)


def dev32(t):
    return t.to(torch.float32).to(DEV) if t.is_floating_point() else t.to(DEV)


def pitched(t, extra=4):
    """the same values as a column slice of a wider buffer (row pitch a multiple of 4, NaN beyond the columns)"""
    buf = torch.full(tuple(t.shape[:-1]) + (C.pad4(t.shape[-1]) + extra,), float("nan"), dtype=t.dtype, device=t.device)
    buf[..., :t.shape[-1]] = t
    return buf[..., :t.shape[-1]]


# ---- GELU ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", [False, True], ids=["dense", "pitched"])
@pytest.mark.parametrize("shape", R.GELU_SHAPES, ids=str)
def test_gelu_forward_and_backward(shape, pitch):
    z, dy = R.gelu_case(*shape)
    zd, dyd = dev32(z), dev32(dy)
    if pitch:
        zd, dyd = pitched(zd), pitched(dyd)
    z32 = z.float()
    h = ops.gelu_fwd(zd)
    assert torch.isfinite(h).all()
    held("gelu %s" % (shape,), h, R.gelu(z32.double()), R.gelu(z32))
    kept = zd.clone()
    dz = ops.gelu_bwd_(zd, dyd)
    assert dz.data_ptr() == dyd.data_ptr() and same_bits(zd, kept) and torch.isfinite(dz).all()
    held("gelu' %s" % (shape,), dz, R.gelu_grad(z32.double()) * dy.float().double(), R.gelu_grad(z32) * dy.float())


def test_gelu_saturates_to_finite_values():
    z = torch.tensor([[-88.0, -10.0, 0.0, 10.0, 88.0, -1e-42, 1e-42]], device=DEV)
    h = ops.gelu_fwd(z).cpu()
    assert torch.isfinite(h).all() and float(h[0, 0]) == 0.0 and float(h[0, 4]) == 88.0 and float(h[0, 2]) == 0.0
    d = ops.gelu_bwd_(z, torch.ones_like(z)).cpu()
    assert torch.isfinite(d).all() and float(d[0, 0]) == 0.0 and float(d[0, 4]) == 1.0 and float(d[0, 2]) == 0.5


def _ref_mlp(x, Ws, bs, acts):
    for W, b, a in zip(Ws, bs, acts):
        x = x @ W + b
        x = R.gelu(x) if a == 4 else C.ACT[a](x)
    return x


def _gelu_mlp_entry(widths, acts):
    """tests/layer_autograd_cases.py's _mlp_entry with GELU in the reference"""
    n = len(acts)
    diff = ["x"] + ["W%d" % i for i in range(n)] + ["b%d" % i for i in range(n)]

    def tol_grad(case):
        M = case["x"].shape[0]
        t = {"x": C.tol_gemm(2e-6, max(widths), n)}
        for i in range(n):
            t["W%d" % i] = C.tol_gemm(4e-6, M, n - i)
            t["b%d" % i] = C.tol_allclose(0.0, 0.0, atol=(n - i) * 1e-5 * math.sqrt(M) * 4)
        return t
    return C.Entry("mlp_gelu_%s" % (acts,), lambda B: C._mlp_build(B, widths, acts, 11), lambda a: L.mlp(a["x"], *C._mlp_parts(a), a["acts"]),
                   lambda a, _: _ref_mlp(a["x"], *C._mlp_parts(a), a["acts"]), diff, lambda case: [C.tol_gemm(2e-6, max(widths), n)],
                   tol_grad, bit_equal=False)


@pytest.mark.parametrize("acts", [(4, 0), (0, 4)], ids=str)
@pytest.mark.parametrize("B", C.BATCHES)
def test_mlp_with_gelu_in_every_gradient_layout(acts, B):
    entry = _gelu_mlp_entry((7, 10, 5), acts)
    case = entry.build(B)
    for k, rec in enumerate(C.recipes_for(2)):
        res = C.run_layer(entry, case, DEV, [rec], seed=B)
        C.check_against_reference(entry, case, res, forward=k == 0)
    res = C.run_layer(entry, case, DEV, [C.recipe_named(2, "base")], frozen=("x",), seed=B)
    assert res["grads"]["x"] is None
    C.check_against_reference(entry, case, res, forward=False)
    pres = {"x": "pitched"}
    res = C.run_layer(entry, case, DEV, [C.recipe_named(2, "hand")], present=pres, seed=B)
    C.check_against_reference(entry, case, res, present=pres)


def test_mlp_relu_tower_is_the_composition_of_its_kernels():
    """codes 0-3 keep their path: acts (1, 0) equals linear_fwd / linear_bwd_dw / linear_bwd_dx composed by hand, bit for bit"""
    case = C._mlp_build(70, (7, 10, 5), (1, 0), 11)
    x, W0, b0, W1, b1 = (dev32(case[k]) for k in ("x", "W0", "b0", "W1", "b1"))
    leaves = [t.clone().requires_grad_(True) for t in (x, W0, b0, W1, b1)]
    y = L.mlp(leaves[0], [leaves[1], leaves[3]], [leaves[2], leaves[4]], (1, 0))
    dy = torch.randn(70, 5, device=DEV)
    y.backward(dy)
    h = ops.linear_fwd(x, W0, b0, 1)
    want = ops.linear_fwd(h, W1, b1, 0)
    assert same_bits(y.detach(), want)
    gW1, gb1 = torch.zeros_like(W1), torch.zeros_like(b1)
    ops.linear_bwd_dw(h, dy, 1.0, gW1, gb1)
    dh = ops.linear_bwd_dx(dy, W1, h)
    gW0, gb0 = torch.zeros_like(W0), torch.zeros_like(b0)
    ops.linear_bwd_dw(x, dh, 1.0, gW0, gb0)
    dx = ops.linear_bwd_dx(dh, W0, None)
    assert same_bits(leaves[0].grad, dx)
    for got, want in zip([t.grad for t in leaves[1:]], (gW0, gb0, gW1, gb1)):      # dW may combine its K slices with fp32 atomics
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)


# ---- embedding ----------------------------------------------------------------------------------------------------------------------
def _embed_ref(c, dtype, rate, seed):
    tok, pos, seg, gamma, beta = (c[k].float().to(dtype).requires_grad_(True) for k in ("tok", "pos", "seg", "gamma", "beta"))
    s = R.embed_sum(c["ids"], c["segment"], tok, pos, seg)
    s.retain_grad()
    y, mean, rstd = R.layer_norm(s, gamma, beta)
    out = R.dropout(y, R.keep_mask(seed, y.numel(), rate), rate)
    (out * c["d_out"].float().to(dtype)).sum().backward()
    Ln = c["ids"].shape[1]
    return dict(out=out.detach(), mean=mean.detach().reshape(-1), rstd=rstd.detach().reshape(-1), d_s=s.grad.reshape(-1, s.shape[-1]),
                d_tok=tok.grad, d_pos=pos.grad[:Ln], d_seg=seg.grad, d_gamma=gamma.grad, d_beta=beta.grad)


@pytest.mark.parametrize("rate", [0.0, 0.1])
@pytest.mark.parametrize("equal_ids", [False, True], ids=["mixed", "equal"])
@pytest.mark.parametrize("shape", R.EMBED_SHAPES, ids=str)
def test_bert_embedding_forward_and_backward(shape, equal_ids, rate):
    B, Ln, D, V, T = shape
    c = R.embed_case(*shape, equal_ids=equal_ids)
    seed = 17
    r64, r32 = _embed_ref(c, torch.float64, rate, seed), _embed_ref(c, torch.float32, rate, seed)
    g = {k: dev32(v) for k, v in c.items()}
    g["tok"][V - 1] = float("nan")                                          # a row nobody references is never read
    out, stats = ops.bert_embed_fwd(g["ids"], g["segment"], g["tok"], g["pos"], g["seg"], g["gamma"], g["beta"], R.LN_EPS, rate, seed)
    tag = "%s rate %g" % (shape, rate)
    held("embed out " + tag, out, r64["out"], r32["out"])
    held("mean " + tag, stats[:, 0], r64["mean"], r32["mean"])
    held("rstd " + tag, stats[:, 1], r64["rstd"], r32["rstd"])
    keep = torch.from_numpy(R.keep_mask(seed, out.numel(), rate)).reshape(out.shape)
    assert torch.equal(out.cpu() != 0, keep & (r64["out"] != 0))              # the mask is the NumPy hash exactly

    def backward():
        d_tok = torch.zeros((V, D), dtype=torch.float32, device=DEV)
        return ops.bert_embed_bwd(g["ids"], g["segment"], g["tok"], g["pos"], g["seg"], g["gamma"], stats, g["d_out"], d_tok, rate,
                                  seed) + (d_tok,)
    d_s, d_gamma, d_beta, d_pos, d_seg, d_tok = backward()
    for name, got in (("d_s", d_s), ("d_gamma", d_gamma), ("d_beta", d_beta), ("d_pos", d_pos), ("d_seg", d_seg), ("d_tok", d_tok)):
        held("%s %s" % (name, tag), got, r64[name], r32[name])
    again = backward()
    for a, b in zip(again, (d_s, d_gamma, d_beta, d_pos, d_seg, d_tok)):
        assert same_bits(a, b)
    start = torch.randn((V, D), device=DEV)                                 # d_tok accumulates
    start[V - 1] = 0
    acc = start.clone()
    ops.bert_embed_bwd(g["ids"], g["segment"], g["tok"], g["pos"], g["seg"], g["gamma"], stats, pitched(g["d_out"].reshape(B * Ln, D)), acc,
                       rate, seed)
    held("d_tok accumulated " + tag, acc, start.cpu().double() + r64["d_tok"], start.cpu() + r32["d_tok"])


def test_bert_embedding_refuses_what_it_cannot_address():
    c = {k: dev32(v) for k, v in R.embed_case(3, 5, 20, 7, 2).items()}
    args = lambda **kw: [kw.get(k, c[k]) for k in ("ids", "segment", "tok", "pos", "seg", "gamma", "beta")]      # noqa: E731
    with pytest.raises(ValueError, match="ids"):
        ops.bert_embed_fwd(*args(ids=c["ids"].t().contiguous().t()))
    with pytest.raises(ValueError, match="segment"):
        ops.bert_embed_fwd(*args(segment=c["segment"].to(torch.int32)))
    with pytest.raises(ValueError, match="tok"):
        ops.bert_embed_fwd(*args(tok=pitched(c["tok"])))
    with pytest.raises(ValueError, match="max_position"):
        ops.bert_embed_fwd(*args(pos=c["pos"][:4].contiguous()))


# ---- softmax cross-entropy over integer labels --------------------------------------------------------------------------------------
ROW_SCALE, DENOM_EPS = 0.25, 1e-5
CE_CONFIGS = [(0.0, True, False), (0.1, True, True), (0.1, False, False)]     # (smoothing, with bias / weight / denom, pitched)


@pytest.mark.parametrize("M", R.CE_ROWS)
@pytest.mark.parametrize("C_", R.CE_COLS)
def test_softmax_ce_ids(C_, M):
    c = R.ce_case(M, C_)
    for smoothing, full, pitch in CE_CONFIGS:
        opt = (lambda t, dt: None if not full else t.float().to(dt))
        refs = [R.softmax_ce_ids(c["logits"].float().to(dt), opt(c["bias"], dt), c["labels"], opt(c["weight"], dt), smoothing, ROW_SCALE,
                                 opt(c["denom"], dt), DENOM_EPS) for dt in (torch.float64, torch.float32)]
        logits = dev32(c["logits"])
        pad = (c["labels"] < 0).to(DEV)
        logits[pad] = float("nan")                                          # a padding row is never read
        bias, weight = (dev32(c[k]) if full else None for k in ("bias", "weight"))
        denom = dev32(c["denom"]).reshape(1) if full else None
        labels = c["labels"].to(DEV)

        def run(path, pitch=pitch):
            x = pitched(logits) if pitch else logits.clone()
            loss = ops.softmax_ce_ids(x, labels, bias, weight, smoothing, ROW_SCALE, denom, DENOM_EPS, _path=path)
            return loss, x
        loss, g = run(0)
        tag = "C %d M %d eps %g %s" % (C_, M, smoothing, "full" if full else "bare")
        held("loss " + tag, loss, refs[0][0], refs[1][0])
        held("g " + tag, g, refs[0][1], refs[1][1])
        assert int(bits(loss[pad]).abs().sum()) == 0 and int(bits(g[pad]).abs().sum()) == 0       # exact +0.0
        # a gradient row sums to 0 exactly; an element g_j = coef (e_j / sum - eps / C - hit) carries at most 8 u coef of error (expf
        # within an ulp = 2 u, the sum and the division another 2 u on a value <= 1, three roundings of values <= 1, the product):
        # C elements are within C u scale with scale = 8 coef
        scale = 8 * ROW_SCALE * (c["weight"] if full else torch.ones(M, dtype=torch.float64)) / ((c["denom"] + DENOM_EPS) if full else 1.0)
        sums = g.cpu().double().sum(1).abs()
        assert bool((sums <= C_ * U * scale).all()), (tag, float((sums / (C_ * U * scale)).max()))
        if C_ <= R.LDS_COLS:                                                # the two paths give the same bits
            (l1, g1), (l2, g2) = run(1), run(2)
            assert same_bits(l1, l2) and same_bits(g1, g2) and same_bits(l1, loss) and same_bits(g1, g)
        else:
            with pytest.raises(ValueError):
                run(1)
            l2, g2 = run(2)
            assert same_bits(l2, loss) and same_bits(g2, g)


def test_softmax_ce_ids_names_the_argument_it_refuses():
    logits, labels = torch.zeros(4, 6, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="logits"):
        ops.softmax_ce_ids(torch.zeros(6, 4, device=DEV).t(), labels)
    with pytest.raises(ValueError, match="labels"):
        ops.softmax_ce_ids(logits, labels.to(torch.int32))
    with pytest.raises(ValueError, match="bias"):
        ops.softmax_ce_ids(logits, labels, bias=torch.zeros(12, device=DEV)[::2])
    with pytest.raises(ValueError, match="weight"):
        ops.softmax_ce_ids(logits, labels, weight=torch.zeros(4, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="denom"):
        ops.softmax_ce_ids(logits, labels, denom=torch.zeros(2, device=DEV))
    assert float(logits.abs().sum()) == 0                                   # nothing was launched


def test_colsum_add_accumulates_in_a_fixed_order():
    g = torch.randn(70, 257, device=DEV)
    start = torch.randn(257, device=DEV)
    a, b = start.clone(), start.clone()
    ops.colsum_add(pitched(g), a)
    ops.colsum_add(g, b)
    assert same_bits(a, b)
    want = start.cpu().double() + g.cpu().double().sum(0)
    assert float((a.cpu().double() - want).abs().max()) <= 70 * U * float(g.abs().sum(0).max() + start.abs().max())


# ---- vocab_cross_entropy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [20, 768])
def test_vocab_cross_entropy_chunked(D):
    M, V = 70, 257
    g = torch.Generator().manual_seed(D)
    t = torch.randn(M, D, generator=g, dtype=torch.float64).float()
    table = (torch.randn(V, D, generator=g, dtype=torch.float64) / math.sqrt(D)).float()
    bias = torch.randn(V, generator=g, dtype=torch.float64).float()
    labels = torch.randint(0, V, (M,), generator=g)
    labels[3], labels[69] = -1, -1
    weight = (torch.rand(M, generator=g, dtype=torch.float64) + 0.5).float()
    denom = weight.double().sum().float()
    t0, b0 = torch.randn(V, D, generator=g).float(), torch.randn(V, generator=g).float()
    assert float((t.double() @ table.double().t() + bias.double()).abs().max()) < 80
    refs = []
    for dt in (torch.float64, torch.float32):
        loss, d_t, d_table, d_bias = R.vocab_cross_entropy(t.to(dt), table.to(dt), bias.to(dt), labels, weight.to(dt), 0.1, 1.0, denom.to(dt),
                                                           DENOM_EPS)
        refs.append((loss, d_t, t0.to(dt) + d_table, b0.to(dt) + d_bias))
    td, tabled, biasd, labelsd, weightd, denomd = (x.to(DEV) for x in (t, table, bias, labels, weight, denom.reshape(1)))

    def run(chunk_rows):
        d_table, d_bias = t0.to(DEV), b0.to(DEV)
        loss, d_t = L.vocab_cross_entropy(td, tabled, biasd, labelsd, weightd, 0.1, 1.0, denomd, DENOM_EPS, d_table, d_bias, chunk_rows)
        return loss, d_t, d_table, d_bias
    for chunk_rows in (70, 7):
        got = run(chunk_rows)
        for name, x, r64, r32 in zip(("loss", "d_t", "d_table", "d_bias"), got, refs[0], refs[1]):
            held("vocab_ce D %d chunk %d %s" % (D, chunk_rows, name), x, r64, r32)
        for a, b in zip(run(chunk_rows), got):                              # run to run: the same bits
            assert same_bits(a, b)
    loss, d_t, _, _ = run(None)
    assert same_bits(loss, got[0]) and same_bits(d_t, got[1])               # per-row results do not depend on the chunking


def test_vocab_cross_entropy_takes_the_table_in_blocks(monkeypatch):
    """the deterministic dW's workspace is bounded by taking the table's rows in blocks: the same values, block by block"""
    M, V, D = 70, 2600, 20
    g = torch.Generator().manual_seed(1)
    t, table = torch.randn(M, D, generator=g).to(DEV), (torch.randn(V, D, generator=g) / math.sqrt(D)).to(DEV)
    labels = torch.randint(0, V, (M,), generator=g).to(DEV)

    def run():
        d_table, d_bias = torch.zeros(V, D, device=DEV), torch.zeros(V, device=DEV)
        return L.vocab_cross_entropy(t, table, None, labels, d_table=d_table, d_bias=d_bias) + (d_table, d_bias)
    whole = run()
    monkeypatch.setattr(L, "VOCAB_CE_WORKSPACE_BYTES", 1)
    blocked = run()
    for k in (0, 1, 3):
        assert same_bits(whole[k], blocked[k])                              # per-row results and the bias gradient do not see the blocks
    assert same_bits(run()[2], blocked[2])                                  # run to run
    r = R.vocab_cross_entropy(t.cpu().double(), table.cpu().double(), None, labels.cpu(), None, 0.0, 1.0, None, 0.0)
    r32 = R.vocab_cross_entropy(t.cpu(), table.cpu(), None, labels.cpu(), None, 0.0, 1.0, None, 0.0)
    held("blocked d_table", blocked[2], r[2], r32[2])


def test_rows_wider_than_the_gather_kernels_take_go_in_pieces():
    from deep_recommenders_amd.keras.models.nlp import bert as B
    mat = torch.randn(40, 768, device=DEV)
    rows = torch.tensor([3, 0, 39, 3, 17], device=DEV)
    assert torch.equal(B._gather_rows(rows, mat), mat[rows])
    acc = torch.zeros_like(mat)
    grads = torch.randn(4, 768, device=DEV)
    B._scatter_rows_add(rows[[0, 1, 2, 4]], grads, acc)
    want = torch.zeros_like(mat)
    want[rows[[0, 1, 2, 4]]] = grads
    assert torch.equal(acc, want)


# ---- masking ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", R.MASK_PS)
@pytest.mark.parametrize("Ln", R.MASK_LENGTHS)
def test_mlm_mask_equals_the_numpy_restatement(Ln, P):
    ids = R.mask_case(Ln)
    for prob in R.MASK_PROBS:
        for seed in (11, 2 ** 64 - 1):
            want = R.mlm_mask(ids, R.MASK_V, R.MASK_SPECIAL, R.MASK_ID, prob, P, seed)
            got = ops.mlm_mask(torch.from_numpy(ids).to(DEV), R.MASK_V, R.MASK_SPECIAL, R.MASK_ID, prob, P, seed)
            for a, b in zip(got, want):
                a = a.cpu().numpy()
                assert a.dtype == b.dtype and np.array_equal(a, b), (Ln, P, prob, seed)


def test_mlm_mask_refuses_what_is_outside_its_domain():
    ids = torch.full((2, 513), 9, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        ops.mlm_mask(ids, 300, 5, 4)
    with pytest.raises(ValueError, match="ids"):
        ops.mlm_mask(ids[:, :8:2], 300, 5, 4)
    with pytest.raises(ValueError):
        ops.mlm_mask(ids[:, :8].contiguous(), 300, 5, 4, max_predictions=129)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def _model(cfg, params, hidden_dropout=0.0, attention_dropout=0.0):
    bert = BERT(cfg["V"], cfg["D"], cfg["layers"], cfg["H"], cfg["F"], cfg["max_position"], cfg["T"], hidden_dropout, attention_dropout,
                seed=3)
    head = BertPretraining(bert, cfg["num_special"], cfg["mask_id"])
    head.load_state_dict({k: v.float().to(DEV) for k, v in params.items()})
    return head


def _small_batch(cfg):
    ids, seg, nsp = R.tiny_batch(0, cfg)
    ids[1, -1] = 0                                                          # one padded key
    out, positions, labels = R.mlm_mask(ids, cfg["V"], cfg["num_special"], cfg["mask_id"], 0.3, cfg["P"], seed=5)
    return tuple(torch.from_numpy(a) for a in (out, seg, positions, labels, nsp))


def test_model_forward_and_every_gradient_of_a_pretrain_step():
    cfg = dict(R.TINY, B=2, L=8)
    params = {k: v.float() for k, v in R.tiny_params(cfg, seed=1, dtype=torch.float64).items()}
    g = torch.Generator().manual_seed(9)
    for k in params:                                                        # biases and norms away from their initial 0 / 1
        params[k] = params[k] + 0.1 * torch.randn(params[k].shape, generator=g)
    ids, seg, positions, labels, nsp = _small_batch(cfg)
    assert int((labels >= 0).sum()) >= 2 and int((labels < 0).sum()) >= 1
    head = _model(cfg, params)
    p64, p32 = {k: v.double() for k, v in params.items()}, params
    seq, pooled = head.bert(ids.to(DEV), seg.to(DEV))
    for dt, p in ((torch.float64, p64),):
        s64, o64 = R.bert_forward(p, ids, seg, None, cfg["layers"], cfg["H"])
    s32, o32 = R.bert_forward(p32, ids, seg, None, cfg["layers"], cfg["H"])
    held("sequence_output", seq, s64, s32), held("pooled_output", pooled, o64, o32)
    m64, n64, g64 = R.pretrain_grads(p64, ids, seg, positions, labels, nsp, cfg["layers"], cfg["H"])
    m32, n32, g32 = R.pretrain_grads(p32, ids, seg, positions, labels, nsp, cfg["layers"], cfg["H"])
    opt = torch.optim.SGD(head.parameters(), lr=0.0)                        # a step that leaves the parameters and keeps the gradients
    mlm, nsp_loss = head.pretrain_step(ids.to(DEV), seg.to(DEV), nsp.to(DEV), opt, masked=(ids.to(DEV), positions.to(DEV), labels.to(DEV)))
    held("mlm_loss", mlm.reshape(1), m64.reshape(1), m32.reshape(1)), held("nsp_loss", nsp_loss.reshape(1), n64.reshape(1), n32.reshape(1))
    lm, ln_ = head.losses(ids.to(DEV), seg.to(DEV), positions.to(DEV), labels.to(DEV), nsp.to(DEV))
    held("losses() mlm", lm.reshape(1), m64.reshape(1), m32.reshape(1)), held("losses() nsp", ln_.reshape(1), n64.reshape(1), n32.reshape(1))
    named = dict(head.named_parameters())
    assert set(named) == set(g64)
    for k in sorted(named):
        assert named[k].grad is not None, k
        held("d_" + k, named[k].grad, g64[k], g32[k])


def test_pretrain_step_with_dropout_is_reproducible_and_masks_on_the_device():
    cfg = dict(R.TINY, B=2, L=8)
    params = R.tiny_params(cfg, seed=1)
    ids, seg, nsp = (torch.from_numpy(a).to(DEV) for a in R.tiny_batch(0, cfg))
    head = _model(cfg, params, 0.1, 0.1)
    opt = torch.optim.SGD(head.parameters(), lr=0.0)
    runs = []
    for _ in range(2):
        head.bert.reset_calls()
        head._mask_calls = 0
        losses_ = head.pretrain_step(ids, seg, nsp, opt, prob=0.3, max_predictions=cfg["P"])
        runs.append([x.clone() for x in losses_] + [p.grad.clone() for _, p in sorted(head.named_parameters())])
    assert head.bert.last_seeds is not None and head.bert.get_config()["hidden_size"] == cfg["D"]
    for a, b in zip(*runs):
        assert same_bits(a.reshape(-1), b.reshape(-1))
    off = _model(cfg, params)
    off.bert.reset_calls()
    a = off.pretrain_step(ids, seg, nsp, torch.optim.SGD(off.parameters(), lr=0.0), prob=0.3, max_predictions=cfg["P"])
    assert not same_bits(a[0].reshape(1), runs[0][0].reshape(1))            # dropout did something


def test_training_on_the_tiny_task_learns():
    cfg = R.TINY
    ref_final = R.final_loss(R.tiny_training(cfg))
    uniform = math.log(cfg["V"] - cfg["num_special"])
    head = _model(cfg, R.tiny_params(cfg))
    opt = optim.Adam(head.parameters(), lr=cfg["lr"])
    hist = []
    for step in range(cfg["steps"]):
        ids, seg, positions, labels, nsp = (torch.from_numpy(a).to(DEV) for a in R.tiny_masked(step, cfg))
        mlm, _ = head.pretrain_step(ids, seg, nsp, opt, masked=(ids, positions, labels))
        hist.append(mlm)
    hist = torch.stack(hist).cpu()
    final = float(hist[-10:].mean())
    midpoint = 0.5 * (ref_final + uniform)
    print("tiny task: masked-LM loss %.4f -> %.4f; restatement %.4f, uniform %.4f, midpoint %.4f" % (float(hist[0]), final, ref_final, uniform,
                                                                                                   midpoint))
    assert final < midpoint
