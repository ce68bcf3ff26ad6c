"""LS-PLM on the device: the kernels of csrc/lsplm.hip, the model and its train_step against the float64 restatement of
tests/lsplm_ref.py.

On integer grids with bags of 0, 1, 2 and 4 ids z equals float64 bit for bit, and every field block of d_rows equals d_z bit for bit.
p, q, loss and d_z: each tensor's error is normalised by the largest absolute float64 value, r32 is the same figure for the restatement's
own float32 run (the reference is measured, never the kernel) and the limit is 16 max(r32, 8 u): tests/test_gpu_afm.py's rule, whose
docstring gives the evidence for the factor 16.  The inputs keep the float64 p and q inside [1e-4, 1 - 1e-4] (asserted on the reference
in tests/test_lsplm_cpu.py).  p + q is within (m + 8) u of 1: sg and sn share one exponential, so their sum is 1 to a rounding."""
import math

import pytest
import torch

import lsplm_ref as R
from deep_recommenders_amd import feature_column as fc
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.ranking import LSPLM                  # the feature: without it this file does not import

pytestmark = pytest.mark.gpu
U = R.U
CASES = [(s, bags) for s in R.SHAPES for bags in (False, True)]
ROW_SCALE = 0.25
_CASES = {}


def case(shape, bags, grid=False):
    """one shape's inputs and float64 / float32 results of the restatement, computed once and left unchanged"""
    key = (shape, bags, grid)
    if key not in _CASES:
        c = R.make_case(*shape, bags=bags, grid=grid)
        B, F, m = shape
        for tag, dt in (("64", torch.float64), ("32", torch.float32)):
            z = R.pool(c["table"].to(dt), c["bias"].to(dt), c["fields"], c["row_base"])
            p, q, _, _ = R.head(z)
            y, wt = c["labels"].to(dt), c["wt"].to(dt)
            c[tag] = {"z": z, "p": p, "q": q, "loss": R.loss_rows(p, q, y, wt), "d_z": R.dz_closed_form(z, c["d_p"].to(dt)),
                      "d_z_loss": R.dz_closed_form(z, R.dp_of_loss(p, q, y, wt, ROW_SCALE))}
        used = torch.zeros(c["table"].shape[0], dtype=torch.bool)
        for f, ids in enumerate(c["fields"]):
            used[(ids + c["row_base"][f])[ids >= 0]] = True
        t = c["table"].float().clone()
        t[~used] = float("nan")                                            # a row nobody references is never read
        c["g"] = {"table": t.cuda(), "bias": c["bias"].float().cuda(), "ids": c["ids"].cuda(), "row_base": c["row_base"].cuda(),
                  "col_start": None if c["col_start"] is None else c["col_start"].cuda(), "labels": c["labels"].float().cuda(),
                  "wt": c["wt"].float().cuda(), "d_p": c["d_p"].float().cuda()}
        _CASES[key] = c
    return _CASES[key]


def bits(t):
    return t.contiguous().view(torch.int32)


def fwd(c, **kw):
    g, (B, F, m) = c["g"], c["shape"]
    return ops.lsplm_fwd(g["ids"], F, g["col_start"], g["row_base"], g["table"], m, g["bias"], **kw)


def loss_fwd(c, **kw):
    g, (B, F, m) = c["g"], c["shape"]
    return ops.lsplm_loss_fwd(g["ids"], F, g["col_start"], g["row_base"], g["table"], m, g["bias"], g["labels"], g["wt"], ROW_SCALE, **kw)


def held(name, x, c, key):
    ref, x32 = c["64"][key], c["32"][key]
    scale = ref.abs().max().item()
    assert scale > 0, name
    r32 = (x32.double() - ref).abs().max().item() / scale
    x = x.cpu().double()
    assert not torch.isnan(x).any(), name
    err = (x - ref).abs().max().item() / scale
    limit = 16 * max(r32, 8 * U)
    print("%s %s: error %.3g = %.2f max(r32, 8u), %.3f of the limit" % (name, c["shape"], err, err / max(r32, 8 * U), err / limit))
    assert err <= limit, (name, err, limit)


@pytest.mark.parametrize("shape, bags", CASES, ids=str)
def test_forward_backward_and_the_one_pass_form(shape, bags):
    c = case(shape, bags)
    g, (B, F, m) = c["g"], shape
    W = 2 * m
    p, q, z = fwd(c)
    held("z", z, c, "z"), held("p", p, c, "p"), held("q", q, c, "q")
    assert ((p.cpu().double() + q.cpu().double()) - 1).abs().max().item() <= (m + 8) * U
    d_z, d_rows = ops.lsplm_bwd(z, F, m, g["d_p"])
    held("d_z", d_z, c, "d_z")
    for f in range(F):                                                     # F copies, bit for bit
        assert torch.equal(bits(d_rows[:, f * W:(f + 1) * W]), bits(d_z)), f
    p1, q1, loss, d_z1, d_rows1 = loss_fwd(c)
    held("loss", loss, c, "loss"), held("d_z of the loss", d_z1, c, "d_z_loss")
    assert torch.equal(bits(p1), bits(p)) and torch.equal(bits(q1), bits(q))
    # the one-pass form against fwd + bwd on the d_p it documents: (row_scale * wt) * (-y / p + (1 - y) / q), fp32 as the kernel rounds it
    y, wt = g["labels"], g["wt"]
    coeff = torch.where(y != 0, -y / p, torch.zeros_like(p)) + torch.where(y != 1, (1 - y) / q, torch.zeros_like(p))
    d_p = (torch.tensor(ROW_SCALE, dtype=torch.float32, device="cuda") * wt) * coeff
    d_z2, d_rows2 = ops.lsplm_bwd(z, F, m, d_p)
    assert torch.equal(bits(d_z2), bits(d_z1)) and torch.equal(bits(d_rows2), bits(d_rows1))
    # no sample weights: wt = 1
    _, _, loss_u, _, _ = ops.lsplm_loss_fwd(g["ids"], F, g["col_start"], g["row_base"], g["table"], m, g["bias"], g["labels"])
    ref = R.loss_rows(c["64"]["p"], c["64"]["q"], c["labels"])
    assert (loss_u.cpu().double() - ref).abs().max().item() <= 16 * 8 * U * max(1.0, ref.abs().max().item()) + \
        16 * (c["32"]["loss"].double() - c["64"]["loss"]).abs().max().item()
    # the bias gradient: the column sum of d_z in a fixed order
    db = ops.lsplm_bias_grad(d_z1, m)
    want = d_z1.cpu().double().sum(0)
    assert (db.cpu().double() - want).abs().max().item() <= R.U * B * d_z1.cpu().double().abs().sum(0).max().item() + 1e-30
    assert torch.equal(bits(ops.lsplm_bias_grad(d_z1, m)), bits(db))


@pytest.mark.parametrize("shape, bags", CASES, ids=str)
def test_integer_grids_give_z_bit_for_bit(shape, bags):
    c = case(shape, bags, grid=True)
    _, _, z = fwd(c)
    assert torch.equal(z.cpu().double(), c["64"]["z"])


@pytest.mark.parametrize("shape, bags", CASES, ids=str)
def test_run_to_run_slices_and_sentinels(shape, bags):
    c = case(shape, bags)
    g, (B, F, m) = c["g"], shape
    W = 2 * m
    a, b = loss_fwd(c), loss_fwd(c)
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))
    p, q, loss, d_z, d_rows = a
    lo, hi = (B // 3, B - B // 4) if B > 2 else (B - 1, B)
    s = ops.lsplm_loss_fwd(g["ids"][lo:hi].contiguous(), F, g["col_start"], g["row_base"], g["table"], m, g["bias"],
                           g["labels"][lo:hi].contiguous(), g["wt"][lo:hi].contiguous(), ROW_SCALE)
    for x, y in zip(s, a):
        assert torch.equal(bits(x), bits(y[lo:hi]))
    S = -7.5
    pad = lambda cols: torch.full((B + 1, cols + 8), S, dtype=torch.float32, device="cuda")
    z_p, dz_p, dr_p = pad(W), pad(W), pad(F * W)
    p2, q2, _ = fwd(c, z=z_p[:B, :W])
    loss_fwd(c, d_z=dz_p[:B, :W], d_rows=dr_p[:B, :F * W])
    assert torch.equal(bits(p2), bits(p)) and torch.equal(bits(q2), bits(q))
    assert torch.equal(bits(dz_p[:B, :W]), bits(d_z)) and torch.equal(bits(dr_p[:B, :F * W]), bits(d_rows))
    dz_b, dr_b = pad(W), pad(F * W)
    ops.lsplm_bwd(z_p[:B, :W], F, m, g["d_p"], d_z=dz_b[:B, :W], d_rows=dr_b[:B, :F * W])
    for buf, cols in ((z_p, W), (dz_p, W), (dr_p, F * W), (dz_b, W), (dr_b, F * W)):
        assert (buf[:B, cols:] == S).all() and (buf[B] == S).all()
    # z is optional
    p3, q3, z3 = fwd(c, want_z=False)
    assert z3 is None and torch.equal(bits(p3), bits(p))


def test_saturated_rows_with_labels_of_exactly_0_and_1_produce_no_nan():
    m, F = 4, 1
    table = torch.zeros(4, 2 * m)
    table[0, m:] = 200.0                                                   # every expert says 1: q = 0
    table[1, m:] = -200.0                                                  # every expert says 0: p = 0
    table[2, :m] = torch.tensor([300.0, -300.0, 0.0, 0.0])                 # a saturated gate
    table[3, m:] = torch.tensor([200.0, -200.0, 200.0, -200.0])
    ids = torch.tensor([[0], [1], [2], [3], [0], [1]]).cuda()
    y = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0, 1.0]).cuda()                # the last two: the label the row excludes
    p, q, loss, d_z, d_rows = ops.lsplm_loss_fwd(ids, F, None, torch.zeros(1, dtype=torch.int64).cuda(), table.cuda(), m,
                                                 torch.zeros(2 * m).cuda(), y)
    for x in (p, q, loss, d_z, d_rows):
        assert not torch.isnan(x).any()
    assert p[0].item() == 1.0 and q[0].item() == 0.0 and loss[0].item() == 0.0 and (d_z[0] == 0).all()
    assert p[1].item() == 0.0 and q[1].item() == 1.0 and loss[1].item() == 0.0 and (d_z[1] == 0).all()
    assert torch.isfinite(loss).all() and loss[4].item() > 60 and loss[5].item() > 60


def test_an_empty_batch_launches_nothing():
    F, m = 3, 4
    table, bias = torch.zeros(15, 2 * m, device="cuda"), torch.zeros(2 * m, device="cuda")
    ids, base = torch.zeros(0, F, dtype=torch.int64, device="cuda"), torch.zeros(F, dtype=torch.int64, device="cuda")
    p, q, z = ops.lsplm_fwd(ids, F, None, base, table, m, bias)
    assert tuple(p.shape) == (0,) and tuple(z.shape) == (0, 2 * m)
    d_z, d_rows = ops.lsplm_bwd(z, F, m, p)
    assert tuple(d_z.shape) == (0, 2 * m) and tuple(d_rows.shape) == (0, F * 2 * m)
    out = ops.lsplm_loss_fwd(ids, F, None, base, table, m, bias, p)
    assert tuple(out[2].shape) == (0,)
    assert (ops.lsplm_bias_grad(d_z, m) == 0).all()
    from deep_recommenders_amd._lib import lib, DR_EINVAL, DR_ESHAPE
    assert lib().dr_lsplm_fwd(None, 0, F, F, None, None, None, m, None, None, 0, None, None, None) == 0
    assert lib().dr_lsplm_fwd(None, 0, F, F, None, None, None, 3, None, None, 0, None, None, None) == DR_ESHAPE
    assert lib().dr_lsplm_fwd(None, 0, 0, F, None, None, None, m, None, None, 0, None, None, None) == DR_EINVAL
    assert lib().dr_lsplm_fwd(None, 0, F, 2, None, None, None, m, None, None, 0, None, None, None) == DR_EINVAL


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
MF, BUCKETS, MM, MB = 3, 5, 4, 32


def _model(seed=0):
    torch.manual_seed(seed)
    model = LSPLM([fc.indicator_column(fc.categorical_column_with_identity("f%d" % i, BUCKETS)) for i in range(MF)], num_regions=MM)
    with torch.no_grad():
        model.bias.copy_(0.1 * torch.randn(2 * MM))
    return model


def _inputs(multi, seed=1):
    g = torch.Generator().manual_seed(seed)
    bags = [torch.randint(0, BUCKETS, (MB, 1), generator=g) for _ in range(MF)]
    bags[0][3, 0] = -1
    if multi:
        bag = torch.randint(0, BUCKETS, (MB, 3), generator=g)
        bag[:, 1][torch.rand(MB, generator=g) < 0.4] = -1
        bag[:, 2][torch.rand(MB, generator=g) < 0.6] = -1
        bag[5] = -1
        bags[1] = bag
    return bags, {"f%d" % f: bags[f] for f in range(MF)}, torch.randint(0, 2, (MB,), generator=g).double()


def _check_step(model, t0, b0, bags, y, loss, lr, wt=None):
    base = BUCKETS * torch.arange(MF)
    t64, b64, l64 = R.train_step(t0, b0, bags, base, y, lr, wt)
    t32, b32, l32 = R.train_step(t0.float(), b0.float(), bags, base, y.float(), lr, None if wt is None else wt.float())
    got = (model.slab.table.detach().cpu().double(), model.bias.detach().cpu().double(), loss.cpu().double().reshape(()))
    for name, x, ref, x32 in zip(("table", "bias", "loss"), got, (t64, b64, l64), (t32, b32, l32)):
        scale = ref.abs().max().item()
        r32 = (x32.double() - ref).abs().max().item() / scale
        err = (x - ref).abs().max().item() / scale
        limit = 16 * max(r32, 8 * U)
        print("%s: error %.3g = %.2f max(r32, 8u), %.3f of the limit" % (name, err, err / max(r32, 8 * U), err / limit))
        assert err <= limit, (name, err, limit)
    changed = (t64 != t0).any(1)
    assert changed.any() and torch.equal(got[0][~changed], t0[~changed])


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_call_loss_and_one_atomic_train_step_against_the_float64_step(multi):
    model = _model()
    bags, inputs, y = _inputs(multi)
    t0, b0 = model.slab.table.detach().cpu().double(), model.bias.detach().cpu().double()
    base = BUCKETS * torch.arange(MF)
    p64, q64, _, _ = R.head(R.pool(t0, b0, bags, base))
    p32, _, _, _ = R.head(R.pool(t0.float(), b0.float(), bags, base))
    lim = 16 * max((p32.double() - p64).abs().max().item(), 8 * U)
    got = model(inputs)
    assert tuple(got.shape) == (MB, 1) and not got.requires_grad
    assert (got.cpu().double()[:, 0] - p64).abs().max().item() <= lim
    assert (torch.from_numpy(model.predict(inputs)).double()[:, 0] - p64).abs().max().item() <= lim
    l64 = R.loss_rows(p64, q64, y).mean().item()
    assert abs(model.loss(inputs, y).item() - l64) <= 16 * 8 * U * max(1.0, l64) + 16 * abs(R.loss_rows(p32, 1 - p32, y.float()).mean().item() - l64)
    wt = 0.5 + torch.rand(MB, generator=torch.Generator().manual_seed(5), dtype=torch.float64).float().double()
    loss = model.train_step(inputs, y, 0.5, sample_weight=wt)
    _check_step(model, t0, b0, bags, y, loss, 0.5, wt)


def test_the_deterministic_train_step_twice_with_identical_bits():
    bags, inputs, y = _inputs(False)
    runs = []
    for _ in range(2):
        model = _model()
        t0, b0 = model.slab.table.detach().cpu().double(), model.bias.detach().cpu().double()
        loss = model.train_step(inputs, y, 0.5, deterministic=True)
        _check_step(model, t0, b0, bags, y, loss, 0.5)
        loss2 = model.train_step(inputs, y, 0.5, deterministic=True)       # the plan is reused
        runs.append((model.slab.table.detach().clone(), model.bias.detach().clone(), loss, loss2))
    for x, y_ in zip(*runs):
        assert torch.equal(bits(x), bits(y_))
    assert runs[0][3].item() < runs[0][2].item()
    with pytest.raises(ValueError, match="single-valued"):
        _model().train_step(_inputs(True)[1], y, 0.5, deterministic=True)


def test_the_mixture_learns_xor_on_the_device():
    """the run of tests/test_lsplm_cpu.py with m = 4, seed 0, on the kernels: below ln 2 / 2, where no additive logit can get; the
    float64 reference ends 17 times lower, so the condition is neither met by chance nor missed by rounding"""
    m, seed = 4, 0
    table, bias = R.xor_init(m, seed)
    model = LSPLM([fc.indicator_column(fc.categorical_column_with_identity(k, 2)) for k in ("a", "b")], num_regions=m)
    with torch.no_grad():
        model.slab.table.copy_(table.float())
    for s in range(300):
        ab, y = R.xor_batch(seed, s, 256)
        model.train_step({"a": ab[:, :1], "b": ab[:, 1:]}, y, 1.0)
    pts = R.XOR_POINTS
    final = model.loss({"a": pts[:, :1], "b": pts[:, 1:]}, (pts[:, 0] ^ pts[:, 1]).double()).item()
    print("xor on the device: %.4f (ln 2 / 2 = %.4f)" % (final, math.log(2.0) / 2))
    assert final < math.log(2.0) / 2
