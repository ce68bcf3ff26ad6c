"""dr_h2_emb_linear_tail_fwd: the fused first layer with the tower tail as its epilogue, against the two launches it replaces
(dr_h2_emb_linear_fwd followed by dr_tower_tail_fused with extra_logit = fm_logit) on the same inputs.

What must hold, and why:
  * Row-wise outputs -- sum_x, fm_logit, the saved first-order weights, prob, d_logit, d_h, dx = d h0, h0 when requested, the amax
    record of dx -- are BIT-IDENTICAL: the epilogue runs the tail's own stage bodies (csrc/tower_tail_core.h) on the same h0 bits, with
    the head product's eight 32-column partials formed and added in the tail's order.
  * dW1, db1, dw2, db2 and the loss are fixed-order fp32 sums of the same row terms, grouped by 256-row blocks instead of the tail's
    strided 32-row chunks.  Both paths are compared with an fp64 evaluation of the step (torch autograd on the fp64 copies of h0 and
    fm_logit, oracle.torch_ref's losses); a path's error is the largest |got - ref| / max |ref| over the five quantities, and the new
    path's must be <= 2 x the old path's: the terms are identical, so a factor 2 allows for the grouping and nothing else.  The
    gradients are written with scale = 1 into zeroed buffers, so the figures are errors of the sums and not of a weight's last bit.
    Each of the small quantities (32 or 1 values, where a ratio of two single roundings says little) is also held to the a-priori
    bound of a fp32 sum of n terms in ANY order, (n + 8) 2^-24 sum |terms| (Higham, gamma_n; 8 covers the terms' own roundings).
    Measured on MI355X (new / old, the eight cases below): 1.00, 1.00, 1.46, 1.07, 0.55, 0.79, 0.84, 1.00 (errors 0.8e-7 .. 2.6e-7).
  * Two launches give bit-equal outputs; arguments outside the domain return DR_ESHAPE and write nothing.
  * DeepFMEngine: three prefetched train_steps with the new path on and off.

Inputs of the first layer sit on a grid (multiples of 1/8, few significant bits: every product and every partial sum of h0 is exact
in both operand terms of the f16x2 mode, as in tests/test_gpu_fwd_image.py), so h0 is the same exact number on every path and the
comparison is not dominated by the operand split.  Tables are small (V <= 4096 rows per field, D = 64)."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as T

pytestmark = pytest.mark.gpu

D, V = 64, 1021


@pytest.fixture(scope="module")
def ops():
    from deep_recommenders_amd import ops as _ops
    return _ops


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# (M, F, dense, H, loss_mode, b1, b2, d_h, out, missing ids); M = None: 256 * (CU count) + 288, some CUs run two tiles
CASES = [
    (32, 1, 0, 32, 0, True, True, True, True, False),          # one live wave
    (288, 2, 13, 16, 1, False, False, False, False, True),     # K = 141: ragged k tail plus a ragged second tile
    (288, 2, 13, 32, 2, True, False, True, False, False),
    (864, 26, 13, 7, 2, True, True, True, False, True),        # K = 1677
    (864, 26, 13, 32, 0, False, True, False, True, False),
    (None, 1, 0, 32, 0, True, False, False, True, False),      # more tiles than CUs
    (None, 1, 0, 16, 1, True, True, True, False, True),
    (288, 2, 13, 7, 0, True, True, True, True, True),
]


def _grid(rng, shape, kmax, p_nonzero=1.0):
    k = rng.integers(-kmax, kmax + 1, shape)
    if p_nonzero < 1.0:
        k = k * (rng.random(shape) < p_nonzero)
    return (k / 8.0).astype(np.float32)


def _case(case):
    M, F, nd, H, mode, has_b1, has_b2, want_dh, want_out, missing = case
    if M is None:
        M = 256 * _cus() + 288
    rng = np.random.default_rng(1000 * F + H + mode)
    K = F * D + nd
    c = dict(M=M, F=F, nd=nd, H=H, mode=mode, K=K, want_dh=want_dh, want_out=want_out)
    c["table"] = _grid(rng, (F * V, D), 2, 0.25)
    c["lin_w"] = _grid(rng, (F * V,), 4)
    c["lin_b"] = np.array([0.25], np.float32)
    ids = rng.integers(0, V, (M, F))
    if missing:
        ids[rng.random((M, F)) < 0.1] = -1
        ids[M // 2] = -1                                           # a row with nothing at all
    c["ids"] = ids.astype(np.int64)
    c["dense"] = None
    if nd:
        dp = np.zeros((M, 32), np.float32)
        dp[:, :nd] = np.abs(_grid(rng, (M, nd), 8))
        c["dense"] = dp
    c["W0"] = _grid(rng, (K, 256), 3)
    c["b0"] = _grid(rng, (256,), 8)
    c["W1"] = (rng.standard_normal((256, H)) / 16.0).astype(np.float32)
    c["b1"] = (rng.standard_normal(H) * 0.1).astype(np.float32) if has_b1 else None
    c["w2"] = (rng.standard_normal((H, 1)) / np.sqrt(H)).astype(np.float32)
    c["b2"] = np.array([0.05], np.float32) if has_b2 else None
    c["labels"] = (rng.random(M) < 0.3).astype(np.float32)
    return c


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(ops, c, new, poison=7.0, split=False):
    """One evaluation of the step; gradients land in zeroed buffers (scale = 1).  Returns a dict of everything written."""
    M, F, H, K = c["M"], c["F"], c["H"], c["K"]
    table, lin_w, lin_b = _dev(c["table"]), _dev(c["lin_w"]), _dev(c["lin_b"])
    ids = _dev(c["ids"])
    rb = torch.arange(F, device="cuda", dtype=torch.int64) * V
    dpad = _dev(c["dense"])
    W0 = _dev(c["W0"])
    wp = ops.H2WeightPlanes(W0)
    tam = ops.h2_amax(table)
    dam = ops.h2_amax(dpad) if dpad is not None else None
    ldh = (H + 3) // 4 * 4
    W1 = torch.zeros((256, ldh), device="cuda")[:, :H]
    W1.copy_(_dev(c["W1"]))
    w2 = torch.zeros((H, 4), device="cuda")[:, :1]
    w2.copy_(_dev(c["w2"]))
    b1, b2 = _dev(c["b1"]), _dev(c["b2"])
    o = dict(sum_x=torch.full((M, D), poison, device="cuda"), fm=torch.full((M,), poison, device="cuda"),
             lv=torch.full((F, M), poison, device="cuda"), prob=torch.full((M,), poison, device="cuda"),
             d_logit=torch.full((M,), poison, device="cuda"), dx=torch.full((M, 256), poison, device="cuda"),
             d_h=torch.full((M, ldh), poison, device="cuda")[:, :H] if (c["want_dh"] or not new) else None,
             h0=torch.full((M, 256), poison, device="cuda") if (c["want_out"] or not new) else None,
             gW1=torch.zeros((256, ldh), device="cuda")[:, :H], gb1=torch.zeros(H, device="cuda") if b1 is not None else None,
             gw2=torch.zeros((H, 4), device="cuda")[:, :1], gb2=torch.zeros(1, device="cuda") if b2 is not None else None,
             loss=torch.full((1,), poison, device="cuda"), rec=ops.h2_record("cuda"))
    o["rec"].fill_(0x7f000000)
    labels = _dev(c["labels"])
    if new:
        ws = ops.h2_emb_linear_tail_workspace(M, "cuda")
        for parts in ((1, 2) if split else (3,)):                   # (split: the kernel raises the record itself, the reduce follows)
            ops.h2_emb_linear_tail_fwd(ids, rb, V, table, tam, lin_w, lin_b, dpad, dam, None, K, wp.wt, _dev(c["b0"]), 1, o["sum_x"], o["fm"],
                                       o["h0"], W1, b1, w2, b2, labels, c["mode"], 1.0, o["dx"], lin_vals_t=o["lv"], dst_W1=o["gW1"],
                                       dst_b1=o["gb1"], dst_W2=o["gw2"], dst_b2=o["gb2"], prob=o["prob"], d_logit=o["d_logit"], d_h=o["d_h"],
                                       loss=o["loss"], workspace=ws, parts=parts, dx_amax=o["rec"] if parts & 1 else None)
    else:
        ops.h2_emb_linear_fwd(ids, rb, V, table, tam, lin_w, lin_b, dpad, dam, None, K, wp.wt, _dev(c["b0"]), 1, o["sum_x"], o["fm"], o["h0"],
                              lin_vals_t=o["lv"])
        ops.tower_tail_fused(o["h0"], W1, b1, w2, b2, o["fm"], labels, c["mode"], 1.0, o["dx"], dst_W1=o["gW1"], dst_b1=o["gb1"],
                             dst_W2=o["gw2"], dst_b2=o["gb2"], prob=o["prob"], d_logit=o["d_logit"], d_h=o["d_h"], loss=o["loss"],
                             dx_amax=o["rec"])
    torch.cuda.synchronize()
    return o


def _fp64(c, h0, fm):
    """The step from h0 and fm_logit on, in fp64: gradients of the mean loss, the loss, and sum |terms| of every sum (for the bounds)."""
    t = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=True)
    H, M = c["H"], c["M"]
    W1, w2 = t(c["W1"]), t(c["w2"])
    b1 = t(c["b1"] if c["b1"] is not None else np.zeros(H, np.float32))
    b2 = t(c["b2"] if c["b2"] is not None else np.zeros(1, np.float32))
    x = h0.double()
    pre = x @ W1 + b1
    pre.retain_grad()
    h1 = torch.relu(pre)
    logit = (h1 @ w2).reshape(-1) + b2 + fm.double()
    logit.retain_grad()
    z = torch.tensor(c["labels"], dtype=torch.float64, device="cuda")
    p = torch.sigmoid(logit)
    lo = T.sigmoid_cross_entropy(z, logit) if c["mode"] == 0 else (T.log_loss(z, p) if c["mode"] == 1 else T.keras_bce(z, p))
    lo.backward()
    dh, dl = pre.grad, logit.grad
    ref = dict(gW1=W1.grad, gb1=b1.grad if c["b1"] is not None else None, gw2=w2.grad, gb2=b2.grad if c["b2"] is not None else None,
               loss=lo.detach().reshape(1))
    mag = dict(gb1=dh.abs().sum(0), gw2=(h1.detach() * dl[:, None]).abs().sum(0).reshape(-1, 1), gb2=dl.abs().sum().reshape(1),
               loss=lo.detach().abs().reshape(1))                    # (every loss term is >= 0: sum |terms| / M is the loss itself)
    return ref, mag


@pytest.fixture(scope="module")
def results(ops):
    """(case, old path, new path, new path again), computed once and shared."""
    out = []
    for case in CASES:
        c = _case(case)
        out.append((c, _run(ops, c, False), _run(ops, c, True), _run(ops, c, True, poison=-3.0)))
    return out


@pytest.mark.parametrize("i", range(len(CASES)))
def test_rowwise_outputs_are_the_two_launches_bits(results, i):
    c, old, new, _ = results[i]
    names = ["sum_x", "fm", "prob", "d_logit", "dx"] + (["d_h"] if c["want_dh"] else []) + (["h0"] if c["want_out"] else [])
    for k in names:
        assert torch.equal(new[k], old[k]), "%s differs from the two launches (case %s)" % (k, CASES[i])
    live = torch.from_numpy(c["ids"] >= 0).cuda().t()
    assert torch.equal(new["lv"][live], old["lv"][live]), "saved first-order weights"
    assert int(new["rec"].item()) == int(old["rec"].item()) == int(new["dx"].abs().max().view(torch.int32).item()), "amax record of dx"
    assert float(new["dx"].abs().max()) < 7.0 and float(new["prob"].max()) < 7.0          # every element written
    if not c["want_out"]:
        assert new["h0"] is None
    rows = np.nonzero((c["ids"] < 0).all(1))[0]
    for r in rows:                                                   # a row whose ids are all missing: zero embeddings
        assert float(new["sum_x"][r].abs().max()) == 0.0


@pytest.mark.parametrize("i", range(len(CASES)))
def test_weight_steps_and_loss_against_fp64(results, i):
    c, old, new, _ = results[i]
    ref, mag = _fp64(c, old["h0"], old["fm"])
    u = 2.0 ** -24
    errs = {}
    for name, o in (("old", old), ("new", new)):
        worst = 0.0
        for k in ("gW1", "gb1", "gw2", "gb2", "loss"):
            if ref[k] is None:
                continue
            e = (o[k].double() - ref[k].reshape(o[k].shape)).abs()
            worst = max(worst, e.max().item() / max(ref[k].abs().max().item(), 1e-300))
            if k in mag:                                             # a fp32 sum of M terms in any order
                bound = (c["M"] + 8) * u * mag[k].reshape(o[k].shape) + 1e-300
                assert bool((e <= bound).all()), "%s path, %s: %.3e over the any-order bound" % (name, k, (e / bound).max().item())
        errs[name] = worst
    print("case %s: max rel error old %.3e new %.3e ratio %.3f" % (CASES[i], errs["old"], errs["new"], errs["new"] / max(errs["old"], 1e-300)))
    assert errs["new"] <= 2.0 * errs["old"], errs


@pytest.mark.parametrize("i", range(len(CASES)))
def test_two_launches_give_equal_bits(results, i):
    c, _, a, b = results[i]
    for k, v in a.items():
        if v is None or k == "lv":
            continue
        assert torch.equal(v, b[k]), k
    live = torch.from_numpy(c["ids"] >= 0).cuda().t()
    assert torch.equal(a["lv"][live], b["lv"][live])


@pytest.mark.parametrize("i", [3, 5])
def test_kernel_and_reduce_as_two_calls(ops, results, i):
    """parts = 1 then parts = 2 (the engine's DR_REDUCE_SIDE schedules run the reduce on another stream): the same bits as one call,
    the record of dx included -- part 1 alone resets it and raises it from the kernel."""
    c, _, a, _ = results[i]
    b = _run(ops, c, True, poison=5.0, split=True)
    for k, v in a.items():
        if v is None or k == "lv":
            continue
        assert torch.equal(v, b[k]), k


def test_outside_the_domain_nothing_is_written(ops):
    assert ops.h2_emb_linear_tail_supported(64, 256, 32) and not ops.h2_emb_linear_tail_supported(64, 128, 32)
    assert not ops.h2_emb_linear_tail_supported(40, 256, 32) and not ops.h2_emb_linear_tail_supported(64, 256, 33)
    base = _case((64, 1, 0, 32, 0, True, True, True, True, False))

    def attempt(M=64, N=256, H=32, rows=V):
        c = dict(base)
        table, lin_w, lin_b = _dev(c["table"]), _dev(c["lin_w"]), _dev(c["lin_b"])
        ids = _dev(c["ids"][:M] if M <= 64 else np.zeros((M, 1), np.int64))
        rb = torch.zeros(1, device="cuda", dtype=torch.int64)
        wp = ops.H2WeightPlanes(torch.zeros((64, N), device="cuda"))
        W1, w2 = torch.zeros((N, H), device="cuda"), torch.zeros((H, 1), device="cuda")
        outs = [torch.full(s, 7.0, device="cuda") for s in ((M, D), (M,), (M, N), (M,), (M,), (M, N), (1,))]
        sum_x, fm, h0, prob, d_logit, dx, loss = outs
        with pytest.raises(RuntimeError, match="DR_ESHAPE"):
            ops.h2_emb_linear_tail_fwd(ids, rb, rows, table, ops.h2_amax(table), lin_w, lin_b, None, None, None, 64, wp.wt, None, 1, sum_x, fm, h0,
                                       W1, None, w2, None, torch.zeros(M, device="cuda"), 0, -0.1, dx, prob=prob, d_logit=d_logit, loss=loss)
        torch.cuda.synchronize()
        for o in outs:
            assert bool((o == 7.0).all()), "a refused call wrote something"
        assert not bool(W1.any()) and not bool(w2.any())
    attempt(N=512)                       # two column tiles
    attempt(N=128)
    attempt(H=33)
    attempt(M=40)                        # not a multiple of 32
    attempt(rows=(1 << 24) + 1)          # dr_h2_emb_linear_fwd's own limit: a field is one 4 GB buffer


@pytest.mark.parametrize("B", [512, 2304])
@pytest.mark.parametrize("units", [[256, 32], [256, 16]])
def test_engine_steps_with_the_tail_in_the_forward(units, B, monkeypatch):
    """Three prefetched train_steps with DR_TAIL_IN_FWD on (default) and off: row-wise tensors and the tables bit-identical after the
    first step, the loss within 1e-6 relative after the third.  Which path ran is asserted: at B = 512 the engine keeps the first layer
    off the register-split GEMMs altogether (ops.planes_worthwhile: B >= 2048), so there is no fused forward for the tail to ride on
    and the switch must change nothing; B = 2304 (nine row tiles) is the smallest shape of this test at which the new path runs."""
    from deep_recommenders_amd.engine import DeepFMEngine
    F, Nd = 3, 3
    g = torch.Generator(device="cuda")
    g.manual_seed(21)
    batches = [(torch.randint(0, 10**12, (B, F), device="cuda", generator=g), torch.rand((B, Nd), device="cuda", generator=g),
                (torch.rand(B, device="cuda", generator=g) < 0.3).float()) for _ in range(3)]

    def run():
        eng = DeepFMEngine(F, 3000, D, units, B, num_dense=Nd, lr=0.05, seed=3, lin_init_std=0.1)
        snap, losses = None, []
        for n in range(3):
            k, d, l = batches[n]
            nk, nd = (batches[n + 1][0], batches[n + 1][1]) if n < 2 else (None, None)
            losses.append(float(eng.train_step(k, d, l, next_keys=nk, next_dense=nd).item()))
            if n == 0:
                torch.cuda.synchronize()
                snap = [t.clone() for t in (eng.prob, eng.d_logit, eng.dhs[0], eng.dhs[-1], eng.sum_x, eng.fm_logit, eng.table, eng.lin_w, eng.Ws[0], eng.hs[0])]
        torch.cuda.synchronize()
        return eng, snap, losses
    on, s_on, l_on = run()
    runs = B >= 2048
    assert on.tail_in_fwd == runs and on._tail_in_fwd_ran == runs and on.fuse_tail and on._tail_done
    monkeypatch.setenv("DR_TAIL_IN_FWD", "0")
    off, s_off, l_off = run()
    assert not off.tail_in_fwd and not off._tail_in_fwd_ran and off.fuse_tail and off._tail_done
    for a, b, what in zip(s_on, s_off, ("prob", "d_logit", "d h0", "d h1", "sum_x", "fm_logit", "table", "lin_w", "W0", "h0")):
        assert torch.equal(a, b), what
    assert abs(l_on[2] - l_off[2]) <= 1e-6 * abs(l_off[2]), (l_on, l_off)
