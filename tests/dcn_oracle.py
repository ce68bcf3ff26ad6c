"""Shared helpers (not a test file): the DCN dense half (dcn_engine.DCNDense) and one DCNEngine training step against a float64 oracle.

Oracle = oracle/torch_ref.py under torch autograd: T.cross (keras/models/ranking/dcn.py:81-88) per cross layer, T.dnn with the ReLU
decisions the implementation under test took (its stored activations h > 0; every unit where they differ from the oracle's own must be
a tie, T.check_ties) and T.sigmoid_cross_entropy.  It is built from the state the device holds when it is called, so every step of a
run is a one-step comparison from identical state.

Two harnesses, used by tests/test_gpu_dcn_matrix.py (the HIP kernels) and tests/test_dcn_oracle_cpu.py (DCNDense on the oracle-backed
primitives of tests/test_sharded_gloo.py in fp32: the harnesses pass a correct run and fail planted errors without a GPU):

  A  run_bucket_harness   DCNDense with a gradient bucket: the bucket's VALUES against the float64 gradients, directly
  B  run_inplace_harness  DCNDense with the SGD step inside the wgrads (CPU), and _dcn_step_vs_oracle for DCNEngine.train_step (tables,
                          hashing and K4 included; started in tests/test_gpu_benchcfg.py for the bench shape and moved here)

The update comparisons (_assert_update, _assert_untouched, _assert_not_vacuous) are tests/engine_oracle.py's.
"""
import math

import numpy as np
import torch

from engine_oracle import _assert_not_vacuous, _assert_untouched, _assert_update       # noqa: F401  (re-exported to the tests)
from oracle import tf_semantics as O
from oracle import torch_ref as T

GRAD_REL = 2e-5          # harness A: max |err| <= GRAD_REL * max |want| per tensor (the figure tests/test_gpu_h2_gemm.py holds the two
                         # operand splits to; one product is bounded at 3e-6 - 5e-6 by the kernel tests; a plain fp32 torch evaluation
                         # of these shapes is within 6e-7 of float64)
UPDATE_REL = 1e-2        # harness B: _assert_update's `rel` for DCN (tests/test_gpu_benchcfg.py)


def _pad4(n):
    return (n + 3) // 4 * 4


def oracle(x0, cross_W, cross_b, Ws, bs, labels, diag, relu_masks=None, dtype=torch.float64):
    """The DCN dense half in `dtype` under autograd, from tensors of any device / precision.
    -> dict(loss, d_x0, g_cross_W, g_cross_b, g_Ws, g_bs: the gradients of the MEAN loss; ties: see T.dnn)."""
    leaf = lambda t: t.detach().cpu().to(dtype).contiguous().requires_grad_(True)
    x0 = leaf(x0)
    cW, cb, Wl, bl = [leaf(w) for w in cross_W], [leaf(b) for b in cross_b], [leaf(w) for w in Ws], [leaf(b) for b in bs]
    x = x0
    for W, b in zip(cW, cb):
        x = T.cross(x0, x, W, b, diag)
    ties = []
    logit = T.dnn(x, Wl, bl, relu_masks=relu_masks, ties=ties).reshape(-1)
    loss = T.sigmoid_cross_entropy(labels.detach().cpu().to(dtype), logit)
    grads = torch.autograd.grad(loss, [x0] + cW + cb + Wl + bl)
    L, n = len(cW), len(Wl)
    return dict(loss=float(loss.detach()), d_x0=grads[0], g_cross_W=list(grads[1:1 + L]), g_cross_b=list(grads[1 + L:1 + 2 * L]),
                g_Ws=list(grads[1 + 2 * L:1 + 2 * L + n]), g_bs=list(grads[1 + 2 * L + n:]), ties=ties)


def gates(dense):
    """The arrangement a DCNDense chose: its operand-split flag, the GEMM family of every cross layer and MLP layer (class names of
    ops.H2WeightPlanes / ops.WeightPlanes / ops.PlainWeight) and whether the cross dgrad accumulates into d_out itself (diag == 0)."""
    return {"h2": bool(dense.h2), "cross": [type(g).__name__ for g in dense.cross_gemm], "mlp": [type(g).__name__ for g in dense.gemm],
            "diag0": dense.diag == 0.0}


def relu_masks(dense):
    """The ReLU decisions of the step that just ran: h > 0 of every stored hidden activation."""
    if dense.hs[0].is_cuda:
        torch.cuda.synchronize()
    return [(h > 0).cpu() for h in dense.hs[:-1]]


# ---- DCNDense on its own (no tables) ------------------------------------------------------------------------------------------------------
class Capture:
    """DCNDense's `k` hook: keeps what step() does not -- every cross layer's output x_{l+1} and, in the f16x2 split, the true max |d_prod|
    of every cross_combine_bwd next to the record the kernel left for it (one record, overwritten per layer)."""

    def __init__(self):
        self.dense, self.xs, self.dp = None, {}, []

    def __call__(self, name, bound, work, fn):
        r = fn()
        if name.startswith("cross_fwd_L"):
            self.xs[int(name[len("cross_fwd_L"):]) + 1] = r[0]
        elif name.startswith("cross_combine_bwd_L") and self.dense is not None and self.dense.h2:
            self.dp.append((name, r.abs().max().view(torch.int32), self.dense.dp_amax.clone()))
        return r


class DenseProblem:
    """Weights laid out as DCNEngine lays them out ([in_dim, ld] storage sliced to in_dim, MLP kernels [d, pad4(u)] sliced to u, glorot /
    truncated-normal initial values, NON-zero cross biases, last bias 0.03: see tests/test_gpu_models.py for the loss kink at logit 0),
    optionally a gradient bucket of the same layout, `steps` batches (x0 [B, ld] ~ N(0, 1 / sqrt(64)) clamped at two sigma like the
    tables, padding columns zero; labels) and the DCNDense on them.  rows = (F, D, distinct): x0's first F * D columns are gathered
    from `distinct` rows per field instead, so that examples share rows the way hot ids make them."""

    def __init__(self, in_dim, L, units, B, diag, device, prims=None, bucket=True, steps=1, seed=7, rows=None):
        from deep_recommenders_amd.dcn_engine import DCNDense
        self.in_dim, self.ld, self.B, self.diag = in_dim, _pad4(in_dim), B, diag
        ld = self.ld
        g = torch.Generator(device=device)
        g.manual_seed(seed)
        f32 = dict(dtype=torch.float32, device=device)
        self.storage, self.used_cols = [], []                     # every parameter's whole buffer, padding included; its used columns
        self.cross_W, self.cross_b, self.Ws, self.bs = [], [], [], []
        for _ in range(L):
            W = torch.empty((in_dim, ld), **f32)
            W.normal_(0.0, 0.01, generator=g).clamp_(-0.02, 0.02)
            b = torch.empty(in_dim, **f32).normal_(0.0, 0.05, generator=g)
            self.storage += [W, b]
            self.used_cols += [in_dim, None]
            self.cross_W.append(W[:, :in_dim])
            self.cross_b.append(b)
        d = in_dim
        for u in list(units) + [1]:
            W = (torch.rand((d, _pad4(u)), device=device, generator=g) * 2 - 1) * math.sqrt(6.0 / (d + u))
            b = torch.zeros(u, **f32)
            self.storage += [W, b]
            self.used_cols += [u, None]
            self.Ws.append(W[:, :u])
            self.bs.append(b)
            d = u
        self.bs[-1].fill_(0.03)
        self.storage0 = [s.clone() for s in self.storage]
        self.grads, self.grad_storage = None, []
        if bucket:
            self.grad_storage = [torch.zeros_like(s) for s in self.storage]
            gs = self.grad_storage
            gcW = [gs[2 * l][:, :in_dim] for l in range(L)]
            gcb = [gs[2 * l + 1] for l in range(L)]
            gW = [gs[2 * L + 2 * i][:, :W.shape[1]] for i, W in enumerate(self.Ws)]
            gb = [gs[2 * L + 2 * i + 1] for i in range(len(self.Ws))]
            self.grads = (gcW, gcb, gW, gb)
        self.batches = []
        std = 1.0 / math.sqrt(64)
        for _ in range(steps):
            x0 = torch.zeros((B, ld), **f32)
            x0[:, :in_dim] = torch.empty((B, in_dim), **f32).normal_(0.0, std, generator=g).clamp_(-2 * std, 2 * std)
            if rows is not None:
                F, D, distinct = rows
                tab = torch.empty((F, distinct, D), **f32).normal_(0.0, std, generator=g).clamp_(-2 * std, 2 * std)
                pick = torch.randint(0, distinct, (B, F), device=device, generator=g)
                x0[:, :F * D] = tab[torch.arange(F, device=device)[None, :], pick].reshape(B, F * D)
            labels = (torch.rand(B, device=device, generator=g) < 0.3).float()
            self.batches.append((x0, labels))
        self.cap = Capture()
        self.dense = DCNDense(self.cross_W, self.cross_b, self.Ws, self.bs, B, in_dim, ld, diag, device, grads=self.grads, k=self.cap,
                              prims=prims)
        self.cap.dense = self.dense

    def oracle(self, i=0, masks=None):
        x0, labels = self.batches[i]
        return oracle(x0[:, :self.in_dim], self.cross_W, self.cross_b, self.Ws, self.bs, labels, self.diag, relu_masks=masks)

    def named_grads(self):
        gcW, gcb, gW, gb = self.grads
        return ([("g cross W%d" % l, t) for l, t in enumerate(gcW)] + [("g cross b%d" % l, t) for l, t in enumerate(gcb)]
                + [("g mlp W%d" % i, t) for i, t in enumerate(gW)] + [("g mlp b%d" % i, t) for i, t in enumerate(gb)])


def _bits(t):
    return int(t.abs().max().view(torch.int32).item()) if t.numel() else 0


def check_records(pb):
    """f16x2 split: every amax record the step wrote holds the float bits of its tensor's true max |.| (the GEMM that takes the tensor as
    an operand scales by it), and a record no f16x2 product needs is still 0.  x_amax[l] <-> x_l; h_amax[i] <-> hs[i] and dh_amax[i] <->
    the gradient of hs[i], written by the epilogue of an f16x2 producer or, where the producer is a plain layer, by the dr_h2_amax pass in
    front of the f16x2 consumer; d_prod's record is read off in the k hook (one record for all cross layers)."""
    from deep_recommenders_amd import ops
    dense, cap = pb.dense, pb.cap
    assert dense.h2
    torch.cuda.synchronize()
    xs = [pb.batches[0][0][:, :pb.in_dim]] + [cap.xs[l + 1] for l in range(len(dense.cross_W))]
    for l, x in enumerate(xs):
        assert int(dense.x_amax[l].item()) == _bits(x), "x_amax[%d]" % l
    h2 = [type(g) is ops.H2WeightPlanes for g in dense.gemm]
    n = len(h2)
    for i in range(n):
        wrote = h2[i] or (i + 1 < n and h2[i + 1])
        dy = dense.dhs[i] if i < n - 1 else dense.d_logit
        for nm, rec, t in (("h_amax", dense.h_amax[i], dense.hs[i]), ("dh_amax", dense.dh_amax[i], dy)):
            assert int(rec.item()) == (_bits(t) if wrote else 0), "%s[%d] (written: %s)" % (nm, i, wrote)
    assert len(cap.dp) >= len(dense.cross_W)
    for name, true, rec in cap.dp:
        assert int(rec.item()) == int(true.item()) and int(true.item()) != 0, "d_prod record after " + name
    cap.dp.clear()


def _rel_err(name, got, want, scale, ratios, rel=GRAD_REL):
    want = want.numpy().astype(np.float64) * scale
    err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max())
    bound = rel * float(np.abs(want).max())
    assert bound > 0, name + ": the oracle gradient is identically zero (test is vacuous)"
    ratios[name] = max(ratios.get(name, 0.0), err / bound)
    assert err <= bound, "%s: max |err| %.3e > %.0e * max |want| = %.3e" % (name, err, rel, bound)


def run_bucket_harness(pb, records=False):
    """Harness A on a DenseProblem with a bucket.  Step 1 on the zeroed bucket: loss to 1e-5 relative, d loss / d x0 and every bucket
    tensor to GRAD_REL of the float64 gradient's largest element; weights (whole buffers) bit-unchanged, the bucket's padding columns
    still zero.  Step 2 with the same inputs, bucket not zeroed: loss and d_x0 BIT-identical to step 1 (nothing is carried over in d_top
    or the aliased d_out), the bucket twice the gradient within the same bound.  -> {name: worst error / tolerance}."""
    dense, (x0, labels) = pb.dense, pb.batches[0]
    ratios = {}
    first = None
    for n in (1, 2):
        d_x0 = dense.step(x0, labels, 1.0)
        loss = float(dense.loss.item())
        if n == 1:
            orc = pb.oracle(0, relu_masks(dense))
            T.check_ties(orc["ties"])
            first = (dense.loss.clone(), d_x0.clone())
        else:
            assert torch.equal(dense.loss, first[0]), "step 2's loss differs from step 1's: %r / %r" % (loss, float(first[0].item()))
            assert torch.equal(d_x0, first[1]), "step 2's d_x0 differs from step 1's in %d elements (worst %.3e)" % (
                int((d_x0 != first[1]).sum()), float((d_x0 - first[1]).abs().max()))
        ratios["loss"] = max(ratios.get("loss", 0.0), abs(loss - orc["loss"]) / (1e-5 * abs(orc["loss"])))
        assert abs(loss - orc["loss"]) <= 1e-5 * abs(orc["loss"]), (n, loss, orc["loss"])
        _rel_err("d_x0", d_x0, orc["d_x0"], 1.0, ratios)
        want = orc["g_cross_W"] + orc["g_cross_b"] + orc["g_Ws"] + orc["g_bs"]
        for (name, got), w in zip(pb.named_grads(), want):
            _rel_err("%s (x%d)" % (name, n), got, w, float(n), ratios)
        for s, s0 in zip(pb.storage, pb.storage0):
            assert torch.equal(s, s0), "a weight buffer changed under grads=(...)"
        for gs, used in zip(pb.grad_storage, pb.used_cols):
            assert used is None or not bool(gs[:, used:].any()), "a padding column of the bucket was written"
        if records:
            check_records(pb)
    return ratios


def run_inplace_harness(pb, lr=1.0):
    """Harness B's update checks on a DenseProblem without a bucket (grads=None: the SGD step inside the wgrads), one step per batch,
    each against a float64 step from the state just before it: loss to 1e-5 relative, every parameter's update through _assert_update
    (rel = UPDATE_REL) and visible in fp32 (_assert_not_vacuous); d loss / d x0 -- what the engines scatter into the tables -- as the
    update it is there, x0 - lr * d_x0.  -> {name: worst error / tolerance}."""
    dense = pb.dense
    ratios = {}
    names = (["cross W%d" % l for l in range(len(pb.cross_W))] + ["cross b%d" % l for l in range(len(pb.cross_b))]
             + ["mlp W%d" % i for i in range(len(pb.Ws))] + ["mlp b%d" % i for i in range(len(pb.bs))])
    for x0, labels in pb.batches:
        params = list(pb.cross_W) + list(pb.cross_b) + list(pb.Ws) + list(pb.bs)
        before = [p.detach().cpu().clone() for p in params]
        # (the oracle differentiates at the state BEFORE the step; the masks are known only after it, so: snapshot, step, then oracle)
        d_x0 = dense.step(x0, labels, lr)
        loss = float(dense.loss.item())
        L, n = len(pb.cross_W), len(pb.Ws)
        orc = oracle(x0[:, :pb.in_dim], before[:L], before[L:2 * L], before[2 * L:2 * L + n], before[2 * L + n:], labels, pb.diag,
                     relu_masks=relu_masks(dense))
        T.check_ties(orc["ties"])
        ratios["loss"] = max(ratios.get("loss", 0.0), abs(loss - orc["loss"]) / (1e-5 * abs(orc["loss"])))
        assert abs(loss - orc["loss"]) <= 1e-5 * abs(orc["loss"]), (loss, orc["loss"])
        want = orc["g_cross_W"] + orc["g_cross_b"] + orc["g_Ws"] + orc["g_bs"]
        x0h = x0[:, :pb.in_dim].detach().cpu()
        items = [(nm, b, p.detach().cpu(), (b.double() - lr * g).float()) for nm, b, p, g in zip(names, before, params, want)]
        items.append(("x0 (d_x0)", x0h, x0h - lr * d_x0.detach().cpu(), (x0h.double() - lr * orc["d_x0"]).float()))
        for nm, b, a, w in items:
            b, a, w = b.numpy(), a.numpy(), w.numpy()
            _assert_not_vacuous(nm, b, w)
            ratios[nm] = max(ratios.get(nm, 0.0), _assert_update(nm, b, a, w, rel=UPDATE_REL))
    return ratios


# ---- DCNEngine.train_step (tables, hashing, K3 / K4 included) --------------------------------------------------------------------------
def make_engine(F, V, D, Nd, L, units, B, diag, lr=1.0, seed=11, gen_seed=3):
    """A DCNEngine with non-zero cross biases and last bias 0.03 (tests/test_gpu_models.py::test_dcn_engine_train_step_matches_oracle:
    the loss kink at logit 0), and the device generator the biases were drawn from -- the callers draw their batches from it."""
    from deep_recommenders_amd.dcn_engine import DCNEngine
    eng = DCNEngine(F, V, D, L, list(units), B, num_dense=Nd, lr=lr, diag_scale=diag, seed=seed)
    g = torch.Generator(device="cuda")
    g.manual_seed(gen_seed)
    with torch.no_grad():
        for b in eng.cross_b:
            b.normal_(0, 0.05, generator=g)
        eng.bs[-1].fill_(0.03)
    return eng, g


def _dcn_step_vs_oracle(eng, keys, dense, labels, tie_aware=True, all_rows=False):
    """One DCNEngine.train_step against the float64 oracle from the state the device holds when this is called; everything is read off
    the engine (F, V, D, Nd, B, lr, diag, its cross stack and MLP).  The host sees the table rows the batch touches (all_rows: every row
    of the table -- small tables, a stray write anywhere shows).  ids are asserted bit-exact against oracle/tf_semantics.py here.
    -> (loss_device, loss_oracle, ties, [(name, before, after_device, after_oracle), ...], touched): "table rows" first, then every
    cross W / b and MLP W / b; touched: bool over the rows of "table rows" (all True unless all_rows)."""
    F, V, D, Nd, B, lr = eng.F, eng.V, eng.D, eng.Nd, eng.B, eng.lr
    k = keys.cpu().numpy()
    ids = np.stack([O.hash_bucket_i64(k[:, f], V) for f in range(F)], axis=1)
    rows = ids + np.arange(F, dtype=np.int64)[None, :] * V
    U = np.arange(F * V, dtype=np.int64) if all_rows else np.unique(rows.reshape(-1))
    cidx = torch.from_numpy(np.searchsorted(U, rows))
    Ud = torch.from_numpy(U).cuda()
    t0 = eng.table[Ud].cpu()
    cW0 = [w.cpu().clone() for w in eng.cross_W]
    cb0 = [b.cpu().clone() for b in eng.cross_b]
    Ws0 = [w.cpu().clone() for w in eng.Ws]
    bs0 = [b.cpu().clone() for b in eng.bs]
    loss = float(eng.train_step(keys, dense, labels).item())
    np.testing.assert_array_equal(eng.ids.cpu().numpy(), ids)
    dd = torch.float64
    x0 = t0.to(dd)[cidx].reshape(B, F * D)
    if Nd:
        x0 = torch.cat([x0, dense.cpu().to(dd)], 1)
    # tie-aware: the fp64 oracle takes the ReLU branches the device took (its stored activations h > 0); every unit where that
    # differs from the oracle's own z > 0 must be within 1e-5 rms(z) of zero (T.check_ties, asserted by the caller)
    orc = oracle(x0, cW0, cb0, Ws0, bs0, labels, eng.diag, relu_masks=relu_masks(eng.dense) if tie_aware else None)
    gt = torch.zeros((len(U), D), dtype=dd).index_add_(0, cidx.reshape(-1), orc["d_x0"][:, :F * D].reshape(-1, D))
    out = [("table rows", t0.numpy(), eng.table[Ud].cpu().numpy(), (t0.to(dd) - lr * gt).float().numpy())]
    for j, (w0, g_) in enumerate(zip(cW0, orc["g_cross_W"])):
        out.append(("cross W%d" % j, w0.numpy(), eng.cross_W[j].cpu().numpy(), (w0.to(dd) - lr * g_).float().numpy()))
    for j, (b0, g_) in enumerate(zip(cb0, orc["g_cross_b"])):
        out.append(("cross b%d" % j, b0.numpy(), eng.cross_b[j].cpu().numpy(), (b0.to(dd) - lr * g_).float().numpy()))
    for j, (w0, g_) in enumerate(zip(Ws0, orc["g_Ws"])):
        out.append(("mlp W%d" % j, w0.numpy(), eng.Ws[j].cpu().numpy(), (w0.to(dd) - lr * g_).float().numpy()))
    for j, (b0, g_) in enumerate(zip(bs0, orc["g_bs"])):
        out.append(("mlp b%d" % j, b0.numpy(), eng.bs[j].cpu().numpy(), (b0.to(dd) - lr * g_).float().numpy()))
    touched = np.zeros(len(U), dtype=bool)
    touched[cidx.reshape(-1).numpy()] = True
    return loss, orc["loss"], orc["ties"], out, touched
