"""Shared helpers (not a test file): one DeepFM training step of an engine against the host oracle, on the rows the batches touch.

The compact-row oracle and the update comparisons started in tests/test_gpu_benchcfg.py (the bench shape) and moved here so that the
small-shape matrix (tests/test_gpu_engine_matrix.py) and the helper's own CPU test (tests/test_engine_oracle_cpu.py) use the same
code.  Everything is parametrised by the engine's own F, V, D, Nd, B; `eng` is a DeepFMEngine or any object with the same parameter
attributes on the host (see HostEngine below: an oracle run of another precision standing in for the device).

Oracle = oracle/torch_ref.py under torch autograd.  dtype float32 is the bench test's (like the reference's TF-CPU path), float64
the matrix's.  Ids of -1 are missing: the field contributes x = 0, no first-order term and no update.
"""
import numpy as np
import torch

from oracle import torch_ref as T


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _assert_update(name, before, after, want_after, rel=2e-3, outliers=1e-4):
    """after - before (device) against want_after - before (oracle), see the module docstring.

    `outliers`: fraction of elements allowed outside the tight tolerance, each still bounded by half its update + 2 rms.
    Two fp32 implementations of a ReLU network cannot agree on every element: a hidden unit whose pre-activation is within
    rounding of zero (a few of the 16.7 M per step) is "on" on one side and "off" on the other, which switches one of the
    ~128 active terms of that example's 1664 input gradients (first seen at 5e-6 of the table elements, errors of ~0.5 % of
    the update).  A wrong kernel moves every element, not 1e-5 of them."""
    b64 = before.astype(np.float64)
    d_gpu, d_cpu = after.astype(np.float64) - b64, want_after.astype(np.float64) - b64
    rms = float(np.sqrt(np.mean(d_cpu * d_cpu)))
    assert rms > 0, name + ": the oracle update is identically zero (test is vacuous)"
    err = np.abs(d_gpu - d_cpu)
    tol = 2 * np.maximum(_ulp(before), _ulp(want_after)) + rel * np.abs(d_cpu) + 1e-3 * rms
    bad = err > tol
    frac = float(bad.mean())
    assert frac <= outliers, "%s: %.2e of %d elements off (allowed %.0e); worst |err| %.3e at update %.3e (rms update %.3e)" % (
        name, frac, bad.size, outliers, float(err[bad].max()), float(np.abs(d_cpu)[bad].max()), rms)
    if bad.any():
        assert bool((err[bad] <= 0.5 * np.abs(d_cpu)[bad] + 2 * rms).all()), "%s: an outlier is not ReLU-tie sized: |err| %.3e (rms %.3e)" % (
            name, float(err[bad].max()), rms)
    return float((err / tol).max())          # (worst error / tolerance, for the callers that report it)


def _assert_close_adam(name, got, want, lr, outliers, mean_tol=2e-3):
    """Adam at this batch size is an amplifier: on step t the update is lr * g / (|g| + eps'), eps' = eps / sqrt(1 - beta2^t)
    ~ 3e-7, and the gradients of a 65 536-example mean are 1e-8 .. 1e-5 -- for |g| < ~1e-6 a change of 1e-8 in g moves the
    update by more than 2 % of a step.  fp32 rounding is far below that, a ReLU tie (see _assert_update) is not: one hidden
    unit switched for one example shifts that example's 1664 embedding-gradient elements by ~0.5 % and, through dy, a whole
    1677-element column of the first layer's weight gradient by ~1e-7.  So: all but `outliers` of the elements within 2 % of a
    step (measured: 4e-4 of the table rows, 7e-3 of W0 with ~1e2 ties per step), the MEAN difference within 0.2 % of a step,
    nothing off by more than one whole step.  A wrong gradient or update rule moves the mean by tens of per cent."""
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    frac = float((err > 2e-2 * lr).mean())
    assert frac <= outliers, "%s: %.2e of %d elements differ by more than 2 %% of an Adam step (allowed %.0e)" % (name, frac, err.size, outliers)
    assert float(err.mean()) <= mean_tol * lr, "%s: mean difference %.3e of a step" % (name, float(err.mean()) / lr)
    assert float(err.max()) <= 1.0 * lr, "%s: worst difference %.3e exceeds one Adam step" % (name, float(err.max()))
    # (worst of the three figures over its bound; an allowance of zero outliers counts as met when there are none)
    return max(frac / outliers if outliers > 0 else float(frac > 0), float(err.mean()) / (mean_tol * lr), float(err.max()) / lr)


def _sync(eng):
    if eng.table.is_cuda:
        torch.cuda.synchronize()


def _dense_moments(eng):
    """(m, v) of the first-order bias, the Dense kernels and the Dense biases, from the engine's flat Adam buffers."""
    fm, fv = eng.flat_m.cpu(), eng.flat_v.cpu()
    bo_ = eng._bias_off
    return (fm[bo_:bo_ + 1].clone(), fv[bo_:bo_ + 1].clone(),
            [fm[wo:wo + k * pu].view(k, pu)[:, :u].clone().contiguous() for wo, k, pu, u, bo in eng._views],
            [fv[wo:wo + k * pu].view(k, pu)[:, :u].clone().contiguous() for wo, k, pu, u, bo in eng._views],
            [fm[bo:bo + u].clone() for wo, k, pu, u, bo in eng._views],
            [fv[bo:bo + u].clone() for wo, k, pu, u, bo in eng._views])


class _CompactOracle:
    """DeepFM training steps on the rows a set of batches touches (oracle/torch_ref.py math, torch autograd for the gradients,
    [TF] B15 Adam from the same module).

    ids_list: one int64 [B, F] array of per-field ids per batch, -1 = missing.  all_rows: the compact set is every row of the tables
    (small tables: a stray write anywhere shows).  dtype: the precision the step is computed in; the state is held in it too, so a
    float64 oracle adopts the device's fp32 values exactly.  optimizer "adam_tf": tf.train.AdamOptimizer's dense rule on EVERY row
    of the compact set (needs all_rows)."""

    def __init__(self, eng, ids_list, optimizer, lr, dtype=torch.float32, all_rows=False):
        F, V = eng.F, eng.V
        self.F, self.V, self.D, self.Nd, self.B = F, V, eng.D, eng.Nd, eng.B
        self.dtype = dtype
        base = np.arange(F, dtype=np.int64)[None, :] * V
        self.valid = [torch.from_numpy(i >= 0) for i in ids_list]
        rows = [np.where(i >= 0, i + base, -1) for i in ids_list]
        for i, r in zip(ids_list, rows):
            assert int(i.max()) < V and int(i.min()) >= -1
        if all_rows:
            self.U = np.arange(F * V, dtype=np.int64)
        else:
            allr = np.concatenate([r.reshape(-1) for r in rows])
            self.U = np.unique(allr[allr >= 0])
        assert optimizer != "adam_tf" or all_rows
        # (a missing slot points at compact row 0 and is masked out of the forward: its gradient is exactly zero)
        self.cidx = [torch.from_numpy(np.where(r >= 0, np.searchsorted(self.U, np.maximum(r, 0)), 0)) for r in rows]
        self.Ud = torch.from_numpy(self.U).to(eng.table.device)
        self.opt, self.lr, self.t = optimizer, lr, 0
        self.resync_from(eng)
        self.table0, self.lin0 = self.table.clone(), self.lin.clone()
        self.Ws0, self.bs0, self.bias0 = [w.clone() for w in self.Ws], [b.clone() for b in self.bs], self.bias.clone()

    def resync_from(self, eng):
        """Adopt the device's state -- touched table rows, first-order weights, bias, dense parameters and (Adam) every moment -- so that
        the next step starts from IDENTICAL state on both sides (compare first, then call this)."""
        Ud, dt = self.Ud, self.dtype
        _sync(eng)
        self.table, self.lin = eng.table[Ud].cpu().to(dt), eng.lin_w[Ud].cpu().to(dt)
        self.bias = eng.lin_bias.cpu().clone().to(dt)
        self.Ws = [w.cpu().clone().contiguous().to(dt) for w in eng.Ws]
        self.bs = [b.cpu().clone().to(dt) for b in eng.bs]
        if self.opt != "sgd" and eng.t == 0:                             # (no Adam step yet: every moment is zero)
            z = torch.zeros_like
            self.mt, self.vt, self.ml, self.vl = z(self.table), z(self.table), z(self.lin), z(self.lin)
            self.mb, self.vb = z(self.bias), z(self.bias)
            self.mW, self.vW = [z(w) for w in self.Ws], [z(w) for w in self.Ws]
            self.mB, self.vB = [z(b) for b in self.bs], [z(b) for b in self.bs]
        elif self.opt != "sgd":
            self.mt, self.vt = eng.m_table[Ud].cpu().to(dt), eng.v_table[Ud].cpu().to(dt)
            self.ml, self.vl = eng.m_lin[Ud].cpu().clone().to(dt), eng.v_lin[Ud].cpu().clone().to(dt)
            mom = eng.dense_moments() if hasattr(eng, "dense_moments") else _dense_moments(eng)
            self.mb, self.vb = mom[0].to(dt), mom[1].to(dt)
            self.mW, self.vW, self.mB, self.vB = [[x.to(dt) for x in lst] for lst in mom[2:]]
            self.t = eng.t

    def logit(self, i, dense, relu_masks=None, ties=None, params=None):
        """The model's logit [B] of batch i from the oracle's current parameters (or `params` = (emb, lw, bias, ks, bs), the leaves
        step() differentiates).  relu_masks None: plain ReLU."""
        cidx, valid = self.cidx[i], self.valid[i]
        if params is None:
            params = (self.table[cidx], self.lin[cidx], self.bias, self.Ws, self.bs)
        emb, lw, bias, ks, bs = params
        vm = valid.to(self.dtype)
        xe = emb * vm[..., None]                                            # [B, F, D]  single-valued fields: x = the row ([TF] B5), 0 when missing
        x = xe.reshape(self.B, self.F * self.D)
        if self.Nd:
            x = torch.cat([x, dense.to(self.dtype)], 1)
        # (Adam amplifies fp32 noise in the gradients -- d step / d g is up to lr / eps' = 3e4 where |g| ~ 3e-7, see _assert_close_adam --
        # so two sides that each carry their OWN state drift apart by ~1e-5 rms in the pre-activations after one step.  Round 5 widened
        # the tie width 20 x for step 2; since round 6 the oracle adopts the device's parameters and moments after every step
        # (resync_from), each step is a one-step comparison from identical state, and a tie is a tie at the step-1 width)
        eps = 1e-5
        return (T.fm_second_order(xe) + (lw * vm).sum(1) + bias
                + T.dnn(x, ks, bs, relu_masks=relu_masks, ties=ties, tie_eps=eps).squeeze(1))                     # deepfm.py:36-47

    def own_relu_masks(self, i, dense):
        """The oracle's own ReLU decisions for batch i (what a host stand-in for the device reports as `its` masks)."""
        with torch.no_grad():
            vm = self.valid[i].to(self.dtype)
            x = (self.table[self.cidx[i]] * vm[..., None]).reshape(self.B, self.F * self.D)
            if self.Nd:
                x = torch.cat([x, dense.to(self.dtype)], 1)
            masks = []
            for W, b in zip(self.Ws[:-1], self.bs[:-1]):
                z = x @ W + b
                masks.append(z > 0)
                x = torch.relu(z)
        return masks

    def step(self, i, dense, labels, relu_masks=None):
        """relu_masks: the device's ReLU decisions of this step (oracle/torch_ref.py dnn: tie-aware comparison); the units where
        they differ from the oracle's own are recorded in self.ties and must be ties (T.check_ties)."""
        D = self.D
        cidx, valid = self.cidx[i], self.valid[i]
        emb = self.table[cidx].requires_grad_(True)
        lw = self.lin[cidx].requires_grad_(True)
        bias = self.bias.clone().requires_grad_(True)
        ks = [k.clone().requires_grad_(True) for k in self.Ws]
        bs = [b.clone().requires_grad_(True) for b in self.bs]
        self.ties = []
        logit = self.logit(i, dense, relu_masks, self.ties, params=(emb, lw, bias, ks, bs))
        loss = T.sigmoid_cross_entropy(labels.to(self.dtype), logit)                          # train_fm_on_movielens_estimator.py:46
        grads = torch.autograd.grad(loss, [emb, lw, bias] + ks + bs)
        self.slot_grads = (grads[0].detach(), grads[1].detach())          # per slot, before the sum over the slots that share a row
        gt = torch.zeros_like(self.table).index_add_(0, cidx.reshape(-1), grads[0].reshape(-1, D))
        gl = torch.zeros_like(self.lin).index_add_(0, cidx.reshape(-1), grads[1].reshape(-1))
        n = len(ks)
        self.t += 1
        self.last_gW, self.last_gb = [g_.detach().clone() for g_ in grads[3:3 + n]], [g_.detach().clone() for g_ in grads[3 + n:3 + 2 * n]]
        # smallest |gradient| an element has seen over the steps: Adam's sensitivity to gradient round-off (see _run_deepfm)
        mins = [g_.detach().abs() for g_ in list(grads[3:3 + n]) + list(grads[3 + n:3 + 2 * n])]
        self.min_abs_g = mins if not hasattr(self, "min_abs_g") else [torch.minimum(a, b_) for a, b_ in zip(self.min_abs_g, mins)]
        with torch.no_grad():
            if self.opt == "sgd":
                self.table -= self.lr * gt
                self.lin -= self.lr * gl
                self.bias -= self.lr * grads[2]
                for j in range(n):
                    self.Ws[j] -= self.lr * grads[3 + j]
                    self.bs[j] -= self.lr * grads[3 + n + j]
            else:
                if self.opt == "adam_tf":                                  # TF: the dense rule on the WHOLE variable, zeros for untouched rows
                    T.adam_dense_step(self.table, gt, self.mt, self.vt, self.lr, self.t)
                    T.adam_dense_step(self.lin, gl, self.ml, self.vl, self.lr, self.t)
                else:
                    touched = torch.unique(cidx[valid])
                    T.adam_rows_step(self.table, gt, touched, self.mt, self.vt, self.lr, self.t)
                    T.adam_rows_step(self.lin, gl, touched, self.ml, self.vl, self.lr, self.t)
                T.adam_dense_step(self.bias, grads[2], self.mb, self.vb, self.lr, self.t)
                for j in range(n):
                    T.adam_dense_step(self.Ws[j], grads[3 + j], self.mW[j], self.vW[j], self.lr, self.t)
                    T.adam_dense_step(self.bs[j], grads[3 + n + j], self.mB[j], self.vB[j], self.lr, self.t)
        return float(loss.detach())

    def touched(self, i):
        """bool [len(U)]: the compact rows batch i reads (missing slots excluded)."""
        m = torch.zeros(len(self.U), dtype=torch.bool)
        m[self.cidx[i][self.valid[i]]] = True
        return m


def _device_relu_masks(eng):
    """The ReLU decisions the device made in the step that just ran, one bool [B, units] per hidden layer: h > 0 of the stored
    activations; the fused head (last hidden layer + Dense(1) + loss in one GEMM epilogue) never stores its h, there the decision is
    read off the gradient it wrote: d_h = d_logit * w2 * (h > 0) with d_logit != 0 and w2 != 0 (both asserted)."""
    torch.cuda.synchronize()
    n_hidden = len(eng.Ws) - 1
    masks = []
    for i in range(n_hidden):
        if eng._head_done and i == n_hidden - 1:
            assert bool((eng.d_logit != 0).all()) and bool((eng.Ws[-1] != 0).all())
            masks.append((eng.dhs[-1] != 0).cpu())
        else:
            masks.append((eng.hs[i] > 0).cpu())
    return masks


def _check_adam_step(eng, orc, lr, step, ratios=None, touched=None):
    """One Adam step of the device against one Adam step of the oracle FROM THE SAME STATE (the oracle was re-synchronised after the
    previous step): the step-1 tolerances apply to every step -- all but 3e-3 of the table rows / first-order weights and 1e-2 of the
    dense weights whose |g| >= 1e-5 within 2 % of a step, mean difference within 0.2 % of a step, nothing off by more than one step
    (an element whose gradient is ~0 may take +lr on one side and -lr on the other: 2 lr) -- and the gradients themselves directly."""
    _sync(eng)
    ratios = {} if ratios is None else ratios

    def note(nm, r):
        ratios[nm] = max(ratios.get(nm, 0.0), r)
    got_t, got_l = eng.table[orc.Ud].cpu().numpy(), eng.lin_w[orc.Ud].cpu().numpy()
    want_t, want_l = orc.table.numpy(), orc.lin.numpy()
    if touched is not None:               # (bool [rows]: the rows this step looked up -- rows at rest must not dilute the fractions)
        tm = np.asarray(touched)
        got_t, got_l, want_t, want_l = got_t[tm], got_l[tm], want_t[tm], want_l[tm]
    note("table", _assert_close_adam("step %d table rows" % step, got_t, want_t, lr, 3e-3))
    note("lin", _assert_close_adam("step %d first-order weights" % step, got_l, want_l, lr, 3e-3))
    note("bias", _assert_close_adam("step %d first-order bias" % step, eng.lin_bias.cpu().numpy(), orc.bias.numpy(), lr, 0.0))
    nW = len(orc.Ws)
    for j in range(nW):
        # the dense gradients (the engine's Adam bucket holds this step's): the direct check.  A ReLU tie moves a whole column of W0's
        # gradient by ~1e-7, hence the rms-relative floor.
        for nm, got, want in (("gW%d" % j, eng.gWs[j], orc.last_gW[j]), ("gb%d" % j, eng.gbs[j], orc.last_gb[j])):
            got, want = got.cpu().numpy().astype(np.float64), want.numpy().astype(np.float64)
            rms = float(np.sqrt(np.mean(want * want)))
            bad = np.abs(got - want) > 1e-3 * np.abs(want) + 2e-2 * rms
            assert float(bad.mean()) <= 1e-3, "step %d %s: %.2e of the gradient elements off (rms %.3e, worst %.3e)" % (
                step, nm, float(bad.mean()), rms, float(np.abs(got - want).max()))
            note(nm, float((np.abs(got - want) / (1e-3 * np.abs(want) + 2e-2 * rms)).max()) if rms > 0 else 0.0)
        # the updated weights.  A step moves an element by ~ lr * g / (|g| + 3e-7): where |g| is within an order of magnitude of 3e-7 a
        # 1e-8 difference in g -- fp32 summation order -- moves the step by per cents; those elements are covered by the gradient check,
        # the update itself is compared where this step's |g| >= 1e-5
        for nm, got, want, g_ in (("W%d" % j, eng.Ws[j], orc.Ws[j], orc.last_gW[j]), ("b%d" % j, eng.bs[j], orc.bs[j], orc.last_gb[j])):
            sel = (g_.abs() >= 1e-5).numpy()
            if sel.sum() >= 16:
                note(nm, _assert_close_adam("step %d %s" % (step, nm), got.cpu().numpy()[sel], want.numpy()[sel], lr, 1e-2, mean_tol=2e-3))
            err = np.abs(got.cpu().numpy().astype(np.float64) - want.numpy().astype(np.float64))
            assert float(err.max()) <= 2.05 * lr, "step %d %s: worst difference %.3e exceeds what one Adam step can differ by" % (step, nm, float(err.max()))
    return ratios


def _assert_untouched(name, before, after, touched):
    """Rows of the compact set that this step did not look up must come out BIT-identical (`before` / `after`: numpy [rows, ...] of the
    same fp32 values the device holds, `touched`: bool [rows])."""
    keep = ~np.asarray(touched)
    b, a = before[keep], after[keep]
    same = (b.view(np.uint32) == a.view(np.uint32))
    assert bool(same.all()), "%s: %d untouched rows changed" % (name, int((~same.reshape(len(b), -1).all(1)).sum()))


def _assert_not_vacuous(name, before, want_after):
    """The oracle's update of this parameter is visible in fp32: its rms is at least 100 spacings of the parameter's rms magnitude."""
    b64 = before.astype(np.float64)
    d = want_after.astype(np.float64) - b64
    rms_d, rms_p = float(np.sqrt(np.mean(d * d))), float(np.sqrt(np.mean(b64 * b64)))
    assert rms_d >= 100 * float(np.spacing(np.float32(rms_p))), "%s: rms update %.3e against rms magnitude %.3e: the comparison is vacuous" % (
        name, rms_d, rms_p)


def _check_sgd_step(eng, orc, before, touched, ratios=None, edge=None):
    """One SGD step of the device against the oracle's from the same state: every parameter through _assert_update with its constants,
    rows of the compact set the batch did not look up bit-identical, and the oracle's update of every parameter visible in fp32.
    `before`: the oracle's state as adopted before the step -- (table, lin, bias, Ws, bs) tensors; `touched`: orc.touched(i).
    `edge`: bool [rows of the compact set], rows to be compared once more ON THEIR OWN (the first and last rows of a field): among a
    few rows a single wrong element is more than _assert_update's outlier fraction, which over the whole table would let one dropped
    row (D of ~1e5 elements) through."""
    _sync(eng)
    ratios = {} if ratios is None else ratios
    f32 = lambda t: t.detach().cpu().float().numpy()
    t0, l0, b0, W0s, b0s = before
    got_t, got_l = eng.table[orc.Ud].cpu().numpy(), eng.lin_w[orc.Ud].cpu().numpy()
    tm = touched.numpy()
    _assert_untouched("table rows", f32(t0), got_t, tm)
    _assert_untouched("first-order weights", f32(l0), got_l, tm)
    items = [("table", f32(t0)[tm], got_t[tm], orc.table.numpy()[tm]), ("lin", f32(l0)[tm], got_l[tm], orc.lin.numpy()[tm]),
             ("bias", f32(b0), eng.lin_bias.cpu().numpy(), orc.bias.numpy())]
    for j in range(len(orc.Ws)):
        items.append(("W%d" % j, f32(W0s[j]), eng.Ws[j].cpu().numpy(), orc.Ws[j].numpy()))
        items.append(("b%d" % j, f32(b0s[j]), eng.bs[j].cpu().numpy(), orc.bs[j].numpy()))
    em = tm & np.asarray(edge) if edge is not None else None
    if em is not None and em.any():
        items.append(("edge table", f32(t0)[em], got_t[em], orc.table.numpy()[em]))
        items.append(("edge lin", f32(l0)[em], got_l[em], orc.lin.numpy()[em]))
    for nm, b_, a_, w_ in items:
        _assert_not_vacuous(nm, b_, w_)
        ratios[nm] = max(ratios.get(nm, 0.0), _assert_update(nm, b_, a_, w_))
    return ratios


class HostEngine:
    """A host stand-in for the device: the same oracle step in another precision (fp32 by default), with the parameter attributes the
    helpers above read off a DeepFMEngine.  Used by tests/test_engine_oracle_cpu.py to show that the helpers pass a correct fp32 step
    and fail planted errors, without a GPU."""

    def __init__(self, F, V, D, Nd, B, units, optimizer, lr, seed, lin_init_std=0.1, dtype=torch.float32):
        g = torch.Generator().manual_seed(seed)
        self.F, self.V, self.D, self.Nd, self.B, self.lr, self.optimizer, self.dtype, self.t = F, V, D, Nd, B, lr, optimizer, dtype, 0
        std = 1.0 / np.sqrt(D)
        self.table = (torch.randn((F * V, D), generator=g) * std).clamp_(-2 * std, 2 * std)
        self.lin_w = torch.randn(F * V, generator=g) * lin_init_std
        self.lin_bias = torch.zeros(1)
        self.Ws, self.bs, d = [], [], F * D + Nd
        for u in list(units) + [1]:
            limit = float(np.sqrt(6.0 / (d + u)))
            self.Ws.append((torch.rand((d, u), generator=g) * 2 - 1) * limit)
            self.bs.append(torch.zeros(u))
            d = u
        self._orc = None

    def dense_moments(self):
        o = self._orc
        f = lambda t: t.float().clone()
        return f(o.mb), f(o.vb), [f(x) for x in o.mW], [f(x) for x in o.vW], [f(x) for x in o.mB], [f(x) for x in o.vB]

    def train_step(self, ids_list, i, dense, labels):
        """One step of batch i in self.dtype from the fp32 parameters held here; the results are rounded back to fp32 attributes, as a
        device would hold them.  Returns (loss, relu masks)."""
        if self._orc is None:
            self._orc = _CompactOracle(self, ids_list, self.optimizer, self.lr, dtype=self.dtype, all_rows=True)
        o = self._orc
        masks = o.own_relu_masks(i, dense)
        loss = o.step(i, dense, labels)
        self.t = o.t
        self.table, self.lin_w, self.lin_bias = o.table.float(), o.lin.float(), o.bias.float()
        self.Ws, self.bs = [w.float() for w in o.Ws], [b.float() for b in o.bs]
        self.gWs, self.gbs = [g_.float() for g_ in o.last_gW], [g_.float() for g_ in o.last_gb]
        if self.optimizer != "sgd":
            self.m_table, self.v_table, self.m_lin, self.v_lin = o.mt.float(), o.vt.float(), o.ml.float(), o.vl.float()
        return loss, masks
