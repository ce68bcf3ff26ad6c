"""Lean DCN training step (BASELINE.json config 4: Criteo-shaped, 3 cross layers + MLP [1024, 512, 256] + Dense(1)):

    x0 = concat(field embeddings [, dense features])                        K1 hash -> K3 gather+pool
    x_{l+1} = x0 * (x_l W_l + b_l + diag * x_l) + x_l,  l = 0..L-1           K8  keras/models/ranking/dcn.py:70-88 of the reference
    logit = Dense(1)(relu-MLP(x_L))                                          K7
    loss = sigmoid cross-entropy                                             K11

stacked exactly like the reference's own test stacks `Cross` layers (tests/keras/test_dcn.py:27-32), with the same kernels the
`Cross` / `dnn` classes use, no autograd tape, every update fused into the producing kernel (SGD: dst += -lr * grad).
The reference ships the layer, not a DCN model class: this engine exists to put an end-to-end number on config 4."""
import math
from typing import List, Sequence

import torch

from . import ops
from .ops import _pad4


class DCNDense:
    """The dense half of a DCN step -- cross stack, MLP, loss, and their backward -- on given weights, shared by DCNEngine (one GPU) and
    sharded.ShardedDCNEngine (row-sharded tables, replicated weights): x0 in, d loss / d x0 out.

    Gradients: `grads` = None applies the SGD step inside the wgrad kernels (dst += -lr * grad on the weights themselves, planes re-split
    right behind each update); `grads` = (g_cross_W, g_cross_b, g_Ws, g_bs) accumulates dst += grad into those tensors instead (a
    data-parallel bucket the caller all-reduces and applies; it then calls refresh_planes()).

    Wide GEMMs run on pre-split weights (ops.planes_worthwhile) in the operand split the library reports at construction
    (ops.get_gemm_split(): "f16x2" -- three matrix instructions per fragment pair, every activation operand with its amax record: x0's
    from one dr_h2_amax pass, every later one from the epilogue of the kernel that produces it -- or "bf16x3")."""

    def __init__(self, cross_W, cross_b, Ws, bs, batch, in_dim, ld, diag_scale, device, grads=None, k=None, prims=None):
        """prims: None = the HIP kernels (ops); anything else (the CPU tests' oracle-backed primitives) provides linear_fwd /
        linear_bwd_dx / linear_bwd_dw / cross_fwd / cross_combine_bwd / bce_fwd_bwd, and every product then runs in the plain family:
        no planes, no workspaces, no call into the library."""
        self.cross_W, self.cross_b, self.Ws, self.bs = list(cross_W), list(cross_b), list(Ws), list(bs)
        self.B, self.in_dim, self.ld, self.diag = batch, in_dim, ld, diag_scale
        self.grads = grads
        self.p = prims if prims is not None else ops
        self._k = k if k is not None else (lambda name, bound, work, fn: fn())
        B = batch
        units = [W.shape[1] for W in self.Ws]
        self.acts = [1] * (len(units) - 1) + [0]
        f32 = dict(dtype=torch.float32, device=device)
        native = prims is None and torch.device(device).type == "cuda"
        wide_cross = native and ops.planes_worthwhile(B, in_dim, in_dim)
        wide = [native and u > 1 and ops.planes_worthwhile(B, W.shape[0], W.shape[1]) for W, u in zip(self.Ws, units)]
        self.h2 = wide_cross and ops.get_gemm_split() == "f16x2"
        self.h2_all_wide = self.h2                               # (bench.py: every planes GEMM of this engine is priced as f16x2)
        WP = ops.H2WeightPlanes if self.h2 else ops.WeightPlanes
        # wide layers: the register-split wgrad (dr_bf3_wgrad / dr_h2_wgrad) on the same condition as the planes forward / dgrad
        self.wg_ws = [ops.bf3_wgrad_workspace(B, W.shape[0], W.shape[1], device) if wd else None for W, wd in zip(self.Ws, wide)]
        self.cross_wg_ws = ops.bf3_wgrad_workspace(B, in_dim, in_dim, device) if wide_cross else None
        self.cross_planes = [WP(W, wgrad_ws=self.cross_wg_ws) if wide_cross else None for W in self.cross_W]
        self.wplanes = [WP(W, wgrad_ws=ws) if wd else None for W, wd, ws in zip(self.Ws, wide, self.wg_ws)]
        # the GEMM family of every product, decided here once: the planes object, or the plain family on `prims`
        dw_ws = lambda K, N: ops.linear_bwd_dw_workspace(B, K, N, device) if native else None
        cross_ws = None if wide_cross else dw_ws(in_dim, in_dim)
        self.cross_gemm = [wp if wp is not None else ops.PlainWeight(W, prims, cross_ws) for W, wp in zip(self.cross_W, self.cross_planes)]
        self.gemm = [wp if wp is not None else ops.PlainWeight(W, prims, dw_ws(*W.shape)) for W, wp in zip(self.Ws, self.wplanes)]
        rec = (lambda: ops.h2_record(device)) if self.h2 else (lambda: None)
        self.x_amax = [rec() for _ in range(len(self.cross_W) + 1)]   # x_0 .. x_L
        self.h_amax = [rec() for _ in units]                          # MLP activations h_i
        self.dh_amax = [rec() for _ in units]                         # their gradients (dy of layer i)
        self.dp_amax = rec()                                          # d_prod of the cross layer being differentiated
        self.hs = [torch.empty((B, _pad4(u)), **f32)[:, :u] for u in units]
        self.dhs = [torch.empty((B, _pad4(u)), **f32)[:, :u] for u in units[:-1]]
        self.d_top = torch.zeros((B, ld), **f32)
        self.zero_logit = torch.zeros(B, **f32)
        self.prob, self.d_logit, self.loss = torch.empty(B, **f32), torch.empty(B, **f32), torch.zeros(1, **f32)
        self.ws = torch.empty(1024, **f32)

    def planes(self):
        return [wp for wp in list(self.cross_planes) + list(self.wplanes) if wp is not None]

    def refresh_planes(self):
        for wp in self.planes():
            wp.refresh()

    def ensure_fresh(self):
        for wp in self.planes():     # weights written from outside since the last refresh: re-split
            wp.ensure_fresh()

    def flops_step(self):
        fl = len(self.cross_W) * 2 * self.B * self.in_dim * self.in_dim
        for W in self.Ws:
            fl += 2 * self.B * W.shape[0] * W.shape[1]
        return 3 * fl

    def step(self, x0_buf, labels, lr):
        """x0_buf [B, ld] (columns >= in_dim zero) -> d loss / d x0 as a [B, in_dim] view; loss in self.loss (mean over the B rows)."""
        B, n_in, p = self.B, self.in_dim, self.p
        inplace = self.grads is None
        sc = -lr if inplace else 1.0
        gcW, gcb, gW, gb = (self.cross_W, self.cross_b, self.Ws, self.bs) if inplace else self.grads
        x0 = x0_buf[:, :n_in]
        if self.h2:
            self._k("h2_amax_x0", "hbm", 4.0 * B * n_in, lambda: ops.h2_amax(x0, self.x_amax[0]))
        xs, prods = [x0], []
        fl_c = 2.0 * B * n_in * n_in
        for l, (g, b) in enumerate(zip(self.cross_gemm, self.cross_b)):
            out, prod, _ = self._k("cross_fwd_L%d" % l, "mfma", fl_c,
                                   lambda x=xs[-1], g=g, b=b, l=l: g.cross_fwd(x0, x, self.x_amax[l], b, self.diag, True,
                                                                               out_amax=self.x_amax[l + 1]))
            xs.append(out)
            prods.append(prod)
        x, xam = xs[-1], self.x_amax[-1]                      # the current MLP input and its record (None: not known)
        for i, (g, b) in enumerate(zip(self.gemm, self.bs)):
            if g.wants_amax and xam is None:
                xam = ops.h2_amax(x, self.h_amax[i - 1])
            xam = self._k("linear_fwd_L%d" % i, "mfma", 2.0 * B * g.W.shape[0] * g.W.shape[1],
                          lambda x=x, g=g, b=b, i=i, xam=xam: g.fwd(x, xam, b, self.acts[i], self.hs[i], out_amax=self.h_amax[i]))
            x = self.hs[i]
        p.bce_fwd_bwd(self.zero_logit, labels, ops.LOSS_SIGMOID_CE, workspace=self.ws, logits_b=self.hs[-1],
                      out=(self.prob, self.d_logit, self.loss))
        # ---- backward: MLP ---------------------------------------------------------------------------------------------
        dy = self.d_logit.reshape(-1, 1)
        dyam = None                                           # record of dy (None: not known, built by a pass when a GEMM wants it)
        for i in range(len(self.Ws) - 1, -1, -1):
            g = self.gemm[i]
            fl = 2.0 * B * g.W.shape[0] * g.W.shape[1]
            if i > 0:
                xin, xinam = self.hs[i - 1], self.h_amax[i - 1]
                dx, rs, dxam = self.dhs[i - 1], (self.hs[i - 1] if self.acts[i - 1] else None), self.dh_amax[i - 1]
            else:
                xin, xinam = xs[-1], self.x_amax[-1]
                dx, rs, dxam = self.d_top[:, :n_in], None, None
            if g.wants_amax and dyam is None:
                dyam = ops.h2_amax(dy, self.dh_amax[i])
            dxam = self._k("linear_bwd_dx_L%d" % i, "mfma", fl,
                           lambda g=g, dy=dy, dyam=dyam, rs=rs, dx=dx, dxam=dxam: g.dgrad(dy, dyam, rs, dx, out_amax=dxam))
            self._k("linear_bwd_dw_L%d" % i, "mfma", fl,
                    lambda g=g, xin=xin, xinam=xinam, dy=dy, dyam=dyam, i=i: g.wgrad(xin, xinam, dy, dyam, sc, gW[i], gb[i]))
            if inplace:
                g.refresh()
            dy, dyam = dx, dxam
        # ---- backward: cross stack.  d_out of layer l -> (d_x0 +=, d_x_l), W_l / b_l updated (or their gradients accumulated) -----
        d_out = self.d_top[:, :n_in]
        d_x0 = torch.zeros((B, self.ld), dtype=torch.float32, device=d_out.device)[:, :n_in]
        dp_kw = {"d_prod_amax": self.dp_amax} if self.h2 else {}
        for l in range(len(self.cross_W) - 1, -1, -1):
            g = self.cross_gemm[l]
            # diag == 0: d_x = d_out + d_prod W^T: the dgrad below ACCUMULATES into the d_out buffer itself (d_out's last reader is the
            # combine kernel) -- no zero-filled d_x, no read-modify-write of it in the combine pass: -1.3 GB per layer
            d_x = d_out if self.diag == 0.0 else torch.zeros((B, self.ld), dtype=torch.float32, device=d_out.device)[:, :n_in]
            d_prod = self._k("cross_combine_bwd_L%d" % l, "hbm", 6.0 * 4 * B * n_in,
                             lambda l=l, d_out=d_out, d_x=d_x: p.cross_combine_bwd(x0, prods[l], d_out, self.diag, d_x0,
                                                                                   None if d_x is d_out else d_x, **dp_kw))
            self._k("cross_bwd_dx_L%d" % l, "mfma", fl_c,
                    lambda g=g, d_prod=d_prod, d_x=d_x: g.dgrad(d_prod, self.dp_amax, None, d_x, accumulate=True))
            self._k("cross_bwd_dw_L%d" % l, "mfma", fl_c,
                    lambda g=g, l=l, d_prod=d_prod: g.wgrad(xs[l], self.x_amax[l], d_prod, self.dp_amax, sc, gcW[l], gcb[l]))
            if inplace:
                g.refresh()
            d_out = d_x
        d_x0.add_(d_out)                                     # the first layer's x IS x0
        return d_x0


class DCNEngine:
    def __init__(self, num_fields: int, vocab_per_field: int, dim: int, num_cross: int, dnn_units: Sequence[int], batch: int,
                 num_dense: int = 0, lr: float = 0.01, diag_scale: float = 0.0, device="cuda", seed: int = 42):
        self.F, self.V, self.D, self.B, self.Nd, self.lr, self.diag = num_fields, vocab_per_field, dim, batch, num_dense, lr, diag_scale
        F, V, D, B = num_fields, vocab_per_field, dim, batch
        g = torch.Generator(device=device)
        g.manual_seed(seed)
        self.R = F * V
        self.table = torch.empty((self.R, D), dtype=torch.float32, device=device)
        std = 1.0 / math.sqrt(D)
        for r0 in range(0, self.R, 1 << 24):
            self.table[r0:r0 + (1 << 24)].normal_(0.0, std, generator=g).clamp_(-2 * std, 2 * std)
        self.in_dim = F * D + num_dense
        self.ld = _pad4(self.in_dim)
        f32 = dict(dtype=torch.float32, device=device)
        # cross layers: full-rank kernels [in_dim, in_dim] (dcn.py:55-68), truncated-normal init like the reference default
        self.cross_W, self.cross_b = [], []
        for _ in range(num_cross):
            W = torch.empty((self.in_dim, self.ld), **f32)
            W.normal_(0.0, 0.01, generator=g).clamp_(-0.02, 0.02)
            self.cross_W.append(W[:, :self.in_dim])
            self.cross_b.append(torch.zeros(self.in_dim, **f32))
        units = list(dnn_units) + [1]
        self.Ws: List[torch.Tensor] = []
        self.bs: List[torch.Tensor] = []
        d = self.in_dim
        for u in units:                                                    # [TF] B8 glorot uniform
            limit = math.sqrt(6.0 / (d + u))
            W = (torch.rand((d, _pad4(u)), device=device, generator=g) * 2 - 1) * limit
            self.Ws.append(W[:, :u])
            self.bs.append(torch.zeros(u, **f32))
            d = u
        self._events = None
        # cross stack + MLP + loss and their backward, every SGD step fused into the wgrad kernels (see DCNDense): forward / dgrad GEMMs
        # on pre-split weights, in the "f16x2" operand split unless ops.set_gemm_split("bf16x3") / DR_GEMM_SPLIT=bf16x3 (read once, by
        # the library) asks for the six-product one
        self.dense = DCNDense(self.cross_W, self.cross_b, self.Ws, self.bs, B, self.in_dim, self.ld, diag_scale, device,
                              k=lambda name, bound, work, fn: self._k(name, bound, work, fn))
        self.row_base = torch.arange(F, device=device, dtype=torch.int64) * V
        self.col_buckets = torch.full((F,), V, dtype=torch.int64, device=device)
        self.ids = torch.empty((B, F), dtype=torch.int64, device=device)
        self.x0 = torch.zeros((B, self.ld), **f32)
        self.plan = ops.SortPlan(B * F, device)
        self.side = torch.cuda.Stream(device=device)
        self.ev_ids, self.ev_sorted = torch.cuda.Event(), torch.cuda.Event()

    # the dense half's state, under the names rounds 1-4 (tests, bench.py) know
    h2 = property(lambda self: self.dense.h2)
    h2_all_wide = property(lambda self: self.dense.h2_all_wide)
    cross_planes = property(lambda self: self.dense.cross_planes)
    wplanes = property(lambda self: self.dense.wplanes)
    hs = property(lambda self: self.dense.hs)
    x_amax = property(lambda self: self.dense.x_amax)
    h_amax = property(lambda self: self.dense.h_amax)
    loss = property(lambda self: self.dense.loss)
    acts = property(lambda self: self.dense.acts)

    def enable_kernel_events(self, on: bool):
        self._events = {} if on else None

    def _k(self, name, bound, work, fn):
        if self._events is None:
            return fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = fn()
        e.record()
        self._events.setdefault(name, [bound, work, []])[2].append((s, e))
        return r

    def kernel_event_summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, (bound, work, evs) in (self._events or {}).items():
            ms = sum(s.elapsed_time(e) for s, e in evs) / len(evs)
            out[name] = {"bound": bound, "ms": ms, "n": len(evs), "alg_bytes" if bound in ("hbm", "overlap") else "alg_flops": work}
        return out

    def flops_step(self):
        return self.dense.flops_step()

    def refresh_planes(self):
        """Re-split every cross / MLP weight into its planes (see ops.WeightPlanes.ensure_fresh for when this is needed)."""
        self.dense.refresh_planes()

    def train_step(self, keys, dense, labels, next_keys=None):
        F, D, B, lr = self.F, self.D, self.B, self.lr
        self.dense.ensure_fresh()                            # weights written from outside since the last refresh: re-split
        # ---- forward -----------------------------------------------------------------------------------------------
        self._k("hash_bucket_i64", "hbm", B * F * 16, lambda: ops.hash_bucket_i64(keys, self.col_buckets, out=self.ids))
        self._k("emb_pool_fwd", "hbm", B * (8 * F * D + 8 * F),
                lambda: ops.emb_pool_fwd(self.ids, F, None, self.row_base, self.table, None, None, ld_concat=self.ld, concat=self.x0,
                                         want_sum_x=False, want_fm=False))
        self.ev_ids.record()
        with torch.cuda.stream(self.side):                   # slot sort for K4: hidden under the first cross GEMM
            self.side.wait_event(self.ev_ids)
            ops.emb_sort_slots(self.ids, self.row_base, self.R, self.plan)
            self.ev_sorted.record(self.side)
        if self.Nd:
            self.x0[:, F * D:F * D + self.Nd].copy_(dense)
        # ---- cross stack, MLP, loss, their backward and SGD steps ---------------------------------------------------------
        d_x0 = self.dense.step(self.x0, labels, lr)
        # ---- K4: scatter the embedding part of d_x0 (sorted, plain read-modify-write, fused SGD) ---------------------------
        torch.cuda.current_stream().wait_event(self.ev_sorted)
        self._k("emb_pool_bwd", "hbm", B * (12 * F * D + 8 * F),
                lambda: ops.emb_pool_bwd_sorted(self.ids, self.row_base, self.plan, D, self.R, d_x0, None, -lr, self.table, None, None))
        return self.loss
