"""Host-side building blocks shared by the reference-shaped model classes: the embedding slab (all
categorical tables of a model in one HBM allocation), and the autograd glue around the C-ABI kernels.

Nothing here computes in PyTorch: forward and backward are launches of the hand-written HIP kernels
(ops.py).  PyTorch supplies device memory, the stream, nn.Parameter bookkeeping and the autograd tape.
"""
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import ops
from .ops import _pad4
from . import feature_column as fc


# --------------------------------------------------------------------------------------------------
# autograd glue
# --------------------------------------------------------------------------------------------------
def _rows(t, pitch4=False, aligned=False, dense=False):
    """The one place where a Function turns a tensor autograd hands it -- an incoming gradient, or an input that may be a view -- into
    rows a kernel can address: [..., W] with unit column stride whose rows lie at ONE pitch >= W, so that a kernel handed that pitch as
    its leading dimension reads every row where it is.  pitch4: the pitch is a multiple of 4 floats; aligned: the base is 16-byte
    aligned; dense: the pitch is W (the kernel takes no leading dimension).  A tensor that already is all of that is returned as it
    is, same storage, same data_ptr -- the gradient a loss produces is, so the models' path has no copy.  Dimensions of size 1 impose
    nothing (torch leaves their strides arbitrary, e.g. 0 after an expand): they are restrided in place, without a copy.  Anything
    else -- a broadcast gradient with a 0 stride, a transposed one, rows at several pitches -- is copied once into a fresh buffer
    (padded to a multiple of 4 columns with pitch4).  Layout only: no value changes."""
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise TypeError("expected an fp32 tensor, got %s" % t.dtype)
    W = t.shape[-1]
    ok = W <= 1 or t.stride(-1) == 1
    pitch, span = None, None
    for d in range(t.dim() - 2, -1, -1):
        n = t.shape[d]
        if n == 1 or not ok:
            continue
        if pitch is None:
            pitch = t.stride(d)
        elif t.stride(d) != span:
            ok = False
        span = t.stride(d) * n
    if pitch is None:                                         # a single row
        pitch = _pad4(W) if pitch4 and not dense else W
    ok = ok and pitch >= W and (not dense or pitch == W) and (not pitch4 or dense or pitch % 4 == 0)
    if ok and aligned and t.numel() and t.data_ptr() % 16 != 0:
        ok = False
    if ok and t.numel() == 0:
        return t
    if ok:
        strides = [1] * t.dim()
        step = pitch
        for d in range(t.dim() - 2, -1, -1):
            strides[d] = step
            step *= t.shape[d]
        if tuple(strides) == tuple(t.stride()):
            return t
        return t.as_strided(t.shape, strides, t.storage_offset())
    buf = torch.empty(tuple(t.shape[:-1]) + (_pad4(W) if pitch4 and not dense else W,), dtype=torch.float32, device=t.device)
    buf = buf[..., :W]
    buf.copy_(t)
    return buf


def _needed_only(backward):
    """Every backward here returns None in the slot of an input that needs no gradient (a frozen parameter, a non-tensor argument):
    what a fused kernel computed for it anyway is dropped here, in one place, instead of travelling on as if it had been asked for."""
    def masked(ctx, *grads):
        out = backward(ctx, *grads)
        out = out if isinstance(out, tuple) else (out,)
        if len(out) != len(ctx.needs_input_grad):
            return out                                        # autograd names the mismatch
        return tuple(g if need else None for g, need in zip(out, ctx.needs_input_grad))
    masked.__name__, masked.__doc__ = backward.__name__, backward.__doc__
    return masked


def _param_grad(p):
    """a zeroed gradient buffer for the parameter p: its shape, row-major whatever p's own strides are (a transposed or expanded view
    of a parameter has strides no kernel writes through; autograd takes a gradient in any layout)"""
    return torch.zeros(p.shape, dtype=torch.float32, device=p.device)


class _EmbPoolFn(torch.autograd.Function):
    """K3 forward / K4 backward.  `sparse_lr` None: dense gradient buffers are produced (small tables,
    any torch optimizer).  `sparse_lr` set: the backward applies the fused SGD update in place to the
    slab (no gradient materialised — the only feasible mode for 10 M-row tables)."""

    @staticmethod
    def forward(ctx, table, lin_w, lin_bias, ids, F, col_start, row_base, ld_concat, sparse_lr, second_order=True):
        concat, sum_x, fm = ops.emb_pool_fwd(ids, F, col_start, row_base, table, lin_w, lin_bias, ld_concat=ld_concat,
                                             second_order=second_order)
        ctx.F, ctx.sparse_lr, ctx.second_order = F, sparse_lr, second_order
        ctx.has_bias = lin_bias is not None
        ctx.bias_data = lin_bias.data if lin_bias is not None else None
        ctx.save_for_backward(table, lin_w, ids, col_start, row_base, concat, sum_x)
        ctx.mark_non_differentiable(sum_x)
        return concat, fm, sum_x

    @staticmethod
    @_needed_only
    def backward(ctx, d_concat, d_fm, _d_sum_x):
        table, lin_w, ids, col_start, row_base, concat, sum_x = ctx.saved_tensors
        F, D = ctx.F, table.shape[1]
        if col_start is None:
            col_start = torch.arange(F + 1, dtype=torch.int32, device=ids.device)
        d_concat, d_fm = _rows(d_concat), _rows(d_fm, dense=True)
        if d_concat is None and d_fm is None:
            return (None,) * 10
        has_bias = ctx.has_bias and d_fm is not None
        if not ctx.second_order:          # first-order-only logit: its gradient reaches lin_w / bias, not the rows
            concat, sum_x = None, None
        if ctx.sparse_lr is None:
            g_table = _param_grad(table)
            g_lin = _param_grad(lin_w) if lin_w is not None else None
            g_bias = torch.zeros(1, dtype=torch.float32, device=table.device) if has_bias else None
            ops.emb_pool_bwd(ids, F, col_start, row_base, D, d_concat, concat, sum_x, d_fm, 1.0, g_table, g_lin, g_bias)
            return g_table, g_lin, g_bias, None, None, None, None, None, None, None
        ops.emb_pool_bwd(ids, F, col_start, row_base, D, d_concat, concat, sum_x, d_fm, -float(ctx.sparse_lr),
                         table.data, lin_w.data if lin_w is not None else None, ctx.bias_data if has_bias else None)
        return None, None, None, None, None, None, None, None, None, None


class _LinFieldsFn(torch.autograd.Function):
    """Per-field first-order outputs [B, F] (FNN's bias-free Dense(1) over each indicator column, fnn.py:53-64)."""

    @staticmethod
    def forward(ctx, lin_w, ids, F, col_start, row_base):
        ctx.F = F
        ctx.save_for_backward(lin_w, ids, col_start, row_base)
        return ops.lin_fields_fwd(ids, F, col_start, row_base, lin_w)

    @staticmethod
    @_needed_only
    def backward(ctx, d_out):
        lin_w, ids, col_start, row_base = ctx.saved_tensors
        g = _param_grad(lin_w)
        ops.lin_fields_bwd(ids, ctx.F, col_start, row_base, _rows(d_out), 1.0, g)
        return g, None, None, None, None


class _Fm2Fn(torch.autograd.Function):
    """K6 stand-alone FM second-order term."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.fm2_fwd(x)

    @staticmethod
    @_needed_only
    def backward(ctx, d_out):
        (x,) = ctx.saved_tensors
        return ops.fm2_bwd(x, _rows(d_out, dense=True).reshape(-1))


class _MlpFn(torch.autograd.Function):
    """K7: a whole Dense tower.  acts[i] in {0: linear, 1: relu (fused into the GEMM epilogue; relu' is folded into the dx epilogue
    of the layer above), 2: sigmoid, 3: tanh (dr_act_fwd on the linear output, dr_act_bwd through the saved output), 4: exact GELU
    (dr_gelu_fwd from the linear output z into a fresh buffer; z is kept, because GELU's derivative is no function of its output:
    dr_gelu_bwd through z)}.
    args: x, acts tuple, then W0, b0, W1, b1, ..."""

    @staticmethod
    def forward(ctx, x, acts, *params):
        n = len(params) // 2
        hs = [x]
        zs = []                          # the pre-activations of the GELU layers, in layer order
        h = x
        for i in range(n):
            h = ops.linear_fwd(h, params[2 * i], params[2 * i + 1], 1 if acts[i] == 1 else 0)
            if acts[i] in (2, 3):
                ops.act_fwd_(h, acts[i])
            elif acts[i] == 4:
                zs.append(h)
                h = ops.gelu_fwd(h)
            hs.append(h)
        ctx.acts = acts
        ctx.save_for_backward(*hs, *params, *zs)
        return h

    @staticmethod
    @_needed_only
    def backward(ctx, dy):
        acts = ctx.acts
        n = len(acts)
        saved = ctx.saved_tensors
        hs, params, zs = saved[:n + 1], saved[n + 1:3 * n + 1], list(saved[3 * n + 1:])
        grads = [None] * (2 * n)
        dy = _rows(dy)
        for i in range(n - 1, -1, -1):
            W, b = params[2 * i], params[2 * i + 1]
            if acts[i] == 4:
                # GELU's derivative through the saved pre-activation (the top layer's incoming gradient is the caller's: cloned)
                dy = ops.gelu_bwd_(zs.pop(), dy.clone(memory_format=torch.contiguous_format) if i == n - 1 else dy)
            elif acts[i] in (2, 3) or (acts[i] == 1 and i == n - 1):
                # the activation's derivative through the saved output (a relu BELOW the top layer is folded into the dx GEMM)
                dy = ops.act_bwd_(hs[i + 1], dy.clone(memory_format=torch.contiguous_format) if i == n - 1 else dy, acts[i])
            need_b = b is not None and ctx.needs_input_grad[3 + 2 * i]
            if ctx.needs_input_grad[2 + 2 * i] or need_b:
                gW = _param_grad(W)
                gb = _param_grad(b) if need_b else None
                ops.linear_bwd_dw(hs[i], dy, 1.0, gW, gb)
                grads[2 * i], grads[2 * i + 1] = gW, gb
            need_dx = i > 0 or ctx.needs_input_grad[0]
            if need_dx:
                relu_src = hs[i] if (i > 0 and acts[i - 1] == 1) else None
                dy = ops.linear_bwd_dx(dy, W, relu_src)
        return (dy if ctx.needs_input_grad[0] else None, None, *grads)


class _DropoutFn(torch.autograd.Function):
    """tf.nn.dropout(x, rate) (estimator/models/feature_interaction/dnn.py:26-27 of the reference)."""

    @staticmethod
    def forward(ctx, x, rate, seed):
        y, mask = ops.dropout_fwd(_rows(x), rate, seed)
        ctx.rate = rate
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    @_needed_only
    def backward(ctx, dy):
        mask, = ctx.saved_tensors
        return ops.dropout_bwd(_rows(dy), mask, ctx.rate), None, None


class _L2Fn(torch.autograd.Function):
    """coeff * sum(w^2): the term a Keras `l2(coeff)` kernel / bias regularizer adds to the model's losses."""

    @staticmethod
    def forward(ctx, w, coeff):
        ctx.coeff = coeff
        ctx.save_for_backward(w)
        return ops.reduce_sum(w, squared=True, alpha=coeff).reshape(())

    @staticmethod
    @_needed_only
    def backward(ctx, d):
        w, = ctx.saved_tensors
        g = _param_grad(w)
        ops.axpy(2.0 * ctx.coeff * float(d), w.contiguous(), g)
        return g, None


class _CrossLowRankFn(torch.autograd.Function):
    """Low-rank DCN cross layer (keras/models/ranking/dcn.py:83-88): prod = (x U) V + b + diag x ; out = x0 * prod + x, with the
    two GEMMs on dr_linear_* and the combine on dr_cross_fwd(W = NULL) / dr_cross_combine_bwd."""

    @staticmethod
    def forward(ctx, x0, x, U, V, b, diag):
        u = ops.linear_fwd(x, U)                                            # [B, p]
        prod = torch.empty((x.shape[0], x.stride(0)), dtype=torch.float32, device=x.device)[:, :x.shape[1]]
        ops.linear_fwd(u, V, None, 0, out=prod)                             # x U V  (bias and diag are added by the combine)
        out, prod = ops.cross_fwd(x0, x, None, b, diag, prod=prod)
        ctx.diag = diag
        ctx.has_b = b is not None
        ctx.save_for_backward(x0, x, U, V, u, prod)
        return out

    @staticmethod
    @_needed_only
    def backward(ctx, d_out):
        x0, x, U, V, u, prod = ctx.saved_tensors
        ld = x.stride(0)
        d_out = _ld_like(d_out, ld)
        d_x0 = torch.zeros((x.shape[0], ld), dtype=torch.float32, device=x.device)[:, :x.shape[1]]
        d_x = torch.zeros((x.shape[0], ld), dtype=torch.float32, device=x.device)[:, :x.shape[1]]
        d_prod = ops.cross_combine_bwd(x0, prod, d_out, ctx.diag, d_x0, d_x)
        gV, gU = _param_grad(V), _param_grad(U)
        gb = torch.zeros(x.shape[1], dtype=torch.float32, device=x.device) if ctx.has_b else None
        ops.linear_bwd_dw(u, d_prod, 1.0, gV, gb)                           # dV = u^T d_prod ; db = colsum(d_prod)
        d_u = ops.linear_bwd_dx(d_prod, V)
        ops.linear_bwd_dw(x, d_u, 1.0, gU)                                  # dU = x^T d_u
        ops.linear_bwd_dx(d_u, U, None, accumulate=True, out=d_x)           # d_x += d_u U^T
        return d_x0, d_x, gU, gV, gb, None


def _ld_like(t, ld):
    """a [M, N] tensor with leading dimension `ld` (the cross kernels want x0 / x / prod / gradients on one pitch)"""
    t = _rows(t)
    if t.shape[0] <= 1 and t.shape[1] <= ld:                  # one row has no pitch of its own
        return t.as_strided(t.shape, (ld, 1), t.storage_offset())
    if t.stride(0) == ld:
        return t
    buf = torch.zeros((t.shape[0], ld), dtype=torch.float32, device=t.device)
    buf[:, :t.shape[1]].copy_(t)
    return buf[:, :t.shape[1]]


class _CrossFn(torch.autograd.Function):
    """K8: out = x0 * (x @ W + b + diag*x) + x   (keras/models/ranking/dcn.py:81-88 of the reference)."""

    @staticmethod
    def forward(ctx, x0, x, W, b, diag_scale):
        out, prod = ops.cross_fwd(x0, x, W, b, diag_scale, want_prod=True)
        ctx.diag = diag_scale
        ctx.same = x0.data_ptr() == x.data_ptr()
        ctx.save_for_backward(x0, x, W, b, prod)
        return out

    @staticmethod
    @_needed_only
    def backward(ctx, d_out):
        x0, x, W, b, prod = ctx.saved_tensors
        M, Dm = x.shape
        ld = prod.stride(0)

        d_out_, x0_ = _ld_like(d_out, ld), _ld_like(x0, ld)
        d_x0 = torch.zeros((M, ld), dtype=torch.float32, device=x.device)[:, :Dm]
        d_x = torch.zeros((M, ld), dtype=torch.float32, device=x.device)[:, :Dm]
        d_prod = ops.cross_combine_bwd(x0_, prod, d_out_, ctx.diag, d_x0, d_x)
        ops.linear_bwd_dx(d_prod, W, None, accumulate=True, out=d_x)
        gW, gb = None, None
        need_b = b is not None and ctx.needs_input_grad[3]
        if ctx.needs_input_grad[2] or need_b:
            gW = _param_grad(W)
            gb = _param_grad(b) if need_b else None
            ops.linear_bwd_dw(x, d_prod, 1.0, gW, gb)
        return d_x0, d_x, gW, gb, None


def fm_second_order(x: torch.Tensor) -> torch.Tensor:
    return _Fm2Fn.apply(x.contiguous())


def mlp(x: torch.Tensor, weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]],
        acts: Sequence[int]) -> torch.Tensor:
    params = []
    for W, b in zip(weights, biases):
        params += [W, b]
    return _MlpFn.apply(x, tuple(int(a) for a in acts), *params)


def cross(x0, x, W, b, diag_scale=0.0):
    return _CrossFn.apply(x0, x, W, b, float(diag_scale))


def cross_low_rank(x0, x, U, V, b, diag_scale=0.0):
    x0 = ops._rowmajor_ld4(x0)
    x = _ld_like(ops._rowmajor_ld4(x), x0.stride(0))
    return _CrossLowRankFn.apply(x0, x, U, V, b, float(diag_scale))


def dropout(x, rate, seed):
    return _DropoutFn.apply(x, float(rate), int(seed))


def l2_penalty(w, coeff):
    return _L2Fn.apply(w, float(coeff))


# --------------------------------------------------------------------------------------------------
# initialisers ([TF] defaults)
# --------------------------------------------------------------------------------------------------
def truncated_normal_(t: torch.Tensor, std: float, mean: float = 0.0):
    return nn.init.trunc_normal_(t, mean=mean, std=std, a=mean - 2 * std, b=mean + 2 * std)


def glorot_uniform_(t: torch.Tensor):
    fan_in, fan_out = t.shape[0], t.shape[1]
    limit = math.sqrt(6.0 / (fan_in + fan_out))
    return nn.init.uniform_(t, -limit, limit)


# --------------------------------------------------------------------------------------------------
# the embedding slab
# --------------------------------------------------------------------------------------------------
class EmbeddingSlab(nn.Module):
    """All categorical tables of one model in a single fp32 HBM slab [R, D] (+ first-order weights
    [R] and bias [1] when indicator columns are given), addressed by per-field base rows.

    Mirrors what F separate `DenseFeatures(embedding_column)` layers + `DenseFeatures(indicator
    columns) -> Dense(1)` hold in the reference (keras/models/ranking/fm.py:47-52, deepfm.py:24-29),
    but gathers every field in one fused kernel launch."""

    def __init__(self, embedding_columns: Sequence[fc.EmbeddingColumn],
                 indicator_columns: Optional[Sequence[fc.IndicatorColumn]] = None, device="cuda"):
        super().__init__()
        if len(embedding_columns) == 0:
            raise ValueError("at least one embedding column is required")
        dims = {c.dimension for c in embedding_columns}
        if len(dims) != 1:
            raise ValueError("FM-family models stack the field embeddings: all dimensions must be equal, got {}".format(
                sorted(dims)))
        self.D = dims.pop()
        if self.D % 4 != 0 or not (4 <= self.D <= 256):
            raise ValueError("embedding dimension must be a multiple of 4 in [4, 256] for the fused kernel")
        self.keys: List[str] = [c.categorical_column.key for c in embedding_columns]
        if len(set(self.keys)) != len(self.keys):
            raise ValueError("duplicate embedding column keys")
        self.columns: Dict[str, fc.CategoricalColumn] = {c.categorical_column.key: c.categorical_column
                                                         for c in embedding_columns}
        self.has_linear = indicator_columns is not None and len(indicator_columns) > 0
        if self.has_linear:
            ind_keys = [c.categorical_column.key for c in indicator_columns]
            if sorted(ind_keys) != sorted(self.keys):
                raise ValueError("indicator and embedding columns must wrap the same categorical columns "
                                 "(as every reference model builds them); got {} vs {}".format(ind_keys, self.keys))
        self.base: Dict[str, int] = {}
        r = 0
        for k in self.keys:
            self.base[k] = r
            r += self.columns[k].num_buckets
        self.R = r
        self.table = nn.Parameter(torch.empty((self.R, self.D), dtype=torch.float32, device=device))
        for c in embedding_columns:   # [TF] B4: truncated normal, sigma = 1/sqrt(D)
            k = c.categorical_column.key
            rows = self.table.data[self.base[k]:self.base[k] + self.columns[k].num_buckets]
            if c.initializer is not None:
                c.initializer(rows)
            else:
                truncated_normal_(rows, 1.0 / math.sqrt(self.D))
        if self.has_linear:           # Dense(1, kernel_initializer="zeros") / linear_model zeros
            self.lin_w = nn.Parameter(torch.zeros(self.R, dtype=torch.float32, device=device))
            self.lin_bias = nn.Parameter(torch.zeros(1, dtype=torch.float32, device=device))
        else:
            self.lin_w, self.lin_bias = None, None
        self.sparse_lr: Optional[float] = None   # set -> fused in-kernel SGD on the slab
        self._rb_cache = {}

    # per-key views (weight import/export; TF names: <scope>/<key>_embedding/embedding_weights)
    def embedding_weights(self, key: str) -> torch.Tensor:
        return self.table.data[self.base[key]:self.base[key] + self.columns[key].num_buckets]

    def linear_weights(self, key: str) -> torch.Tensor:
        return self.lin_w.data[self.base[key]:self.base[key] + self.columns[key].num_buckets]

    def transform(self, inputs: Dict[str, object], field_keys: Sequence[str]):
        """raw features -> (ids [B, C] int64, col_start int32 [F+1] or None, row_base int64 [F])"""
        dev = self.table.device
        mats = [self.columns[k].ids(inputs[k], dev) for k in field_keys]
        widths = [m.shape[1] for m in mats]
        ids = mats[0] if len(mats) == 1 else torch.cat(mats, dim=1)
        ck = (tuple(field_keys), tuple(widths))
        cached = self._rb_cache.get(ck)
        if cached is None:
            row_base = torch.tensor([self.base[k] for k in field_keys], dtype=torch.int64, device=dev)
            if all(w == 1 for w in widths) and len(widths) <= 64:
                col_start = None
            else:
                cs = [0]
                for w in widths:
                    cs.append(cs[-1] + w)
                col_start = torch.tensor(cs, dtype=torch.int32, device=dev)
            cached = (col_start, row_base)
            self._rb_cache[ck] = cached
        return ids.contiguous(), cached[0], cached[1]

    def forward(self, inputs: Dict[str, object], field_keys: Sequence[str], ld_concat: Optional[int] = None,
                second_order: bool = True):
        """-> concat [B, ld] (first F*D columns valid), fm_logit [B] (first-order + bias + second-order; with
        second_order=False the first-order + bias only: WDL's "wide" logit), sum_x"""
        ids, col_start, row_base = self.transform(inputs, field_keys)
        F = len(field_keys)
        concat, fm, sum_x = _EmbPoolFn.apply(self.table, self.lin_w, self.lin_bias, ids, F, col_start, row_base,
                                             ld_concat, self.sparse_lr, second_order)
        return concat, fm, sum_x

    def first_order_fields(self, inputs: Dict[str, object], field_keys: Sequence[str]):
        """[B, F]: every field's own first-order output sum_bag w[id] (no bias) -- FNN's `concat_weights`."""
        ids, col_start, row_base = self.transform(inputs, field_keys)
        return _LinFieldsFn.apply(self.lin_w, ids, len(field_keys), col_start, row_base)


# --------------------------------------------------------------------------------------------------
# tf.feature_column.input_layer
# --------------------------------------------------------------------------------------------------
class _GatherColsFn(torch.autograd.Function):
    """x[:, j] = num[:, map[j]] or emb[:, -map[j]-1] (dr_gather_cols); the backward gathers the embedding columns back out."""

    @staticmethod
    def forward(ctx, num, emb, col_map, emb_map, K):
        out = torch.empty((num.shape[0], K), dtype=torch.float32, device=emb.device)
        ops.gather_cols(_rows(num), _rows(emb), col_map, out)
        ctx.save_for_backward(emb_map)
        ctx.emb_shape = emb.shape
        return out

    @staticmethod
    @_needed_only
    def backward(ctx, d_out):
        emb_map, = ctx.saved_tensors
        d_out = _rows(d_out)
        d_emb = torch.empty(ctx.emb_shape, dtype=torch.float32, device=d_out.device)
        ops.gather_cols(d_out, None, emb_map, d_emb)
        return None, d_emb, None, None, None


class InputLayer(nn.Module):
    """tf.feature_column.input_layer over numeric_column and embedding_column (TF1 semantics): the columns sorted by name, each a
    contiguous block of one [B, K] fp32 matrix.  Numeric values are assembled on the host and reach the device as ONE copy per batch;
    the embedding columns are mean-pooled by the fused gather of an EmbeddingSlab (gradients flow into its table); a mixed set is
    interleaved by one dr_gather_cols launch.  TF names: input_layer/<key>_embedding/embedding_weights."""

    def __init__(self, feature_columns, device="cuda"):
        super().__init__()
        self.layout, self.K = fc.input_layer_layout(feature_columns)
        self.numeric = [(name, c) for name, c, _, _ in self.layout if isinstance(c, fc.NumericColumn)]
        emb = [c for _, c, _, _ in self.layout if isinstance(c, fc.EmbeddingColumn)]
        self.slab = EmbeddingSlab(emb, device=device) if emb else None
        self.emb_keys = [c.categorical_column.key for c in emb]
        self.device = torch.device(device)
        num_off, emb_off = 0, 0
        col_map, emb_map = [], []
        for name, c, off, w in self.layout:
            if isinstance(c, fc.NumericColumn):
                col_map += list(range(num_off, num_off + w))
                num_off += w
            else:
                col_map += [-(emb_off + i) - 1 for i in range(w)]
                emb_map += list(range(off, off + w))
                emb_off += w
        self.K_num, self.K_emb = num_off, emb_off
        # the numeric block / the pooled embeddings ARE the input when they are all of it (no interleave launch)
        self.mixed = self.K_num > 0 and self.K_emb > 0
        self._col_map = torch.tensor(col_map, dtype=torch.int32, device=self.device) if self.mixed else None
        self._emb_map = torch.tensor(emb_map, dtype=torch.int32, device=self.device) if self.mixed else None

    def numeric_block(self, features, batch_size):
        """[B, K_num] on the device: the numeric columns in name order, one host-to-device copy"""
        blocks = [c.host_block(features, batch_size) for _, c in self.numeric]
        host = blocks[0] if len(blocks) == 1 else np.concatenate(blocks, axis=1)
        t = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32))
        if self.device.type == "cuda":
            t = t.pin_memory() if t.numel() >= (1 << 16) else t
            return t.to(self.device, non_blocking=True)
        return t.to(self.device)

    def batch_size(self, features):
        for name, c, _, _ in self.layout:
            k = c.key if isinstance(c, fc.NumericColumn) else c.categorical_column.key
            if k in features:
                v = features[k]
                return int(v.shape[0]) if hasattr(v, "shape") else len(v)
        raise KeyError("none of the input_layer's features is present")

    def forward(self, features):
        B = self.batch_size(features)
        num = self.numeric_block(features, B) if self.K_num else None
        if self.K_emb == 0:
            return num
        concat, _, _ = self.slab(features, self.emb_keys, second_order=False)
        emb = concat[:, :self.K_emb]
        if not self.mixed:
            return emb
        return _GatherColsFn.apply(num, emb, self._col_map, self._emb_map, self.K)


# --------------------------------------------------------------------------------------------------
# graph aggregation (keras/models/retrieval/gcn.py:44-52): A @ X for a sparse or dense adjacency
# --------------------------------------------------------------------------------------------------
class SparseAdjacency:
    """A graph's adjacency as a device CSR (row_ptr int64, col int32, val fp32), built once.  Accepts a torch sparse COO / CSR tensor,
    a scipy sparse matrix or `(indices [nnz, 2], values [nnz], shape)` (a tf.SparseTensor's fields).  Duplicate coordinates are summed
    and the indices sorted on the host, as tf.sparse.sparse_dense_matmul sums them; the long-row plan and the device-built transpose
    (the backward's operand) are made on first use and kept."""

    def __init__(self, adj, shape=None, device="cuda"):
        import scipy.sparse as sp
        if isinstance(adj, SparseAdjacency):
            raise TypeError("already a SparseAdjacency")
        if isinstance(adj, torch.Tensor):
            if adj.layout == torch.sparse_csr:
                adj = adj.to_sparse_coo()
            if adj.layout != torch.sparse_coo:
                raise TypeError("SparseAdjacency: a torch tensor must be sparse (COO or CSR); pass a dense adjacency to GCN as is")
            adj = adj.coalesce().cpu()
            idx = adj.indices().numpy()
            m = sp.coo_matrix((adj.values().numpy().astype(np.float32), (idx[0], idx[1])), shape=tuple(adj.shape))
        elif sp.issparse(adj):
            m = adj.tocoo()
        elif isinstance(adj, (tuple, list)) and len(adj) == 3:
            indices, values, shp = adj
            indices = np.asarray(indices, dtype=np.int64).reshape(-1, 2)
            m = sp.coo_matrix((np.asarray(values, dtype=np.float32).reshape(-1), (indices[:, 0], indices[:, 1])),
                              shape=tuple(int(s) for s in shp))
        else:
            raise TypeError("SparseAdjacency: expected a torch sparse tensor, a scipy sparse matrix or (indices, values, shape)")
        if shape is not None and tuple(shape) != tuple(m.shape):
            raise ValueError("shape %s does not match the adjacency's %s" % (tuple(shape), tuple(m.shape)))
        n_rows, n_cols = m.shape
        if n_rows >= 2 ** 31 or n_cols >= 2 ** 31:
            raise ValueError("SparseAdjacency: at most 2^31 - 1 rows and columns (int32 column indices)")
        csr = sp.csr_matrix((m.data.astype(np.float32), (m.row, m.col)), shape=m.shape)   # sums duplicates
        csr.sum_duplicates()
        csr.sort_indices()
        self.shape = (int(n_rows), int(n_cols))
        self.nnz = int(csr.nnz)
        self.device = torch.device(device)
        self.row_ptr = torch.from_numpy(csr.indptr.astype(np.int64)).to(self.device)
        self.col = torch.from_numpy(csr.indices.astype(np.int32)).to(self.device)
        self.val = torch.from_numpy(csr.data.astype(np.float32)).to(self.device)
        self._plan = None
        self._t = None
        self._ws = {}

    @classmethod
    def _from_device(cls, row_ptr, col, val, shape):
        self = cls.__new__(cls)
        self.shape, self.nnz, self.device = tuple(shape), int(col.numel()), row_ptr.device
        self.row_ptr, self.col, self.val = row_ptr, col, val
        self._plan, self._t, self._ws = None, None, {}
        return self

    def plan(self):
        if self._plan is None:
            self._plan = ops.csr_plan(self.row_ptr, self.shape[0], self.nnz)
        return self._plan

    def transpose(self):
        """A^T as a SparseAdjacency, built on the device once (sources ascending inside each column: a fixed backward sum order)"""
        if self._t is None:
            t = ops.csr_transpose(self.row_ptr, self.col, self.val, self.shape[0], self.shape[1], self.nnz)
            self._t = SparseAdjacency._from_device(*t, (self.shape[1], self.shape[0]))
            self._t._t = self
        return self._t

    def workspace(self, D):
        if D not in self._ws:
            self._ws[D] = ops.csr_spmm_workspace(self.nnz, D, self.device)
        return self._ws[D]

    def spmm(self, X, relu_src=None, accumulate=False, out=None):
        """(A @ X) on dr_csr_spmm, no autograd"""
        if X.shape[0] != self.shape[1]:
            raise ValueError("A is %s, X has %d rows" % (self.shape, X.shape[0]))
        return ops.csr_spmm(self.row_ptr, self.col, self.val, self.shape[0], self.nnz, X, self.plan(), self.workspace(X.shape[1]),
                            relu_src=relu_src, accumulate=accumulate, out=out)

    def to_dense(self):
        """host float64 copy (tests)"""
        import scipy.sparse as sp
        return sp.csr_matrix((self.val.cpu().numpy(), self.col.cpu().numpy(), self.row_ptr.cpu().numpy()), shape=self.shape).toarray()


def as_adjacency(adj, device="cuda"):
    """SparseAdjacency for a sparse adjacency, None for a dense one"""
    import scipy.sparse as sp
    if isinstance(adj, SparseAdjacency):
        return adj
    if isinstance(adj, torch.Tensor) and adj.layout in (torch.sparse_coo, torch.sparse_csr):
        return SparseAdjacency(adj, device=device)
    if sp.issparse(adj) or (isinstance(adj, (tuple, list)) and len(adj) == 3):
        return SparseAdjacency(adj, device=device)
    return None


class _SpmmFn(torch.autograd.Function):
    """A @ X (tf.sparse.sparse_dense_matmul); backward dX = A^T dAgg on the transpose.  No gradient reaches A (a graph input)."""

    @staticmethod
    def forward(ctx, X, adj):
        ctx.adj = adj
        return adj.spmm(X)

    @staticmethod
    @_needed_only
    def backward(ctx, d):
        if not ctx.needs_input_grad[0]:
            return None, None
        return ctx.adj.transpose().spmm(_rows(d, pitch4=True, aligned=True)), None


class _DenseAggFn(torch.autograd.Function):
    """adj @ X for a dense adjacency (tf.linalg.matmul, gcn.py:47-48) on the GEMM path; dX = adj^T dAgg with a workspace (fixed order)"""

    @staticmethod
    def forward(ctx, X, adj):
        ctx.save_for_backward(adj)
        return ops.linear_fwd(adj, X)

    @staticmethod
    @_needed_only
    def backward(ctx, d):
        if not ctx.needs_input_grad[0]:
            return None, None
        (adj,) = ctx.saved_tensors
        M, K = adj.shape
        N = d.shape[1]
        dX = torch.zeros((K, N), dtype=torch.float32, device=d.device)
        ops.linear_bwd_dw(adj, _rows(d), 1.0, dX, None, workspace=ops.linear_bwd_dw_workspace(M, K, N, d.device))
        return dX, None


def aggregate(adj, X):
    """adj @ X with autograd: dr_csr_spmm for a SparseAdjacency, the GEMM for a dense [N, M] fp32 tensor"""
    if isinstance(adj, SparseAdjacency):
        return _SpmmFn.apply(X, adj)
    return _DenseAggFn.apply(X, adj)


class SampledBlock:
    """One layer of a sampled mini-batch: adj, a SparseAdjacency [n_dst, n_src] whose rows sum to 1, over the nodes src_ids int64
    [n_src] (on the device); its first n_dst entries are the block's destination nodes, so h[:n_dst] are their own rows."""
    __slots__ = ("adj", "src_ids", "n_dst")

    def __init__(self, adj, src_ids, n_dst):
        self.adj, self.src_ids, self.n_dst = adj, src_ids, n_dst

    @property
    def n_src(self):
        return self.adj.shape[1]


def _layer_seed(seed, k):
    """the seed of layer k's draws: layers must not share one (a node's sample is a function of (seed, node))"""
    return (int(seed) + 0x9E3779B97F4A7C15 * (k + 1)) & (2 ** 64 - 1)


def sample_blocks(adjacency, seeds, fanouts, seed, importance=None, add_self=False):
    """The blocks of a mini-batch of seed nodes for a len(fanouts)-layer network, outermost (input) layer first: blocks[k] aggregates
    layer k's input rows, blocks[0].src_ids are the nodes whose raw features are read and blocks[-1]'s destinations are the seeds.
    Layer k keeps up to fanouts[k] neighbours per node: uniformly without replacement (dr_neighbor_sample, GraphSAGE), or, with
    importance = dict(num_walks=R, walk_length=L), the most visited nodes of R random walks of L nodes from it, weighted by their visit
    counts (dr_random_walk + dr_walk_neighbors, PinSage).  add_self puts every destination into its own row (the `gcn` aggregator).
    The whole chain -- sample, frontier, block CSR, per layer, innermost first -- runs on the device over buffers of the largest size
    the fanouts allow; ONE device-to-host copy per call, at the end, reads every layer's counts (destinations, sources, entries) and
    the blocks are views of those buffers.  The result is a function of (seed, seeds, graph) alone.  No gradient reaches a block."""
    if not isinstance(adjacency, SparseAdjacency):
        raise TypeError("sample_blocks: adjacency must be a SparseAdjacency (build it once per graph)")
    fanouts = [int(f) for f in fanouts]
    if not fanouts:
        raise ValueError("sample_blocks: fanouts must name at least one layer")
    for f in fanouts:
        if not 1 <= f <= ops.SAMPLE_MAX_FANOUT:
            raise ValueError("sample_blocks: every fanout must be in [1, %d], got %s" % (ops.SAMPLE_MAX_FANOUT, fanouts))
    R = Lw = None
    if importance is not None:
        R, Lw = int(importance["num_walks"]), int(importance["walk_length"])
        if R < 1 or Lw < 2 or R * (Lw - 1) > ops.WALK_MAX_VISITS:
            raise ValueError("sample_blocks: importance needs num_walks >= 1, walk_length >= 2 and num_walks (walk_length - 1) <= %d, got %s"
                             % (ops.WALK_MAX_VISITS, dict(importance)))
    dst = torch.as_tensor(seeds)
    if dst.dtype != torch.int64 or dst.dim() != 1:
        raise ValueError("sample_blocks: seeds must be int64 [B], got %s %s" % (dst.dtype, tuple(dst.shape)))
    dst = dst.to(adjacency.device).contiguous()
    n_rows = adjacency.shape[0]
    made = []
    for k in reversed(range(len(fanouts))):
        s = _layer_seed(seed, k)
        if importance is None:
            nbr, cnt = ops.neighbor_sample(adjacency.row_ptr, adjacency.col, n_rows, dst, fanouts[k], s)
            weight = None
        else:
            walks = ops.random_walk(adjacency.row_ptr, adjacency.col, n_rows, dst.repeat_interleave(R), Lw, s)
            nbr, weight, cnt = ops.walk_neighbors(walks.view(-1, R, Lw), fanouts[k])
        src, counts, local = ops.frontier_build(dst, nbr, id_bound=n_rows)
        row_ptr, col, val = ops.block_csr(cnt, local, weight, add_self=add_self, n_valid=counts[:1])
        made.append((src, counts, row_ptr, col, val))
        dst = src
    sizes = torch.cat([torch.cat((counts, row_ptr[-1:])) for _, counts, row_ptr, _, _ in made]).cpu().tolist()    # the one read-back
    blocks = []
    for j, (src, _, row_ptr, col, val) in enumerate(made):
        n_dst, n_src, nnz = sizes[3 * j: 3 * j + 3]
        adj = SparseAdjacency._from_device(row_ptr[:n_dst + 1], col[:nnz], val[:nnz], (n_dst, n_src))
        blocks.append(SampledBlock(adj, src[:n_src], n_dst))
    return blocks[::-1]


class TypedBlock:
    """One layer of a sampled mini-batch over R relations: adj, a SparseAdjacency [n_dst * R, n_src] whose virtual row v * R + r holds
    the type-(r + 1) neighbours of destination v (row-normalised; empty when v has none of that type), over the nodes src_ids int64
    [n_src]; the first n_dst of them are the destinations.  adj.spmm(h) viewed [n_dst, R, D] is the per-type mean, and
    adj.transpose().spmm(d_agg) scatters all R gradients back in one launch."""
    __slots__ = ("adj", "src_ids", "n_dst", "R")

    def __init__(self, adj, src_ids, n_dst, R):
        self.adj, self.src_ids, self.n_dst, self.R = adj, src_ids, n_dst, R

    @property
    def n_src(self):
        return self.adj.shape[1]


def sample_typed_blocks(adjacencies, seeds, fanouts, seed):
    """sample_blocks over R relations of one node set (IntentGC's heterogeneous neighbourhoods): one TypedBlock per layer, outermost
    first.  Layer k draws up to fanouts[k] neighbours of every destination from EACH relation (dr_neighbor_sample, seeded per (layer,
    relation)), builds one frontier from all of them (one dr_frontier_build over nbr [n_dst, R * fanout]) and one CSR with a row per
    (destination, relation) (one dr_block_csr over [n_dst * R, fanout]).  As sample_blocks: everything on the device, ONE read-back per
    call, the result a function of (seed, seeds, graphs) alone; seeds may repeat."""
    adjacencies = list(adjacencies)
    if not adjacencies or not all(isinstance(a, SparseAdjacency) for a in adjacencies):
        raise TypeError("sample_typed_blocks: adjacencies must be a non-empty list of SparseAdjacency (build each once per graph)")
    R = len(adjacencies)
    if R > ops.INTENT_MAX_TYPES:
        raise ValueError("sample_typed_blocks: at most %d relations, got %d" % (ops.INTENT_MAX_TYPES, R))
    n_rows = adjacencies[0].shape[0]
    for a in adjacencies:
        if a.shape != (n_rows, n_rows) or a.device != adjacencies[0].device:
            raise ValueError("sample_typed_blocks: every relation must be [%d, %d] over the same nodes on one device, got %s on %s"
                             % (n_rows, n_rows, a.shape, a.device))
    fanouts = [int(f) for f in fanouts]
    if not fanouts:
        raise ValueError("sample_typed_blocks: fanouts must name at least one layer")
    for f in fanouts:
        if not 1 <= f <= ops.SAMPLE_MAX_FANOUT:
            raise ValueError("sample_typed_blocks: every fanout must be in [1, %d], got %s" % (ops.SAMPLE_MAX_FANOUT, fanouts))
    dst = torch.as_tensor(seeds)
    if dst.dtype != torch.int64 or dst.dim() != 1:
        raise ValueError("sample_typed_blocks: seeds must be int64 [B], got %s %s" % (dst.dtype, tuple(dst.shape)))
    dst = dst.to(adjacencies[0].device).contiguous()
    made = []
    for k in reversed(range(len(fanouts))):
        n = dst.numel()
        drawn = [ops.neighbor_sample(a.row_ptr, a.col, n_rows, dst, fanouts[k], _layer_seed(seed, k * R + r))
                 for r, a in enumerate(adjacencies)]
        nbr = torch.cat([d[0] for d in drawn], dim=1)                       # [n, R * fanout]
        cnt = torch.stack([d[1] for d in drawn], dim=1).contiguous()        # [n, R]
        src, counts, local = ops.frontier_build(dst, nbr, id_bound=n_rows)
        row_ptr, col, val = ops.block_csr(cnt.view(n * R), local.view(n * R, fanouts[k]), None, add_self=False, n_valid=counts[:1] * R)
        made.append((src, counts, row_ptr, col, val))
        dst = src
    sizes = torch.cat([torch.cat((counts, row_ptr[-1:])) for _, counts, row_ptr, _, _ in made]).cpu().tolist()    # the one read-back
    blocks = []
    for j, (src, _, row_ptr, col, val) in enumerate(made):
        n_dst, n_src, nnz = sizes[3 * j: 3 * j + 3]
        adj = SparseAdjacency._from_device(row_ptr[:n_dst * R + 1], col[:nnz], val[:nnz], (n_dst * R, n_src))
        blocks.append(TypedBlock(adj, src[:n_src], n_dst, R))
    return blocks[::-1]


class _SoftmaxRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = ops.softmax_rows_fwd(_rows(x))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @_needed_only
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.softmax_rows_bwd(y, _rows(dy))


def softmax_rows(logits):
    """softmax over the last axis; the result remembers its logits (`_dr_logits`) so that losses.categorical_crossentropy can take
    the fused softmax-CE path, as Keras' backend does when its input is a Softmax op"""
    y = _SoftmaxRowsFn.apply(logits)
    y._dr_logits = logits
    return y


class _AddFn(torch.autograd.Function):
    """out + x on dr_axpy (the GCN residual, gcn.py:54-55)"""

    @staticmethod
    def forward(ctx, out, x):
        y = out.contiguous().clone() if out.is_contiguous() else out.contiguous()
        ops.axpy(1.0, x.contiguous(), y)
        return y

    @staticmethod
    @_needed_only
    def backward(ctx, d):
        return d, d


# --------------------------------------------------------------------------------------------------
# Transformer package (keras/models/nlp of the reference) on csrc/attention.hip
# --------------------------------------------------------------------------------------------------
class _AttentionFn(torch.autograd.Function):
    """ScaledDotProductAttention over the heads of projected [B, L, H * dh] tensors: dr_attn_fwd / dr_attn_bwd.  The dropout mask
    is a function of (seed, b, h, query, key) and is regenerated in the backward; only (max, sum) per row is saved."""

    @staticmethod
    def forward(ctx, q, k, v, key_mask, n_heads, future, rate, seed):
        out, stats = ops.attn_fwd(q, k, v, n_heads, key_mask, future, rate, seed)
        ctx.cfg = (n_heads, future, rate, seed)
        ctx.key_mask = key_mask
        ctx.save_for_backward(q, k, v, stats)
        return out

    @staticmethod
    @_needed_only
    def backward(ctx, d_out):
        q, k, v, stats = ctx.saved_tensors
        n_heads, future, rate, seed = ctx.cfg
        dq, dk, dv = ops.attn_bwd(q, k, v, n_heads, _rows(d_out), stats, ctx.key_mask, future, rate, seed)
        return dq, dk, dv, None, None, None, None, None


def attention(q, k, v, n_heads, key_mask=None, future=False, rate=0.0, seed=0):
    """softmax(q k^T / sqrt(dh) + key_mask * (-2^32 + 1) [future: entries above the diagonal replaced]) -> dropout -> . v for every
    head; q [B, Lq, H * dh], k, v [B, Lk, H * dh], key_mask [B, Lk] (True = padded)"""
    return _AttentionFn.apply(q, k, v, key_mask, int(n_heads), bool(future), float(rate), int(seed))


class _AddLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, gamma, beta, eps):
        shape = a.shape
        a2 = a.reshape(-1, shape[-1])
        b2 = b.reshape(-1, shape[-1]) if b is not None else None
        y, stats = ops.add_layernorm_fwd(a2, b2, gamma, beta, eps)
        ctx.has_b = b is not None
        ctx.save_for_backward(a2, b2, gamma, stats)
        return y.reshape(shape)

    @staticmethod
    @_needed_only
    def backward(ctx, dy):
        a2, b2, gamma, stats = ctx.saved_tensors
        d_s, d_gamma, d_beta = ops.add_layernorm_bwd(a2, b2, gamma, stats, _rows(dy).reshape(a2.shape))
        d_s = d_s.reshape(dy.shape)
        return d_s, (d_s if ctx.has_b else None), d_gamma, d_beta, None


def add_layer_norm(a, b, gamma, beta, eps=1e-8):
    """LayerNormalization(a + b) over the last axis (b may be None): population variance, eps inside the root"""
    return _AddLayerNormFn.apply(a, b, gamma, beta, float(eps))


class _TokenEmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, ids, pos, rate, seed):
        ctx.cfg = (rate, seed)
        ctx.save_for_backward(ids)
        ctx.table_shape = table.shape
        return ops.token_embedding_fwd(ids, table, pos, rate, seed)

    @staticmethod
    @_needed_only
    def backward(ctx, d_out):
        (ids,) = ctx.saved_tensors
        rate, seed = ctx.cfg
        d_table = torch.zeros(ctx.table_shape, dtype=torch.float32, device=d_out.device)
        ops.token_embedding_bwd(ids, _rows(d_out, dense=True), d_table, rate, seed)
        return d_table, None, None, None, None


def token_embedding(table, ids, pos=None, rate=0.0, seed=0):
    """dropout(table[ids] * sqrt(D) + pos): ids [B, L] integer, pos the [L, D] position table or None; the table's gradient is
    dense [V, D] and summed in a fixed order"""
    return _TokenEmbeddingFn.apply(table, ids.to(torch.int64), pos, float(rate), int(seed))


class _TiedProjectionFn(torch.autograd.Function):
    """x @ table^T (the pre-softmax projection that shares the embedding matrix, transformer.py:264); the table's gradient
    d_logits^T x goes through the deterministic split-K reduction"""

    @staticmethod
    def forward(ctx, x, table):
        ctx.save_for_backward(x, table)
        return ops.scores_nt(x, table)

    @staticmethod
    @_needed_only
    def backward(ctx, d):
        x, table = ctx.saved_tensors
        d = _rows(d)
        M, V = d.shape
        D = table.shape[1]
        dx = ops.linear_fwd(d, table) if ctx.needs_input_grad[0] else None
        d_table = None
        if ctx.needs_input_grad[1]:
            d_table = _param_grad(table)
            ops.linear_bwd_dw(d, x, 1.0, d_table, None, workspace=ops.linear_bwd_dw_workspace(M, V, D, d.device))
        return dx, d_table


def tied_projection(x, table):
    """x [M, D] @ table[V, D]^T -> [M, V]"""
    return _TiedProjectionFn.apply(x, table)


_POOL_CACHE = {}


def global_average_pooling_1d(x):
    """tf.keras.layers.GlobalAveragePooling1D: the mean over axis 1 of [B, L, C], as the CSR product with the [B, B * L] pooling
    matrix (1 / L in every entry of a row's own L columns) -- dr_csr_spmm forward, its transpose backward, both in a fixed order"""
    B, L, C = x.shape
    key = (B, L, x.device)
    if key not in _POOL_CACHE:
        row_ptr = torch.arange(0, B + 1, dtype=torch.int64, device=x.device) * L
        col = torch.arange(0, B * L, dtype=torch.int32, device=x.device)
        val = torch.full((B * L,), 1.0 / L, dtype=torch.float32, device=x.device)
        _POOL_CACHE.clear()
        _POOL_CACHE[key] = SparseAdjacency._from_device(row_ptr, col, val, (B, B * L))
    return aggregate(_POOL_CACHE[key], x.reshape(B * L, C))


# ---- DIN: Dice and the fused interest pooling (csrc/din.hip) ----------------------------------------------------------------------------
class _DiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alpha, eps):
        ctx.eps = eps
        ctx.save_for_backward(x, alpha)
        return ops.dice_fwd(x, alpha, eps)

    @staticmethod
    @_needed_only
    def backward(ctx, dy):
        x, alpha = ctx.saved_tensors
        dx, dalpha = ops.dice_bwd(x, alpha, _rows(dy), ctx.eps)
        return dx, dalpha, None


def dice(x, alpha, eps=1e-8):
    """Dice over the rows of x [M, N] with the per-feature PReLU parameter alpha [N] (din.py:88-130 of the reference, literally: the
    standard deviation gets a second square root).  Where a row is constant (always for N == 1) the gradient's term through the
    standard deviation is taken as zero; TensorFlow returns NaN there."""
    return _DiceFn.apply(x, alpha, float(eps))


class _DinPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, query, keys, mask, W, b, w_out, b_out, mode, act, alpha, eps):
        out, scores = ops.din_pool_fwd(query, keys, mask, W, b, w_out, b_out, mode, act, alpha, eps)
        ctx.cfg = (mode, act, eps, w_out.shape)
        ctx.save_for_backward(query, keys, mask, W, b, w_out, b_out, alpha)
        return out, scores

    @staticmethod
    @_needed_only
    def backward(ctx, d_out, d_scores):
        query, keys, mask, W, b, w_out, b_out, alpha = ctx.saved_tensors
        mode, act, eps, wo_shape = ctx.cfg
        d_q, d_k, dW, db, d_wo, d_bo, dalpha = ops.din_pool_bwd(query, keys, mask, W, b, w_out, b_out, mode, act,
                                                                _rows(d_out, aligned=True, dense=True), _rows(d_scores, dense=True), alpha, eps)
        return d_q, d_k, None, dW, db, d_wo.reshape(wo_shape), d_bo, None, None, (dalpha if alpha is not None else None), None


def din_interest_pooling(query, keys, mask, W, b, w_out, b_out, mode, act, alpha=None, eps=1e-8):
    """(out [B, D], scores [B, T]): DIN's local activation unit Dense(1)(act(concat([q, k, inter(q, k)]) W + b)) scored for every key
    keys[b, t] against query[b], zero where mask[b, t] == 0 (mask None: all valid), and out[b] = sum_t scores[b, t] keys[b, t] -- no
    softmax, as in the paper.  mode 0 / 1 / 2: no interacter / q - k / q * k; act 0..3 as in mlp, 4 = Dice over the hidden units with
    alpha [U] and eps.  Masked keys are skipped, not multiplied by zero: what they hold reaches no result and their gradient is exactly
    0.  One kernel forward; the backward recomputes the hidden layer and keeps only its [B * T, U] gradient."""
    return _DinPoolFn.apply(query, keys, mask, W, b, w_out, b_out, int(mode), int(act), alpha, float(eps))


# ---- xDeepFM: the CIN layer with its sum pooling, and a stack of them (csrc/cin_pool.hip) -------------------------------------------------
class _CinPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, x, W, bias, act, want_out):
        out, pooled = ops.cin_pool_fwd(x0, x, W, bias, act, want_out=want_out or act != 0)
        ctx.act, ctx.has_bias = act, bias is not None
        ctx.save_for_backward(x0, x, W, out)
        if not want_out:
            return None, pooled
        return out, pooled

    @staticmethod
    @_needed_only
    def backward(ctx, d_out, d_pooled):
        x0, x, W, out = ctx.saved_tensors
        if d_out is None and d_pooled is None:
            return None, None, None, None, None, None
        # one layer cannot know what else feeds x0: d_x0 is returned and autograd adds (cin_stack below is where accumulate_x0 is used)
        d_x0, d_x, dW, dbias = ops.cin_pool_bwd(x0, x, W, ctx.act, out, _rows(d_out, dense=True), _rows(d_pooled, dense=True),
                                                want_bias=ctx.has_bias)
        return d_x0, d_x, dW, dbias, None, None


def cin_pool(x0, x, W, bias=None, act=0, want_out=True):
    """(out [B, Fm, D] | None, pooled [B, Fm]) of one CIN layer: out = act(conv1d(x0 (x) x, W) + bias), pooled = out.sum(-1), one kernel.
    want_out=False returns no out (a stack's last layer is only read through its pooling); with a non-linear act it is still computed
    and kept for the backward.  The backward takes either gradient being absent and returns d_x0 for autograd to add."""
    return _CinPoolFn.apply(x0, x, W, bias, int(act), bool(want_out))


class _CinStackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, act, n, *params):
        Ws, biases = params[:n], params[n:]
        outs, pooled = [], []
        x = x0
        for k in range(n):
            last = k == n - 1
            out, p = ops.cin_pool_fwd(x0, x, Ws[k], biases[k], act, want_out=not last or act != 0)
            outs.append(out)
            pooled.append(p)
            x = out
        ctx.act, ctx.n = act, n
        ctx.has_bias = [b is not None for b in biases]
        ctx.last_out = outs[-1] is not None
        ctx.save_for_backward(x0, *Ws, *[o for o in outs if o is not None])
        return torch.cat(pooled, dim=1) if n > 1 else pooled[0]

    @staticmethod
    @_needed_only
    def backward(ctx, d_res):
        n = ctx.n
        saved = ctx.saved_tensors
        x0, Ws = saved[0], saved[1:1 + n]
        outs = list(saved[1 + n:]) + ([] if ctx.last_out else [None])
        sizes = [W.shape[1] for W in Ws]
        offs = [sum(sizes[:k]) for k in range(n)]
        # every layer sends a gradient to the same x0: the last layer's call writes d_x0 and the others add to it in the kernel
        # (accumulate_x0); only the first layer's d_x, whose x IS x0, costs an elementwise add
        d_x0, d_next = None, None
        d_res = _rows(d_res)
        dWs, dbs = [None] * n, [None] * n
        for k in reversed(range(n)):
            xk = x0 if k == 0 else outs[k - 1]
            d_x0, d_next, dWs[k], dbs[k] = ops.cin_pool_bwd(x0, xk, Ws[k], ctx.act, outs[k], d_next, _rows(d_res[:, offs[k]:offs[k] + sizes[k]], dense=True),
                                                            want_bias=ctx.has_bias[k], d_x0=d_x0)
        d_x0 += d_next
        return (d_x0, None, None) + tuple(dWs) + tuple(dbs)


def cin_stack(x0, Ws, biases, act=0):
    """[B, sum Fm_k]: the pooled outputs of x_k = CIN(x0, x_{k-1}; Ws[k], biases[k]), x_0 = x0, concatenated (xDeepFM's direct connection).
    The last layer's out is not written when act is linear.  One autograd node, so the backward accumulates d_x0 inside the kernels."""
    n = len(Ws)
    if n == 0 or len(biases) != n:
        raise ValueError("cin_stack: one W and one bias (or None) per layer, at least one layer")
    return _CinStackFn.apply(x0, int(act), n, *Ws, *biases)


# ---- DLRM: the pairwise dot interaction (csrc/dot_interact.hip) ------------------------------------------------------------------------
class _DotInteractFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dense, emb, F, D, self_interaction):
        ctx.F, ctx.D, ctx.self_interaction = F, D, self_interaction
        ctx.emb_shape = emb.shape
        ctx.save_for_backward(dense, emb)
        return ops.dot_interact_fwd(dense, emb, F, D, self_interaction)

    @staticmethod
    @_needed_only
    def backward(ctx, d_out):
        dense, emb = ctx.saved_tensors
        d_out = _rows(d_out, pitch4=True, aligned=True)       # the kernel reads rows at a pitch that is a multiple of 4
        d_dense, d_emb = ops.dot_interact_bwd(dense, emb, ctx.F, ctx.D, d_out, ctx.self_interaction)
        return d_dense, d_emb.reshape(ctx.emb_shape), None, None, None


def dot_interaction(dense, emb, self_interaction=False):
    """[B, c0 + P]: DLRM's interaction of the vectors T = [dense; emb's fields] of every example -- dense [B, D] (or None) copied to the
    first c0 = D columns (c0 = 0 without it), then the row-major lower triangle of T T^T (the diagonal included only with
    self_interaction), P = N (N -+ 1) / 2 columns.  emb: [B, F, D] contiguous; a [B, F * D] matrix (a column-strided view of the slab's
    concat is read in place) needs dense to tell D, or else pass it as [B, F, D].  One kernel each way; no [B, N, N] matrix."""
    if emb.dim() == 3:
        F, D = int(emb.shape[1]), int(emb.shape[2])
    elif emb.dim() == 2 and dense is not None and dense.dim() == 2 and dense.shape[1] > 0 and emb.shape[1] % dense.shape[1] == 0:
        D = int(dense.shape[1])
        F = int(emb.shape[1]) // D
    else:
        raise ValueError("dot_interaction: emb must be [B, F, D], or [B, F * D] next to a dense [B, D]; got emb %s, dense %s"
                         % (tuple(emb.shape), None if dense is None else tuple(dense.shape)))
    return _DotInteractFn.apply(dense, emb, F, D, bool(self_interaction))


# ---- AFM: attention pooling over field pairs (csrc/afm_pool.hip) -----------------------------------------------------------------------
class _AfmPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, W, b, h, F, want_attention):
        out, lse, attn = ops.afm_pool_fwd(emb, W, b, h, F, want_attention)
        ctx.F = F
        ctx.emb_shape = emb.shape
        ctx.save_for_backward(emb, W, b, h, out, lse)
        if attn is None:
            return out, None
        ctx.mark_non_differentiable(attn)
        return out, attn

    @staticmethod
    @_needed_only
    def backward(ctx, d_out, _d_attn):
        emb, W, b, h, out, lse = ctx.saved_tensors
        d_emb, dW, db, dh = ops.afm_pool_bwd(emb, W, b, h, ctx.F, out, lse, _rows(d_out, pitch4=True, aligned=True))
        return d_emb.reshape(ctx.emb_shape), dW, db, dh, None, None


def afm_pooling(emb, W, b, h, want_attention=False, F=None):
    """(out [B, D], attn [B, P] | None): AFM's attention pooling of the pair products e_i * e_j (j < i, P = F (F - 1) / 2 pairs in
    DotInteraction's order): z = p W + b, s = relu(z) h, attn = softmax over the pairs, out = sum_q attn_q p_q.  emb: [B, F, D]
    contiguous, or a [B, F * D] matrix (a column-strided view of the slab's concat is read in place) together with F; W [D, A], b [A],
    h [A].  One kernel each way, no [B, P, .] tensor; attn carries no gradient."""
    if emb.dim() == 3:
        if F is not None and int(F) != emb.shape[1]:
            raise ValueError("afm_pooling: F = %d does not match emb %s" % (int(F), tuple(emb.shape)))
        F = int(emb.shape[1])
    elif emb.dim() != 2 or F is None:
        raise ValueError("afm_pooling: emb must be [B, F, D], or [B, F * D] together with F; got emb %s, F %s" % (tuple(emb.shape), F))
    return _AfmPoolFn.apply(emb, W, b, h, int(F), bool(want_attention))


# ---- PNN: the outer-product layer (csrc/pnn_outer.hip) ------------------------------------------------------------------------------------
class _PnnOuterFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, W, addend, F):
        out, u = ops.pnn_outer_fwd(emb, W, F, addend)
        ctx.F = F
        ctx.emb_shape = emb.shape
        ctx.has_addend = addend is not None
        ctx.save_for_backward(u, W)
        return out

    @staticmethod
    @_needed_only
    def backward(ctx, d_out):
        u, W = ctx.saved_tensors
        d_emb, dW = ops.pnn_outer_bwd(u, W, ctx.F, _rows(d_out, pitch4=True, aligned=True))
        return d_emb.reshape(ctx.emb_shape), dW, (d_out if ctx.has_addend else None), None


def pnn_outer(emb, W, addend=None, F=None):
    """[B, N]: PNN's outer-product layer.  With u = the sum of the F field rows of an example, out[n] = sum_{d,e} u_d u_e W[d * D + e, n]
    (+ addend[n]): (u (x) u) flattened row-major times W [D * D, N], without the [B, D * D] matrix.  emb: [B, F, D] contiguous, or a
    [B, F * D] matrix (a column-strided view of the slab's concat is read in place) together with F.  The backward keeps u only; the
    addend's gradient is the output's."""
    if emb.dim() == 3:
        if F is not None and int(F) != emb.shape[1]:
            raise ValueError("pnn_outer: F = %d does not match emb %s" % (int(F), tuple(emb.shape)))
        F = int(emb.shape[1])
    elif emb.dim() != 2 or F is None:
        raise ValueError("pnn_outer: emb must be [B, F, D], or [B, F * D] together with F; got emb %s, F %s" % (tuple(emb.shape), F))
    return _PnnOuterFn.apply(emb, W, addend, int(F))


class _ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        y = ops.act_fwd_(x.clone(memory_format=torch.contiguous_format), act)
        ctx.act = act
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @_needed_only
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.act_bwd_(y, dy.clone(memory_format=torch.contiguous_format), ctx.act), None


def activation(x, act):
    """act(x) for a [M, N] matrix that is the sum of several layers' outputs; act: 0 linear, 1 relu, 2 sigmoid, 3 tanh (dr_act_fwd)"""
    return x if int(act) == 0 else _ActFn.apply(x, int(act))


# ---- DIEN: the GRU / AUGRU recurrence and the evolution layer's attention (csrc/dien.hip) -------------------------------------------------
class _GruSeqFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xp, U, h0, lengths, att):
        hs, h_last = ops.gru_seq_fwd(xp, U, h0, lengths, att)
        ctx.lengths = lengths
        ctx.save_for_backward(xp, U, h0, att, hs)
        return hs, h_last

    @staticmethod
    @_needed_only
    def backward(ctx, d_hs, d_h_last):
        xp, U, h0, att, hs = ctx.saved_tensors
        d_xp, dU, d_h0, d_att = ops.gru_seq_bwd(xp, U, h0, ctx.lengths, att, hs, _rows(d_hs, pitch4=True, aligned=True),
                                                _rows(d_h_last, dense=True))
        return d_xp, dU, (d_h0 if h0 is not None else None), None, d_att


def gru_sequence(xp, U, h0=None, lengths=None, att=None):
    """(hs [B, T, H], h_last [B, H]): the GRU recurrence over the input-side pre-activations xp [B, T, 3H] = x W + b (gate columns
    [u | r | c], the paper's form: h_t = (1 - u) h_{t-1} + u c with c = tanh(xp_c + r * (h_{t-1} U_c))), U [H, 3H], h0 [B, H] (None:
    zeros).  lengths [B]: steps t >= lengths[b] carry the state, give hs[b, t] = 0 and read neither xp nor att there.  att [B, T]
    turns it into DIEN's AUGRU (the update gate is scaled by att[b, t]) and receives a gradient.  One kernel forward (the time loop
    runs on chip); the backward recomputes the gates and keeps nothing per step but hs."""
    return _GruSeqFn.apply(xp, U, h0, lengths, att)


class _SeqAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hs, q, lengths):
        a = ops.seq_attn_fwd(hs, q, lengths)
        ctx.lengths = lengths
        ctx.save_for_backward(hs, q, a)
        return a

    @staticmethod
    @_needed_only
    def backward(ctx, d_a):
        hs, q, a = ctx.saved_tensors
        d_hs, d_q = ops.seq_attn_bwd(hs, q, ctx.lengths, a, _rows(d_a, dense=True))
        return d_hs, d_q, None


def sequence_attention(hs, q, lengths=None):
    """a [B, T]: the softmax over the valid steps t < lengths[b] of <hs[b, t], q[b]>, 0 at masked steps (a row of zeros when
    lengths[b] == 0)."""
    return _SeqAttnFn.apply(hs, q, lengths)


# ---- FFM: the field-aware interaction (csrc/ffm.hip) -------------------------------------------------------------------------------------
class _FfmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, F, k):
        ctx.F, ctx.k = F, k
        ctx.rows_shape = rows.shape
        ctx.save_for_backward(rows)
        return ops.ffm_fwd(rows, F, k)

    @staticmethod
    @_needed_only
    def backward(ctx, d_inter):
        rows, = ctx.saved_tensors
        d_rows = ops.ffm_bwd(rows, ctx.F, ctx.k, _rows(d_inter, dense=True))
        return d_rows.reshape(ctx.rows_shape), None, None


def ffm_interaction(rows, F, k):
    """inter [B]: FFM's sum over the pairs of fields j < i of <A[i, j, :], A[j, i, :]>, A [F, F, k] being the example's F gathered rows of
    F k-vectors each (block j of row i = field i's factor towards field j).  rows: [B, F, F, k] or [B, F, F * k] contiguous, or a
    [B, F * F * k] matrix (a column-strided view of the slab's concat is read in place).  One kernel each way; the diagonal blocks are
    never read and get a gradient of exactly 0."""
    return _FfmFn.apply(rows, int(F), int(k))


class _FfmGatherFn(torch.autograd.Function):
    """dr_ffm_gather_fwd forward; dr_ffm_gather_bwd then K4 backward.  `sparse_lr` as in _EmbPoolFn: None produces dense gradient
    buffers, a value applies the fused SGD update in place to the slab."""

    @staticmethod
    def forward(ctx, table, lin_w, lin_bias, ids, row_base, F, k, sparse_lr):
        inter, first = ops.ffm_gather_fwd(ids, row_base, table, F, k, lin_w, lin_bias)
        ctx.F, ctx.k, ctx.sparse_lr = F, k, sparse_lr
        ctx.has_bias = lin_bias is not None and lin_w is not None
        ctx.bias_data = lin_bias.data if ctx.has_bias else None
        ctx.save_for_backward(table, lin_w, ids, row_base)
        return inter, first

    @staticmethod
    @_needed_only
    def backward(ctx, d_inter, d_first):
        table, lin_w, ids, row_base = ctx.saved_tensors
        F, k = ctx.F, ctx.k
        if lin_w is None:
            d_first = None
        if d_inter is None and d_first is None:
            return (None,) * 8
        d_rows = ops.ffm_gather_bwd(ids, row_base, table, F, k, _rows(d_inter, dense=True)) if d_inter is not None else None
        d_first = _rows(d_first, dense=True)
        has_bias = ctx.has_bias and d_first is not None
        col_start = torch.arange(F + 1, dtype=torch.int32, device=ids.device)
        if ctx.sparse_lr is None:
            g_table = _param_grad(table)
            g_lin = _param_grad(lin_w) if lin_w is not None else None
            g_bias = torch.zeros(1, dtype=torch.float32, device=table.device) if has_bias else None
            ops.emb_pool_bwd(ids, F, col_start, row_base, F * k, d_rows, None, None, d_first, 1.0, g_table, g_lin, g_bias)
            return g_table, g_lin, g_bias, None, None, None, None, None
        ops.emb_pool_bwd(ids, F, col_start, row_base, F * k, d_rows, None, None, d_first, -float(ctx.sparse_lr), table.data,
                         lin_w.data if lin_w is not None else None, ctx.bias_data if has_bias else None)
        return (None,) * 8


def ffm_gather(table, lin_w, lin_bias, ids, row_base, F, k, sparse_lr=None):
    """(inter [B], first_order [B] | None) for single-valued fields, ids [B, F]: FFM's interaction computed straight from the table rows
    table[row_base[f] + ids[b, f]] ([R, F * k]; an id < 0 is a row of zeros) without writing them, and lin_bias + sum_f lin_w[row] when
    lin_w is given.  The backward writes d_rows once (dr_ffm_gather_bwd) and hands it to K4, which owns duplicate rows, the first-order
    gradient and, with `sparse_lr`, the fused SGD step."""
    return _FfmGatherFn.apply(table, lin_w, lin_bias, ids, row_base, int(F), int(k), sparse_lr)


# ---- skip-gram with negative sampling (csrc/sgns.hip) -------------------------------------------------------------------------------------
def sgns_apply_rows(table, ids, d_rows, scale, plan=None, scratch=None, row_base=None):
    """table[ids[b, f], :] += scale * d_rows[b, f * D : (f + 1) * D] for every id >= 0 of ids [B, F] through K4: dr_emb_pool_bwd (fp32
    atomics) without a plan; with an ops.SortPlan the plan is rebuilt for these ids and dr_emb_pool_bwd_sorted sums the slots of a
    shared row in a fixed order, hot rows through `scratch` ([B * F, D], clobbered; allocated when None).  `row_base` (int64 [F] on
    the device) makes field f's row row_base[f] + ids[b, f], as the slab's fields share one table; None: every field starts at row 0.
    Returns the plan used."""
    B, F = ids.shape
    D = table.shape[1]
    if row_base is None:
        row_base = torch.zeros(F, dtype=torch.int64, device=ids.device)
    if plan is None:
        col_start = torch.arange(F + 1, dtype=torch.int32, device=ids.device)
        ops.emb_pool_bwd(ids, F, col_start, row_base, D, d_rows, None, None, None, scale, table, None, None)
        return None
    plan = ops.emb_sort_slots(ids, row_base, table.shape[0], plan)
    if scratch is None or scratch.shape[0] < B * F:
        scratch = torch.empty((B * F, D), dtype=torch.float32, device=ids.device)
    ops.emb_pool_bwd_sorted(ids, row_base, plan, D, table.shape[0], d_rows, None, scale, table, x_sorted=scratch)
    return plan


class _SgnsFn(torch.autograd.Function):
    """dr_sgns_fwd forward; dr_sgns_bwd then K4 on each table backward.  `sparse_lr` as in _EmbPoolFn.  `plans`: None, or a pair of
    ops.SortPlan (for ids [B, 1] and [B, 1 + K]): the sorted K4, bit-reproducible on hot rows."""

    @staticmethod
    def forward(ctx, in_table, out_table, centers, contexts, negatives, sample_weight, skip_equal, sparse_lr, plans):
        loss, coeff, _, _, _ = ops.sgns_fwd(in_table, out_table, centers, contexts, negatives, sample_weight, skip_equal)
        ctx.skip_equal, ctx.sparse_lr, ctx.plans = skip_equal, sparse_lr, plans
        ctx.save_for_backward(in_table, out_table, centers, contexts, negatives, coeff)
        return loss

    @staticmethod
    @_needed_only
    def backward(ctx, d_loss):
        in_table, out_table, centers, contexts, negatives, coeff = ctx.saved_tensors
        if d_loss is None:
            return (None,) * 9
        B = centers.shape[0]
        d_center, d_ctx = ops.sgns_bwd(in_table, out_table, centers, contexts, negatives, coeff, _rows(d_loss, dense=True), ctx.skip_equal)
        ids_in = centers.reshape(B, 1)
        ids_out = contexts.reshape(B, 1) if negatives is None else torch.cat([contexts.reshape(B, 1), negatives], dim=1)
        plan_in, plan_out = ctx.plans if ctx.plans is not None else (None, None)
        want_in, want_out = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if ctx.sparse_lr is None:                 # both gradients come from the rows as the forward read them
            g_in = _param_grad(in_table) if want_in else None
            g_out = _param_grad(out_table) if want_out else None
            if want_in:
                sgns_apply_rows(g_in, ids_in, d_center, 1.0, plan_in)
            if want_out:
                sgns_apply_rows(g_out, ids_out, d_ctx, 1.0, plan_out)
            return g_in, g_out, None, None, None, None, None, None, None
        if want_in:                               # d_center and d_ctx are complete before either table is touched
            sgns_apply_rows(in_table.data, ids_in, d_center, -float(ctx.sparse_lr), plan_in)
        if want_out:
            sgns_apply_rows(out_table.data, ids_out, d_ctx, -float(ctx.sparse_lr), plan_out)
        return (None,) * 9


def sgns_loss(in_table, out_table, centers, contexts, negatives, sample_weight=None, skip_equal=True, sparse_lr=None, plans=None):
    """loss_rows [B] of skip-gram with negative sampling: w_b (softplus(-<u, v_0>) + sum_{j >= 1} softplus(<u, v_j>)) with u =
    in_table[centers[b]], v_0 = out_table[contexts[b]], v_j = out_table[negatives[b, j - 1]].  An example whose center or context is < 0
    is skipped (loss 0), so is a negative < 0 and, with skip_equal, a negative equal to the context.  One gather kernel each way; the
    table gradients go through K4 (`sparse_lr` None: dense .grad buffers; a value: the fused SGD step in place; `plans`: a pair of
    ops.SortPlan for the deterministic K4)."""
    return _SgnsFn.apply(in_table, out_table, centers, contexts, negatives, sample_weight, bool(skip_equal), sparse_lr, plans)


# ---- skip-gram with side information (csrc/eges.hip) ---------------------------------------------------------------------------------------
class _EgesFn(torch.autograd.Function):
    """dr_eges_fwd forward; dr_eges_bwd then K4 on each of the three tables backward (side_table: ids side_ids with row_base; att: ids
    att_ids as [B, 1], its rows d_att [B, pad4(S)]; out_table: ids [contexts | negatives]).  `sparse_lr` as in _SgnsFn.  `plans`:
    None, or three ops.SortPlan in that order: the sorted K4, bit-reproducible on shared rows."""

    @staticmethod
    def forward(ctx, side_table, att, out_table, row_base, side_ids, att_ids, contexts, negatives, sample_weight, skip_equal, sparse_lr,
                plans):
        loss, coeff, alpha, _, _, _, _ = ops.eges_fwd(side_table, row_base, side_ids, att, att_ids, out_table, contexts, negatives,
                                                      sample_weight, skip_equal)
        ctx.skip_equal, ctx.sparse_lr, ctx.plans, ctx.has_att = skip_equal, sparse_lr, plans, att is not None
        ctx.save_for_backward(side_table, att, out_table, row_base, side_ids, att_ids, contexts, negatives, coeff, alpha)
        return loss

    @staticmethod
    @_needed_only
    def backward(ctx, d_loss):
        side_table, att, out_table, row_base, side_ids, att_ids, contexts, negatives, coeff, alpha = ctx.saved_tensors
        if d_loss is None:
            return (None,) * 12
        B = side_ids.shape[0]
        d_side, d_att, d_ctx = ops.eges_bwd(side_table, row_base, side_ids, att, att_ids, out_table, contexts, negatives, coeff, alpha,
                                            _rows(d_loss, dense=True), ctx.skip_equal)
        ids_out = contexts.reshape(B, -1) if negatives is None else torch.cat([contexts.reshape(B, -1), negatives], dim=1)
        plan_side, plan_att, plan_out = ctx.plans if ctx.plans is not None else (None, None, None)
        want_side, want_att, want_out = ctx.needs_input_grad[0], ctx.has_att and ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if want_att and att.shape[1] != d_att.shape[1]:
            raise ValueError("eges_loss: a trainable att must be [R, %d] (S rounded up to a multiple of 4: K4's row), got %s"
                             % (d_att.shape[1], tuple(att.shape)))
        if ctx.sparse_lr is None:                 # all three gradients come from the rows as the forward read them
            g_side = _param_grad(side_table) if want_side else None
            g_att = _param_grad(att) if want_att else None
            g_out = _param_grad(out_table) if want_out else None
            scale = 1.0
        else:                                     # the three buffers are complete before any table is touched
            g_side, g_att, g_out = side_table.data, att.data if want_att else None, out_table.data
            scale = -float(ctx.sparse_lr)
        if want_side:
            sgns_apply_rows(g_side, side_ids, d_side, scale, plan_side, row_base=row_base)
        if want_att:
            sgns_apply_rows(g_att, att_ids.reshape(B, 1), d_att, scale, plan_att)
        if want_out:
            sgns_apply_rows(g_out, ids_out, d_ctx, scale, plan_out)
        if ctx.sparse_lr is not None:
            return (None,) * 12
        return (g_side, g_att, g_out) + (None,) * 9


def eges_loss(side_table, row_base, side_ids, att, att_ids, out_table, contexts, negatives, sample_weight=None, skip_equal=True,
              sparse_lr=None, plans=None):
    """loss_rows [B] of skip-gram with side information (EGES): sgns_loss whose centre vector is sum_s alpha_s w_s over the fields of
    the example that are present (side_ids[b, s] >= 0), w_s = side_table[row_base[s] + side_ids[b, s]], alpha = softmax of
    att[att_ids[b], :S] over those fields (att None or att_ids[b] < 0: their average, the cold-start rule).  contexts int64 [B, P]
    (or [B]) are positives, negatives int64 [B, K]; an example with no field or contexts[b, 0] < 0 is skipped (loss 0), so is a slot
    with an id < 0 and, with skip_equal, a negative equal to one of the example's positives.  One gather kernel each way; the
    gradients of side_table, att ([R, S rounded up to a multiple of 4]) and out_table go through K4 (`sparse_lr` None: dense .grad
    buffers; a value: the fused SGD step in place; `plans`: three ops.SortPlan for the deterministic K4)."""
    return _EgesFn.apply(side_table, att, out_table, row_base, side_ids, att_ids, contexts, negatives, sample_weight, bool(skip_equal),
                         sparse_lr, plans)


def skipgram_pairs(seqs, window):
    """(centers, contexts), both int64 [N * L * 2 * window]: for every position (n, t) of seqs [N, L] (padded with -1) and every offset
    o in (-window .. -1, 1 .. window), the pair (seqs[n, t], seqs[n, t + o]).  An entry is -1 where the partner lies outside the
    sequence or either side is padding; nothing is compacted, the SGNS kernel skips those pairs.  Integer indexing in torch on seqs'
    device."""
    if seqs.dtype != torch.int64 or seqs.dim() != 2:
        raise ValueError("skipgram_pairs: seqs must be int64 [N, L], got %s %s" % (seqs.dtype, tuple(seqs.shape)))
    window = int(window)
    if window < 1:
        raise ValueError("skipgram_pairs: window must be >= 1, got %d" % window)
    N, L = seqs.shape
    offs = torch.tensor([o for o in range(-window, window + 1) if o != 0], dtype=torch.int64, device=seqs.device)
    pos = torch.arange(L, dtype=torch.int64, device=seqs.device)[:, None] + offs[None, :]            # [L, 2 window]
    inside = (pos >= 0) & (pos < L)
    partner = seqs[:, pos.clamp(0, max(L - 1, 0)).reshape(-1)].reshape(N, L, 2 * window)
    center = seqs[:, :, None].expand(N, L, 2 * window)
    ok = inside[None, :, :] & (partner >= 0) & (center >= 0)
    minus = torch.full_like(partner, -1)
    return torch.where(ok, center, minus).reshape(-1), torch.where(ok, partner, minus).reshape(-1)


# ---- sampled softmax (csrc/sampled_softmax.hip) ---------------------------------------------------------------------------------------------
def sampled_softmax(u, table, labels, sampled, log_q_true=None, log_q_sampled=None, sample_weight=None, remove_accidental_hits=True,
                    row_scale=1.0):
    """(loss_rows [B], d_u [B, D], d_true [B, D], d_sampled [S, D]) of tf.nn.sampled_softmax_loss with num_true = 1 and NO per-class bias
    (the paper's softmax has none; TensorFlow's users pass zeros): loss_i = w_i (log(exp(t_i) + sum_j exp(s_ij)) - t_i), t_i =
    u_i . table[labels_i] - log_q_true_i, s_ij = u_i . table[sampled_j] - log_q_sampled_j over the S classes `sampled` that the whole
    batch shares, an accidental hit (sampled_j == labels_i) left out.  A training-step op like ops.sgns_fwd with row_scale, computed on
    u.detach(): the three buffers are the gradients of row_scale * sum(loss_rows); the caller continues with u.backward(d_u) and hands
    d_true (ids labels [B, 1]) and d_sampled (ids sampled [S, 1]) to sgns_apply_rows.  A row with labels_i < 0 is padding (loss 0, zero
    gradient rows, its u_i never read as a value); a sampled id < 0 is left out.  No [B, S] tensor is written."""
    ud, td = u.detach(), table.detach()
    ws = ops.sampled_softmax_workspace(ud.shape[0], sampled.shape[0], td.shape[1], td.device) if ud.dim() == 2 and td.dim() == 2 else None
    true_logit, row_lse, loss_rows, _ = ops.sampled_softmax_fwd(ud, td, labels, sampled, log_q_true, log_q_sampled, sample_weight,
                                                                remove_accidental_hits, workspace=ws)
    d_u, d_true, d_sampled = ops.sampled_softmax_bwd(ud, td, labels, sampled, true_logit, row_lse, log_q_sampled, sample_weight,
                                                     remove_accidental_hits, row_scale, workspace=ws)
    return loss_rows, d_u, d_true, d_sampled


# ---- full-vocabulary cross-entropy over integer labels (csrc/bert.hip) ---------------------------------------------------------------------
VOCAB_CE_BUFFER_BYTES = 256 << 20      # the default chunk_rows keeps the [chunk, pad4(V)] logits buffer at or below this
VOCAB_CE_WORKSPACE_BYTES = 128 << 20   # the split-K partials of the table's gradient: the table's rows are taken in blocks that fit


def vocab_cross_entropy(t, table, bias, labels, weight=None, smoothing=0.0, row_scale=1.0, denom=None, denom_eps=0.0, d_table=None,
                        d_bias=None, chunk_rows=None):
    """(loss_rows [M], d_t [M, D]) of the softmax cross-entropy of t @ table^T + bias against integer labels [M] (a masked-LM head
    whose decoder is tied to the token table [V, D]), and d_table [V, D] / d_bias [V] += their gradients where given.  loss_r and the
    gradient are dr_softmax_ce_ids': weight w_r, label smoothing, a negative label = padding; the buffers hold the gradients of
    row_scale / (denom + denom_eps) * sum(loss_rows), denom a one-element DEVICE tensor (BERT's sum of the weights: no host read),
    and loss_rows is NOT divided by it.  A training-step op on detached inputs, like sampled_softmax: the caller continues with
    t.backward(d_t).  The [M, V] logits are never whole in memory: for each chunk of chunk_rows rows, in ascending order,
    ops.scores_nt writes the chunk's logits into one reused buffer, ops.softmax_ce_ids turns them into the gradient in place, the
    dx GEMM g @ table (ops.linear_fwd, the product tied_projection's backward runs) gives d_t's rows, ops.linear_bwd_dw
    (deterministic split-K form) adds into d_table and ops.colsum_add into d_bias.  chunk_rows defaults to the largest value that
    keeps the buffer at or below 256 MiB.
    For a FIXED chunk_rows everything is bit-identical from run to run.  Across different chunk_rows only agreement within fp32
    summation error is promised: d_table and d_bias are accumulated chunk by chunk, so their summation order follows the chunking
    (loss_rows and d_t are per-row results and do not change)."""
    td, tb = t.detach(), table.detach()
    if td.dim() != 2 or tb.dim() != 2 or td.shape[1] != tb.shape[1] or td.dtype != torch.float32 or tb.dtype != torch.float32:
        raise ValueError("vocab_cross_entropy: t must be fp32 [M, D] and table fp32 [V, D], got %s and %s" % (tuple(t.shape), tuple(table.shape)))
    M, D = td.shape
    V = tb.shape[0]
    dev = td.device
    if D % 4 != 0 or not tb.is_contiguous():
        raise ValueError("vocab_cross_entropy: table must be contiguous with a width that is a multiple of 4, got %s" % (tuple(tb.shape),))
    if td.stride(1) != 1 or td.stride(0) % 4 != 0 or td.stride(0) < D or td.data_ptr() % 16 != 0:
        td = td.contiguous()                                  # rows the GEMMs read as float4
    bias = bias.detach() if bias is not None else None
    if labels.dtype != torch.int64 or tuple(labels.shape) != (M,) or not labels.is_contiguous():
        raise ValueError("vocab_cross_entropy: labels must be contiguous int64 [M]")
    if weight is not None and (weight.dtype != torch.float32 or tuple(weight.shape) != (M,) or not weight.is_contiguous()):
        raise ValueError("vocab_cross_entropy: weight must be contiguous fp32 [M]")
    if d_table is not None and (d_table.dtype != torch.float32 or tuple(d_table.shape) != (V, D) or not d_table.is_contiguous()):
        raise ValueError("vocab_cross_entropy: d_table must be contiguous fp32 [V, D]")
    Vp = _pad4(V)
    if chunk_rows is None:
        chunk_rows = max(1, VOCAB_CE_BUFFER_BYTES // (4 * Vp))
    chunk_rows = max(1, min(int(chunk_rows), max(M, 1)))
    loss_rows = torch.empty(M, dtype=torch.float32, device=dev)
    d_t = torch.empty((M, _pad4(D)), dtype=torch.float32, device=dev)[:, :D]
    if M == 0:
        return loss_rows, d_t
    buf = torch.empty((chunk_rows, Vp), dtype=torch.float32, device=dev)
    ws_dw, ws_cs, v_block = None, None, V
    if d_table is not None:
        # the deterministic dW keeps `split` partial [rows, D] products: the table's rows go in blocks (a function of the shapes
        # alone) small enough for that workspace to stay at or below VOCAB_CE_WORKSPACE_BYTES, one buffer for every chunk and block
        sizes = {chunk_rows, M % chunk_rows or chunk_rows}
        need = lambda vb: max(ops.lib().dr_linear_bwd_dw_workspace_bytes(m, v, D) for m in sizes for v in {vb, V % vb or vb})   # noqa: E731
        while v_block > 1024 and need(v_block) > VOCAB_CE_WORKSPACE_BYTES:
            v_block = _pad4((v_block + 1) // 2)
        ws_dw = torch.empty(max(1, need(v_block) // 4), dtype=torch.float32, device=dev)
    if d_bias is not None:
        ws_cs = ops.colsum_add_workspace(chunk_rows, V, dev)
    for r0 in range(0, M, chunk_rows):
        r1 = min(M, r0 + chunk_rows)
        t_c = td[r0:r1]
        g = buf[:r1 - r0, :V]
        ops.scores_nt(t_c, tb, out=g)
        ops.softmax_ce_ids(g, labels[r0:r1], bias, weight[r0:r1] if weight is not None else None, smoothing, row_scale, denom, denom_eps,
                           row_loss=loss_rows[r0:r1])
        ops.linear_fwd(g, tb, out=d_t[r0:r1])                        # d_t = g @ table, as tied_projection's backward
        if d_table is not None:
            for v0 in range(0, V, v_block):
                v1 = min(V, v0 + v_block)
                ops.linear_bwd_dw(g[:, v0:v1], t_c, 1.0, d_table[v0:v1], None, workspace=ws_dw)
        if d_bias is not None:
            ops.colsum_add(g, d_bias, ws_cs)
    return loss_rows, d_t


# ---- margin ranking loss (csrc/margin_rank.hip) -----------------------------------------------------------------------------------------------
def margin_rank(q, pos, neg=None, pos_ids=None, neg_ids=None, sample_weight=None, margin=0.2, metric="cosine", num_hard_negatives=0,
                row_scale=1.0):
    """(row_loss [B], row_active int32 [B], d_q [B, D], d_pos [B, D], d_neg [S, D] | None) of EBR's triplet loss: loss_i =
    w_i sum_{j in N(i)} max(0, margin - s(q_i, pos_i) + s(q_i, neg_j)), s the cosine (metric "dot": the dot product) and N(i) the kept
    negatives of row i, or its num_hard_negatives highest-scoring ones (online hard-negative mining).  neg=None is in-batch: the
    negatives of a row are the pos rows of the others; the part of the gradient that reaches pos as a negative is then already added,
    d_pos = d_pos + 1 * d_neg elementwise, and None is returned for d_neg.  A training-step op like sampled_softmax, computed on
    detached inputs: the buffers are the gradients of row_scale * sum(row_loss) with respect to the RAW q, pos and neg (the L2
    normalisation is inside the kernels); the caller continues with torch.autograd.backward([q, pos], [d_q, d_pos]).  A row with
    pos_ids_i < 0 is padding (loss 0, zero gradient rows, its q_i never read as a value); a negative with id < 0 is left out; with
    both id arrays a negative carrying the row's pos id is left out.  No [B, S] tensor is written."""
    qd, pd = q.detach(), pos.detach()
    nd = None if neg is None else neg.detach()
    _, K = ops.margin_rank_options(qd.shape[-1], metric, num_hard_negatives)
    ws = None
    if qd.dim() == 2 and (nd is None or nd.dim() == 2) and qd.shape[0] > 0:
        ws = ops.margin_rank_workspace(qd.shape[0], qd.shape[0] if nd is None else nd.shape[0], qd.shape[1], K, qd.device)
    pos_score, row_loss, row_active, hard_idx, _ = ops.margin_rank_fwd(qd, pd, nd, pos_ids, neg_ids, sample_weight, margin, metric, K,
                                                                       workspace=ws)
    d_q, d_pos, d_neg = ops.margin_rank_bwd(qd, pd, nd, pos_score, hard_idx, pos_ids, neg_ids, sample_weight, margin, metric, K,
                                            row_scale, workspace=ws)
    if nd is None:
        if d_pos.numel() > 0:
            ops.axpy(1.0, d_neg, d_pos)
        d_neg = None
    return row_loss, row_active, d_q, d_pos, d_neg
