"""Thin, shape-checked Python wrappers over the C-ABI kernels (one function per entry point), plus the
torch.autograd.Function glue that lets the reference-shaped model classes train with loss.backward().

Every function launches hand-written HIP kernels on torch's current stream; nothing here computes in
PyTorch.  Reference citations (relative to the reference root) are on the C-ABI declarations in
include/dr_hotpath.h.
"""
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr


def _c(t: torch.Tensor, dtype) -> torch.Tensor:
    if t.dtype != dtype:
        raise TypeError("expected %s, got %s" % (dtype, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


# ----------------------------------------------------------------------------------------------
# K1 / K2   integer id path
# ----------------------------------------------------------------------------------------------
def hash_bucket_i64(keys: torch.Tensor, col_buckets: torch.Tensor, out: Optional[torch.Tensor] = None):
    """keys [B, C] int64 -> ids [B, C]; col_buckets [C] uint64-as-int64 (0 = pass-through column)."""
    keys = _c(keys, torch.int64)
    B, C = keys.shape
    col_buckets = _c(col_buckets, torch.int64)
    assert col_buckets.numel() == C
    if out is None:
        out = torch.empty_like(keys)
    check(lib().dr_hash_bucket_i64(ptr(keys), B, C, ptr(col_buckets), ptr(out), stream_ptr()), "dr_hash_bucket_i64")
    return out


def _csr_bytes(values: Sequence, device):
    import numpy as np
    flat = [v if isinstance(v, (bytes, bytearray)) else str(v).encode("utf-8") for v in values]
    offs = np.zeros(len(flat) + 1, dtype=np.int64)
    if flat:
        offs[1:] = np.cumsum([len(b) for b in flat])
    blob = np.frombuffer(b"".join(flat) + b"\0", dtype=np.uint8).copy()
    return torch.from_numpy(blob).to(device), torch.from_numpy(offs).to(device), len(flat)


def hash_bucket_strings(values: Sequence, num_buckets: int, device="cuda"):
    """list of str/bytes -> ids [n]; "" -> -1.  (host strings are packed to CSR bytes, hashed on device)"""
    blob, offs, n = _csr_bytes(values, device)
    out = torch.empty(n, dtype=torch.int64, device=device)
    check(lib().dr_hash_bucket_bytes(ptr(blob), ptr(offs), n, int(num_buckets), ptr(out), stream_ptr()),
          "dr_hash_bucket_bytes")
    return out


def vocab_lookup_i64(keys: torch.Tensor, vocab: torch.Tensor):
    keys = _c(keys, torch.int64)
    vocab = _c(vocab, torch.int64)
    out = torch.empty_like(keys)
    check(lib().dr_vocab_lookup_i64(ptr(keys), keys.numel(), ptr(vocab), vocab.numel(), ptr(out), stream_ptr()),
          "dr_vocab_lookup_i64")
    return out


def vocab_lookup_strings(values: Sequence, vocab: Sequence, device="cuda"):
    blob, offs, n = _csr_bytes(values, device)
    vblob, voffs, m = _csr_bytes(vocab, device)
    out = torch.empty(n, dtype=torch.int64, device=device)
    check(lib().dr_vocab_lookup_bytes(ptr(blob), ptr(offs), n, ptr(vblob), ptr(voffs), m, ptr(out), stream_ptr()),
          "dr_vocab_lookup_bytes")
    return out


# ----------------------------------------------------------------------------------------------
# K3 / K4   fused embedding gather + pool (+ first-order + FM)
# ----------------------------------------------------------------------------------------------
def emb_pool_fwd(ids, F, col_start, row_base, table, lin_w=None, lin_bias=None, ld_concat=None,
                 want_sum_x=True, want_fm=True, concat=None, sum_x=None, fm_logit=None, second_order=True):
    ids = _c(ids, torch.int64)
    B, C = ids.shape
    D = table.shape[1]
    ld = F * D if ld_concat is None else ld_concat
    dev = ids.device
    if concat is None:
        concat = torch.empty((B, ld), dtype=torch.float32, device=dev)
        if ld > F * D:
            concat[:, F * D:].zero_()
    if want_sum_x and sum_x is None:
        sum_x = torch.empty((B, D), dtype=torch.float32, device=dev)
    if want_fm and fm_logit is None:
        fm_logit = torch.empty((B,), dtype=torch.float32, device=dev)
    check(lib().dr_emb_pool_fwd(ptr(ids), B, F, C, ptr(col_start), ptr(row_base), ptr(table), D, ptr(lin_w),
                                ptr(lin_bias), ptr(concat), ld, ptr(sum_x) if want_sum_x else None,
                                ptr(fm_logit) if want_fm else None, 0 if second_order else 1, stream_ptr()),
          "dr_emb_pool_fwd")
    return concat, sum_x, fm_logit


def lin_fields_fwd(ids, F, col_start, row_base, lin_w):
    """out[b, f] = sum over field f's bag of lin_w[row_base[f] + id] (FNN's per-field first-order inputs)."""
    ids = _c(ids, torch.int64)
    B, C = ids.shape
    out = torch.empty((B, _pad4(F)), dtype=torch.float32, device=ids.device)[:, :F]
    check(lib().dr_lin_fields_fwd(ptr(ids), B, F, C, ptr(col_start), ptr(row_base), ptr(lin_w), ptr(out), out.stride(0),
                                  stream_ptr()), "dr_lin_fields_fwd")
    return out


def lin_fields_bwd(ids, F, col_start, row_base, d_out, scale, dst_lin):
    ids = _c(ids, torch.int64)
    B, C = ids.shape
    _check_ld(d_out, "lin_fields_bwd: d_out")
    check(lib().dr_lin_fields_bwd(ptr(ids), B, F, C, ptr(col_start), ptr(row_base), ptr(d_out), d_out.stride(0), float(scale),
                                  ptr(dst_lin), stream_ptr()), "dr_lin_fields_bwd")


def emb_pool_bwd(ids, F, col_start, row_base, D, d_concat, concat, sum_x, d_fm_logit, scale, dst_table, dst_lin,
                 dst_bias=None):
    ids = _c(ids, torch.int64)
    B, C = ids.shape
    _check_ld(d_concat, "emb_pool_bwd: d_concat")
    check(lib().dr_emb_pool_bwd(ptr(ids), B, F, C, ptr(col_start), ptr(row_base), D,
                                ptr(d_concat), d_concat.stride(0) if d_concat is not None else 0,
                                ptr(concat), concat.stride(0) if concat is not None else 0,
                                ptr(sum_x), ptr(d_fm_logit), float(scale), ptr(dst_table), ptr(dst_lin),
                                ptr(dst_bias), stream_ptr()), "dr_emb_pool_bwd")


# ----------------------------------------------------------------------------------------------
# K6   stand-alone FM second order
# ----------------------------------------------------------------------------------------------
def fm2_fwd(x):
    x = _c(x, torch.float32)
    B, F, D = x.shape
    out = torch.empty((B, 1), dtype=torch.float32, device=x.device)
    check(lib().dr_fm2_fwd(ptr(x), B, F, D, ptr(out), stream_ptr()), "dr_fm2_fwd")
    return out


def fm2_bwd(x, d_out):
    x = _c(x, torch.float32)
    d_out = _c(d_out, torch.float32)
    B, F, D = x.shape
    dx = torch.empty_like(x)
    check(lib().dr_fm2_bwd(ptr(x), ptr(d_out), B, F, D, ptr(dx), stream_ptr()), "dr_fm2_bwd")
    return dx


# ----------------------------------------------------------------------------------------------
# K7 / K8   dense layers on fp32 MFMA
# ----------------------------------------------------------------------------------------------
def _pad4(n):
    return (n + 3) // 4 * 4


def _status(st, what):
    """check() for the entry points that validate their whole domain in C: an argument they refuse is a ValueError, as it is where
    the Python side sees it first"""
    if st in (_lib.DR_EINVAL, _lib.DR_ESHAPE):
        raise ValueError("%s: %s (outside the kernel's domain, or a base address that is not 16-byte aligned)" % (what, _lib._ERR[st]))
    check(st, what)


def _row_pitch(family, t, cols, what, written_to_pitch=False):
    """row stride of a [B, cols] fp32 matrix with unit column stride; ValueError (in `family`'s name) unless it is a multiple of 4 and
    >= cols.  A single row has no pitch to speak of, except where the kernel writes up to it (written_to_pitch: dot_interact's zero
    padding)."""
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != cols:
        raise ValueError("%s: %s must be fp32 [B, %d], got %s %s" % (family, what, cols, t.dtype, tuple(t.shape)))
    ok = t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= cols
    if not ok and t.shape[0] <= 1 and t.stride(1) == 1 and (cols % 4 == 0 or not written_to_pitch):
        return _pad4(cols)
    if not ok:
        raise ValueError("%s: %s needs unit column stride and a row stride that is a multiple of 4 and >= %d, got strides %s"
                         % (family, what, cols, tuple(t.stride())))
    return t.stride(0)


def _check_ld(t, what):
    """t [M, N] goes to a kernel with t.stride(0) as its leading dimension: unit column stride and, with more than one row, a row
    stride >= N.  A smaller one (0 for an expanded tensor) is no layout: every example would read the same or overlapping rows."""
    if t is None:
        return
    if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError("%s must be fp32 [M, N] with unit column stride and a row stride >= N, got %s %s with strides %s"
                         % (what, t.dtype, tuple(t.shape), tuple(t.stride())))


def _dense_arg(t, what, dtype=torch.float32, shape=None, numel=None, copy=True):
    """An argument a kernel addresses densely (row-major, no leading dimension): None passes; another dtype, shape or element count
    is a ValueError naming the argument; a view (transposed, pitched, expanded) is copied once when the kernel only reads it, and
    refused (copy=False) when the kernel writes to it -- a copy would swallow the result."""
    if t is None:
        return None
    if t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)) or (numel is not None and t.numel() != numel):
        raise ValueError("%s must be %s%s, got %s %s" % (what, dtype, " %s" % (tuple(shape),) if shape is not None else
                                                          " with %d elements" % numel if numel is not None else "", t.dtype,
                                                          tuple(t.shape)))
    if t.is_contiguous():
        return t
    if not copy:
        raise ValueError("%s must be contiguous (the kernel writes to it), got strides %s for shape %s"
                         % (what, tuple(t.stride()), tuple(t.shape)))
    return t.contiguous()


# The argument checks the model-layer and retrieval families share.  Each raises a ValueError that names the family and the argument;
# a family's own domain (its field counts, option codes, workspace sizes) stays with the family.
def _slab_width(family, D, what="D", lo=4, hi=256):
    """a row width the kernels vectorise over: a multiple of 4 in [lo, hi] ([4, 256] is the embedding slab's domain); returns it as an int"""
    D = int(D)
    if D % 4 != 0 or not lo <= D <= hi:
        raise ValueError("%s: %s must be a multiple of 4 in [%d, %d], got %d" % (family, what, lo, hi, D))
    return D


def _vec_arg(family, t, n, what, dtype=torch.float32, none_ok=False, device=None):
    """t as a contiguous [n] (a copy only where it is no such view already): one value per example, id or slot.  None passes where
    none_ok; another dtype or element count, or (device given) another device, is a ValueError."""
    if t is None and none_ok:
        return None
    if t.dtype != dtype or t.numel() != n:
        raise ValueError("%s: %s must be %s with %d values (one value per example, id or slot), got %s %s"
                         % (family, what, dtype, n, t.dtype, tuple(t.shape)))
    if device is not None and t.device != device:
        raise ValueError("%s: %s is on %s, the call's other tensors on %s" % (family, what, t.device, device))
    return t.reshape(n).contiguous()


def _ids_arg(family, t, what, cols=None, rows=None):
    """int64 [rows, cols] ids (None: any number of rows / columns), returned contiguous"""
    if t.dtype != torch.int64 or t.dim() != 2 or (cols is not None and t.shape[1] != cols) or (rows is not None and t.shape[0] != rows):
        raise ValueError("%s: %s must be int64 [%s, %s], got %s %s" % (family, what, "B" if rows is None else rows,
                                                                      "C" if cols is None else cols, t.dtype, tuple(t.shape)))
    return t.contiguous()


def _table_arg(family, t, what, cols=None):
    """a table whose rows the kernel reads in place by id: contiguous fp32 [R, cols] (cols None: any width); a view is refused"""
    if t.dtype != torch.float32 or t.dim() != 2 or (cols is not None and t.shape[1] != cols) or not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous fp32 [R, %s], got %s %s with strides %s"
                         % (family, what, "D" if cols is None else cols, t.dtype, tuple(t.shape), tuple(t.stride())))


def _rows_arg(family, t, cols, what, shapes=(), rows=None, device=None):
    """(t as [B, cols], its row pitch) of an fp32 matrix of rows a kernel reads or writes where it lies (_row_pitch's rule).  A
    contiguous N-d tensor whose trailing shape is one of `shapes` is taken as [B, cols].  rows given: t must have that many rows, and a
    None t is allocated [rows, cols] on `device`."""
    if t is None and rows is not None:
        t = torch.empty((rows, cols), dtype=torch.float32, device=device)
    if t.dtype != torch.float32:
        raise ValueError("%s: %s must be fp32, got %s" % (family, what, t.dtype))
    if t.dim() > 2:
        if tuple(t.shape[1:]) not in shapes or not t.is_contiguous():
            raise ValueError("%s: a %d-d %s must be contiguous [B, ...] with trailing shape %s, got %s with strides %s"
                             % (family, t.dim(), what, " or ".join(str(tuple(s)) for s in shapes) or "(%d,)" % cols, tuple(t.shape),
                                tuple(t.stride())))
        t = t.reshape(t.shape[0], cols)
    if rows is not None and (t.dim() != 2 or t.shape[0] != rows):
        raise ValueError("%s: %s must be fp32 [%d, %d], got %s %s" % (family, what, rows, cols, t.dtype, tuple(t.shape)))
    return t, _row_pitch(family, t, cols, what)


def _pitched(family, t, what, cols=None, rows=None, min_rows=False, mult4=False, aligned=False, tight_row=False):
    """the row pitch of an fp32 [rows, cols] matrix (None: any number of rows; any width >= 1) that a kernel takes where it lies: nothing
    is copied, and a layout outside the policy is a ValueError.  Always: unit column stride and, with more than one row, a pitch >= the
    width.  mult4: that pitch is a multiple of 4 floats.  aligned: the base address is 16-byte aligned.  min_rows: `rows` or more rows
    (the source rows of a block, whose first `rows` are the destinations).  One row has no pitch: its stride is handed on where that
    is a legal pitch, and the width otherwise -- or always, with tight_row."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] < 1 if cols is None else t.shape[1] != cols) or \
            (rows is not None and (t.shape[0] < rows if min_rows else t.shape[0] != rows)):
        raise ValueError("%s: %s must be fp32 [%s%s, %s], got %s" % (
            family, what, ">= " if min_rows else "", "M" if rows is None else rows, cols or "N >= 1",
            "%s %s" % (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
    M, N = t.shape
    ld = t.stride(0)
    legal = ld >= N and not (mult4 and ld % 4)
    if (N > 1 and t.stride(1) != 1) or (M > 1 and not legal):
        raise ValueError("%s: %s needs unit column stride and a row pitch %s>= %d, got strides %s"
                         % (family, what, "that is a multiple of 4 and " if mult4 else "", N, tuple(t.stride())))
    if aligned and t.data_ptr() % 16 != 0:
        raise ValueError("%s: %s must start at a 16-byte aligned address (a view that begins inside a row does not)" % (family, what))
    return ld if M > 1 or (legal and not tight_row) else _pad4(N) if mult4 else N


def _one_device(family, anchor, device, **tensors):
    """every tensor one call is handed lives on one device: `device`, where the argument named `anchor` is"""
    for what, t in tensors.items():
        if t is not None and t.device != device:
            raise ValueError("%s: %s is on %s, %s on %s; one call takes tensors of one device" % (family, what, t.device, anchor, device))


def _vec_f32(b):
    """a bias / per-column vector the kernel reads densely (an expanded one has a 0 stride and a single element behind it)"""
    return None if b is None else _c(b, torch.float32)


def _rowmajor_ld4(t):
    """Returns a [M, K] fp32 view whose row stride is a multiple of 4 floats and base 16-B aligned."""
    assert t.dim() == 2 and t.dtype == torch.float32
    if t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t      # the kernel takes float4 loads only when base and pitch are 16-B aligned
    if t.shape[1] == 1 and t.stride(0) >= 1:
        return t
    M, K = t.shape
    buf = torch.zeros((M, _pad4(K)), dtype=torch.float32, device=t.device)
    buf[:, :K].copy_(t)
    return buf[:, :K]


def linear_fwd(x, W, b=None, act=0, out=None):
    """y = act(x @ W + b); x [M,K] (row stride % 4 == 0), W [K,N] row-major."""
    x = _rowmajor_ld4(x)
    W = _rowmajor_ld4(W)
    b = _vec_f32(b)
    M, K = x.shape
    N = W.shape[1]
    if out is None:
        out = torch.empty((M, _pad4(N)), dtype=torch.float32, device=x.device)[:, :N]
    check(lib().dr_linear_fwd(ptr(x), x.stride(0), ptr(W), W.stride(0), ptr(b), M, K, N, int(act), ptr(out),
                              out.stride(0), stream_ptr()), "dr_linear_fwd")
    return out


def linear_bwd_dx(dy, W, relu_src=None, accumulate=False, out=None):
    dy = _rowmajor_ld4(dy)
    W = _rowmajor_ld4(W)
    M, N = dy.shape
    K = W.shape[0]
    if out is None:
        assert not accumulate
        out = torch.empty((M, _pad4(K)), dtype=torch.float32, device=dy.device)[:, :K]
    check(lib().dr_linear_bwd_dx(ptr(dy), dy.stride(0), ptr(W), W.stride(0), M, K, N, ptr(relu_src),
                                 relu_src.stride(0) if relu_src is not None else 0, int(bool(accumulate)), ptr(out),
                                 out.stride(0), stream_ptr()), "dr_linear_bwd_dx")
    return out


def linear_fwd_splitk_workspace(M, K, N, device):
    return torch.empty(max(1, lib().dr_linear_fwd_splitk_workspace_bytes(int(M), int(K), int(N)) // 4), dtype=torch.float32,
                       device=device)


def linear_fwd_splitk(x, W, out, workspace=None):
    """out += x @ W with the reduction split over the grid (few output tiles, long K); slices summed in a fixed order."""
    x = _rowmajor_ld4(x)
    W = _rowmajor_ld4(W)
    M, K = x.shape
    N = W.shape[1]
    assert W.shape[0] == K and out.shape == (M, N) and out.stride(1) == 1
    if workspace is None or workspace.numel() * 4 < lib().dr_linear_fwd_splitk_workspace_bytes(M, K, N):
        workspace = linear_fwd_splitk_workspace(M, K, N, x.device)
    check(lib().dr_linear_fwd_splitk(ptr(x), x.stride(0), ptr(W), W.stride(0), M, K, N, ptr(out), out.stride(0), ptr(workspace),
                                     workspace.numel() * 4, stream_ptr()), "dr_linear_fwd_splitk")
    return out


def linear_bwd_dw_workspace(M, K, N, device):
    return torch.empty(max(1, lib().dr_linear_bwd_dw_workspace_bytes(int(M), int(K), int(N)) // 4), dtype=torch.float32,
                       device=device)


def linear_bwd_dw(x, dy, scale, dstW, dstb=None, workspace=None):
    """dstW += scale * x^T @ dy ; dstb += scale * colsum(dy).  With a workspace the split-K partials are combined
    deterministically by a reduce kernel; without, by fp32 atomics."""
    x = _rowmajor_ld4(x)
    dy = _rowmajor_ld4(dy)
    M, K = x.shape
    N = dy.shape[1]
    assert dstW.shape == (K, N) and dstW.stride(1) == 1
    check(lib().dr_linear_bwd_dw(ptr(x), x.stride(0), ptr(dy), dy.stride(0), M, K, N, float(scale), ptr(dstW),
                                 dstW.stride(0), ptr(dstb), ptr(workspace),
                                 workspace.numel() * 4 if workspace is not None else 0, stream_ptr()), "dr_linear_bwd_dw")


def linear_bwd_narrow_supported(M, K, N):
    """Shape domain of the fused narrow-layer backward (dr_linear_bwd_narrow)."""
    return N <= 32 and K in (128, 256, 512) and M > 0 and M % 32 == 0


def linear_bwd_narrow_workspace(M, K, N, device):
    return torch.empty(max(64, lib().dr_linear_bwd_narrow_workspace_bytes(int(M), int(K), int(N)) // 4),
                       dtype=torch.float32, device=device)


def linear_bwd_narrow(x, dy, W, scale, dstW, dstb, dx, relu_mask=True, workspace=None, parts=3, dx_amax=None):
    """One pass over x: dx = (dy @ W^T) * (x > 0 if relu_mask); dstW += scale * x^T dy; dstb += scale * colsum(dy).
    dx uses the pre-update W even when dstW is W.  Raises RuntimeError(DR_ESHAPE) outside the kernel's domain."""
    M, K = x.shape
    N = dy.shape[1]
    assert x.stride(1) == 1 and dy.stride(1) == 1 and W.stride(1) == 1 and dstW.stride(1) == 1 and dx.stride(1) == 1
    assert W.shape == (K, N) and dstW.shape == (K, N) and dx.shape == (M, K)
    if workspace is None:
        workspace = linear_bwd_narrow_workspace(M, K, N, x.device)
    # parts 1: the one-pass kernel, 2: the reduce that applies the partials (may run on another stream); dx_amax: also leave max |dx| in
    # the record (the f16x2 GEMMs that take dx as an operand want it)
    check(lib().dr_linear_bwd_narrow(ptr(x), x.stride(0), ptr(dy), dy.stride(0), ptr(W), W.stride(0), M, K, N,
                                     1 if relu_mask else 0, float(scale), ptr(dstW), dstW.stride(0), ptr(dstb), ptr(dx),
                                     dx.stride(0), ptr(workspace), workspace.numel() * 4, int(parts), ptr(dx_amax), stream_ptr()),
          "dr_linear_bwd_narrow")
    return dx


def tower_tail_supported(M, K, H):
    """Shape domain of the one-pass tower tail (dr_tower_tail_fused)."""
    return H <= 32 and K in (128, 256) and M > 0 and M % 32 == 0


def tower_tail_workspace(M, K, device):
    return torch.empty(max(128, lib().dr_tower_tail_workspace_bytes(int(M), int(K)) // 4), dtype=torch.float32, device=device)


def tower_tail_fused(x, W1, b1, W2, b2, extra_logit, labels, loss_mode, scale, dx, dst_W1="inplace", dst_b1="inplace", dst_W2="inplace",
                     dst_b2="inplace", prob=None, d_logit=None, d_h=None, loss=None, workspace=None, n_total=0, parts=3, dx_amax=None):
    """tower_head_fwd_bwd (relu) + linear_bwd_narrow (relu mask) of the same layer W1 in ONE pass over x (dr_tower_tail_fused).
    dst_* += scale * gradient: the parameters themselves by default (fused SGD, scale = -lr) or gradient buffers (scale = 1).
    Returns (loss, prob, d_logit, dx)."""
    M, K = x.shape
    H = W1.shape[1]
    dev = x.device
    dst_W1 = W1 if isinstance(dst_W1, str) else dst_W1
    dst_b1 = b1 if isinstance(dst_b1, str) else dst_b1
    dst_W2 = W2 if isinstance(dst_W2, str) else dst_W2
    dst_b2 = b2 if isinstance(dst_b2, str) else dst_b2
    assert x.stride(1) == 1 and W1.stride(1) == 1 and dst_W1.stride(1) == 1 and dx.stride(1) == 1 and W2.shape == (H, 1) and dx.shape == (M, K)
    prob = prob if prob is not None else torch.empty(M, dtype=torch.float32, device=dev)
    d_logit = d_logit if d_logit is not None else torch.empty(M, dtype=torch.float32, device=dev)
    loss = loss if loss is not None else torch.empty(1, dtype=torch.float32, device=dev)
    if workspace is None:
        workspace = tower_tail_workspace(M, K, dev)
    check(lib().dr_tower_tail_fused(ptr(x), x.stride(0), ptr(W1), W1.stride(0), ptr(b1), M, int(n_total), K, H, ptr(W2), W2.stride(0), ptr(b2),
                                    ptr(extra_logit), ptr(labels), int(loss_mode), float(scale), ptr(dst_W1), dst_W1.stride(0), ptr(dst_b1),
                                    ptr(dst_W2), dst_W2.stride(0) if dst_W2 is not None else 0, ptr(dst_b2), ptr(prob), ptr(d_logit), ptr(d_h),
                                    d_h.stride(0) if d_h is not None else 0, ptr(dx), dx.stride(0), ptr(loss), ptr(workspace),
                                    workspace.numel() * 4, int(parts), ptr(dx_amax), stream_ptr()), "dr_tower_tail_fused")
    return loss, prob, d_logit, dx


def tower_head_workspace(M, device):
    return torch.empty(max(64, lib().dr_tower_head_workspace_bytes(int(M)) // 4), dtype=torch.float32, device=device)


def tower_head_fwd_bwd(x, W1, b1, W2, b2, extra_logit, labels, loss_mode, scale, act=1, h_out=None, prob=None, d_logit=None,
                       d_h=None, loss=None, workspace=None, dst_W2="inplace", dst_b2="inplace", n_total=0, parts=3):
    """Last hidden layer (H <= 32) + Dense(1) + extra logit + BCE loss + the Dense(1) backward, fused.
    W2: [H, 1] (any row stride).  dst_W2 / dst_b2 += scale * gradient: by default the parameters themselves (fused SGD,
    scale = -lr); pass gradient buffers with scale = 1 for data-parallel training, or None to skip.  n_total: size of
    the batch the loss is a mean over when x is one slice of it (0 = M).
    Returns (loss, prob, d_logit, d_h)."""
    if isinstance(dst_W2, str):
        dst_W2 = W2
    if isinstance(dst_b2, str):
        dst_b2 = b2
    M, K = x.shape
    H = W1.shape[1]
    dev = x.device
    assert x.stride(1) == 1 and W1.stride(1) == 1 and W2.shape == (H, 1)
    prob = prob if prob is not None else torch.empty(M, dtype=torch.float32, device=dev)
    d_logit = d_logit if d_logit is not None else torch.empty(M, dtype=torch.float32, device=dev)
    d_h = d_h if d_h is not None else torch.empty((M, _pad4(H)), dtype=torch.float32, device=dev)[:, :H]
    loss = loss if loss is not None else torch.empty(1, dtype=torch.float32, device=dev)
    if workspace is None:
        workspace = tower_head_workspace(M, dev)
    # parts 1: GEMM + head kernel, 2: the finish kernel (partials -> dst_W2 / dst_b2 / loss; may run on another stream)
    check(lib().dr_tower_head_fwd_bwd(ptr(x), x.stride(0), ptr(W1), W1.stride(0), ptr(b1), M, int(n_total), K, H, int(act), ptr(W2),
                                      W2.stride(0), ptr(b2), ptr(extra_logit), ptr(labels), int(loss_mode), float(scale),
                                      ptr(dst_W2), dst_W2.stride(0) if dst_W2 is not None else 0, ptr(dst_b2),
                                      ptr(h_out), h_out.stride(0) if h_out is not None else 0, ptr(prob), ptr(d_logit),
                                      ptr(d_h), d_h.stride(0), ptr(loss), ptr(workspace), workspace.numel() * 4, int(parts),
                                      stream_ptr()), "dr_tower_head_fwd_bwd")
    return loss, prob, d_logit, d_h


def cross_fwd(x0, x, W, b, diag_scale=0.0, want_prod=False, prod=None):
    """out = x0 * (x @ W + b + diag*x) + x.  W None: `prod` holds x @ W (low-rank path) and is finished in place."""
    x0 = _rowmajor_ld4(x0)
    x = _rowmajor_ld4(x)
    if x0.stride(0) != x.stride(0):
        x = _rowmajor_ld4(x.contiguous())
        x0 = _rowmajor_ld4(x0.contiguous())
    M, Dm = x.shape
    ld = x.stride(0)
    b = _vec_f32(b)
    out = torch.empty((M, ld), dtype=torch.float32, device=x.device)[:, :Dm]
    if W is not None:
        W = _rowmajor_ld4(W)
        if want_prod:
            prod = torch.empty((M, ld), dtype=torch.float32, device=x.device)[:, :Dm]
        ldw = W.stride(0)
    else:
        assert prod is not None and prod.stride(0) == ld
        ldw = 0
    check(lib().dr_cross_fwd(ptr(x0), ptr(x), ld, ptr(W), ldw, ptr(b), float(diag_scale), M, Dm, ptr(out),
                             ptr(prod) if (want_prod or W is None) else None, stream_ptr()), "dr_cross_fwd")
    return out, prod


def cross_combine_bwd(x0, prod, d_out, diag_scale, d_x0_accum, d_x_accum, d_prod_amax=None):
    M, Dm = d_out.shape
    ld = d_out.stride(0)
    for t in (x0, prod, d_x0_accum, d_x_accum):
        assert t is None or t.stride(0) == ld, "cross tensors must share one leading dimension"
    d_prod = torch.empty((M, ld), dtype=torch.float32, device=d_out.device)[:, :Dm]
    # d_prod_amax: also the amax record of d_prod (operand of the cross layer's f16x2 dgrad / wgrad)
    check(lib().dr_cross_combine_bwd(ptr(x0), ptr(prod), ptr(d_out), M, Dm, ld, float(diag_scale), ptr(d_prod),
                                     ptr(d_x0_accum), ptr(d_x_accum), ptr(d_prod_amax), stream_ptr()), "dr_cross_combine_bwd")
    return d_prod


# ----------------------------------------------------------------------------------------------
# K11   fused sigmoid + BCE
# ----------------------------------------------------------------------------------------------
LOSS_SIGMOID_CE, LOSS_LOG_LOSS, LOSS_KERAS_BCE = 0, 1, 2


def bce_fwd_bwd(logits, labels, mode=LOSS_SIGMOID_CE, want_prob=True, want_grad=True, workspace=None, logits_b=None,
                out=None):
    logits = _c(logits.reshape(-1), torch.float32)
    labels = _c(labels.reshape(-1), torch.float32)
    n = logits.numel()
    if labels.numel() != n:
        raise ValueError("bce_fwd_bwd: labels must have one value per logit (%d), got %d" % (n, labels.numel()))
    dev = logits.device
    if out is not None:
        prob, d_logit, loss = out
    else:
        prob = torch.empty(n, dtype=torch.float32, device=dev) if want_prob else None
        d_logit = torch.empty(n, dtype=torch.float32, device=dev) if want_grad else None
        loss = torch.empty(1, dtype=torch.float32, device=dev)
    if workspace is None:
        workspace = torch.empty(1024, dtype=torch.float32, device=dev)
    ldb = 0
    if logits_b is not None:
        assert logits_b.dim() == 2 and logits_b.shape[0] == n and logits_b.dtype == torch.float32
        ldb = logits_b.stride(0)
    check(lib().dr_bce_fwd_bwd(ptr(logits), ptr(logits_b), ldb, ptr(labels), n, int(mode), ptr(prob), ptr(d_logit),
                               ptr(loss), ptr(workspace), stream_ptr()), "dr_bce_fwd_bwd")
    return loss, prob, d_logit


def sigmoid_fwd(x):
    x = _c(x, torch.float32)
    y = torch.empty_like(x)
    check(lib().dr_sigmoid_fwd(ptr(x), x.numel(), ptr(y), stream_ptr()), "dr_sigmoid_fwd")
    return y


def sigmoid_bwd(y, dy):
    y = _c(y, torch.float32)
    dy = _c(dy, torch.float32)
    if dy.numel() != y.numel():
        raise ValueError("sigmoid_bwd: dy must have y's %d elements, got %d" % (y.numel(), dy.numel()))
    dx = torch.empty_like(y)
    check(lib().dr_sigmoid_bwd(ptr(y), ptr(dy), y.numel(), ptr(dx), stream_ptr()), "dr_sigmoid_bwd")
    return dx


def bce_prob_fwd_bwd(prob, labels, mode, want_grad=True, workspace=None):
    prob = _c(prob.reshape(-1), torch.float32)
    labels = _c(labels.reshape(-1), torch.float32)
    n = prob.numel()
    if labels.numel() != n:
        raise ValueError("bce_prob_fwd_bwd: labels must have one value per probability (%d), got %d" % (n, labels.numel()))
    d_prob = torch.empty_like(prob) if want_grad else None
    loss = torch.empty(1, dtype=torch.float32, device=prob.device)
    if workspace is None:
        workspace = torch.empty(1024, dtype=torch.float32, device=prob.device)
    check(lib().dr_bce_prob_fwd_bwd(ptr(prob), ptr(labels), n, int(mode), ptr(d_prob), ptr(loss), ptr(workspace),
                                    stream_ptr()), "dr_bce_prob_fwd_bwd")
    return loss, d_prob


# ----------------------------------------------------------------------------------------------
# row-sharded tables: bucketing + owner-side gather / scatter, dense axpy
# ----------------------------------------------------------------------------------------------
def shard_dedup_slots(ids, row_base, num_rows, plan, out=None):
    """(rep, unique_flags) of a micro-batch: rep[p] int64 = the lowest slot that looks up the same row as slot p (dr_shard_dedup_slots
    over `plan` = emb_sort_slots(ids, row_base, num_rows)); unique_flags = the plan's per-slot flags (row shared by no other slot)."""
    B, F = ids.shape
    n = B * F
    if out is None or out.numel() < n:
        out = torch.empty(n, dtype=torch.int64, device=ids.device)
    check(lib().dr_shard_dedup_slots(ptr(plan.rows), ptr(plan.slots), ptr(plan.dup_count), n, int(num_rows), ptr(out), stream_ptr()),
          "dr_shard_dedup_slots")
    return out, plan.flags


def shard_bucket_ids(ids, rows_per_shard, world, counts=None, send_rows=None, pos=None, workspace=None, rep=None):
    ids = _c(ids, torch.int64)
    B, C = ids.shape
    n = B * C
    dev = ids.device
    if counts is None:
        counts = torch.empty(world, dtype=torch.int64, device=dev)
    if send_rows is None:
        send_rows = torch.empty(n, dtype=torch.int64, device=dev)
    if pos is None:
        pos = torch.empty((B, C), dtype=torch.int64, device=dev)
    if workspace is None:
        nbytes = lib().dr_shard_bucket_workspace_bytes(n, world)
        workspace = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    check(lib().dr_shard_bucket_ids(ptr(ids), ptr(rep), n, C, int(rows_per_shard), int(world), ptr(counts), ptr(send_rows),
                                    ptr(pos), ptr(workspace), stream_ptr()), "dr_shard_bucket_ids")
    return counts, send_rows, pos


def rows_gather(rows, table, lin_w=None, out_rows=None, out_lin=None):
    """(out_rows [n, D], out_lin [n] | None): table[rows] and lin_w[rows].  The kernel addresses table as row-major [R, D] and lin_w as
    [R]: a view of either is refused by name (a table is a parameter, and a silent copy of one per call is no layout fix)."""
    rows = _c(rows, torch.int64)
    n = rows.numel()
    if table.dtype != torch.float32 or table.dim() != 2 or not table.is_contiguous():
        raise ValueError("rows_gather: table must be contiguous fp32 [R, D], got %s %s with strides %s"
                         % (table.dtype, tuple(table.shape), tuple(table.stride())))
    R, D = table.shape
    lin_w = _dense_arg(lin_w, "rows_gather: lin_w", numel=R, copy=False)
    if out_rows is None:
        out_rows = torch.empty((n, D), dtype=torch.float32, device=rows.device)
    elif out_rows.dtype != torch.float32 or not out_rows.is_contiguous() or out_rows.numel() < n * D:
        raise ValueError("rows_gather: out_rows must be contiguous fp32 with room for %s, got %s %s" % ((n, D), out_rows.dtype, tuple(out_rows.shape)))
    if out_lin is None and lin_w is not None:
        out_lin = torch.empty(n, dtype=torch.float32, device=rows.device)
    elif out_lin is not None and (out_lin.dtype != torch.float32 or not out_lin.is_contiguous() or out_lin.numel() < n):
        raise ValueError("rows_gather: out_lin must be contiguous fp32 with room for %d, got %s %s" % (n, out_lin.dtype, tuple(out_lin.shape)))
    check(lib().dr_rows_gather(ptr(rows), n, ptr(table), D, ptr(lin_w), ptr(out_rows), ptr(out_lin), stream_ptr()),
          "dr_rows_gather")
    return out_rows, out_lin


def rows_scatter_add(rows, grads, lin_grads, scale, table, lin_w):
    """table[rows] += scale * grads, lin_w[rows] += scale * lin_grads (fp32 atomics).  grads [n, D] and lin_grads [n] are read
    densely: a view is copied once; table and lin_w are written to and must be contiguous."""
    rows = _c(rows, torch.int64)
    n = rows.numel()
    if table.dtype != torch.float32 or table.dim() != 2 or not table.is_contiguous():
        raise ValueError("rows_scatter_add: table must be contiguous fp32 [R, D], got %s %s with strides %s"
                         % (table.dtype, tuple(table.shape), tuple(table.stride())))
    R, D = table.shape
    grads = _dense_arg(grads, "rows_scatter_add: grads", shape=(n, D))
    lin_grads = _dense_arg(lin_grads, "rows_scatter_add: lin_grads", numel=n)
    lin_w = _dense_arg(lin_w, "rows_scatter_add: lin_w", numel=R, copy=False)
    check(lib().dr_rows_scatter_add(ptr(rows), n, ptr(grads), D, ptr(lin_grads), float(scale), ptr(table), ptr(lin_w),
                                    stream_ptr()), "dr_rows_scatter_add")


def axpy(alpha, x, y):
    assert x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()
    check(lib().dr_axpy(x.numel(), float(alpha), ptr(x), ptr(y), stream_ptr()), "dr_axpy")


# ----------------------------------------------------------------------------------------------
# K4 deterministic form: sort slots by row, segment-sum, plain read-modify-write
# ----------------------------------------------------------------------------------------------
def emb_sort_workspace(n, device):
    return torch.empty(lib().dr_emb_sort_workspace_bytes(int(n)), dtype=torch.uint8, device=device)


class SortPlan:
    """Per-batch outputs of dr_emb_sort_slots (all preallocated, reusable across steps)."""

    def __init__(self, n, device):
        self.n = int(n)                      # capacity in slots: a plan serves any batch of <= n slots
        self.rows = torch.empty(n, dtype=torch.int64, device=device)
        self.slots = torch.empty(n, dtype=torch.int32, device=device)
        self.flags = torch.empty(n, dtype=torch.uint8, device=device)
        self.dup_heads = torch.empty(n, dtype=torch.int32, device=device)
        self.dup_count = torch.zeros(4, dtype=torch.int32, device=device)     # [work-list entries, length of the sorted arrays]
        self.workspace = emb_sort_workspace(n, device)

    def sorted_len(self):
        """Length of the sorted (rows, slots) arrays of the last plan built here: only the slots of shared rows (claim path) or
        all slots (radix path).  Host read -- tests / debugging."""
        return int(self.dup_count[1].item())


def emb_sort_slots(ids, row_base, num_rows, plan=None):
    ids = _c(ids, torch.int64)
    B, F = ids.shape
    if plan is None or plan.n < B * F:       # a reused plan sized for a smaller batch would be rejected (DR_EINVAL)
        plan = SortPlan(B * F, ids.device)
    check(lib().dr_emb_sort_slots(ptr(ids), B, F, ptr(row_base), int(num_rows), ptr(plan.rows), ptr(plan.slots),
                                  ptr(plan.flags), ptr(plan.dup_heads), ptr(plan.dup_count), ptr(plan.workspace),
                                  plan.workspace.numel(), stream_ptr()), "dr_emb_sort_slots")
    return plan


def hash_sort_slots(keys, col_buckets, row_base, num_rows, ids_out, ids_t_out=None, plan=None, parts=3):
    """hash_bucket_i64(keys -> ids_out) + ids_transpose_i32(ids_out -> ids_t_out, optional) + emb_sort_slots(ids_out) as one chain whose
    first kernel does the work of the first four (dr_hash_sort_slots): same outputs, bit for bit.
    parts (dr_hash_sort_slots_parts): 1 = the launches that write ids_out / ids_t_out, 2 = the rest of the plan (same stream, same
    arguments, nothing touching the plan in between), 3 = both."""
    keys = _c(keys, torch.int64)
    B, F = keys.shape
    assert ids_out.shape == (B, F) and ids_out.dtype == torch.int64 and ids_out.is_contiguous()
    if ids_t_out is not None:
        assert ids_t_out.shape == (F, B) and ids_t_out.dtype == torch.int32 and ids_t_out.is_contiguous()
    if plan is None or plan.n < B * F:
        plan = SortPlan(B * F, keys.device)
    if parts != 3:
        check(lib().dr_hash_sort_slots_parts(ptr(keys), B, F, ptr(col_buckets), ptr(ids_out), ptr(ids_t_out), ptr(row_base), int(num_rows),
                                             ptr(plan.rows), ptr(plan.slots), ptr(plan.flags), ptr(plan.dup_heads), ptr(plan.dup_count),
                                             ptr(plan.workspace), plan.workspace.numel(), int(parts), stream_ptr()),
              "dr_hash_sort_slots_parts")
        return plan
    check(lib().dr_hash_sort_slots(ptr(keys), B, F, ptr(col_buckets), ptr(ids_out), ptr(ids_t_out), ptr(row_base), int(num_rows),
                                   ptr(plan.rows), ptr(plan.slots), ptr(plan.flags), ptr(plan.dup_heads), ptr(plan.dup_count),
                                   ptr(plan.workspace), plan.workspace.numel(), stream_ptr()), "dr_hash_sort_slots")
    return plan


def emb_plan_set_small_limit(limit):
    """largest shared-row list the plan's one-block LDS sort takes (0: radix path whenever a row is shared); returns the previous"""
    return int(lib().dr_emb_plan_set_small_limit(int(limit)))


def emb_snapshot_sorted_rows(plan, table, num_rows, out):
    """out[i, :] = table[plan.rows[i], :] for every work-list head i of the plan (dr_emb_snapshot_sorted_rows): the x of the slots
    that share rows, taken before K4 updates the table -- needed when the forward did not store `concat`."""
    assert out.is_contiguous() and out.shape[0] >= plan.n and out.shape[1] == table.shape[1]
    check(lib().dr_emb_snapshot_sorted_rows(ptr(plan.rows), ptr(plan.dup_heads), ptr(plan.dup_count), ptr(table), table.shape[1],
                                            int(num_rows), ptr(out), stream_ptr()), "dr_emb_snapshot_sorted_rows")
    return out


def ids_transpose_i32(ids, out=None):
    """ids [B, F] int64 -> [F, B] int32 (field-major), for bf3_wgrad_emb"""
    ids = _c(ids, torch.int64)
    B, F = ids.shape
    if out is None:
        out = torch.empty((F, B), dtype=torch.int32, device=ids.device)
    check(lib().dr_ids_transpose_i32(ptr(ids), B, F, ptr(out), stream_ptr()), "dr_ids_transpose_i32")
    return out


def emb_pool_bwd_sorted(ids, row_base, plan, D, num_rows, grad, d_fm_logit, scale, dst_table, dst_lin=None, dst_bias=None,
                        concat=None, sum_x=None, slot_lin_grad=None, x_sorted=None, parts=3, lin_old_t=None, table_amax=None):
    """K4 on the slot plan.  x_sorted ([B * F, D] scratch; with the FM term and no `concat` it must hold the snapshot of
    emb_snapshot_sorted_rows) also makes the update of rows hit more than 32 times deterministic: it is clobbered.  parts: 1 = the
    update kernel, 2 = the ordered combination of hot rows' parked pieces, 3 = both (dr_emb_pool_bwd_sorted).
    lin_old_t: first-order weights as this step's forward read them, [F, B]: unique rows get one write, no RMW.
    table_amax: running amax record of dst_table (ops.h2_record), raised to the largest magnitude written."""
    ids = _c(ids, torch.int64)
    B, F = ids.shape
    assert grad.stride(1) == 1
    assert lin_old_t is None or (lin_old_t.shape == (F, B) and lin_old_t.is_contiguous() and lin_old_t.dtype == torch.float32)
    check(lib().dr_emb_pool_bwd_sorted(ptr(ids), ptr(row_base), ptr(plan.rows), ptr(plan.slots), ptr(plan.flags),
                                       ptr(plan.dup_heads), ptr(plan.dup_count), B, F, D, int(num_rows), ptr(grad),
                                       grad.stride(0), ptr(concat), concat.stride(0) if concat is not None else 0,
                                       ptr(sum_x), ptr(d_fm_logit), ptr(slot_lin_grad), float(scale), ptr(dst_table), ptr(dst_lin),
                                       ptr(dst_bias), ptr(x_sorted), ptr(lin_old_t), int(parts), ptr(table_amax), stream_ptr()),
          "dr_emb_pool_bwd_sorted")


def emb_pool_bwd_dups_apply(ids, row_base, plan, D, num_rows, grad, d_fm_logit, scale, dst_table, dst_lin, dst_bias, sum_x, x_sorted,
                            lin_old_t, table_amax, wg_workspace, wg_R, wg_scale, dstW, dstb=None, wg_h2=True, parts=1, refresh=None):
    """emb_pool_bwd_sorted(parts | 8) whose first launch also applies the first layer's wgrad (dr_emb_pool_bwd_dups_apply): extra blocks
    behind the duplicate pass run the fixed-order reduce of the product that part 1 of h2_wgrad_emb (or of bf3_wgrad_emb: wg_h2=False)
    left in wg_workspace -- dstW += wg_scale * sum of the partials, dstb likewise.  parts: 1 or 3 (| 8 is implied).
    refresh: what H2WeightPlanes(dstW).hand_off() returned -- the plane refresh of dstW rides along (dr_emb_pool_bwd_dups_apply_refresh):
    the amax words in part 1, record + both images in part 2, the hot rows' launch, which may then also be called alone (parts=2)."""
    ids = _c(ids, torch.int64)
    B, F = ids.shape
    wg_F, wg_N = dstW.shape
    assert grad.stride(1) == 1 and dstW.stride(1) == 1
    assert lin_old_t is None or (lin_old_t.shape == (F, B) and lin_old_t.is_contiguous() and lin_old_t.dtype == torch.float32)
    if refresh is not None:
        w, wt, amax, words = refresh
        assert (w.rows, w.cols) == (wg_F, wg_N) and (wt.rows, wt.cols) == (wg_N, wg_F) and words.numel() >= 1024
        check(lib().dr_emb_pool_bwd_dups_apply_refresh(
            ptr(ids), ptr(row_base), ptr(plan.rows), ptr(plan.slots), ptr(plan.flags), ptr(plan.dup_heads), ptr(plan.dup_count), B, F, D,
            int(num_rows), ptr(grad), grad.stride(0), ptr(sum_x), ptr(d_fm_logit), float(scale), ptr(dst_table), ptr(dst_lin), ptr(dst_bias),
            ptr(x_sorted), ptr(lin_old_t), int(parts) | 8, ptr(table_amax), ptr(wg_workspace), wg_workspace.numel() * 4, int(wg_R), wg_F,
            wg_N, 1 if wg_h2 else 0, float(wg_scale), ptr(dstW), dstW.stride(0), ptr(dstb), ptr(w.buf), w.plane_stride, w.ld, ptr(wt.buf),
            wt.plane_stride, wt.ld, ptr(amax), ptr(words), stream_ptr()), "dr_emb_pool_bwd_dups_apply_refresh")
        return
    check(lib().dr_emb_pool_bwd_dups_apply(ptr(ids), ptr(row_base), ptr(plan.rows), ptr(plan.slots), ptr(plan.flags), ptr(plan.dup_heads),
                                           ptr(plan.dup_count), B, F, D, int(num_rows), ptr(grad), grad.stride(0), ptr(sum_x),
                                           ptr(d_fm_logit), float(scale), ptr(dst_table), ptr(dst_lin), ptr(dst_bias), ptr(x_sorted),
                                           ptr(lin_old_t), int(parts) | 8, ptr(table_amax), ptr(wg_workspace), wg_workspace.numel() * 4,
                                           int(wg_R), wg_F, wg_N, 1 if wg_h2 else 0, float(wg_scale), ptr(dstW), dstW.stride(0), ptr(dstb),
                                           stream_ptr()), "dr_emb_pool_bwd_dups_apply")


def h2_dgrad_emb_sgd(dy, dy_amax, w: "H2Planes", ids_t, plan, row_base, table, lin_w, lin_old_t, sum_x, d_fm_logit, scale, d_concat,
                     table_amax=None):
    """First-layer dgrad + K4's unique-row pass in one launch (dr_h2_dgrad_emb_sgd): the rows of `table` (and `lin_w`) that exactly one
    slot of the batch looked up receive their SGD update; the gradient rows of all other slots are stored to `d_concat` [M, >= 64 F]
    for emb_pool_bwd_sorted(..., parts=... | 8).  w: the layer's kernel as H2Planes (rows = input columns, >= 64 F of them)."""
    F, M = ids_t.shape
    K = dy.shape[1]
    assert dy.stride(1) == 1 and d_concat.stride(1) == 1 and table.is_contiguous() and table.shape[1] == 64 and sum_x.is_contiguous()
    assert ids_t.dtype == torch.int32 and ids_t.is_contiguous() and dy.shape[0] == M and w.rows >= 64 * F
    assert (lin_w is None) == (lin_old_t is None)
    assert lin_old_t is None or (lin_old_t.shape == (F, M) and lin_old_t.is_contiguous())
    check(lib().dr_h2_dgrad_emb_sgd(ptr(dy), dy.stride(0), ptr(dy_amax), ptr(w.buf), w.plane_stride, w.ld, ptr(w.amax), M, F, K,
                                    ptr(ids_t), ptr(plan.flags), ptr(row_base), ptr(table), ptr(lin_w), ptr(lin_old_t), ptr(sum_x),
                                    ptr(d_fm_logit), float(scale), ptr(d_concat), d_concat.stride(0), ptr(table_amax), stream_ptr()),
          "dr_h2_dgrad_emb_sgd")


def emb_lin_update_unique(ids, row_base, plan, d_fm_logit, scale, dst_lin, slot_lin_grad=None):
    """dst_lin[row] += scale * gradient for every slot whose row is unique in the batch (plan.flags): the part of K4's first-order
    update that emb_pool_bwd_sorted(parts=... | 4) leaves out (dr_emb_lin_update_unique)."""
    ids = _c(ids, torch.int64)
    B, F = ids.shape
    check(lib().dr_emb_lin_update_unique(ptr(ids), ptr(plan.flags), B, F, ptr(row_base), ptr(d_fm_logit), ptr(slot_lin_grad),
                                         float(scale), ptr(dst_lin), stream_ptr()), "dr_emb_lin_update_unique")


def adam_lr_t(lr, beta1, beta2, step):
    """[TF] B15: lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t), t = step counted from 1."""
    return lr * (1.0 - beta2 ** step) ** 0.5 / (1.0 - beta1 ** step)


def emb_pool_bwd_sorted_adam(ids, row_base, plan, D, num_rows, grad, d_fm_logit, lr_t, beta1, beta2, eps, table, m_table,
                             v_table, lin_w=None, m_lin=None, v_lin=None, concat=None, sum_x=None, slot_lin_grad=None, x_sorted=None,
                             lin_old_t=None, table_amax=None):
    """Sorted K4 with a fused row-wise Adam update (see dr_emb_pool_bwd_sorted_adam in include/dr_hotpath.h)."""
    ids = _c(ids, torch.int64)
    B, F = ids.shape
    assert grad.stride(1) == 1
    assert lin_old_t is None or (lin_old_t.shape == (F, B) and lin_old_t.is_contiguous())
    check(lib().dr_emb_pool_bwd_sorted_adam(ptr(ids), ptr(row_base), ptr(plan.rows), ptr(plan.slots), ptr(plan.flags),
                                            ptr(plan.dup_heads), ptr(plan.dup_count), B, F, D, int(num_rows), ptr(grad),
                                            grad.stride(0), ptr(concat), concat.stride(0) if concat is not None else 0,
                                            ptr(sum_x), ptr(d_fm_logit), ptr(slot_lin_grad), float(lr_t), float(beta1),
                                            float(beta2), float(eps), ptr(table), ptr(m_table), ptr(v_table), ptr(lin_w),
                                            ptr(m_lin), ptr(v_lin), ptr(x_sorted), ptr(lin_old_t), ptr(table_amax), stream_ptr()),
          "dr_emb_pool_bwd_sorted_adam")


def adam_catchup_rows(ids, row_base, table, m_table, v_table, lin_w, m_lin, v_lin, row_step, upto, stamp, lr, beta1=0.9,
                      beta2=0.999, eps=1e-8):
    """TF's non-lazy sparse Adam evaluated lazily (dr_adam_catchup_rows): replays the decay-only steps the rows named by
    ids [B, F] have missed, up to step `upto`, and stamps them `stamp` in row_step [R] int32."""
    ids = _c(ids, torch.int64)
    B, F = ids.shape
    assert row_step.dtype == torch.int32 and row_step.is_contiguous()
    check(lib().dr_adam_catchup_rows(ptr(ids), B * F, F, ptr(row_base), table.shape[1], ptr(table), ptr(m_table), ptr(v_table),
                                     ptr(lin_w), ptr(m_lin), ptr(v_lin), ptr(row_step), int(upto), int(stamp), float(lr),
                                     float(beta1), float(beta2), float(eps), stream_ptr()), "dr_adam_catchup_rows")


def adam_step(param, grad, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """Dense Adam step over flat fp32 buffers (in place)."""
    assert param.is_contiguous() and grad.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    n = param.numel()
    assert grad.numel() == n and m.numel() == n and v.numel() == n
    check(lib().dr_adam_step(ptr(param), ptr(grad), ptr(m), ptr(v), n, float(lr_t), float(beta1), float(beta2), float(eps),
                             float(grad_scale), stream_ptr()), "dr_adam_step")


def ftrl_step(param, grad, accum, linear, lr, lr_power=-0.5, l1=0.0, l2=0.0, grad_scale=1.0):
    """Dense FTRL-Proximal step, TensorFlow formulation, over flat fp32 buffers (in place)."""
    assert param.is_contiguous() and grad.is_contiguous() and accum.is_contiguous() and linear.is_contiguous()
    n = param.numel()
    assert grad.numel() == n and accum.numel() == n and linear.numel() == n
    check(lib().dr_ftrl_step(ptr(param), ptr(grad), ptr(accum), ptr(linear), n, float(lr), float(lr_power), float(l1), float(l2),
                             float(grad_scale), stream_ptr()), "dr_ftrl_step")


def linear_bwd_dx_fm(dy, W, d_fm_logit, sum_x, concat, D, FD, out):
    """First-layer dgrad with the FM second-order gradient folded into the epilogue."""
    dy = _rowmajor_ld4(dy)
    W = _rowmajor_ld4(W)
    M, N = dy.shape
    K = W.shape[0]
    check(lib().dr_linear_bwd_dx_fm(ptr(dy), dy.stride(0), ptr(W), W.stride(0), M, K, N, ptr(d_fm_logit), ptr(sum_x),
                                    ptr(concat), concat.stride(0), int(D), int(FD), ptr(out), out.stride(0),
                                    stream_ptr()), "dr_linear_bwd_dx_fm")
    return out


# ----------------------------------------------------------------------------------------------
# K9 / K10   two-tower retrieval
# ----------------------------------------------------------------------------------------------
def _check_inbatch_shapes(q, c, cand_prob, cand_ids, sample_weight):
    """The fused K9 kernels assume a square in-batch problem (one candidate per query): they take B from q and index every
    per-candidate / per-query vector with it.  Anything else must go through the explicit score matrix (sbcnm.Retrieval does)."""
    B, D = q.shape
    if c.dim() != 2 or c.shape[0] != B or c.shape[1] != D:
        raise ValueError("in-batch softmax kernels need candidates of shape %s, got %s" % ((B, D), tuple(c.shape)))
    for name, t in (("candidate_sampling_probability", cand_prob), ("candidate_ids", cand_ids), ("sample_weight", sample_weight)):
        if t is not None and t.numel() != B:
            raise ValueError("%s must have %d elements, got %d" % (name, B, t.numel()))
    return (_dense_arg(cand_prob, "candidate_sampling_probability", numel=B), _dense_arg(cand_ids, "candidate_ids", torch.int64, numel=B),
            _dense_arg(sample_weight, "sample_weight", numel=B))


def inbatch_softmax_fwd(q, c, cand_prob=None, cand_ids=None, sample_weight=None, inv_temperature=1.0):
    q = _c(q, torch.float32)
    c = _c(c, torch.float32)
    cand_prob, cand_ids, sample_weight = _check_inbatch_shapes(q, c, cand_prob, cand_ids, sample_weight)
    B, D = q.shape
    dev = q.device
    row_lse = torch.empty(B, dtype=torch.float32, device=dev)
    pos = torch.empty(B, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    nbytes = lib().dr_inbatch_softmax_workspace_bytes(B)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    check(lib().dr_inbatch_softmax_fwd(ptr(q), ptr(c), B, D, ptr(cand_prob), ptr(cand_ids), ptr(sample_weight),
                                       float(inv_temperature), ptr(row_lse), ptr(pos), ptr(loss), ptr(ws), nbytes,
                                       stream_ptr()), "dr_inbatch_softmax_fwd")
    return loss, row_lse, pos


def inbatch_softmax_grad_scores(q, c, row_lse, d_loss, cand_prob=None, cand_ids=None, sample_weight=None,
                                inv_temperature=1.0):
    cand_prob, cand_ids, sample_weight = _check_inbatch_shapes(q, c, cand_prob, cand_ids, sample_weight)
    B, D = q.shape
    q = _c(q, torch.float32)
    c = _c(c, torch.float32)
    row_lse = _dense_arg(row_lse, "inbatch_softmax_grad_scores: row_lse", numel=B)
    G = torch.empty((B, _pad4(B)), dtype=torch.float32, device=q.device)[:, :B]
    # with a workspace the pass may run on the f16x2 register-split kernel (it needs the candidates as fp16 planes)
    nbytes = lib().dr_inbatch_softmax_workspace_bytes(B)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device)
    check(lib().dr_inbatch_softmax_grad_scores(ptr(q), ptr(c), B, D, ptr(cand_prob), ptr(cand_ids), ptr(sample_weight),
                                               float(inv_temperature), ptr(row_lse), float(d_loss), ptr(G), G.stride(0),
                                               ptr(ws), nbytes, stream_ptr()), "dr_inbatch_softmax_grad_scores")
    return G


def scores_nt(a, b, out=None):
    a = _rowmajor_ld4(a)
    b = _rowmajor_ld4(b)
    M, D = a.shape
    N = b.shape[0]
    if b.shape[1] != D:
        raise ValueError("scores_nt: a %s and b %s differ in width" % (tuple(a.shape), tuple(b.shape)))
    if out is None:
        out = torch.empty((M, _pad4(N)), dtype=torch.float32, device=a.device)[:, :N]
    check(lib().dr_scores_nt(ptr(a), a.stride(0), ptr(b), b.stride(0), M, N, D, ptr(out), out.stride(0), stream_ptr()),
          "dr_scores_nt")
    return out


def topk_state(Bq, k, device):
    return (torch.empty((Bq, k), dtype=torch.float32, device=device), torch.empty((Bq, k), dtype=torch.int64, device=device))


def topk_select(scores, k, index_base=0, init=True, state=None):
    """row-wise top-k of an explicit [Bq, n] score matrix, folded into `state` (scores, index)."""
    if scores.dtype != torch.float32 or scores.dim() != 2 or (scores.shape[1] > 1 and scores.stride(1) != 1) or \
            (scores.shape[0] > 1 and scores.stride(0) < scores.shape[1]):
        raise ValueError("topk_select: scores must be fp32 [Bq, n] with unit column stride and a row stride >= n, got %s %s with strides %s"
                         % (scores.dtype, tuple(scores.shape), tuple(scores.stride())))
    Bq, n = scores.shape
    if state is None:
        state = topk_state(Bq, k, scores.device)
    check(lib().dr_topk_select(ptr(scores), scores.stride(0), Bq, n, int(k), int(index_base), int(bool(init)),
                               ptr(state[0]), ptr(state[1]), stream_ptr()), "dr_topk_select")
    return state


class TopKIndex:
    """The corpus side of an exact top-K index (dr_topk_index_build; BruteForce.index / Streaming's candidates of the reference:
    candidates are handed over once, queries arrive many times): the corpus' amax record and fp16 planes, which dr_topk_mips would
    otherwise derive from the corpus on every call.  `topk_mips(q, index, k)` takes it in place of the corpus; the result is the same
    bit for bit.  The planes follow the corpus tensor: written in place since the build (`_version`), they are rebuilt on the next use.
    Corpora the planes do not cover (D not a multiple of 4, D > 512, empty) keep `buf` None and take the plain path."""

    def __init__(self, cand):
        # `cand` must be the caller's own fp32 tensor: staleness is detected through ITS version counter (a copy made here would
        # never see the caller's later writes; writes through raw pointers -- another library -- are not seen either: call rebuild())
        self.cand = _c(cand, torch.float32)
        N, D = self.cand.shape
        self.buf = None
        self._able = N > 0 and D % 4 == 0 and 4 <= D <= 512 and self.cand.is_cuda
        self._ver = None
        self.ensure_fresh()

    def _wanted(self):
        # the planes are only read by the f16x2 scan on the matrix-pipe GEMM mode (dr_topk_mips_indexed ignores them otherwise): a second
        # copy of the corpus is not allocated for a split that will not use it -- it is built on the first use that does
        return self._able and get_gemm_split() == "f16x2" and get_gemm_mode() == "bf16x3"

    def ensure_fresh(self):
        if not self._wanted():
            return
        if self.buf is None:
            N, D = self.cand.shape
            self.buf = torch.empty(lib().dr_topk_index_bytes(N, D) // 4, dtype=torch.float32, device=self.cand.device)
            assert self.buf.data_ptr() % 256 == 0
            self._ver = None
        if self._ver != self.cand._version:
            self.rebuild()

    def rebuild(self):
        """Recompute the record and the planes from the corpus as it stands (also after writes torch's version counter cannot see)."""
        if self.buf is not None:
            N, D = self.cand.shape
            check(lib().dr_topk_index_build(ptr(self.cand), N, D, ptr(self.buf), self.buf.numel() * 4, stream_ptr()), "dr_topk_index_build")
            self._ver = self.cand._version

    @property
    def shape(self):
        return self.cand.shape


def topk_mips(q, cand, k, index_base=0, init=True, state=None, workspace=None):
    """cand: the corpus [N, D] fp32, or a TopKIndex built from it."""
    q = _c(q, torch.float32)
    index = cand if isinstance(cand, TopKIndex) else None
    cand = index.cand if index is not None else _c(cand, torch.float32)
    Bq, D = q.shape
    N = cand.shape[0]
    if state is None:
        state = topk_state(Bq, k, q.device)
    if workspace is None:
        workspace = torch.empty(max(1, lib().dr_topk_workspace_bytes(Bq, N, int(k)) // 4), dtype=torch.float32, device=q.device)
    if index is not None:
        index.ensure_fresh()
    if index is not None and index.buf is not None and index._wanted():
        rc = lib().dr_topk_mips_indexed(ptr(q), Bq, ptr(cand), ptr(index.buf), N, D, int(k), int(index_base), int(bool(init)),
                                        ptr(state[0]), ptr(state[1]), ptr(workspace), workspace.numel() * 4, stream_ptr())
    else:
        rc = lib().dr_topk_mips(ptr(q), Bq, ptr(cand), N, D, int(k), int(index_base), int(bool(init)), ptr(state[0]),
                                ptr(state[1]), ptr(workspace), workspace.numel() * 4, stream_ptr())
    if rc == _lib.DR_ESHAPE:
        raise ValueError("Tried to retrieve k={k} top items, but candidate batch too small."
                         "To resolve this, 1. increase batch-size, 2. set `drop_remainder`=True, "
                         "3. set `handle_incomplete_batches`=True in constructor.".format(k=k))
    check(rc, "dr_topk_mips")
    return state


IVF_BUILD_MAX_LISTS = 8192          # IVB_MAXLIST of csrc/ivf.hip


def ivf_build_lists(assign, nlist):
    """(order [N] int64, list_start [nlist + 1] int64): the vectors grouped by coarse list, input order kept inside a list
    (dr_ivf_build_lists: stable counting sort on the device)."""
    assign = _c(assign, torch.int64)
    N = assign.numel()
    if int(nlist) > IVF_BUILD_MAX_LISTS:
        # more coarse lists than the kernel's LDS histogram holds (8192; the reference's own examples use 100): a stable sort by list
        # through torch -- index build, not the search path
        valid = (assign >= 0) & (assign < int(nlist))
        key = torch.where(valid, assign, torch.full_like(assign, int(nlist)))
        order = torch.sort(key, stable=True).indices[:int(valid.sum())]
        list_start = torch.zeros(int(nlist) + 1, dtype=torch.int64, device=assign.device)
        list_start[1:] = torch.cumsum(torch.bincount(assign[valid], minlength=int(nlist)), 0)
        return order, list_start
    order = torch.empty(max(N, 1), dtype=torch.int64, device=assign.device)[:N]
    list_start = torch.empty(int(nlist) + 1, dtype=torch.int64, device=assign.device)
    nb = lib().dr_ivf_build_workspace_bytes(N, int(nlist))
    ws = torch.empty(max(1, nb // 8), dtype=torch.int64, device=assign.device)
    check(lib().dr_ivf_build_lists(ptr(assign), N, int(nlist), ptr(order), ptr(list_start), ptr(ws), ws.numel() * 8, stream_ptr()),
          "dr_ivf_build_lists")
    return order, list_start


def ivf_pack(cand, order, list_start, ids=None):
    """IVF-Flat storage: lists padded to 64-vector blocks, each block dimension-major.  -> (packed, packed_ids, blk_off)"""
    cand = _c(cand, torch.float32)
    N, D = cand.shape
    nlist = list_start.numel() - 1
    counts = (list_start[1:] - list_start[:-1])
    nblk = (counts + 63) // 64
    blk_off = torch.zeros(nlist + 1, dtype=torch.int64, device=cand.device)
    blk_off[1:] = torch.cumsum(nblk, 0)
    total = int(blk_off[-1].item())
    packed = torch.empty(max(total, 1) * D * 64, dtype=torch.float32, device=cand.device)
    packed_ids = torch.empty(max(total, 1) * 64, dtype=torch.int64, device=cand.device)
    check(lib().dr_ivf_pack(ptr(cand), N, D, ptr(_c(order, torch.int64)), ptr(_c(list_start, torch.int64)), ptr(blk_off), nlist,
                            total, ptr(ids), ptr(packed), ptr(packed_ids), stream_ptr()), "dr_ivf_pack")
    return packed, packed_ids, blk_off


def ivf_scan(q, probes, blk_off, packed, packed_ids, k):
    q = _c(q, torch.float32)
    probes = _c(probes, torch.int64)
    Bq, D = q.shape
    s, i = topk_state(Bq, k, q.device)
    check(lib().dr_ivf_scan(ptr(q), Bq, D, ptr(probes), probes.shape[1], ptr(blk_off), ptr(packed), ptr(packed_ids), int(k), ptr(s),
                            ptr(i), stream_ptr()), "dr_ivf_scan")
    return s, i


PQ_KSUB = 256                       # codewords per sub-quantiser (one byte per code)
PQ_MAX_K = 128                      # drtk::KMAX


def pq_check(D, m):
    """validates the domain of dr_pq_encode / dr_ivfpq_scan; returns (D, m, dsub) as ints"""
    D, m = int(D), int(m)
    if m % 4 != 0 or not 4 <= m <= 64:
        raise ValueError("ivfpq: the number of sub-quantisers m must be a multiple of 4 in [4, 64], got m = %d" % m)
    if not 1 <= D <= 1024:
        raise ValueError("ivfpq: the dimension D must lie in [1, 1024], got D = %d" % D)
    if D % m != 0:
        raise ValueError("ivfpq: D must be a multiple of m, got D = %d, m = %d" % (D, m))
    if D // m > 64:
        raise ValueError("ivfpq: a sub-vector holds D / m <= 64 components (its codebook slice sits in LDS), got D = %d, m = %d, "
                         "D / m = %d" % (D, m, D // m))
    return D, m, D // m


def _pq_k(k, what):
    k = int(k)
    if not 1 <= k <= PQ_MAX_K:
        raise ValueError("ivfpq: %s must lie in [1, %d], got %d" % (what, PQ_MAX_K, k))
    return k


def _pq_mat(t, what, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError("%s must be a 2-d %s tensor, got %s" % (what, dtype, tuple(t.shape) if hasattr(t, "shape") else type(t)))
    return _dense_arg(t, what, dtype=dtype)


def pq_encode(x, codebooks, assign=None, centroids=None):
    """codes int32 [N, m / 4] (code j of a vector in bits 8 * (j % 4) of word j / 4) of x [N, D] against codebooks [m, 256, D / m]:
    the nearest codeword of every sub-vector of x - centroids[assign] (assign / centroids None: of x itself).  dr_pq_encode."""
    if not isinstance(codebooks, torch.Tensor) or codebooks.dim() != 3 or codebooks.shape[1] != PQ_KSUB:
        raise ValueError("pq_encode: codebooks must be fp32 [m, %d, D / m], got %s" % (PQ_KSUB, tuple(getattr(codebooks, "shape", ()))))
    x = _pq_mat(x, "pq_encode: x")
    N, D = x.shape
    m = codebooks.shape[0]
    D, m, dsub = pq_check(D, m)
    codebooks = _dense_arg(codebooks, "pq_encode: codebooks", shape=(m, PQ_KSUB, dsub))
    if (assign is None) != (centroids is None):
        raise ValueError("pq_encode: assign and centroids come together (both None: x is the residual)")
    nlist = 0
    if assign is not None:
        centroids = _pq_mat(centroids, "pq_encode: centroids")
        nlist = centroids.shape[0]
        if centroids.shape[1] != D or nlist < 1:
            raise ValueError("pq_encode: centroids must be fp32 [nlist >= 1, %d], got %s" % (D, tuple(centroids.shape)))
        assign = _dense_arg(assign, "pq_encode: assign", dtype=torch.int64, numel=N)
    codes = torch.empty((N, m // 4), dtype=torch.int32, device=x.device)
    check(lib().dr_pq_encode(ptr(x), ptr(assign), ptr(centroids), nlist, ptr(codebooks), N, D, m, ptr(codes), stream_ptr()),
          "dr_pq_encode")
    return codes


def ivfpq_scan(q, probes, probe_scores, blk_off, packed_codes, packed_rows, codebooks, k):
    """(scores [Bq, k], rows [Bq, k] int64): the ADC top k of each query over its probed lists (dr_ivfpq_scan).  probes / probe_scores
    [Bq, nprobe] as ops.topk_mips(q, centroids, nprobe) returns them (a probe < 0 is skipped); packed_codes (int32 words, or the fp32
    view ops.ivf_pack returns), packed_rows and blk_off in ops.ivf_pack's layout; codebooks [m, 256, D / m]."""
    if not isinstance(codebooks, torch.Tensor) or codebooks.dim() != 3 or codebooks.shape[1] != PQ_KSUB:
        raise ValueError("ivfpq_scan: codebooks must be fp32 [m, %d, D / m], got %s" % (PQ_KSUB, tuple(getattr(codebooks, "shape", ()))))
    q = _pq_mat(q, "ivfpq_scan: q")
    Bq, D = q.shape
    m = codebooks.shape[0]
    D, m, dsub = pq_check(D, m)
    k = _pq_k(k, "k")
    codebooks = _dense_arg(codebooks, "ivfpq_scan: codebooks", shape=(m, PQ_KSUB, dsub))
    probes = _pq_mat(probes, "ivfpq_scan: probes", dtype=torch.int64)
    nprobe = probes.shape[1]
    if probes.shape[0] != Bq or nprobe < 1:
        raise ValueError("ivfpq_scan: probes must be int64 [%d, nprobe >= 1], got %s" % (Bq, tuple(probes.shape)))
    probe_scores = _dense_arg(probe_scores, "ivfpq_scan: probe_scores", shape=(Bq, nprobe))
    blk_off = _dense_arg(blk_off, "ivfpq_scan: blk_off", dtype=torch.int64)
    if blk_off.dim() != 1 or blk_off.numel() < 2:
        raise ValueError("ivfpq_scan: blk_off must be int64 [nlist + 1], got %s" % (tuple(blk_off.shape),))
    if packed_codes.dtype not in (torch.int32, torch.float32) or not packed_codes.is_contiguous() or \
            packed_codes.numel() % (64 * (m // 4)) != 0:
        raise ValueError("ivfpq_scan: packed_codes must be contiguous int32 (or fp32-viewed) words, a whole number of 64-vector blocks "
                         "of m / 4 = %d words, got %s with %d elements" % (m // 4, packed_codes.dtype, packed_codes.numel()))
    packed_rows = _dense_arg(packed_rows, "ivfpq_scan: packed_rows", dtype=torch.int64, numel=packed_codes.numel() // (m // 4))
    s, i = topk_state(Bq, k, q.device)
    check(lib().dr_ivfpq_scan(ptr(q), ptr(probes), ptr(probe_scores), ptr(blk_off), ptr(packed_codes), ptr(packed_rows), ptr(codebooks),
                              Bq, D, m, nprobe, k, ptr(s), ptr(i), stream_ptr()), "dr_ivfpq_scan")
    return s, i


def rerank_topk(q, cand, rows, k):
    """(scores [Bq, k], rows [Bq, k] int64): the exact fp32 inner products of q [Bq, D] with cand[rows[b, t]] (rows [Bq, kin <= 128]
    int64, entries < 0: none), top k by score descending, ties to the lower row (dr_rerank_topk)."""
    q = _pq_mat(q, "rerank_topk: q")
    cand = _pq_mat(cand, "rerank_topk: cand")
    Bq, D = q.shape
    if cand.shape[1] != D or not 1 <= D <= 1024:
        raise ValueError("rerank_topk: q [Bq, D] and cand [N, D] share D in [1, 1024], got %s and %s" % (tuple(q.shape), tuple(cand.shape)))
    rows = _pq_mat(rows, "rerank_topk: rows", dtype=torch.int64)
    kin = rows.shape[1]
    if rows.shape[0] != Bq:
        raise ValueError("rerank_topk: rows must be int64 [%d, kin], got %s" % (Bq, tuple(rows.shape)))
    _pq_k(kin, "kin (the width of rows)")
    k = _pq_k(k, "k")
    s, i = topk_state(Bq, k, q.device)
    check(lib().dr_rerank_topk(ptr(q), ptr(cand), ptr(rows), Bq, cand.shape[0], D, kin, k, ptr(s), ptr(i), stream_ptr()),
          "dr_rerank_topk")
    return s, i


def topk_merge(sa, ia, sb, ib, k):
    Bq = sa.shape[0]
    out = topk_state(Bq, k, sa.device)
    check(lib().dr_topk_merge(ptr(sa), ptr(ia), sa.shape[1], ptr(sb), ptr(ib), sb.shape[1], Bq, int(k), ptr(out[0]),
                              ptr(out[1]), stream_ptr()), "dr_topk_merge")
    return out


def rows_scale(x, s, mode=0, fallback=None, out=None):
    """out[r, :] = x[r, :] * f(s[r]) (dr_rows_scale): mode 0 f = s; 1 f = 1 / sqrt(s), rows with s == 0 unchanged; 2 f = 1 / s, rows with
    s == 0 taken from `fallback`."""
    x = _c(x, torch.float32)
    s = _c(s, torch.float32).reshape(-1)
    M, D = x.shape
    assert s.numel() == M and (fallback is None or (fallback.shape == x.shape and fallback.is_contiguous()))
    if out is None:
        out = torch.empty_like(x)
    else:
        _dense_arg(out, "rows_scale: out", shape=(M, D), copy=False)
    check(lib().dr_rows_scale(ptr(x), ptr(s), int(mode), ptr(fallback), M, D, ptr(out), stream_ptr()), "dr_rows_scale")
    return out


def rowdot(a, b):
    a = _c(a, torch.float32)
    b = _c(b, torch.float32)
    if a.dim() != 2 or b.shape != a.shape:
        raise ValueError("rowdot: a and b must be [M, D] alike, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    out = torch.empty((a.shape[0], 1), dtype=torch.float32, device=a.device)
    check(lib().dr_rowdot(ptr(a), ptr(b), a.shape[0], a.shape[1], ptr(out), stream_ptr()), "dr_rowdot")
    return out


def gather_i64(src, idx):
    src = _c(src, torch.int64)
    idx = _c(idx, torch.int64)
    out = torch.empty_like(idx)
    check(lib().dr_gather_i64(ptr(src), src.numel(), ptr(idx), idx.numel(), ptr(out), stream_ptr()), "dr_gather_i64")
    return out


def take_along_rows(arr, idx):
    idx = _c(idx, torch.int64)
    arr = arr if arr.stride(1) == 1 else arr.contiguous()
    B, C = arr.shape
    if idx.dim() != 2 or idx.shape[0] != B or (B > 1 and arr.stride(0) < C):
        raise ValueError("take_along_rows: arr [B, C] with a row stride >= C and idx [B, K], got %s with strides %s and %s"
                         % (tuple(arr.shape), tuple(arr.stride()), tuple(idx.shape)))
    K = idx.shape[1]
    out = torch.empty((B, K), dtype=arr.dtype, device=arr.device)
    if arr.dtype == torch.float32:
        fn, nm = lib().dr_take_along_rows_f32, "dr_take_along_rows_f32"
    elif arr.dtype == torch.int64:
        fn, nm = lib().dr_take_along_rows_i64, "dr_take_along_rows_i64"
    else:
        raise TypeError("take_along_rows supports float32 / int64, got %s" % arr.dtype)
    check(fn(ptr(arr), arr.stride(0), B, C, ptr(idx), K, ptr(out), stream_ptr()), nm)
    return out


def topk_hits(pos, topk, ks, hits):
    """hits[t] += number of rows whose positive is within the top ks[t] ([TF] in_top_k semantics)."""
    pos = _c(pos.reshape(-1), torch.float32)
    topk = _c(topk, torch.float32)
    check(lib().dr_topk_hits(ptr(pos), ptr(topk), pos.numel(), topk.shape[1], ptr(ks), ks.numel(), ptr(hits), stream_ptr()),
          "dr_topk_hits")


def exclude_adjust(scores, ids, exclude):
    scores = _c(scores, torch.float32)
    ids = _c(ids, torch.int64)
    exclude = _c(exclude, torch.int64)
    out = torch.empty_like(scores)
    check(lib().dr_exclude_adjust(ptr(scores), ptr(ids), scores.shape[0], scores.shape[1], ptr(exclude), exclude.shape[1],
                                  ptr(out), stream_ptr()), "dr_exclude_adjust")
    return out


def logits_adjust(logits, labels=None, cand_prob=None, cand_ids=None, add_label_scale=0.0):
    logits = _c(logits, torch.float32)
    if logits.dim() != 2:
        raise ValueError("logits_adjust: logits must be [B, C], got %s" % (tuple(logits.shape),))
    labels = _dense_arg(labels, "logits_adjust: labels", shape=logits.shape)
    cand_prob = _dense_arg(cand_prob, "logits_adjust: cand_prob", numel=logits.shape[1])
    cand_ids = _dense_arg(cand_ids, "logits_adjust: cand_ids", torch.int64, numel=logits.shape[1])
    if (cand_ids is not None or add_label_scale) and labels is None:
        raise ValueError("logits_adjust: cand_ids and add_label_scale need labels")
    out = torch.empty_like(logits)
    check(lib().dr_logits_adjust(ptr(logits), ptr(labels), logits.shape[0], logits.shape[1], ptr(cand_prob), ptr(cand_ids),
                                 float(add_label_scale), ptr(out), stream_ptr()), "dr_logits_adjust")
    return out


def topk_init(Bq, k, device):
    """empty running top-k lists (scores -inf, index -1)"""
    state = topk_state(Bq, k, device)
    check(lib().dr_topk_select(None, 0, Bq, 0, int(k), 0, 1, ptr(state[0]), ptr(state[1]), stream_ptr()), "dr_topk_select")
    return state


def softmax_ce_rows(logits, labels, inv_temperature=1.0, sample_weight=None):
    logits = _c(logits, torch.float32)
    labels = _dense_arg(labels, "softmax_ce_rows: labels", shape=logits.shape)
    B, C = logits.shape
    sample_weight = _dense_arg(sample_weight, "softmax_ce_rows: sample_weight", numel=B)
    row = torch.empty(B, dtype=torch.float32, device=logits.device)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    check(lib().dr_softmax_ce_rows(ptr(logits), ptr(labels), B, C, float(inv_temperature), ptr(sample_weight), ptr(row),
                                   ptr(loss), stream_ptr()), "dr_softmax_ce_rows")
    return loss.reshape(())


def softmax_ce_rows_bwd(logits, labels, inv_temperature, sample_weight, d_loss, cols=None, out=None):
    """gradient of softmax_ce_rows w.r.t. logits; with `cols` scattered into the pre-zeroed matrix `out`."""
    logits = _c(logits, torch.float32)
    labels = _dense_arg(labels, "softmax_ce_rows_bwd: labels", shape=logits.shape)
    B, C = logits.shape
    sample_weight = _dense_arg(sample_weight, "softmax_ce_rows_bwd: sample_weight", numel=B)
    if cols is not None and (cols.dtype != torch.int64 or tuple(cols.shape) != (B, C)):
        raise ValueError("softmax_ce_rows_bwd: cols must be int64 %s, got %s %s" % ((B, C), cols.dtype, tuple(cols.shape)))
    if out is None:
        if cols is not None:
            raise ValueError("softmax_ce_rows_bwd: cols scatter into a pre-zeroed `out`")
        out = torch.empty((B, C), dtype=torch.float32, device=logits.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or (cols is None and out.shape[1] != C) or \
            (out.shape[1] > 1 and out.stride(1) != 1) or (B > 1 and out.stride(0) < out.shape[1]):
        raise ValueError("softmax_ce_rows_bwd: out must be fp32 [%d, N] with unit column stride and a row stride >= N, got %s %s with strides %s"
                         % (B, out.dtype, tuple(out.shape), tuple(out.stride())))
    check(lib().dr_softmax_ce_rows_bwd(ptr(logits), ptr(labels), B, C, float(inv_temperature), ptr(sample_weight), float(d_loss),
                                       ptr(_c(cols, torch.int64)) if cols is not None else None, ptr(out), out.stride(0),
                                       stream_ptr()), "dr_softmax_ce_rows_bwd")
    return out


def emb_pack_grads(pos, D, d_concat, concat, sum_x, d_fm_logit, out_rows, out_lin=None, bias_sum=None, unique_flags=None):
    pos = _c(pos, torch.int64)
    B, F = pos.shape
    # unique_flags: de-duplicated exchange -- several slots per destination, shared rows accumulate (zero-filled buffers)
    check(lib().dr_emb_pack_grads(ptr(pos), ptr(unique_flags), B, F, D, ptr(d_concat), d_concat.stride(0), ptr(concat),
                                  concat.stride(0) if concat is not None else 0, ptr(sum_x), ptr(d_fm_logit), ptr(out_rows),
                                  ptr(out_lin), ptr(bias_sum), stream_ptr()), "dr_emb_pack_grads")


# ---- GEMM product mode (include/dr_hotpath.h: DR_GEMM_BF16X3 / DR_GEMM_NATIVE_F32) ------------------------------
GEMM_BF16X3, GEMM_NATIVE_F32 = 0, 1
_GEMM_MODES = {"bf16x3": GEMM_BF16X3, "native": GEMM_NATIVE_F32}


def set_gemm_mode(mode):
    """'bf16x3' (default: fp32 products as six bf16 MFMA products of exact three-way splits) or 'native'
    (v_mfma_f32_32x32x2_f32).  Returns the previous mode's name.  Process-wide."""
    m = _GEMM_MODES[mode] if isinstance(mode, str) else int(mode)
    prev = _lib.lib().dr_set_gemm_mode(m)
    if prev < 0:
        raise ValueError("unknown GEMM mode %r" % (mode,))
    return "native" if prev == GEMM_NATIVE_F32 else "bf16x3"


def get_gemm_mode():
    return "native" if _lib.lib().dr_get_gemm_mode() == GEMM_NATIVE_F32 else "bf16x3"


GEMM_SPLIT_BF16X3, GEMM_SPLIT_F16X2 = 0, 1
_GEMM_SPLITS = {"bf16x3": GEMM_SPLIT_BF16X3, "f16x2": GEMM_SPLIT_F16X2}


def set_gemm_split(split):
    """'f16x2' (default) or 'bf16x3': the operand split the engines (at construction) and the exact top-K scan (at every call) use
    for their register-split GEMMs -- the library's dr_set_gemm_split, the one switch (and the one parser of DR_GEMM_SPLIT).
    Returns the previous split's name.  Process-wide."""
    v = _GEMM_SPLITS[split] if isinstance(split, str) else int(split)
    prev = _lib.lib().dr_set_gemm_split(v)
    if prev < 0:
        raise ValueError("unknown GEMM split %r" % (split,))
    return "f16x2" if prev == GEMM_SPLIT_F16X2 else "bf16x3"


def get_gemm_split():
    return "f16x2" if _lib.lib().dr_get_gemm_split() == GEMM_SPLIT_F16X2 else "bf16x3"


# ---- K7p: first tower layer on pre-split operands ("planes": three bf16 terms per fp32 value, include/dr_hotpath.h) -------
class Planes:
    """planes[3][rows_alloc][ld] bf16 in HBM holding an fp32 matrix [rows, cols] exactly (v = (v2 + v1) + v0).
    rows_alloc = roundup(rows, 32) and ld = roundup(cols, 32), zero-filled: both paddings are read by the GEMMs."""

    def __init__(self, rows, cols, device):
        self.rows, self.cols = int(rows), int(cols)
        self.rows_alloc = (self.rows + 31) // 32 * 32
        self.ld = (self.cols + 31) // 32 * 32
        self.buf = torch.zeros((3, self.rows_alloc, self.ld), dtype=torch.bfloat16, device=device)

    @property
    def plane_stride(self):
        return self.rows_alloc * self.ld


def bf3_split(src, planes: Planes, row_offset=0, col_offset=0, transpose=False):
    """fp32 [R, C] -> planes[p][row_offset + r][col_offset + c] (or [row_offset + c][col_offset + r] when transpose)."""
    assert src.dim() == 2 and src.stride(1) == 1 and src.dtype == torch.float32
    R, C = src.shape
    check(lib().dr_bf3_split(ptr(src), src.stride(0), R, C, ptr(planes.buf), planes.plane_stride, planes.ld, row_offset,
                             col_offset, 1 if transpose else 0, stream_ptr()), "dr_bf3_split")
    return planes


def bf3_join(planes: Planes, out=None):
    if out is None:
        out = torch.empty((planes.rows, planes.cols), dtype=torch.float32, device=planes.buf.device)
    check(lib().dr_bf3_join(ptr(planes.buf), planes.plane_stride, planes.ld, planes.rows, planes.cols, ptr(out),
                            out.stride(0), stream_ptr()), "dr_bf3_join")
    return out


def bf3_gemm_nt(a: Planes, b: Planes, bias=None, act=0, mask=None, out=None):
    """out[m, n] = act(sum_k A[m, k] B[n, k] + bias[n]), zeroed where mask <= 0.  A = a (rows M), B = b (rows N)."""
    M, N = a.rows, b.rows
    assert a.ld == b.ld, "operands must share the padded reduction length"
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.buf.device)
    assert out.shape == (M, N) and out.stride(1) == 1
    check(lib().dr_bf3_gemm_nt(ptr(a.buf), a.plane_stride, a.ld, ptr(b.buf), b.plane_stride, b.ld, M, N, a.ld, ptr(bias),
                               int(act), ptr(mask), mask.stride(0) if mask is not None else 0, ptr(out), out.stride(0),
                               stream_ptr()), "dr_bf3_gemm_nt")
    return out


def bf3_linear_nt(a, b: Planes, bias=None, act=0, mask=None, accumulate=False, out=None):
    """out[m, n] (+)= act(sum_k a[m, k] B[n, k] + bias[n]) (zeroed where mask <= 0): fp32 activations x pre-split weights.
    b holds the weights as planes with rows = output features and cols = the reduction (W^T for the forward, W for the dgrad)."""
    a = _rowmajor_ld4(a)
    M, K = a.shape
    if a.stride(0) % 4 or a.data_ptr() % 16:          # the kernel reads 16-byte vectors: rows must start 16-byte aligned
        buf = torch.zeros((M, _pad4(K)), dtype=torch.float32, device=a.device)
        buf[:, :K].copy_(a)
        a = buf[:, :K]
    N = b.rows
    assert b.cols == K, "weights' planes must have the reduction length as columns"
    if out is None:
        assert not accumulate
        out = torch.empty((M, _pad4(N)), dtype=torch.float32, device=a.device)[:, :N]
    assert out.shape == (M, N) and out.stride(1) == 1
    check(lib().dr_bf3_linear_nt(ptr(a), a.stride(0), ptr(b.buf), b.plane_stride, b.ld, M, N, K, ptr(bias), int(act), ptr(mask),
                                 mask.stride(0) if mask is not None else 0, int(bool(accumulate)), ptr(out), out.stride(0),
                                 stream_ptr()), "dr_bf3_linear_nt")
    return out


def bf3_linear_nt_pack(dy, w: Planes, pos, d_fm_logit, out_rows, out_lin=None, bias_sum=None, sum_x=None, x=None):
    """First-layer dgrad + emb_pack_grads in one launch (dr_bf3_linear_nt_pack): out_rows[pos[m, f], :] = (dy @ W^T)[m, 64 f : 64 f + 64]
    + d_fm_logit[m] * (sum_x[m] - x[m, 64 f : 64 f + 64]); out_lin[pos[m, f]] = d_fm_logit[m]; bias_sum += sum(d_fm_logit).
    w: the layer's W as planes (rows = input features).  D is 64."""
    dy = _rowmajor_ld4(dy)
    M, K = dy.shape
    pos = _c(pos, torch.int64)
    F = pos.shape[1]
    assert w.cols == K and w.rows >= 64 * F and out_rows.is_contiguous() and out_rows.shape[1] == 64
    check(lib().dr_bf3_linear_nt_pack(ptr(dy), dy.stride(0), ptr(w.buf), w.plane_stride, w.ld, M, w.rows, K, ptr(pos), F,
                                      ptr(d_fm_logit), ptr(sum_x), ptr(x), x.stride(0) if x is not None else 0, ptr(out_rows),
                                      ptr(out_lin), ptr(bias_sum), stream_ptr()), "dr_bf3_linear_nt_pack")
    return out_rows


def h2_linear_nt_pack(dy, dy_amax, w: "H2Planes", pos, d_fm_logit, out_rows, out_lin=None, bias_sum=None, sum_x=None, x=None):
    """bf3_linear_nt_pack in the f16x2 operand mode (dr_h2_linear_nt_pack): dy with its amax record, w the layer's W as H2Planes."""
    dy = _rowmajor_ld4(dy)
    M, K = dy.shape
    pos = _c(pos, torch.int64)
    F = pos.shape[1]
    assert w.cols == K and w.rows >= 64 * F and out_rows.is_contiguous() and out_rows.shape[1] == 64
    check(lib().dr_h2_linear_nt_pack(ptr(dy), dy.stride(0), ptr(dy_amax), ptr(w.buf), w.plane_stride, w.ld, ptr(w.amax), M, w.rows, K,
                                     ptr(pos), F, ptr(d_fm_logit), ptr(sum_x), ptr(x), x.stride(0) if x is not None else 0,
                                     ptr(out_rows), ptr(out_lin), ptr(bias_sum), stream_ptr()), "dr_h2_linear_nt_pack")
    return out_rows


def bf3_cross_fwd(x0, x, wt: Planes, b=None, diag_scale=0.0, want_prod=False, prod=None):
    """DCN cross layer on pre-split weights (wt = W^T planes): out = x0 * (x @ W + b + diag * x) + x; (out, prod) as cross_fwd."""
    M, Dm = x.shape
    assert x0.shape == x.shape and x0.stride(0) == x.stride(0) and wt.rows == Dm and wt.cols == Dm
    ld = x.stride(0)
    out = torch.empty((M, ld), dtype=torch.float32, device=x.device)[:, :Dm]
    if want_prod and prod is None:
        prod = torch.empty((M, ld), dtype=torch.float32, device=x.device)[:, :Dm]
    if prod is not None:
        assert prod.stride(0) == ld
    check(lib().dr_bf3_cross_fwd(ptr(x0), ptr(x), ld, ptr(wt.buf), wt.plane_stride, wt.ld, ptr(b), float(diag_scale), M, Dm, ptr(out),
                                 ptr(prod), stream_ptr()), "dr_bf3_cross_fwd")
    return out, prod


def bf3_emb_linear_fwd(ids, row_base, field_rows_max, table, lin_w, lin_bias, dense_pad, concat, K, wt: Planes, bias, act, sum_x, fm_logit, out,
                       lin_vals_t=None):
    """K3 + first Dense in one launch (dr_bf3_emb_linear_fwd): gathers the field embeddings of ids [M, F] from table [R, 64] as the
    GEMM's activation operand, writes them to concat[:, :64 F], the FM terms to sum_x / fm_logit, and
    out = act([embeddings, dense_pad[:, :K - 64 F]] @ W + bias).  dense_pad: [M, 32] zero-padded dense features (None iff
    K == 64 F); field_rows_max: the longest field's row count.  Raises RuntimeError(DR_ESHAPE) for D != 64, more than 32 dense
    features or a field of more than 2^24 rows."""
    ids = _c(ids, torch.int64)
    M, F = ids.shape
    assert (concat is None or concat.stride(1) == 1) and out.stride(1) == 1 and wt.cols == K and out.shape == (M, wt.rows)
    assert dense_pad is None or (dense_pad.shape == (M, 32) and dense_pad.is_contiguous())
    # lin_vals_t: also save every slot's first-order weight, field-major [F, M] (emb_pool_bwd_sorted's lin_old_t)
    assert lin_vals_t is None or (lin_vals_t.shape == (F, M) and lin_vals_t.is_contiguous() and lin_vals_t.dtype == torch.float32)
    check(lib().dr_bf3_emb_linear_fwd(ptr(ids), M, F, ptr(row_base), int(field_rows_max), ptr(table), table.shape[1], ptr(lin_w), ptr(lin_bias),
                                      ptr(dense_pad), ptr(concat), concat.stride(0) if concat is not None else 0, int(K), ptr(wt.buf), wt.plane_stride, wt.ld,
                                      wt.rows, ptr(bias), int(act), ptr(sum_x), ptr(fm_logit), ptr(out), out.stride(0), ptr(lin_vals_t),
                                      stream_ptr()), "dr_bf3_emb_linear_fwd")
    return out


def bf3_wgrad_workspace(R, F, N, device):
    return torch.empty(max(64, lib().dr_bf3_wgrad_workspace_bytes(int(R), int(F), int(N)) // 4), dtype=torch.float32, device=device)


def bf3_wgrad_emb(ids_t, row_base, table, dense_pad, dy, scale, dstW, dstb=None, workspace=None, parts=3):
    """bf3_wgrad of the first tower layer with x gathered from the tables (dr_bf3_wgrad_emb): ids_t [nf, R] int32 field-major,
    dense_pad [R, 32] or None; dstW [64 nf + Nd, N]."""
    nf, R = ids_t.shape
    F, N = dstW.shape
    assert ids_t.dtype == torch.int32 and ids_t.is_contiguous() and dy.stride(1) == 1 and dstW.stride(1) == 1 and dy.shape == (R, N)
    assert dense_pad is None or (dense_pad.shape == (R, 32) and dense_pad.is_contiguous())
    if workspace is None:
        workspace = bf3_wgrad_workspace(R, F, N, dy.device)
    # parts 1: the split-K GEMM into the workspace, 2: the reduce that applies it (may run on another stream)
    check(lib().dr_bf3_wgrad_emb(ptr(ids_t), R, nf, ptr(row_base), ptr(table), table.shape[1], ptr(dense_pad), ptr(dy), dy.stride(0),
                                 F, N, float(scale), ptr(dstW), dstW.stride(0), ptr(dstb), ptr(workspace), workspace.numel() * 4,
                                 int(parts), stream_ptr()), "dr_bf3_wgrad_emb")
    return dstW


def bf3_wgrad(x, dy, scale, dstW, dstb=None, workspace=None):
    """dstW += scale * x^T @ dy ; dstb += scale * colsum(dy): register-split wgrad on fp32 activations (deterministic)."""
    R, F = x.shape
    N = dy.shape[1]
    assert x.stride(1) == 1 and dy.stride(1) == 1 and dstW.shape == (F, N) and dstW.stride(1) == 1 and dy.shape[0] == R
    if workspace is None:
        workspace = bf3_wgrad_workspace(R, F, N, x.device)
    check(lib().dr_bf3_wgrad(ptr(x), x.stride(0), ptr(dy), dy.stride(0), R, F, N, float(scale), ptr(dstW), dstW.stride(0),
                             ptr(dstb), ptr(workspace), workspace.numel() * 4, stream_ptr()), "dr_bf3_wgrad")
    return dstW


class WeightPlanes:
    """Both pre-split forms of a Dense kernel W [K, N]: `wt` = W^T planes (rows N: the forward's B operand) and `w` = W planes
    (rows K: the dgrad's B operand).  refresh() after every update of W (two dr_bf3_split launches).

    One of the three GEMM families of a weight (WeightPlanes, H2WeightPlanes, PlainWeight): fwd / dgrad / wgrad / cross_fwd (and, on the
    two planes families, the first layer's emb_linear_fwd / wgrad_emb / linear_nt_pack) take the same arguments in every family and
    are direct calls of that family's kernels.  Amax records: a family with wants_amax False ignores the record arguments; a method
    returns the record it left for its output, or None.  wgrad_ws: the bf3_wgrad_workspace the wgrads run in (None: one per call)."""
    wants_amax = False

    def __init__(self, W, wgrad_ws=None):
        K, N = W.shape
        self.W = W
        self.wgrad_ws = wgrad_ws
        self.wt = Planes(N, K, W.device)
        self.w = Planes(K, N, W.device)
        self.refresh()

    def fwd(self, x, x_amax, bias, act, out, out_amax=None):
        bf3_linear_nt(x, self.wt, bias=bias, act=act, out=out)

    def dgrad(self, dy, dy_amax, mask, out, accumulate=False, out_amax=None):
        bf3_linear_nt(dy, self.w, mask=mask, accumulate=accumulate, out=out)

    def wgrad(self, x, x_amax, dy, dy_amax, scale, dstW, dstb):
        bf3_wgrad(x, dy, scale, dstW, dstb, workspace=self.wgrad_ws)

    def cross_fwd(self, x0, x, x_amax, b, diag, want_prod, out_amax=None):
        """-> (out, prod, the record left for out)"""
        return bf3_cross_fwd(x0, x, self.wt, b, diag, want_prod=want_prod) + (None,)

    def emb_linear_fwd(self, ids, row_base, field_rows_max, table, table_amax, lin_w, lin_bias, dense_pad, dense_amax, concat, K, bias, act,
                       sum_x, fm_logit, out, lin_vals_t=None):
        bf3_emb_linear_fwd(ids, row_base, field_rows_max, table, lin_w, lin_bias, dense_pad, concat, K, self.wt, bias, act, sum_x, fm_logit,
                           out, lin_vals_t=lin_vals_t)

    def wgrad_emb(self, ids_t, row_base, table, table_amax, dense_pad, dense_amax, dy, dy_amax, scale, dstW, dstb, parts):
        bf3_wgrad_emb(ids_t, row_base, table, dense_pad, dy, scale, dstW, dstb, workspace=self.wgrad_ws, parts=parts)

    def linear_nt_pack(self, dy, dy_amax, pos, d_fm_logit, out_rows, out_lin, bias_sum, sum_x, x):
        bf3_linear_nt_pack(dy, self.w, pos, d_fm_logit, out_rows, out_lin, bias_sum, sum_x=sum_x, x=x)

    def refresh(self):
        bf3_split(self.W, self.wt, transpose=True)
        bf3_split(self.W, self.w)
        self._ver = self.W._version

    def ensure_fresh(self):
        """Planes are SHADOW copies: forward / dgrad read them, not W.  The engines refresh them after their own (kernel-side)
        updates; a write to W from outside -- checkpoint restore, W.copy_ / fill_ in a test, a broadcast -- bumps torch's version
        counter of the parameter buffer, which is what this checks at the top of every step (host compare, no launch)."""
        if self.W._version != self._ver:
            self.refresh()


# ---- "f16x2" operand mode of the first tower layer's GEMMs (dr_h2_*, include/dr_hotpath.h) -------------------------------------------
def h2_record(device):
    """An amax record: one uint32 (held as int32) with max |x| of a tensor as float bits; 0 = nothing seen yet."""
    return torch.zeros(1, dtype=torch.int32, device=device)


def h2_amax(src, amax=None, reset=True):
    """amax = max(0 if reset else amax, max |src|) as float bits (dr_h2_amax); src fp32 [R, C] with unit inner stride (or 1-D)."""
    if src.dim() == 1:
        src = src.view(1, -1)
    assert src.dim() == 2 and src.stride(1) == 1 and src.dtype == torch.float32
    if amax is None:
        amax = h2_record(src.device)
    R, C = src.shape
    check(lib().dr_h2_amax(ptr(src), src.stride(0) if R > 1 else max(C, 1), R, C, ptr(amax), 1 if reset else 0, stream_ptr()), "dr_h2_amax")
    return amax


def h2_amax_value(amax):
    """The record as a float (host sync; tests and diagnostics)."""
    return float(amax.view(torch.float32).item())


class H2Planes:
    """planes[2][rows_alloc][ld] fp16 in HBM: the two terms of W * s, s from the record `amax` (shared by the W and W^T planes of one
    weight).  Same padding rules as Planes."""

    def __init__(self, rows, cols, device, amax=None):
        self.rows, self.cols = int(rows), int(cols)
        self.rows_alloc = (self.rows + 31) // 32 * 32
        self.ld = (self.cols + 31) // 32 * 32
        self.buf = torch.zeros((2, self.rows_alloc, self.ld), dtype=torch.float16, device=device)
        self.amax = amax if amax is not None else h2_record(device)

    @property
    def plane_stride(self):
        return self.rows_alloc * self.ld


def h2_split(src, planes: H2Planes, row_offset=0, col_offset=0, transpose=False):
    """fp32 [R, C] * s(planes.amax) -> two fp16 planes (layout of bf3_split).  planes.amax must already cover src (h2_amax)."""
    assert src.dim() == 2 and src.stride(1) == 1 and src.dtype == torch.float32
    R, C = src.shape
    check(lib().dr_h2_split(ptr(src), src.stride(0), R, C, ptr(planes.buf), planes.plane_stride, planes.ld, row_offset, col_offset,
                            1 if transpose else 0, ptr(planes.amax), stream_ptr()), "dr_h2_split")
    return planes


def h2_linear_nt(a, a_amax, b: H2Planes, bias=None, act=0, mask=None, accumulate=False, out=None, out_amax=None):
    """bf3_linear_nt in the f16x2 mode: a fp32 [M, K] with its amax record, b the weights as H2Planes.  out_amax (a record, optional)
    receives max |out|: what the next GEMM needs to take `out` as ITS operand."""
    a = _rowmajor_ld4(a)
    M, K = a.shape
    if a.stride(0) % 4 or a.data_ptr() % 16:
        buf = torch.zeros((M, _pad4(K)), dtype=torch.float32, device=a.device)
        buf[:, :K].copy_(a)
        a = buf[:, :K]
    N = b.rows
    assert b.cols == K, "weights' planes must have the reduction length as columns"
    if out is None:
        assert not accumulate
        out = torch.empty((M, _pad4(N)), dtype=torch.float32, device=a.device)[:, :N]
    assert out.shape == (M, N) and out.stride(1) == 1
    check(lib().dr_h2_linear_nt(ptr(a), a.stride(0), ptr(a_amax), ptr(b.buf), b.plane_stride, b.ld, ptr(b.amax), M, N, K, ptr(bias), int(act),
                                ptr(mask), mask.stride(0) if mask is not None else 0, int(bool(accumulate)), ptr(out), out.stride(0),
                                ptr(out_amax), stream_ptr()), "dr_h2_linear_nt")
    return out


def h2_cross_fwd(x0, x, x_amax, wt: H2Planes, b=None, diag_scale=0.0, want_prod=False, prod=None, out_amax=None):
    """bf3_cross_fwd in the f16x2 mode (x_amax: the record of x; out_amax: receives the record of out)."""
    M, Dm = x.shape
    assert x0.shape == x.shape and x0.stride(0) == x.stride(0) and wt.rows == Dm and wt.cols == Dm
    ld = x.stride(0)
    out = torch.empty((M, ld), dtype=torch.float32, device=x.device)[:, :Dm]
    if want_prod and prod is None:
        prod = torch.empty((M, ld), dtype=torch.float32, device=x.device)[:, :Dm]
    if prod is not None:
        assert prod.stride(0) == ld
    check(lib().dr_h2_cross_fwd(ptr(x0), ptr(x), ld, ptr(x_amax), ptr(wt.buf), wt.plane_stride, wt.ld, ptr(wt.amax), ptr(b), float(diag_scale),
                                M, Dm, ptr(out), ptr(prod), ptr(out_amax), stream_ptr()), "dr_h2_cross_fwd")
    return out, prod


def h2_emb_linear_fwd(ids, row_base, field_rows_max, table, table_amax, lin_w, lin_bias, dense_pad, dense_amax, concat, K, wt: H2Planes, bias, act,
                      sum_x, fm_logit, out, lin_vals_t=None):
    """bf3_emb_linear_fwd in the f16x2 mode (dr_h2_emb_linear_fwd): table_amax >= max |table|, dense_amax the record of dense_pad."""
    ids = _c(ids, torch.int64)
    M, F = ids.shape
    assert (concat is None or concat.stride(1) == 1) and out.stride(1) == 1 and wt.cols == K and out.shape == (M, wt.rows)
    assert dense_pad is None or (dense_pad.shape == (M, 32) and dense_pad.is_contiguous())
    assert lin_vals_t is None or (lin_vals_t.shape == (F, M) and lin_vals_t.is_contiguous() and lin_vals_t.dtype == torch.float32)
    check(lib().dr_h2_emb_linear_fwd(ptr(ids), M, F, ptr(row_base), int(field_rows_max), ptr(table), table.shape[1], ptr(table_amax), ptr(lin_w),
                                     ptr(lin_bias), ptr(dense_pad), ptr(dense_amax), ptr(concat), concat.stride(0) if concat is not None else 0,
                                     int(K), ptr(wt.buf), wt.plane_stride, wt.ld, ptr(wt.amax), wt.rows, ptr(bias), int(act), ptr(sum_x),
                                     ptr(fm_logit), ptr(out), out.stride(0), ptr(lin_vals_t), stream_ptr()), "dr_h2_emb_linear_fwd")
    return out


def h2_emb_linear_tail_supported(M, N, H):
    """Shape domain of the fused first layer with the tower tail as its epilogue (dr_h2_emb_linear_tail_fwd)."""
    return N == 256 and 0 < H <= 32 and M > 0 and M % 32 == 0


def h2_emb_linear_tail_workspace(M, device):
    return torch.empty(max(128, lib().dr_h2_emb_linear_tail_fwd_workspace_bytes(int(M)) // 4), dtype=torch.float32, device=device)


def h2_emb_linear_tail_fwd(ids, row_base, field_rows_max, table, table_amax, lin_w, lin_bias, dense_pad, dense_amax, concat, K, wt: H2Planes, bias,
                           act, sum_x, fm_logit, out, W1, b1, W2, b2, labels, loss_mode, scale, dx, lin_vals_t=None, dst_W1="inplace",
                           dst_b1="inplace", dst_W2="inplace", dst_b2="inplace", prob=None, d_logit=None, d_h=None, loss=None, workspace=None,
                           parts=3, dx_amax=None):
    """h2_emb_linear_fwd + tower_tail_fused (extra_logit = fm_logit) in one kernel and the tail's reduce (dr_h2_emb_linear_tail_fwd): the
    tail runs on the forward GEMM's accumulators.  out (h0) may be None: it is then not written.  Returns (loss, prob, d_logit, dx)."""
    ids = _c(ids, torch.int64)
    M, F = ids.shape
    N, H = wt.rows, W1.shape[1]
    dev = table.device
    dst_W1 = W1 if isinstance(dst_W1, str) else dst_W1
    dst_b1 = b1 if isinstance(dst_b1, str) else dst_b1
    dst_W2 = W2 if isinstance(dst_W2, str) else dst_W2
    dst_b2 = b2 if isinstance(dst_b2, str) else dst_b2
    assert (concat is None or concat.stride(1) == 1) and wt.cols == K and (out is None or (out.stride(1) == 1 and out.shape == (M, N)))
    assert dense_pad is None or (dense_pad.shape == (M, 32) and dense_pad.is_contiguous())
    assert lin_vals_t is None or (lin_vals_t.shape == (F, M) and lin_vals_t.is_contiguous() and lin_vals_t.dtype == torch.float32)
    assert W1.shape[0] == N and W1.stride(1) == 1 and dst_W1.stride(1) == 1 and W2.shape == (H, 1) and dx.shape == (M, N) and dx.stride(1) == 1
    assert labels.numel() == M and labels.is_contiguous() and labels.dtype == torch.float32
    prob = prob if prob is not None else torch.empty(M, dtype=torch.float32, device=dev)
    d_logit = d_logit if d_logit is not None else torch.empty(M, dtype=torch.float32, device=dev)
    loss = loss if loss is not None else torch.empty(1, dtype=torch.float32, device=dev)
    if workspace is None:
        workspace = h2_emb_linear_tail_workspace(M, dev)
    check(lib().dr_h2_emb_linear_tail_fwd(
        ptr(ids), M, F, ptr(row_base), int(field_rows_max), ptr(table), table.shape[1], ptr(table_amax), ptr(lin_w), ptr(lin_bias),
        ptr(dense_pad), ptr(dense_amax), ptr(concat), concat.stride(0) if concat is not None else 0, int(K), ptr(wt.buf), wt.plane_stride,
        wt.ld, ptr(wt.amax), N, ptr(bias), int(act), ptr(sum_x), ptr(fm_logit), ptr(out), out.stride(0) if out is not None else 0,
        ptr(lin_vals_t), ptr(W1), W1.stride(0), ptr(b1), H, ptr(W2), W2.stride(0), ptr(b2), ptr(labels), int(loss_mode), float(scale),
        ptr(dst_W1), dst_W1.stride(0), ptr(dst_b1), ptr(dst_W2), dst_W2.stride(0) if dst_W2 is not None else 0, ptr(dst_b2), ptr(prob),
        ptr(d_logit), ptr(d_h), d_h.stride(0) if d_h is not None else 0, ptr(dx), dx.stride(0), ptr(loss), ptr(workspace),
        workspace.numel() * 4, int(parts), ptr(dx_amax), stream_ptr()), "dr_h2_emb_linear_tail_fwd")
    return loss, prob, d_logit, dx


def h2_wgrad(x, x_amax, dy, dy_amax, scale, dstW, dstb=None, workspace=None):
    """bf3_wgrad in the f16x2 mode."""
    R, F = x.shape
    N = dy.shape[1]
    assert x.stride(1) == 1 and dy.stride(1) == 1 and dstW.shape == (F, N) and dstW.stride(1) == 1 and dy.shape[0] == R
    if workspace is None:
        workspace = bf3_wgrad_workspace(R, F, N, x.device)
    check(lib().dr_h2_wgrad(ptr(x), x.stride(0), ptr(x_amax), ptr(dy), dy.stride(0), ptr(dy_amax), R, F, N, float(scale), ptr(dstW),
                            dstW.stride(0), ptr(dstb), ptr(workspace), workspace.numel() * 4, stream_ptr()), "dr_h2_wgrad")
    return dstW


def h2_wgrad_emb(ids_t, row_base, table, table_amax, dense_pad, dense_amax, dy, dy_amax, scale, dstW, dstb=None, workspace=None, parts=3):
    """bf3_wgrad_emb in the f16x2 mode."""
    nf, R = ids_t.shape
    F, N = dstW.shape
    assert ids_t.dtype == torch.int32 and ids_t.is_contiguous() and dy.stride(1) == 1 and dstW.stride(1) == 1 and dy.shape == (R, N)
    assert dense_pad is None or (dense_pad.shape == (R, 32) and dense_pad.is_contiguous())
    if workspace is None:
        workspace = bf3_wgrad_workspace(R, F, N, dy.device)
    check(lib().dr_h2_wgrad_emb(ptr(ids_t), R, nf, ptr(row_base), ptr(table), table.shape[1], ptr(table_amax), ptr(dense_pad), ptr(dense_amax),
                                ptr(dy), dy.stride(0), ptr(dy_amax), F, N, float(scale), ptr(dstW), dstW.stride(0), ptr(dstb), ptr(workspace),
                                workspace.numel() * 4, int(parts), stream_ptr()), "dr_h2_wgrad_emb")
    return dstW


class H2WeightPlanes:
    """WeightPlanes in the f16x2 mode: W^T and W as two fp16 planes each, one amax record; refresh() = dr_h2_amax + two dr_h2_split."""

    wants_amax = True       # every activation operand comes with its record; out_amax (a record) receives the output's

    def __init__(self, W, double_buffer=False, wgrad_ws=None):
        """double_buffer: refresh() writes the W image (`w`) and the record into a SECOND buffer pair and then makes them current, so a
        kernel still reading the previous `w` (with the previous record) may run beside the refresh -- the caller keeps the H2Planes
        object it took before calling refresh().  `wt` is single: nothing may read it while a refresh runs."""
        K, N = W.shape
        self.W = W
        self.wgrad_ws = wgrad_ws
        self.amax = h2_record(W.device)
        self.wt = H2Planes(N, K, W.device, self.amax)
        self.w = H2Planes(K, N, W.device, self.amax)
        self._w_alt = H2Planes(K, N, W.device, h2_record(W.device)) if double_buffer else None
        self._parts = None
        self._ride_words = None
        self.refresh()

    def _swap(self):
        if self._w_alt is not None:
            self.w, self._w_alt = self._w_alt, self.w
            self.amax = self.w.amax
            self.wt.amax = self.amax

    def hand_off(self):
        """refresh()'s bookkeeping without its launches: the image swap, the record pointers and the version stamp, for a caller whose own
        launch on the current stream writes the record and both images (ops.emb_pool_bwd_dups_apply(refresh=...)) before anything reads
        them.  Returns (w, wt, record, 1024 words of scratch for that launch)."""
        if self._ride_words is None:
            self._ride_words = torch.zeros(1024, dtype=torch.int32, device=self.W.device)
        self._swap()
        self._ver = self.W._version
        return self.w, self.wt, self.amax, self._ride_words

    def refresh(self):
        # record + both images in two launches (dr_h2_refresh_weight: no memset, no atomic pass; same record, same planes as
        # dr_h2_amax + two dr_h2_split)
        if self._parts is None:
            self._parts = torch.zeros(256, dtype=torch.int32, device=self.W.device)
        K, N = self.W.shape
        self._swap()
        check(lib().dr_h2_refresh_weight(ptr(self.W), self.W.stride(0), K, N, ptr(self.w.buf), self.w.plane_stride, self.w.ld,
                                         ptr(self.wt.buf), self.wt.plane_stride, self.wt.ld, ptr(self.amax), ptr(self._parts),
                                         stream_ptr()), "dr_h2_refresh_weight")
        self._ver = self.W._version

    def ensure_fresh(self):
        if self.W._version != self._ver:
            self.refresh()

    def fwd(self, x, x_amax, bias, act, out, out_amax=None):
        h2_linear_nt(x, x_amax, self.wt, bias=bias, act=act, out=out, out_amax=out_amax)
        return out_amax

    def dgrad(self, dy, dy_amax, mask, out, accumulate=False, out_amax=None):
        h2_linear_nt(dy, dy_amax, self.w, mask=mask, accumulate=accumulate, out=out, out_amax=out_amax)
        return out_amax

    def wgrad(self, x, x_amax, dy, dy_amax, scale, dstW, dstb):
        h2_wgrad(x, x_amax, dy, dy_amax, scale, dstW, dstb, workspace=self.wgrad_ws)

    def cross_fwd(self, x0, x, x_amax, b, diag, want_prod, out_amax=None):
        return h2_cross_fwd(x0, x, x_amax, self.wt, b, diag, want_prod=want_prod, out_amax=out_amax) + (out_amax,)

    def emb_linear_fwd(self, ids, row_base, field_rows_max, table, table_amax, lin_w, lin_bias, dense_pad, dense_amax, concat, K, bias, act,
                       sum_x, fm_logit, out, lin_vals_t=None):
        h2_emb_linear_fwd(ids, row_base, field_rows_max, table, table_amax, lin_w, lin_bias, dense_pad, dense_amax, concat, K, self.wt, bias,
                          act, sum_x, fm_logit, out, lin_vals_t=lin_vals_t)

    def wgrad_emb(self, ids_t, row_base, table, table_amax, dense_pad, dense_amax, dy, dy_amax, scale, dstW, dstb, parts):
        h2_wgrad_emb(ids_t, row_base, table, table_amax, dense_pad, dense_amax, dy, dy_amax, scale, dstW, dstb, workspace=self.wgrad_ws,
                     parts=parts)

    def linear_nt_pack(self, dy, dy_amax, pos, d_fm_logit, out_rows, out_lin, bias_sum, sum_x, x):
        h2_linear_nt_pack(dy, dy_amax, self.w, pos, d_fm_logit, out_rows, out_lin, bias_sum, sum_x=sum_x, x=x)


class PlainWeight:
    """The third GEMM family of a weight W [K, N] (see WeightPlanes): no planes, the dr_linear_* / dr_cross_fwd kernels split both
    operands themselves.  `prims`: whatever provides linear_fwd / linear_bwd_dx / linear_bwd_dw / cross_fwd (default: this module;
    the CPU tests pass oracle-backed ones).  dw_ws: the linear_bwd_dw workspace (None: fp32 atomics -- and off the GPU)."""
    wants_amax = False

    def __init__(self, W, prims=None, dw_ws=None):
        self.W, self.dw_ws = W, dw_ws
        self._fwd, self._bwd_dx, self._bwd_dw, self._cross = ((linear_fwd, linear_bwd_dx, linear_bwd_dw, cross_fwd) if prims is None else
                                                              (prims.linear_fwd, prims.linear_bwd_dx, prims.linear_bwd_dw, getattr(prims, "cross_fwd", None)))

    def refresh(self):
        pass

    ensure_fresh = refresh

    def fwd(self, x, x_amax, bias, act, out, out_amax=None):
        self._fwd(x, self.W, bias, act, out=out)

    def dgrad(self, dy, dy_amax, mask, out, accumulate=False, out_amax=None):
        self._bwd_dx(dy, self.W, relu_src=mask, accumulate=accumulate, out=out)

    def wgrad(self, x, x_amax, dy, dy_amax, scale, dstW, dstb):
        self._bwd_dw(x, dy, scale, dstW, dstb, workspace=self.dw_ws)

    def cross_fwd(self, x0, x, x_amax, b, diag, want_prod, out_amax=None):
        return tuple(self._cross(x0, x, self.W, b, diag, want_prod=want_prod)) + (None,)


def planes_worthwhile(M, K, N):
    """Shapes the register-split GEMM (256 x 256 tiles) is built for; smaller layers stay on dr_linear_*."""
    return get_gemm_mode() == "bf16x3" and M >= 2048 and N >= 128 and K >= 64


def bf3_gemm_tn_workspace(R, F, N, device):
    return torch.empty(max(64, lib().dr_bf3_gemm_tn_workspace_bytes(int(R), int(F), int(N)) // 4), dtype=torch.float32,
                       device=device)


def bf3_gemm_tn(x: Planes, y: Planes, scale, dstW, y_colsum=None, dstb=None, workspace=None):
    """dstW[f, n] += scale * sum_r X[r, f] Y[r, n];  dstb += scale * y_colsum."""
    R, F, N = x.rows, x.cols, y.cols
    assert y.rows == R and dstW.shape == (F, N) and dstW.stride(1) == 1
    if workspace is None:
        workspace = bf3_gemm_tn_workspace(R, F, N, x.buf.device)
    check(lib().dr_bf3_gemm_tn(ptr(x.buf), x.plane_stride, x.ld, ptr(y.buf), y.plane_stride, y.ld, R, F, N, float(scale),
                               ptr(dstW), dstW.stride(0), ptr(y_colsum), ptr(dstb), ptr(workspace), workspace.numel() * 4,
                               stream_ptr()), "dr_bf3_gemm_tn")
    return dstW


# ---- CIN (xDeepFM) and the DIN ActivationUnit input ---------------------------------------------------------------------------
ACT_CODES = {None: 0, "linear": 0, "relu": 1, "sigmoid": 2, "tanh": 3}


def cin_fwd(x0, x, W, bias=None, act=2):
    """out[b, f, d] = act(sum_ij W[i * Hk + j, f] x0[b, i, d] x[b, j, d] + bias[f]);  x0 [B, H0, D], x [B, Hk, D], W [H0 * Hk, Fm]."""
    x0, x, W = _c(x0, torch.float32), _c(x, torch.float32), _c(W, torch.float32)
    B, H0, D = x0.shape
    Hk = x.shape[1]
    Fm = W.shape[1]
    if x.shape != (B, Hk, D) or W.shape[0] != H0 * Hk:
        raise ValueError("cin_fwd: shapes do not agree (x0 %s, x %s, W %s)" % (tuple(x0.shape), tuple(x.shape), tuple(W.shape)))
    bias = _dense_arg(bias, "cin_fwd: bias", numel=Fm)
    out = torch.empty((B, Fm, D), dtype=torch.float32, device=x0.device)
    check(lib().dr_cin_fwd(ptr(x0), ptr(x), B, H0, Hk, D, ptr(W), Fm, ptr(bias), int(act), ptr(out), stream_ptr()), "dr_cin_fwd")
    return out


def cin_bwd(x0, x, W, act, out, d_out, want_bias=False):
    x0, x, W, d_out = _c(x0, torch.float32), _c(x, torch.float32), _c(W, torch.float32), _c(d_out, torch.float32)
    B, H0, D = x0.shape
    Hk, Fm = x.shape[1], W.shape[1]
    if x.shape != (B, Hk, D) or W.shape[0] != H0 * Hk:
        raise ValueError("cin_bwd: shapes do not agree (x0 %s, x %s, W %s)" % (tuple(x0.shape), tuple(x.shape), tuple(W.shape)))
    out = _dense_arg(out, "cin_bwd: out", shape=(B, Fm, D))
    d_out = _dense_arg(d_out, "cin_bwd: d_out", shape=(B, Fm, D))
    d_x0, d_x, dW = torch.empty_like(x0), torch.empty_like(x), torch.empty_like(W)
    dbias = torch.empty(Fm, dtype=torch.float32, device=x0.device) if want_bias else None
    check(lib().dr_cin_bwd(ptr(x0), ptr(x), B, H0, Hk, D, ptr(W), Fm, int(act), ptr(out), ptr(d_out), ptr(d_x0), ptr(d_x), ptr(dW),
                           ptr(dbias), stream_ptr()), "dr_cin_bwd")
    return d_x0, d_x, dW, dbias


def _cin_pool_dims(x0, x, W):
    if x0.dim() != 3 or x.dim() != 3 or W.dim() != 2:
        raise ValueError("cin_pool: x0 [B, H0, D], x [B, Hk, D], W [H0 * Hk, Fm] (got %s, %s, %s)"
                         % (tuple(x0.shape), tuple(x.shape), tuple(W.shape)))
    B, H0, D = x0.shape
    Hk, Fm = x.shape[1], W.shape[1]
    if x.shape != (B, Hk, D) or W.shape[0] != H0 * Hk:
        raise ValueError("cin_pool: shapes do not agree (x0 %s, x %s, W %s)" % (tuple(x0.shape), tuple(x.shape), tuple(W.shape)))
    return B, H0, Hk, D, Fm


def cin_pool_fwd(x0, x, W, bias=None, act=0, want_out=True, want_pooled=True):
    """(out [B, Fm, D] | None, pooled [B, Fm] | None) of dr_cin_pool_fwd: cin_fwd's out and pooled = out.sum(-1) in one launch."""
    x0, x, W = _c(x0, torch.float32), _c(x, torch.float32), _c(W, torch.float32)
    B, H0, Hk, D, Fm = _cin_pool_dims(x0, x, W)
    out = torch.empty((B, Fm, D), dtype=torch.float32, device=x0.device) if want_out else None
    pooled = torch.empty((B, Fm), dtype=torch.float32, device=x0.device) if want_pooled else None
    check(lib().dr_cin_pool_fwd(ptr(x0), ptr(x), B, H0, Hk, D, ptr(W), Fm, ptr(None if bias is None else _c(bias, torch.float32)), int(act),
                                ptr(out), ptr(pooled), stream_ptr()), "dr_cin_pool_fwd")
    return out, pooled


def cin_pool_bwd_partials(B, H0, Hk, D, Fm):
    """how many per-chunk partials of dW dr_cin_pool_bwd adds for these sizes, from the workspace size (include/dr_hotpath.h's formula)"""
    nb = lib().dr_cin_pool_bwd_workspace_bytes(B, H0, Hk, D, Fm)
    packed = H0 * ((Hk + 31) // 32) * ((Fm + 7) // 8) * 256
    return (nb // 4 - packed) // (H0 * Hk * Fm + Fm)


def cin_pool_bwd(x0, x, W, act, out, d_out, d_pooled, want_bias=False, d_x0=None, workspace=None):
    """(d_x0, d_x, dW, dbias | None) of dr_cin_pool_bwd.  d_out [B, Fm, D] or d_pooled [B, Fm] may be None; out may be None for act 0.
    d_x0 given: the gradient is added to it in place (accumulate_x0) and it is returned.  workspace: an fp32 tensor to use instead of
    allocating dr_cin_pool_bwd_workspace_bytes."""
    x0, x, W = _c(x0, torch.float32), _c(x, torch.float32), _c(W, torch.float32)
    B, H0, Hk, D, Fm = _cin_pool_dims(x0, x, W)
    d_out = None if d_out is None else _c(d_out, torch.float32)
    d_pooled = None if d_pooled is None else _c(d_pooled, torch.float32)
    if (d_out is not None and d_out.shape != (B, Fm, D)) or (d_pooled is not None and d_pooled.shape != (B, Fm)) or \
            (out is not None and out.shape != (B, Fm, D)):
        raise ValueError("cin_pool backward: shapes do not agree")
    accumulate = d_x0 is not None
    if accumulate and (d_x0.shape != x0.shape or d_x0.dtype != torch.float32 or not d_x0.is_contiguous()):
        raise ValueError("cin_pool backward: d_x0 to accumulate into must be a contiguous fp32 tensor shaped like x0")
    if not accumulate:
        d_x0 = torch.empty_like(x0)
    d_x, dW = torch.empty_like(x), torch.empty_like(W)
    dbias = torch.empty(Fm, dtype=torch.float32, device=x0.device) if want_bias else None
    ws = workspace
    if ws is None:
        ws = torch.empty(max(lib().dr_cin_pool_bwd_workspace_bytes(B, H0, Hk, D, Fm) // 4, 4), dtype=torch.float32, device=x0.device)
    check(lib().dr_cin_pool_bwd(ptr(x0), ptr(x), B, H0, Hk, D, ptr(W), Fm, int(act), ptr(out), ptr(d_out), ptr(d_pooled), ptr(d_x0),
                                int(accumulate), ptr(d_x), ptr(dW), ptr(dbias), ptr(ws), ws.numel() * 4, stream_ptr()), "dr_cin_pool_bwd")
    return d_x0, d_x, dW, dbias


# ---- DLRM: the pairwise dot interaction (csrc/dot_interact.hip) ------------------------------------------------------------------------
def _di_dims(dense, emb, F, D, self_interaction):
    """validates the domain of dr_dot_interact_*; returns (emb as [B, F * D], its row pitch, B, N, c0, P)"""
    F, D = int(F), _slab_width("dot_interact", D)
    N = F + (0 if dense is None else 1)
    if F < 1 or not 2 <= N <= 64:
        raise ValueError("dot_interact: needs 2 <= N <= 64 vectors per example (F fields + the dense vector), got F = %d, N = %d" % (F, N))
    emb, ld_emb = _rows_arg("dot_interact", emb, F * D, "emb", ((F, D),))
    B = emb.shape[0]
    if dense is not None and dense.shape[0] != B:
        raise ValueError("dot_interact: dense and emb disagree on the batch size")
    c0 = 0 if dense is None else D
    P = N * (N + 1) // 2 if self_interaction else N * (N - 1) // 2
    return emb, ld_emb, B, N, c0, P


def dot_interact_width(F, D, dense=True, self_interaction=False):
    """columns of the interaction output: c0 + P"""
    N = F + (1 if dense else 0)
    return (D if dense else 0) + (N * (N + 1) // 2 if self_interaction else N * (N - 1) // 2)


def dot_interact_fwd(dense, emb, F, D, self_interaction=False, out=None, ld_out=None):
    """out [B, c0 + P] (a view of a [B, ld_out] buffer, zero beyond c0 + P) of dr_dot_interact_fwd: dense [B, D] (or None) copied to the
    first D columns, then the row-major lower triangle of T T^T for T = [dense; emb's F rows].  emb: [B, F, D] contiguous, or
    [B, F * D] with any row stride that is a multiple of 4.  out: a [B, c0 + P] view to write into (its row stride is ld_out)."""
    emb, ld_emb, B, N, c0, P = _di_dims(dense, emb, F, D, self_interaction)
    ld_dense = 0 if dense is None else _row_pitch("dot_interact", dense, D, "dense")
    if out is None:
        ld_out = _pad4(c0 + P) if ld_out is None else int(ld_out)
        if ld_out % 4 != 0 or ld_out < c0 + P:
            raise ValueError("dot_interact: ld_out must be a multiple of 4 and >= %d, got %d" % (c0 + P, ld_out))
        out = torch.empty((B, ld_out), dtype=torch.float32, device=emb.device)[:, :c0 + P]
    else:
        ld_out = _row_pitch("dot_interact", out, c0 + P, "out", written_to_pitch=True)
    if B == 0:
        return out
    st = lib().dr_dot_interact_fwd(ptr(dense), ld_dense, ptr(emb), ld_emb, B, int(F), int(D), int(bool(self_interaction)), ptr(out),
                                   ld_out, stream_ptr())
    _status(st, "dr_dot_interact_fwd")
    return out


def dot_interact_bwd(dense, emb, F, D, d_out, self_interaction=False, d_dense=None, d_emb=None):
    """(d_dense [B, D] | None, d_emb [B, F * D]) of dr_dot_interact_bwd from d_out [B, c0 + P] (row stride a multiple of 4; columns
    beyond c0 + P are not read).  d_dense / d_emb: buffers to overwrite (only their first D / F * D columns are written)."""
    emb, ld_emb, B, N, c0, P = _di_dims(dense, emb, F, D, self_interaction)
    ld_dense = 0 if dense is None else _row_pitch("dot_interact", dense, D, "dense")
    ld_dout = _row_pitch("dot_interact", d_out, c0 + P, "d_out")
    if d_emb is None:
        d_emb = torch.empty((B, F * D), dtype=torch.float32, device=emb.device)
    if dense is not None and d_dense is None:
        d_dense = torch.empty((B, D), dtype=torch.float32, device=emb.device)
    ld_demb = _row_pitch("dot_interact", d_emb, F * D, "d_emb")
    ld_ddense = 0 if dense is None else _row_pitch("dot_interact", d_dense, D, "d_dense")
    if B == 0:
        return (d_dense if dense is not None else None), d_emb
    st = lib().dr_dot_interact_bwd(ptr(dense), ld_dense, ptr(emb), ld_emb, ptr(d_out), ld_dout, B, int(F), int(D),
                                   int(bool(self_interaction)), ptr(d_dense) if dense is not None else None, ld_ddense, ptr(d_emb), ld_demb,
                                   stream_ptr())
    _status(st, "dr_dot_interact_bwd")
    return (d_dense if dense is not None else None), d_emb


# ---- AFM: attention pooling over field pairs (csrc/afm_pool.hip) -----------------------------------------------------------------------
def afm_num_pairs(F):
    """P = F (F - 1) / 2: the pairs (i, j), j < i, numbered q = i (i - 1) / 2 + j"""
    return int(F) * (int(F) - 1) // 2


def _afm_dims(emb, W, b, h, F):
    """validates the domain of dr_afm_pool_* (include/dr_hotpath.h) without a device; returns (emb as [B, F * D], its row pitch, B, F, D,
    A, P)"""
    F = int(F)
    if W.dim() != 2 or b.dim() != 1 or h.dim() != 1 or b.shape[0] != W.shape[1] or h.shape[0] != W.shape[1]:
        raise ValueError("afm_pool: W [D, A], b [A], h [A] expected, got %s, %s, %s" % (tuple(W.shape), tuple(b.shape), tuple(h.shape)))
    if any(t.dtype != torch.float32 for t in (emb, W, b, h)):
        raise ValueError("afm_pool: fp32 tensors only")
    D, A = _slab_width("afm_pool", W.shape[0]), int(W.shape[1])
    if not 1 <= A <= 128:
        raise ValueError("afm_pool: the attention factor A must be in [1, 128], got %d" % A)
    if not 2 <= F <= 64:
        raise ValueError("afm_pool: needs 2 <= F <= 64 fields, got %d" % F)
    pow2 = lambda n: 1 << (n - 1).bit_length()                                                 # noqa: E731
    DT, AT, P = pow2((D + 15) // 16), pow2((A + 15) // 16), F * (F - 1) // 2
    if DT * AT > 32:
        raise ValueError("afm_pool: D = %d with A = %d is outside the kernels' register budget (ceil(D / 16) * ceil(A / 16), each rounded "
                         "up to a power of two, must not exceed 32)" % (D, A))
    PE, PW = 16 * DT + 4, 16 * AT + 4
    if 16 * DT * PW + 32 * AT + (P + 15) // 16 * 16 + 2 * F * PE + 16 * DT + 16 * PW + 16 * PE > 40000:
        raise ValueError("afm_pool: F = %d, D = %d, A = %d do not fit the LDS" % (F, D, A))
    emb, ld_emb = _rows_arg("afm_pool", emb, F * D, "emb", ((F, D),))
    return emb, ld_emb, int(emb.shape[0]), F, D, A, P


def afm_pool_fwd(emb, W, b, h, F, want_attention=False, out=None):
    """(out [B, D], lse [B], attn [B, P] | None) of dr_afm_pool_fwd.  emb: [B, F, D] contiguous, or [B, F * D] with any row stride that
    is a multiple of 4 (the slab's concat, read in place); W [D, A], b [A], h [A].  out: a [B, D] view to write into."""
    emb, ld_emb, B, F, D, A, P = _afm_dims(emb, W, b, h, F)
    if out is None:
        out = torch.empty((B, D), dtype=torch.float32, device=emb.device)
    ld_out = _row_pitch("afm_pool", out, D, "out")
    lse = torch.empty((B,), dtype=torch.float32, device=emb.device)
    attn = torch.empty((B, P), dtype=torch.float32, device=emb.device) if want_attention else None
    if B == 0:
        return out, lse, attn
    W, b, h = W.contiguous(), b.contiguous(), h.contiguous()
    st = lib().dr_afm_pool_fwd(ptr(emb), ld_emb, ptr(W), ptr(b), ptr(h), B, F, D, A, ptr(out), ld_out, ptr(lse), ptr(attn), P,
                               stream_ptr())
    _status(st, "dr_afm_pool_fwd")
    return out, lse, attn


def afm_pool_bwd(emb, W, b, h, F, out, lse, d_out, d_emb=None, workspace=None):
    """(d_emb [B, F * D], dW [D, A], db [A], dh [A]) of dr_afm_pool_bwd from d_out [B, D], with out and lse of afm_pool_fwd.  d_emb: a
    [B, F * D] buffer to overwrite; workspace: fp32, at least dr_afm_pool_bwd_workspace_bytes(B, F, D, A) bytes (allocated when None)."""
    emb, ld_emb, B, F, D, A, P = _afm_dims(emb, W, b, h, F)
    ld_out = _row_pitch("afm_pool", out, D, "out")
    ld_dout = _row_pitch("afm_pool", d_out, D, "d_out")
    if lse.dtype != torch.float32 or tuple(lse.shape) != (B,) or not lse.is_contiguous():
        raise ValueError("afm_pool: lse must be contiguous fp32 [%d], got %s %s" % (B, lse.dtype, tuple(lse.shape)))
    if out.shape[0] != B or d_out.shape[0] != B:
        raise ValueError("afm_pool: emb, out and d_out disagree on the batch size")
    if d_emb is None:
        d_emb = torch.empty((B, F * D), dtype=torch.float32, device=emb.device)
    ld_demb = _row_pitch("afm_pool", d_emb, F * D, "d_emb")
    dW = torch.empty((D, A), dtype=torch.float32, device=emb.device)
    db = torch.empty((A,), dtype=torch.float32, device=emb.device)
    dh = torch.empty((A,), dtype=torch.float32, device=emb.device)
    if B == 0:
        return d_emb, dW.zero_(), db.zero_(), dh.zero_()
    need = lib().dr_afm_pool_bwd_workspace_bytes(B, F, D, A)
    if need < 0:
        _status(int(need), "dr_afm_pool_bwd_workspace_bytes")
    if workspace is None:
        workspace = torch.empty((max(need // 4, 4),), dtype=torch.float32, device=emb.device)
    elif workspace.numel() * workspace.element_size() < need:
        raise ValueError("afm_pool: the workspace holds %d bytes, dr_afm_pool_bwd_workspace_bytes asks for %d"
                         % (workspace.numel() * workspace.element_size(), need))
    W, b, h = W.contiguous(), b.contiguous(), h.contiguous()
    st = lib().dr_afm_pool_bwd(ptr(emb), ld_emb, ptr(W), ptr(b), ptr(h), ptr(out), ld_out, ptr(lse), ptr(d_out), ld_dout, B, F, D, A,
                               ptr(d_emb), ld_demb, ptr(dW), ptr(db), ptr(dh), ptr(workspace),
                               workspace.numel() * workspace.element_size(), stream_ptr())
    _status(st, "dr_afm_pool_bwd")
    return d_emb, dW, db, dh


# ---- PNN: the outer-product layer (csrc/pnn_outer.hip) ------------------------------------------------------------------------------------
def _pnn_dims(emb, W, F):
    """validates the domain of dr_pnn_outer_* (include/dr_hotpath.h) without a device; returns (emb as [B, F * D], B, F, D, N)"""
    F = int(F)
    if not 1 <= F <= 64:
        raise ValueError("pnn_outer: needs 1 <= F <= 64 fields, got %d" % F)
    if emb.dtype != torch.float32 or W.dtype != torch.float32:
        raise ValueError("pnn_outer: fp32 tensors only")
    if emb.dim() == 3:
        if emb.shape[1] != F or not emb.is_contiguous():
            raise ValueError("pnn_outer: a 3-d emb must be contiguous [B, %d, D], got %s" % (F, tuple(emb.shape)))
        emb = emb.reshape(emb.shape[0], F * emb.shape[2])
    elif emb.dim() != 2 or emb.shape[1] % F != 0:
        raise ValueError("pnn_outer: emb must be [B, %d, D] or [B, %d * D], got %s" % (F, F, tuple(emb.shape)))
    D = _slab_width("pnn_outer", int(emb.shape[1]) // F, hi=128)
    if W.dim() != 2 or W.shape[0] != D * D:
        raise ValueError("pnn_outer: W must be [D * D, N] = [%d, N], got %s" % (D * D, tuple(W.shape)))
    N = int(W.shape[1])
    if not 1 <= N <= 4096:
        raise ValueError("pnn_outer: N must be in [1, 4096], got %d" % N)
    return emb, int(emb.shape[0]), F, D, N


def _pnn_rows(t, rows, cols, what, may_copy):
    """a [rows, cols] fp32 matrix with unit column stride and a row stride that is a multiple of 4 and >= cols, every row readable up
    to 4 ceil(cols / 4) floats.  An input in another layout is copied into a padded buffer (as _rowmajor_ld4 does); an output is a
    ValueError."""
    if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (rows, cols):
        raise ValueError("pnn_outer: %s must be fp32 [%d, %d], got %s %s" % (what, rows, cols, t.dtype, tuple(t.shape)))
    if not may_copy:
        _row_pitch("pnn_outer", t, cols, what)                 # used in place or refused; the pitch handed to C is _pnn_ld's
        return t
    if t.stride(1) == 1 and (t.stride(0) % 4 == 0 and t.stride(0) >= cols or rows <= 1 and cols % 4 == 0):
        return t                                               # a single row has no pitch to speak of (_pnn_ld)
    buf = torch.zeros((rows, _pad4(cols)), dtype=torch.float32, device=t.device)
    buf[:, :cols].copy_(t)
    return buf[:, :cols]


def _pnn_ld(t):
    return t.stride(0) if t.shape[0] > 1 else _pad4(t.shape[1])


def pnn_outer_fwd(emb, W, F, addend=None, out=None):
    """(out [B, N], u [B, D]) of dr_pnn_outer_fwd: u = the sum of the F rows of every example, out = (u (x) u) W + addend.  emb: [B, F, D]
    contiguous, or [B, F * D] with any row stride that is a multiple of 4 (the slab's concat, read in place); W [D * D, N], row d * D + e
    for u_d u_e; addend [B, N] or None; out: a [B, N] view to write into."""
    emb, B, F, D, N = _pnn_dims(emb, W, F)
    emb = _pnn_rows(emb, B, F * D, "emb", False)
    if addend is not None:
        addend = _pnn_rows(addend, B, N, "addend", True)
    if out is None:
        out = torch.empty((B, _pad4(N)), dtype=torch.float32, device=emb.device)[:, :N]
    out = _pnn_rows(out, B, N, "out", False)
    u = torch.empty((B, D), dtype=torch.float32, device=emb.device)
    if B == 0:
        return out, u
    W = _pnn_rows(W, D * D, N, "W", True)
    st = lib().dr_pnn_outer_fwd(ptr(emb), _pnn_ld(emb), ptr(W), _pnn_ld(W), ptr(addend), _pnn_ld(addend) if addend is not None else 0,
                                B, F, D, N, ptr(u), D, ptr(out), _pnn_ld(out), stream_ptr())
    _status(st, "dr_pnn_outer_fwd")
    return out, u


def pnn_outer_bwd_workspace(B, F, D, N, device):
    """an fp32 buffer of dr_pnn_outer_bwd_workspace_bytes(B, F, D, N) bytes; ValueError outside the domain"""
    need = int(lib().dr_pnn_outer_bwd_workspace_bytes(int(B), int(F), int(D), int(N)))
    if need < 0:
        _status(need, "dr_pnn_outer_bwd_workspace_bytes")
    return torch.empty((max(need // 4, 4),), dtype=torch.float32, device=device)


def pnn_outer_bwd(u, W, F, d_out, d_emb=None, accumulate=False, workspace=None):
    """(d_emb [B, F * D], dW [D * D, N]) of dr_pnn_outer_bwd from d_out [B, N] and the forward's u [B, D].  d_emb: a [B, F * D] buffer
    to overwrite, or to add to with accumulate=True (then it is required); workspace: fp32, as pnn_outer_bwd_workspace gives it
    (allocated when None)."""
    F = int(F)
    if not 1 <= F <= 64:
        raise ValueError("pnn_outer: needs 1 <= F <= 64 fields, got %d" % F)
    if u.dim() != 2 or u.dtype != torch.float32:
        raise ValueError("pnn_outer: u must be fp32 [B, D], got %s %s" % (u.dtype, tuple(u.shape)))
    _, B, _, D, N = _pnn_dims(u, W, 1)
    if accumulate and d_emb is None:
        raise ValueError("pnn_outer: accumulate=True needs the d_emb to add to")
    u = _pnn_rows(u, B, D, "u", True)
    d_out = _pnn_rows(d_out, B, N, "d_out", True)
    if d_emb is None:
        d_emb = torch.empty((B, F * D), dtype=torch.float32, device=u.device)
    d_emb = _pnn_rows(d_emb, B, F * D, "d_emb", False)
    dW = torch.empty((D * D, _pad4(N)), dtype=torch.float32, device=u.device)[:, :N]
    if B == 0:
        return d_emb, dW.zero_()
    need = int(lib().dr_pnn_outer_bwd_workspace_bytes(B, F, D, N))
    if need < 0:
        _status(need, "dr_pnn_outer_bwd_workspace_bytes")
    if workspace is None:
        workspace = torch.empty((max(need // 4, 4),), dtype=torch.float32, device=u.device)
    elif workspace.numel() * workspace.element_size() < need:
        raise ValueError("pnn_outer: the workspace holds %d bytes, dr_pnn_outer_bwd_workspace_bytes asks for %d"
                         % (workspace.numel() * workspace.element_size(), need))
    W = _pnn_rows(W, D * D, N, "W", True)
    st = lib().dr_pnn_outer_bwd(ptr(u), _pnn_ld(u), ptr(W), _pnn_ld(W), ptr(d_out), _pnn_ld(d_out), B, F, D, N, ptr(d_emb),
                                _pnn_ld(d_emb), 1 if accumulate else 0, ptr(dW), _pnn_ld(dW), ptr(workspace),
                                workspace.numel() * workspace.element_size(), stream_ptr())
    _status(st, "dr_pnn_outer_bwd")
    return d_emb, dW


# ---- DIEN: the GRU / AUGRU recurrence and the evolution layer's attention (csrc/dien.hip) -------------------------------------------------
def _gru_seq3(t, B, T, width, what, may_copy=True):
    """(tensor, ld) of a [B, T, width] fp32 tensor whose rows (b, t) lie at the uniform pitch ld (a multiple of 4, >= width) from a
    16-byte aligned base -- what dr_gru_seq_* address.  Any other layout (a [:, :-1] view, a pitch that is no multiple of 4) is copied
    when may_copy, else a ValueError; a misaligned base is always a ValueError."""
    if t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape) != (B, T, width):
        raise ValueError("gru_seq: %s must be fp32 [%d, %d, %d], got %s %s" % (what, B, T, width, t.dtype, tuple(t.shape)))
    if B * T <= 1:
        ld, ok = _pad4(width), t.stride(2) == 1 or width == 1
    elif T == 1:
        ld, ok = t.stride(0), t.stride(2) == 1
    else:
        ld, ok = t.stride(1), t.stride(2) == 1 and (B == 1 or t.stride(0) == T * t.stride(1))
    ok = ok and ld % 4 == 0 and ld >= width
    if not ok:
        if not may_copy:
            raise ValueError("gru_seq: %s needs unit column stride and rows (b, t) at one pitch that is a multiple of 4 and >= %d, got "
                             "strides %s" % (what, width, tuple(t.stride())))
        t, ld = t.contiguous(), width
    if t.numel() and t.data_ptr() % 16 != 0:
        raise ValueError("gru_seq: %s must start at a 16-byte aligned address" % what)
    return t, ld


def _gru_dense(t, shape, what, dtype=torch.float32, aligned=False):
    if t is None:
        return None
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError("gru_seq: %s must be %s %s, got %s %s" % (what, dtype, list(shape), t.dtype, tuple(t.shape)))
    t = t.contiguous()
    if aligned and t.numel() and t.data_ptr() % 16 != 0:
        raise ValueError("gru_seq: %s must start at a 16-byte aligned address" % what)
    return t


def _gru_lengths(lengths, B):
    """int32 [B]; values outside [0, T] are clamped by the kernels (no host check: it would wait for the device)"""
    if lengths is None:
        return None
    if lengths.dim() != 1 or lengths.shape[0] != B or lengths.dtype not in (torch.int32, torch.int64):
        raise ValueError("gru_seq: lengths must be int32 or int64 [%d], got %s %s" % (B, lengths.dtype, tuple(lengths.shape)))
    return lengths.to(torch.int32).contiguous()


def _gru_dims(xp, U):
    """validates the domain of dr_gru_seq_* (include/dr_hotpath.h) without a device; returns (B, T, H)"""
    if U.dim() != 2 or U.dtype != torch.float32 or U.shape[1] != 3 * U.shape[0]:
        raise ValueError("gru_seq: U must be fp32 [H, 3H], got %s %s" % (U.dtype, tuple(U.shape)))
    H = _slab_width("gru_seq", U.shape[0], "H", hi=128)
    if xp.dim() != 3 or xp.shape[2] != 3 * H:
        raise ValueError("gru_seq: xp must be [B, T, %d], got %s" % (3 * H, tuple(xp.shape)))
    B, T = int(xp.shape[0]), int(xp.shape[1])
    if T < 1:
        raise ValueError("gru_seq: needs T >= 1 time steps, got %d" % T)
    return B, T, H


def gru_seq_fwd(xp, U, h0=None, lengths=None, att=None, hs=None):
    """(hs [B, T, H], h_last [B, H]) of dr_gru_seq_fwd: the GRU (att None) or AUGRU recurrence over xp [B, T, 3H] = x W + b with gate
    columns [u | r | c], U [H, 3H], h0 [B, H] (None: zeros), lengths [B] (None: all T; clamped to [0, T]), att [B, T].  hs: a
    [B, T, H] buffer to write into (rows at one pitch)."""
    B, T, H = _gru_dims(xp, U)
    xp, ld_xp = _gru_seq3(xp, B, T, 3 * H, "xp")
    U = _gru_dense(U, (H, 3 * H), "U")
    h0 = _gru_dense(h0, (B, H), "h0", aligned=True)
    att = _gru_dense(att, (B, T), "att")
    lengths = _gru_lengths(lengths, B)
    if hs is None:
        hs = torch.empty((B, T, H), dtype=torch.float32, device=xp.device)
    hs, ld_hs = _gru_seq3(hs, B, T, H, "hs", may_copy=False)
    h_last = torch.empty((B, H), dtype=torch.float32, device=xp.device)
    if B == 0:
        return hs, h_last
    st = lib().dr_gru_seq_fwd(ptr(xp), ld_xp, ptr(U), ptr(h0), ptr(lengths), ptr(att), B, T, H, ptr(hs), ld_hs, ptr(h_last), stream_ptr())
    _status(st, "dr_gru_seq_fwd")
    return hs, h_last


def gru_seq_bwd_workspace(B, T, H, device):
    need = lib().dr_gru_seq_bwd_workspace_bytes(int(B), int(T), int(H))
    if need < 0:
        _status(int(need), "dr_gru_seq_bwd_workspace_bytes")
    return torch.empty((max(need // 4, 4),), dtype=torch.float32, device=device)


def gru_seq_bwd(xp, U, h0, lengths, att, hs, d_hs=None, d_h_last=None, d_xp=None, workspace=None):
    """(d_xp [B, T, 3H], dU [H, 3H], d_h0 [B, H], d_att [B, T] | None) of dr_gru_seq_bwd from d_hs [B, T, H] and d_h_last [B, H] (None:
    zeros), with the forward's inputs and its hs.  d_xp: a [B, T, 3H] buffer to overwrite; workspace: fp32, at least
    dr_gru_seq_bwd_workspace_bytes(B, T, H) bytes (allocated when None)."""
    B, T, H = _gru_dims(xp, U)
    xp, ld_xp = _gru_seq3(xp, B, T, 3 * H, "xp")
    U = _gru_dense(U, (H, 3 * H), "U")
    h0 = _gru_dense(h0, (B, H), "h0", aligned=True)
    att = _gru_dense(att, (B, T), "att")
    lengths = _gru_lengths(lengths, B)
    hs, ld_hs = _gru_seq3(hs, B, T, H, "hs")
    ld_dhs = H
    if d_hs is not None:
        d_hs, ld_dhs = _gru_seq3(d_hs, B, T, H, "d_hs")
    d_h_last = _gru_dense(d_h_last, (B, H), "d_h_last")
    dev = xp.device
    if d_xp is None:
        d_xp = torch.empty((B, T, 3 * H), dtype=torch.float32, device=dev)
    d_xp, ld_dxp = _gru_seq3(d_xp, B, T, 3 * H, "d_xp", may_copy=False)
    dU = torch.empty((H, 3 * H), dtype=torch.float32, device=dev)
    d_h0 = torch.empty((B, H), dtype=torch.float32, device=dev)
    d_att = torch.empty((B, T), dtype=torch.float32, device=dev) if att is not None else None
    if B == 0:
        return d_xp, dU.zero_(), d_h0, d_att
    need = lib().dr_gru_seq_bwd_workspace_bytes(B, T, H)
    if need < 0:
        _status(int(need), "dr_gru_seq_bwd_workspace_bytes")
    if workspace is None:
        workspace = torch.empty((max(need // 4, 4),), dtype=torch.float32, device=dev)
    elif workspace.numel() * workspace.element_size() < need:
        raise ValueError("gru_seq: the workspace holds %d bytes, dr_gru_seq_bwd_workspace_bytes asks for %d"
                         % (workspace.numel() * workspace.element_size(), need))
    st = lib().dr_gru_seq_bwd(ptr(xp), ld_xp, ptr(U), ptr(h0), ptr(lengths), ptr(att), ptr(hs), ld_hs, B, T, H, ptr(d_hs), ld_dhs,
                              ptr(d_h_last), ptr(d_xp), ld_dxp, ptr(dU), ptr(d_h0), ptr(d_att), ptr(workspace),
                              workspace.numel() * workspace.element_size(), stream_ptr())
    _status(st, "dr_gru_seq_bwd")
    return d_xp, dU, d_h0, d_att


def _seq_attn_dims(hs, q):
    if hs.dim() != 3 or q.dim() != 2 or q.dtype != torch.float32 or q.shape[0] != hs.shape[0] or q.shape[1] != hs.shape[2]:
        raise ValueError("seq_attn: hs [B, T, H] and q [B, H] fp32 expected, got %s and %s" % (tuple(hs.shape), tuple(q.shape)))
    B, T, H = (int(s) for s in hs.shape)
    _slab_width("seq_attn", H, "H", hi=128)
    if T < 1:
        raise ValueError("seq_attn: needs T >= 1 time steps, got %d" % T)
    return B, T, H


def seq_attn_fwd(hs, q, lengths=None):
    """a [B, T] of dr_seq_attn_fwd: the softmax over t < lengths[b] of <hs[b, t], q[b]>, 0 at masked steps (hs is not read there)."""
    B, T, H = _seq_attn_dims(hs, q)
    hs, ld_hs = _gru_seq3(hs, B, T, H, "hs")
    q = _gru_dense(q, (B, H), "q", aligned=True)
    lengths = _gru_lengths(lengths, B)
    a = torch.empty((B, T), dtype=torch.float32, device=hs.device)
    if B == 0:
        return a
    _status(lib().dr_seq_attn_fwd(ptr(hs), ld_hs, ptr(q), ptr(lengths), B, T, H, ptr(a), stream_ptr()), "dr_seq_attn_fwd")
    return a


def seq_attn_bwd(hs, q, lengths, a, d_a):
    """(d_hs [B, T, H], d_q [B, H]) of dr_seq_attn_bwd from d_a [B, T], with the forward's a."""
    B, T, H = _seq_attn_dims(hs, q)
    hs, ld_hs = _gru_seq3(hs, B, T, H, "hs")
    q = _gru_dense(q, (B, H), "q", aligned=True)
    lengths = _gru_lengths(lengths, B)
    a = _gru_dense(a, (B, T), "a")
    d_a = _gru_dense(d_a, (B, T), "d_a")
    d_hs = torch.empty((B, T, H), dtype=torch.float32, device=hs.device)
    d_q = torch.empty((B, H), dtype=torch.float32, device=hs.device)
    if B == 0:
        return d_hs, d_q
    _status(lib().dr_seq_attn_bwd(ptr(hs), ld_hs, ptr(q), ptr(lengths), ptr(a), ptr(d_a), B, T, H, ptr(d_hs), H, ptr(d_q),
                                      stream_ptr()), "dr_seq_attn_bwd")
    return d_hs, d_q


def din_concat_fwd(x, y, mode):
    x, y = _c(x, torch.float32), _c(y, torch.float32)
    B, D = x.shape
    if y.shape != (B, D) or int(mode) not in (0, 1, 2):
        raise ValueError("din_concat_fwd: x %s and y %s must be [B, D] alike, mode 0, 1 or 2 (got %r)" % (tuple(x.shape), tuple(y.shape), mode))
    n = (3 if mode else 2) * D
    out = torch.zeros((B, _pad4(n)), dtype=torch.float32, device=x.device)[:, :n]
    check(lib().dr_din_concat_fwd(ptr(x), ptr(y), B, D, int(mode), ptr(out), out.stride(0), stream_ptr()), "dr_din_concat_fwd")
    return out


def din_concat_bwd(x, y, mode, d_out):
    x, y = _c(x, torch.float32), _c(y, torch.float32)
    B, D = x.shape
    _check_ld(d_out, "din_concat_bwd: d_out")
    if y.shape != (B, D) or int(mode) not in (0, 1, 2) or tuple(d_out.shape) != (B, (3 if mode else 2) * D):
        raise ValueError("din_concat_bwd: x %s, y %s and d_out %s do not agree for mode %r" % (tuple(x.shape), tuple(y.shape), tuple(d_out.shape), mode))
    d_x, d_y = torch.empty_like(x), torch.empty_like(y)
    check(lib().dr_din_concat_bwd(ptr(x), ptr(y), B, D, int(mode), ptr(d_out), d_out.stride(0), ptr(d_x), ptr(d_y), stream_ptr()),
          "dr_din_concat_bwd")
    return d_x, d_y


# ---- element-wise pieces around the GEMM path (csrc/elementwise.hip) ------------------------------------------------------------
def act_fwd_(x, act):
    """in place: x = act(x) for act in {2: sigmoid, 3: tanh} (1 = relu also accepted); x [M, N] with unit column stride"""
    _check_ld(x, "act_fwd_: x")
    check(lib().dr_act_fwd(ptr(x), x.shape[0], x.shape[1], x.stride(0), int(act), stream_ptr()), "dr_act_fwd")
    return x


def act_bwd_(y, dy, act):
    """in place: dy *= act'(.) expressed through the saved output y"""
    assert y.shape == dy.shape
    _check_ld(y, "act_bwd_: y")
    _check_ld(dy, "act_bwd_: dy")
    check(lib().dr_act_bwd(ptr(y), y.stride(0), ptr(dy), dy.stride(0), y.shape[0], y.shape[1], int(act), stream_ptr()), "dr_act_bwd")
    return dy


def dropout_fwd(x, rate, seed):
    _check_ld(x, "dropout_fwd: x")
    M, N = x.shape
    y = torch.empty((M, _pad4(N)), dtype=torch.float32, device=x.device)[:, :N]
    mask = torch.empty(M * N, dtype=torch.uint8, device=x.device)
    check(lib().dr_dropout_fwd(ptr(x), x.stride(0), M, N, float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(y), y.stride(0), ptr(mask),
                               stream_ptr()), "dr_dropout_fwd")
    return y, mask


def dropout_bwd(dy, mask, rate):
    _check_ld(dy, "dropout_bwd: dy")
    M, N = dy.shape
    dx = torch.empty((M, _pad4(N)), dtype=torch.float32, device=dy.device)[:, :N]
    check(lib().dr_dropout_bwd(ptr(dy), dy.stride(0), ptr(mask), M, N, float(rate), ptr(dx), dx.stride(0), stream_ptr()),
          "dr_dropout_bwd")
    return dx


def reduce_sum(x, squared=False, alpha=1.0, out=None, accumulate=False):
    """out[0] (+)= alpha * sum(x) or alpha * sum(x^2) over a contiguous fp32 tensor (deterministic)."""
    x = _dense_arg(x, "reduce_sum: x")
    if out is None:
        out = torch.zeros(1, dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or out.numel() < 1:
        raise ValueError("reduce_sum: out must be an fp32 tensor of at least one element, got %s %s" % (out.dtype, tuple(out.shape)))
    ws = torch.empty(1024, dtype=torch.float32, device=x.device)
    check(lib().dr_reduce_sum(ptr(x), x.numel(), int(bool(squared)), float(alpha), int(bool(accumulate)), ptr(out), ptr(ws),
                              stream_ptr()), "dr_reduce_sum")
    return out


def copy_nt(src, dst):
    """dst = src as a streaming 16-byte nontemporal copy (dr_copy_nt): the measured HBM ceiling bench.py reports."""
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() * src.element_size() == dst.numel() * dst.element_size()
    check(lib().dr_copy_nt(ptr(src), ptr(dst), src.numel() * src.element_size(), stream_ptr()), "dr_copy_nt")
    return dst


CONFUSION_HIST_MAX_THRESHOLDS = 4096


def confusion_hist_workspace(n, num_thresholds, device="cuda"):
    """The scratch buffer dr_confusion_hist_update needs for up to n examples (the per-block partial histograms)."""
    nbytes = lib().dr_confusion_hist_workspace_bytes(int(n), int(num_thresholds))
    return torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=device)


def confusion_hist_update(pred, labels, thresholds, hist, weights=None, from_logits=False, workspace=None):
    """hist[label != 0][#{t : pred > thresholds[t]}] += weight over flat fp32 pred / labels (/ weights) of equal length
    (dr_confusion_hist_update).  thresholds: ascending fp32 [T] on the device; hist: fp64 [2, T + 1], accumulated into.  Enqueues on
    the current stream and returns hist; nothing here waits for the device."""
    pred, labels, thresholds = _c(pred, torch.float32), _c(labels, torch.float32), _c(thresholds, torch.float32)
    n, T = pred.numel(), thresholds.numel()
    if labels.numel() != n or (weights is not None and weights.numel() != n):
        raise ValueError("pred, labels and weights must hold the same number of elements")
    if hist.dtype != torch.float64 or not hist.is_contiguous() or hist.numel() != 2 * (T + 1):
        raise ValueError("hist must be a contiguous fp64 tensor of 2 * (T + 1) elements")
    if weights is not None:
        weights = _c(weights, torch.float32)
    if workspace is None or workspace.numel() * workspace.element_size() < lib().dr_confusion_hist_workspace_bytes(n, T):
        workspace = confusion_hist_workspace(n, T, pred.device)
    check(lib().dr_confusion_hist_update(ptr(pred), ptr(labels), ptr(weights), n, ptr(thresholds), T, int(bool(from_logits)),
                                         ptr(hist), ptr(workspace), stream_ptr()), "dr_confusion_hist_update")
    return hist


def clock_stamp(buf, index):
    """buf[index] (int64 device tensor) = the device wall clock (100 MHz ticks) when the current stream reaches this point
    (dr_clock_stamp: a one-thread kernel; measurement plumbing for bench.py's exposed-wait report)."""
    assert buf.dtype == torch.int64 and buf.is_contiguous() and 0 <= index < buf.numel()
    check(lib().dr_clock_stamp(buf.data_ptr() + 8 * int(index), stream_ptr()), "dr_clock_stamp")


# ---- multi-task learning (csrc/multitask.hip + the grouped entry points of csrc/dense.hip) -----------------------------------------
def _f32_2d(t, what):
    if t.dtype != torch.float32:
        raise TypeError("%s: expected float32, got %s" % (what, t.dtype))
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("%s: expected a row-major 2-D tensor with unit column stride" % what)
    return t


def linear_fwd_grouped(x, ld_x, x_gs, W, ld_w, w_gs, b, b_gs, M, K, N, G, act, y, ld_y, y_gs):
    """Grouped Dense forward over raw layouts: every tensor is the base of its G groups (see dr_linear_fwd_grouped)."""
    for t in (x, W, y) + ((b,) if b is not None else ()):
        if t.dtype != torch.float32:
            raise TypeError("linear_fwd_grouped: float32 tensors only")
    check(lib().dr_linear_fwd_grouped(ptr(x), ld_x, x_gs, ptr(W), ld_w, w_gs, ptr(b), b_gs, M, K, N, G, int(act), ptr(y), ld_y, y_gs,
                                      stream_ptr()), "dr_linear_fwd_grouped")
    return y


def linear_bwd_dx_grouped(dy, ld_dy, dy_gs, W, ld_w, w_gs, M, K, N, G, relu_src, ld_rs, rs_gs, accumulate, dx, ld_dx, dx_gs):
    for t in (dy, W, dx):
        if t.dtype != torch.float32:
            raise TypeError("linear_bwd_dx_grouped: float32 tensors only")
    check(lib().dr_linear_bwd_dx_grouped(ptr(dy), ld_dy, dy_gs, ptr(W), ld_w, w_gs, M, K, N, G, ptr(relu_src), ld_rs, rs_gs,
                                         int(bool(accumulate)), ptr(dx), ld_dx, dx_gs, stream_ptr()), "dr_linear_bwd_dx_grouped")
    return dx


def linear_bwd_dw_grouped_workspace(M, K, N, G, device):
    return torch.empty(max(1, lib().dr_linear_bwd_dw_grouped_workspace_bytes(int(M), int(K), int(N), int(G)) // 4),
                       dtype=torch.float32, device=device)


def linear_bwd_dw_grouped(x, ld_x, x_gs, dy, ld_dy, dy_gs, M, K, N, G, scale, dstW, ld_w, w_gs, dstb=None, b_gs=0, workspace=None):
    for t in (x, dy, dstW):
        if t.dtype != torch.float32:
            raise TypeError("linear_bwd_dw_grouped: float32 tensors only")
    check(lib().dr_linear_bwd_dw_grouped(ptr(x), ld_x, x_gs, ptr(dy), ld_dy, dy_gs, M, K, N, G, float(scale), ptr(dstW), ld_w, w_gs,
                                         ptr(dstb), b_gs, ptr(workspace), workspace.numel() * 4 if workspace is not None else 0,
                                         stream_ptr()), "dr_linear_bwd_dw_grouped")


def mmoe_gate_mix_fwd(h, logits, E, T, U):
    """h [B, >= E*U], logits [B, >= T*E] -> (p [B, T*E], out [B, T*U])."""
    _f32_2d(h, "h")
    _f32_2d(logits, "logits")
    B = h.shape[0]
    if logits.shape[0] != B or h.shape[1] < E * U or logits.shape[1] < T * E:
        raise ValueError("mmoe_gate_mix_fwd: h %s / logits %s do not hold E=%d, T=%d, U=%d" % (tuple(h.shape), tuple(logits.shape), E, T, U))
    p = torch.empty((B, T * E), dtype=torch.float32, device=h.device)
    out = torch.empty((B, T * U), dtype=torch.float32, device=h.device)
    check(lib().dr_mmoe_gate_mix_fwd(ptr(h), h.stride(0), ptr(logits), logits.stride(0), B, E, T, U, ptr(p), p.stride(0), ptr(out),
                                     out.stride(0), stream_ptr()), "dr_mmoe_gate_mix_fwd")
    return p, out


def mmoe_gate_mix_bwd(h, p, d_out, E, T, U, d_h=None, d_l=None):
    _f32_2d(h, "h")
    _f32_2d(p, "p")
    _f32_2d(d_out, "d_out")
    B = h.shape[0]
    if p.shape[0] != B or d_out.shape[0] != B or d_out.shape[1] < T * U or p.shape[1] < T * E:
        raise ValueError("mmoe_gate_mix_bwd: shapes do not match E=%d, T=%d, U=%d" % (E, T, U))
    if d_h is None:
        d_h = torch.empty((B, E * U), dtype=torch.float32, device=h.device)
    if d_l is None:
        d_l = torch.empty((B, T * E), dtype=torch.float32, device=h.device)
    check(lib().dr_mmoe_gate_mix_bwd(ptr(h), h.stride(0), ptr(p), p.stride(0), ptr(d_out), d_out.stride(0), B, E, T, U, ptr(d_h),
                                     d_h.stride(0), ptr(d_l), d_l.stride(0), stream_ptr()), "dr_mmoe_gate_mix_bwd")
    return d_h, d_l


def mse_fwd_bwd(pred, labels, want_grad=True):
    """pred [B, T], labels [B, T] -> (loss [T], d_pred [B, T] or None)."""
    _f32_2d(pred, "pred")
    _f32_2d(labels, "labels")
    if pred.shape != labels.shape:
        raise ValueError("mse_fwd_bwd: pred %s vs labels %s" % (tuple(pred.shape), tuple(labels.shape)))
    B, T = pred.shape
    loss = torch.empty(T, dtype=torch.float32, device=pred.device)
    d = torch.empty((B, T), dtype=torch.float32, device=pred.device) if want_grad else None
    nbytes = lib().dr_mse_workspace_bytes(T)
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=pred.device)
    check(lib().dr_mse_fwd_bwd(ptr(pred), pred.stride(0), ptr(labels), labels.stride(0), B, T, ptr(loss), ptr(d),
                               d.stride(0) if d is not None else 0, ptr(ws), nbytes, stream_ptr()), "dr_mse_fwd_bwd")
    return loss, d


def esmm_head_fwd(logits):
    """logits [B, 2] (cvr, ctr) -> p_cvr, p_ctr, p_ctcvr, each [B]."""
    _f32_2d(logits, "logits")
    if logits.shape[1] != 2:
        raise ValueError("esmm_head_fwd: logits must be [B, 2], got %s" % (tuple(logits.shape),))
    B = logits.shape[0]
    outs = torch.empty((3, B), dtype=torch.float32, device=logits.device)
    check(lib().dr_esmm_head_fwd(ptr(logits), logits.stride(0), B, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), stream_ptr()),
          "dr_esmm_head_fwd")
    return outs[0], outs[1], outs[2]


def esmm_head_bwd(p_cvr, p_ctr, d_cvr=None, d_ctr=None, d_ctcvr=None):
    B = p_cvr.shape[0]
    gs = []
    for g in (d_cvr, d_ctr, d_ctcvr):
        if g is not None:
            g = _c(g.reshape(-1), torch.float32)
            if g.numel() != B:
                raise ValueError("esmm_head_bwd: gradient of %d elements for a batch of %d" % (g.numel(), B))
        gs.append(g)
    d_logits = torch.empty((B, 2), dtype=torch.float32, device=p_cvr.device)
    check(lib().dr_esmm_head_bwd(ptr(_c(p_cvr, torch.float32)), ptr(_c(p_ctr, torch.float32)), ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), B,
                                 ptr(d_logits), d_logits.stride(0), stream_ptr()), "dr_esmm_head_bwd")
    return d_logits


def adam_step_2d(param, grad, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """Adam on a 2-D block whose rows may be strided (a column slice of a concatenated parameter); m / v contiguous."""
    if param.dim() == 1:
        param, grad, m, v = (t.reshape(1, -1) for t in (param, grad, m, v))
    for t in (param, grad, m, v):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError("adam_step_2d: 2-D float32 blocks with unit column stride")
    rows, cols = param.shape
    assert grad.shape == param.shape and m.shape == param.shape and v.shape == param.shape and m.stride(0) == v.stride(0)
    check(lib().dr_adam_step_2d(ptr(param), param.stride(0), ptr(grad), grad.stride(0), ptr(m), ptr(v), m.stride(0), rows, cols,
                                float(lr_t), float(beta1), float(beta2), float(eps), float(grad_scale), stream_ptr()),
          "dr_adam_step_2d")


def gather_cols(a, b, col_map, out):
    """out[:, j] = a[:, map[j]] if map[j] >= 0 else b[:, -map[j] - 1]; col_map int32 [N] on the device."""
    M, N = out.shape
    if col_map.dtype != torch.int32 or col_map.numel() != N:
        raise ValueError("gather_cols: col_map must be int32 [%d]" % N)
    _check_ld(a, "gather_cols: a")            # dr_gather_cols takes lda / ldb as they come
    _check_ld(b, "gather_cols: b")
    _check_ld(out, "gather_cols: out")
    check(lib().dr_gather_cols(ptr(a), a.stride(0) if a is not None else 0, ptr(b), b.stride(0) if b is not None else 0, ptr(col_map),
                               M, N, ptr(out), out.stride(0), stream_ptr()), "dr_gather_cols")
    return out


# ---- graph convolution (csrc/graph.hip) -----------------------------------------------------------------------------------------
def _ld4_f32(t):
    """[M, D] fp32 with unit column stride, a row pitch that is a multiple of 4 floats and a 16-byte aligned base (copied into such
    a buffer otherwise) -- the layout dr_csr_spmm takes."""
    assert t.dim() == 2 and t.dtype == torch.float32
    if t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0:
        return t
    M, D = t.shape
    buf = torch.empty((M, _pad4(D)), dtype=torch.float32, device=t.device)
    buf[:, :D].copy_(t)
    return buf[:, :D]


def empty_ld4(M, D, device, zero=False):
    buf = (torch.zeros if zero else torch.empty)((M, _pad4(D)), dtype=torch.float32, device=device)
    return buf[:, :D]


def csr_plan(row_ptr, n_rows, nnz):
    """the long-row plan of a CSR (int64 device buffer), built once per graph"""
    dev = row_ptr.device
    plan = torch.empty(max(1, lib().dr_csr_plan_bytes(int(nnz)) // 8), dtype=torch.int64, device=dev)
    ws = torch.empty(max(1, lib().dr_csr_plan_workspace_bytes(int(n_rows)) // 8), dtype=torch.int64, device=dev)
    check(lib().dr_csr_plan(ptr(row_ptr), int(n_rows), int(nnz), ptr(plan), plan.numel() * 8, ptr(ws), ws.numel() * 8, stream_ptr()),
          "dr_csr_plan")
    return plan


def csr_spmm_workspace(nnz, D, device):
    n = lib().dr_csr_spmm_workspace_bytes(int(nnz), int(D))
    return torch.empty(max(1, n // 4), dtype=torch.float32, device=device) if n > 0 else None


def csr_spmm(row_ptr, col, val, n_rows, nnz, X, plan, workspace=None, relu_src=None, accumulate=False, out=None):
    """out = (A @ X) [* (relu_src > 0)] [+ out]; A the CSR (row_ptr int64, col int32, val fp32)"""
    X = _ld4_f32(X)
    D = X.shape[1]
    if out is None:
        assert not accumulate
        out = empty_ld4(n_rows, D, X.device)
    assert out.shape == (n_rows, D)
    if relu_src is not None:
        relu_src = _ld4_f32(relu_src)
    need = lib().dr_csr_spmm_workspace_bytes(int(nnz), int(D))
    if need > 0 and (workspace is None or workspace.numel() * 4 < need):
        workspace = csr_spmm_workspace(nnz, D, X.device)
    check(lib().dr_csr_spmm(ptr(row_ptr), ptr(col), ptr(val), int(n_rows), int(nnz), ptr(X), X.stride(0), int(D), ptr(relu_src),
                            relu_src.stride(0) if relu_src is not None else 0, int(bool(accumulate)), ptr(out), out.stride(0),
                            ptr(plan), ptr(workspace), workspace.numel() * 4 if workspace is not None else 0, stream_ptr()),
          "dr_csr_spmm")
    return out


def csr_transpose(row_ptr, col, val, n_rows, n_cols, nnz):
    """(t_row_ptr, t_col, t_val): the CSR of A^T, source rows ascending inside every column"""
    dev = row_ptr.device
    t_row_ptr = torch.empty(n_cols + 1, dtype=torch.int64, device=dev)
    t_col = torch.empty(max(1, nnz), dtype=torch.int32, device=dev)[:nnz]
    t_val = torch.empty(max(1, nnz), dtype=torch.float32, device=dev)[:nnz]
    ws = torch.empty(max(1, lib().dr_csr_transpose_workspace_bytes(int(nnz), int(n_cols))), dtype=torch.uint8, device=dev)
    check(lib().dr_csr_transpose(ptr(row_ptr), ptr(col), ptr(val), int(n_rows), int(n_cols), int(nnz), ptr(t_row_ptr), ptr(t_col),
                                 ptr(t_val), ptr(ws), ws.numel(), stream_ptr()), "dr_csr_transpose")
    return t_row_ptr, t_col, t_val


def softmax_rows_fwd(x, out=None):
    _check_ld(x, "softmax_rows_fwd: x")
    B, C = x.shape
    if out is None:
        out = torch.empty((B, C), dtype=torch.float32, device=x.device)
    check(lib().dr_softmax_rows_fwd(ptr(x), x.stride(0), B, C, ptr(out), out.stride(0), stream_ptr()), "dr_softmax_rows_fwd")
    return out


def softmax_rows_bwd(y, dy, out=None):
    assert y.shape == dy.shape
    _check_ld(y, "softmax_rows_bwd: y")
    _check_ld(dy, "softmax_rows_bwd: dy")
    B, C = y.shape
    if out is None:
        out = torch.empty((B, C), dtype=torch.float32, device=y.device)
    check(lib().dr_softmax_rows_bwd(ptr(y), y.stride(0), ptr(dy), dy.stride(0), B, C, ptr(out), out.stride(0), stream_ptr()),
          "dr_softmax_rows_bwd")
    return out


def cce_prob_rows(p, labels, sample_weight=None, want_grad=True):
    """(row_loss [B], grad [B, C] or None) of Keras' categorical_crossentropy on probabilities, rows weighted by sample_weight"""
    _check_ld(p, "cce_prob_rows: p")
    _check_ld(labels, "cce_prob_rows: labels")
    if labels.shape != p.shape:
        raise ValueError("cce_prob_rows: p %s and labels %s differ in shape" % (tuple(p.shape), tuple(labels.shape)))
    B, C = p.shape
    sample_weight = _dense_arg(sample_weight, "cce_prob_rows: sample_weight", numel=B)
    row = torch.empty(B, dtype=torch.float32, device=p.device)
    grad = torch.empty((B, C), dtype=torch.float32, device=p.device) if want_grad else None
    check(lib().dr_cce_prob_rows(ptr(p), p.stride(0), ptr(labels), labels.stride(0), B, C, ptr(sample_weight), ptr(row), ptr(grad),
                                 grad.stride(0) if grad is not None else 0, stream_ptr()), "dr_cce_prob_rows")
    return row, grad


# ---- Transformer package (csrc/attention.hip) -----------------------------------------------------------------------------------------
def _attn_view(t, what):
    """[B, L, W] fp32 with unit column stride whose (b, l) rows are equally pitched: returns (tensor, B, L, W, pitch)"""
    if t.dtype != torch.float32 or t.dim() != 3:
        raise TypeError("%s must be a [B, L, H * dh] fp32 tensor" % what)
    B, L, W = t.shape
    if not (t.stride(2) == 1 and t.stride(1) >= W and t.stride(0) == L * t.stride(1)) and B * L > 0:
        t = t.contiguous()
    return t, B, L, W, (t.stride(1) if B * L > 0 else W)


def _attn_mask(key_mask, B, Lk):
    if key_mask is None:
        return None
    if key_mask.dtype == torch.bool:
        key_mask = key_mask.view(torch.uint8) if key_mask.is_contiguous() else key_mask.contiguous().view(torch.uint8)
    if key_mask.dtype != torch.uint8 or key_mask.shape != (B, Lk):
        raise TypeError("key_mask must be a [B, Lk] bool / uint8 tensor (1 = padded)")
    return key_mask.contiguous()


def attn_fwd(q, k, v, n_heads, key_mask=None, future=False, rate=0.0, seed=0, out=None):
    """(out [B, Lq, H * dh], stats [B * H * Lq, 2]) of dr_attn_fwd: softmax(q k^T / sqrt(dh) + mask) -> dropout -> . v per head, the
    heads being column blocks of the projected tensors.  Refused arguments raise with the status code in the message."""
    q, B, Lq, W, ld_q = _attn_view(q, "q")
    k, Bk, Lk, Wk, ld_k = _attn_view(k, "k")
    v, Bv, Lv, Wv, ld_v = _attn_view(v, "v")
    H = int(n_heads)
    if not (B == Bk == Bv and Lk == Lv and W == Wk == Wv and H > 0 and W % H == 0):
        raise ValueError("attention shapes do not agree: q %s k %s v %s heads %d" % (tuple(q.shape), tuple(k.shape), tuple(v.shape), H))
    key_mask = _attn_mask(key_mask, B, Lk)
    if out is None:
        out = torch.empty((B, Lq, _pad4(W)), dtype=torch.float32, device=q.device)[:, :, :W]
    stats = torch.empty((B * H * Lq, 2), dtype=torch.float32, device=q.device)
    check(lib().dr_attn_fwd(ptr(q), ld_q, ptr(k), ld_k, ptr(v), ld_v, ptr(key_mask), B, H, Lq, Lk, W // H, int(bool(future)),
                            float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out), out.stride(1), ptr(stats), stream_ptr()),
          "dr_attn_fwd")
    return out, stats


def attn_bwd(q, k, v, n_heads, d_out, stats, key_mask=None, future=False, rate=0.0, seed=0):
    """(dq, dk, dv) of dr_attn_bwd, in the layout of q, k, v (densely packed)"""
    q, B, Lq, W, ld_q = _attn_view(q, "q")
    k, _, Lk, _, ld_k = _attn_view(k, "k")
    v, _, _, _, ld_v = _attn_view(v, "v")
    d_out, _, _, _, ld_do = _attn_view(d_out, "d_out")
    H = int(n_heads)
    if d_out.shape != (B, Lq, W) or k.shape != (B, Lk, W) or v.shape != (B, Lk, W) or W % H:
        raise ValueError("attention backward shapes do not agree")
    key_mask = _attn_mask(key_mask, B, Lk)
    dev = q.device
    dq = torch.empty((B, Lq, _pad4(W)), dtype=torch.float32, device=dev)[:, :, :W]
    dk = torch.empty((B, Lk, _pad4(W)), dtype=torch.float32, device=dev)[:, :, :W]
    dv = torch.empty((B, Lk, _pad4(W)), dtype=torch.float32, device=dev)[:, :, :W]
    delta = torch.empty(max(1, B * H * Lq), dtype=torch.float32, device=dev)
    check(lib().dr_attn_bwd(ptr(q), ld_q, ptr(k), ld_k, ptr(v), ld_v, ptr(key_mask), ptr(d_out), ld_do, ptr(stats),
                            B, H, Lq, Lk, W // H, int(bool(future)), float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(dq), dq.stride(1),
                            ptr(dk), dk.stride(1), ptr(dv), dv.stride(1), ptr(delta), stream_ptr()), "dr_attn_bwd")
    return dq, dk, dv


def _rows_f32(t, what):
    if t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError("%s must be a [M, D] fp32 tensor" % what)
    if t.shape[0] == 0 or ((t.stride(1) == 1 or t.shape[1] == 1) and t.stride(0) >= t.shape[1] and t.shape[0] > 1):
        return t
    if t.shape[0] == 1 and (t.stride(1) == 1 or t.shape[1] == 1):     # one row has no pitch: name a legal one (no copy)
        return t.as_strided(t.shape, (t.shape[1], 1), t.storage_offset())
    return t.contiguous()


def add_layernorm_fwd(a, b, gamma, beta, eps=1e-8):
    """(y, stats [M, 2]) with y = gamma * (s - mean) / sqrt(var + eps) + beta over the last axis, s = a + b (b may be None)"""
    a = _rows_f32(a, "a")
    M, D = a.shape
    if b is not None:
        b = _rows_f32(b, "b")
        if b.shape != (M, D):
            raise ValueError("add_layernorm: the addends differ in shape")
    if gamma.shape != (D,) or beta.shape != (D,):
        raise ValueError("add_layernorm: gamma / beta must be [D]")
    y = torch.empty((M, D), dtype=torch.float32, device=a.device)
    stats = torch.empty((M, 2), dtype=torch.float32, device=a.device)
    check(lib().dr_add_layernorm_fwd(ptr(a), a.stride(0), ptr(b), b.stride(0) if b is not None else 0, ptr(_c(gamma, torch.float32)),
                                     ptr(_c(beta, torch.float32)), M, D, float(eps), ptr(y), y.stride(0), ptr(stats), stream_ptr()),
          "dr_add_layernorm_fwd")
    return y, stats


def add_layernorm_bwd(a, b, gamma, stats, dy):
    """(d_s, d_gamma, d_beta); d_s is the gradient of both addends"""
    a = _rows_f32(a, "a")
    dy = _rows_f32(dy, "dy")
    M, D = a.shape
    if b is not None:
        b = _rows_f32(b, "b")
    dev = a.device
    d_s = torch.empty((M, D), dtype=torch.float32, device=dev)
    d_gamma = torch.empty(D, dtype=torch.float32, device=dev)
    d_beta = torch.empty(D, dtype=torch.float32, device=dev)
    nb = lib().dr_add_layernorm_bwd_workspace_bytes(M, D)
    ws = torch.empty(max(1, nb // 4), dtype=torch.float32, device=dev)
    check(lib().dr_add_layernorm_bwd(ptr(a), a.stride(0), ptr(b), b.stride(0) if b is not None else 0, ptr(_c(gamma, torch.float32)),
                                     ptr(stats), ptr(dy), dy.stride(0), M, D, ptr(d_s), d_s.stride(0), ptr(d_gamma), ptr(d_beta), ptr(ws),
                                     ws.numel() * 4, stream_ptr()), "dr_add_layernorm_bwd")
    return d_s, d_gamma, d_beta


def token_embedding_fwd(ids, table, pos=None, rate=0.0, seed=0):
    """out [B, L, D] = dropout(table[ids] * sqrt(D) + pos[l]); ids [B, L] int64, pos [L, D] or None"""
    if ids.dtype != torch.int64 or ids.dim() != 2:
        raise TypeError("ids must be a [B, L] int64 tensor")
    ids = ids.contiguous()
    B, L = ids.shape
    table = _c(table, torch.float32)
    V, D = table.shape
    if pos is not None:
        pos = _c(pos, torch.float32)
        if pos.shape != (L, D):
            raise ValueError("the position table must be [L, D]")
    out = torch.empty((B, L, D), dtype=torch.float32, device=table.device)
    if B * L > 0:
        check(lib().dr_token_embedding_fwd(ptr(ids), B * L, L, ptr(table), V, D, ptr(pos), float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           ptr(out), D, stream_ptr()), "dr_token_embedding_fwd")
    return out


def token_embedding_bwd(ids, d_out, d_table, rate=0.0, seed=0):
    """d_table [V, D] += sqrt(D) * (the kept d_out rows / (1 - rate)) summed per id in ascending position order (deterministic)"""
    B, L = ids.shape
    V, D = d_table.shape
    assert d_table.is_contiguous() and d_table.dtype == torch.float32
    d_out = _c(d_out.reshape(B * L, D), torch.float32)
    if B * L == 0:
        return d_table
    sorted_ids, order = torch.sort(ids.reshape(-1), stable=True)     # plumbing: the order of the row owners' sums
    check(lib().dr_token_embedding_bwd(ptr(sorted_ids), ptr(order), B * L, V, D, ptr(d_out), d_out.stride(0), float(rate),
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(d_table), stream_ptr()), "dr_token_embedding_bwd")
    return d_table


# ---- DIN (csrc/din.hip) ----------------------------------------------------------------------------------------------------------------
def dice_fwd(x, alpha, eps=1e-8):
    """y [M, N] of dr_dice_fwd: the reference's Dice over the rows of x (a view with a row pitch is read in place)"""
    x = _rows_f32(x, "x")
    M, N = x.shape
    if N < 1 or alpha.shape != (N,):
        raise ValueError("dice: alpha must be [N] with N >= 1 (x is %s)" % (tuple(x.shape),))
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    check(lib().dr_dice_fwd(ptr(x), x.stride(0) if M else N, ptr(_c(alpha, torch.float32)), M, N, float(eps), ptr(y), N, stream_ptr()),
          "dr_dice_fwd")
    return y


def dice_bwd(x, alpha, dy, eps=1e-8):
    """(dx [M, N], dalpha [N]) of dr_dice_bwd; dalpha is summed over the rows in a fixed order"""
    x = _rows_f32(x, "x")
    dy = _rows_f32(dy, "dy")
    M, N = x.shape
    if N < 1 or alpha.shape != (N,) or dy.shape != (M, N):
        raise ValueError("dice backward: shapes do not agree")
    dev = x.device
    dx = torch.empty((M, N), dtype=torch.float32, device=dev)
    dalpha = torch.empty(N, dtype=torch.float32, device=dev)
    nb = lib().dr_dice_bwd_workspace_bytes(M, N)
    ws = torch.empty(max(1, nb // 4), dtype=torch.float32, device=dev)
    check(lib().dr_dice_bwd(ptr(x), x.stride(0) if M else N, ptr(_c(alpha, torch.float32)), ptr(dy), dy.stride(0) if M else N, M, N,
                            float(eps), ptr(dx), N, ptr(dalpha), ptr(ws), ws.numel() * 4, stream_ptr()), "dr_dice_bwd")
    return dx, dalpha


DIN_POOL_DOMAIN = "D % 4 == 0, 4 <= D <= 128, 1 <= U <= 128, T >= 1"


def _din_pool_args(query, keys, mask, W, b, w_out, b_out, mode, act, alpha):
    if query.dtype != torch.float32 or keys.dtype != torch.float32 or query.dim() != 2 or keys.dim() != 3:
        raise TypeError("din_pool: query must be [B, D] and keys [B, T, D], fp32")
    B, T, D = keys.shape
    mode, act = int(mode), int(act)
    if mode not in (0, 1, 2) or act not in (0, 1, 2, 3, 4):
        raise ValueError("din_pool: mode must be 0 (none) / 1 (q - k) / 2 (q * k) and act 0..4 (linear, relu, sigmoid, tanh, Dice)")
    n_in = 2 if mode == 0 else 3
    U = W.shape[1] if W.dim() == 2 else -1
    if query.shape != (B, D) or W.dim() != 2 or W.shape[0] != n_in * D:
        raise ValueError("din_pool: query %s, keys %s and W %s do not agree (W is [%d * D, U] for mode %d)"
                         % (tuple(query.shape), tuple(keys.shape), tuple(W.shape), n_in, mode))
    if not (D % 4 == 0 and 4 <= D <= 128 and 1 <= U <= 128 and T >= 1):
        raise ValueError("din_pool: D = %d, U = %d, T = %d is outside the kernels' domain (%s); there is no composed fallback"
                         % (D, U, T, DIN_POOL_DOMAIN))
    if w_out.numel() != U or (b is not None and b.shape != (U,)) or (b_out is not None and b_out.numel() != 1):
        raise ValueError("din_pool: b must be [U], w_out [U] or [U, 1], b_out [1]")
    if act == 4 and (alpha is None or alpha.shape != (U,)):
        raise ValueError("din_pool: Dice (act 4) needs alpha [U]")
    query = _rows_f32(query, "query")
    if B * T > 0 and not (keys.stride(2) == 1 and keys.stride(1) >= D and keys.stride(1) % 4 == 0 and keys.stride(0) == T * keys.stride(1)
                          and keys.data_ptr() % 16 == 0):
        keys = keys.contiguous()
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.contiguous().view(torch.uint8)
        if mask.dtype != torch.uint8 or mask.shape != (B, T):
            raise TypeError("din_pool: mask must be a [B, T] bool / uint8 tensor (nonzero = valid)")
        mask = mask.contiguous()
    f32 = torch.float32
    return (query, keys, mask, _c(W, f32), None if b is None else _c(b, f32), _c(w_out, f32).reshape(-1), None if b_out is None else _c(b_out, f32),
            None if alpha is None else _c(alpha, f32), B, T, D, U, mode, act)


def din_pool_fwd(query, keys, mask, W, b, w_out, b_out, mode, act, alpha=None, eps=1e-8):
    """(out [B, D], scores [B, T]) of dr_din_pool_fwd: DIN's activation unit scored for every key against the example's query and the
    keys summed with those scores; masked keys (mask == 0) are never read.  A shape outside the domain raises ValueError."""
    query, keys, mask, W, b, w_out, b_out, alpha, B, T, D, U, mode, act = _din_pool_args(query, keys, mask, W, b, w_out, b_out, mode, act, alpha)
    out = torch.empty((B, D), dtype=torch.float32, device=keys.device)
    scores = torch.empty((B, T), dtype=torch.float32, device=keys.device)
    check(lib().dr_din_pool_fwd(ptr(query), query.stride(0) if B else D, ptr(keys), keys.stride(1) if B else D, ptr(mask), ptr(W), ptr(b),
                                ptr(w_out), ptr(b_out), ptr(alpha), B, T, D, U, mode, act, float(eps), ptr(out), D, ptr(scores),
                                stream_ptr()), "dr_din_pool_fwd")
    return out, scores


def din_pool_bwd(query, keys, mask, W, b, w_out, b_out, mode, act, d_out, d_scores=None, alpha=None, eps=1e-8):
    """(d_query, d_keys, dW, db, d_w_out, d_b_out, dalpha) of dr_din_pool_bwd; db / d_b_out / dalpha are None where the forward had no
    such parameter.  Every reduction over examples runs in a fixed order."""
    query, keys, mask, W, b, w_out, b_out, alpha, B, T, D, U, mode, act = _din_pool_args(query, keys, mask, W, b, w_out, b_out, mode, act, alpha)
    dev = keys.device
    d_out = _c(d_out, torch.float32)
    if d_out.shape != (B, D) or (d_scores is not None and d_scores.shape != (B, T)):
        raise ValueError("din_pool backward: d_out must be [B, D] and d_scores [B, T]")
    if d_scores is not None:
        d_scores = _c(d_scores, torch.float32)
    d_query = torch.empty((B, D), dtype=torch.float32, device=dev)
    d_keys = torch.empty((B, T, D), dtype=torch.float32, device=dev)
    dW = torch.empty_like(W)
    db = torch.empty(U, dtype=torch.float32, device=dev) if b is not None else None
    d_w_out = torch.empty(U, dtype=torch.float32, device=dev)
    d_b_out = torch.empty(1, dtype=torch.float32, device=dev) if b_out is not None else None
    dalpha = torch.empty(U, dtype=torch.float32, device=dev) if act == 4 else None
    nb = lib().dr_din_pool_bwd_workspace_bytes(B, T, D, U)
    ws = torch.empty(max(4, nb // 4), dtype=torch.float32, device=dev)
    check(lib().dr_din_pool_bwd(ptr(query), query.stride(0) if B else D, ptr(keys), keys.stride(1) if B else D, ptr(mask), ptr(W), ptr(b),
                                ptr(w_out), ptr(b_out), ptr(alpha), ptr(d_out), D, ptr(d_scores), B, T, D, U, mode, act, float(eps),
                                ptr(d_query), D, ptr(d_keys), D, ptr(dW), ptr(db), ptr(d_w_out), ptr(d_b_out), ptr(dalpha), ptr(ws),
                                ws.numel() * 4, stream_ptr()), "dr_din_pool_bwd")
    return d_query, d_keys, dW, db, d_w_out, d_b_out, dalpha


# ---- FFM: the field-aware interaction (csrc/ffm.hip) -------------------------------------------------------------------------------------
def _ffm_dims(F, k):
    """validates the domain of dr_ffm_*; returns (F, k) as ints"""
    F, k = int(F), _slab_width("ffm", k, "the latent size k", hi=128)
    if not 2 <= F <= 64:
        raise ValueError("ffm: needs 2 <= F <= 64 fields, got F = %d" % F)
    if F * k > 256:
        raise ValueError("ffm: a table row holds one k-vector per field and F * k <= 256 is the slab's limit, got F = %d, k = %d, "
                         "F * k = %d" % (F, k, F * k))
    return F, k


def ffm_row_width(F, k):
    """F * k: the width of an FFM table row (one k-vector towards every field); an example's gathered rows are F of them"""
    F, k = _ffm_dims(F, k)
    return F * k


def ffm_fwd(rows, F, k):
    """inter [B] of dr_ffm_fwd: sum over the pairs j < i of <A[i, j, :], A[j, i, :]> with A [F, F, k] the example's gathered rows.  rows:
    [B, F, F, k] or [B, F, F * k] contiguous, or [B, F * F * k] with any row stride that is a multiple of 4 (the slab's concat, in place)."""
    F, k = _ffm_dims(F, k)
    rows, ld = _rows_arg("ffm", rows, F * F * k, "rows (F * F * k columns)", ((F, F, k), (F, F * k)))
    B = rows.shape[0]
    inter = torch.empty((B,), dtype=torch.float32, device=rows.device)
    if B == 0:
        return inter
    _status(lib().dr_ffm_fwd(ptr(rows), ld, B, F, k, ptr(inter), stream_ptr()), "dr_ffm_fwd")
    return inter


def ffm_bwd(rows, F, k, d_inter, d_rows=None):
    """d_rows [B, F * F * k] of dr_ffm_bwd: d_rows[b, i, j, :] = d_inter[b] * A[b, j, i, :], the diagonal blocks +0.0.  d_rows: a buffer to
    overwrite (only its first F * F * k columns are written)."""
    F, k = _ffm_dims(F, k)
    rows, ld = _rows_arg("ffm", rows, F * F * k, "rows (F * F * k columns)", ((F, F, k), (F, F * k)))
    B = rows.shape[0]
    d_inter = _vec_arg("ffm", d_inter, B, "d_inter")
    d_rows, ld_d = _rows_arg("ffm", d_rows, F * F * k, "d_rows (F * F * k columns)", ((F, F, k), (F, F * k)), rows=B, device=rows.device)
    if B == 0:
        return d_rows
    _status(lib().dr_ffm_bwd(ptr(rows), ld, ptr(d_inter), B, F, k, ptr(d_rows), ld_d, stream_ptr()), "dr_ffm_bwd")
    return d_rows


def _ffm_gather_args(ids, row_base, table, F, k):
    F, k = _ffm_dims(F, k)
    ids = _ids_arg("ffm", ids, "ids", F)
    row_base = _vec_arg("ffm", row_base, F, "row_base", torch.int64)
    _table_arg("ffm", table, "table", F * k)
    return F, k, ids, row_base


def ffm_gather_fwd(ids, row_base, table, F, k, lin_w=None, lin_bias=None):
    """(inter [B], first_order [B] | None) of dr_ffm_gather_fwd for single-valued fields: the rows table[row_base[f] + ids[b, f]] are read
    from the table and written nowhere; an id < 0 is a row of zeros.  first_order = lin_bias + sum_f lin_w[row] when lin_w is given."""
    F, k, ids, row_base = _ffm_gather_args(ids, row_base, table, F, k)
    B = ids.shape[0]
    inter = torch.empty((B,), dtype=torch.float32, device=ids.device)
    first = torch.empty((B,), dtype=torch.float32, device=ids.device) if lin_w is not None else None
    if B == 0:
        return inter, first
    _status(lib().dr_ffm_gather_fwd(ptr(ids), B, F, ptr(row_base), ptr(table), k, ptr(lin_w), ptr(lin_bias), ptr(inter), ptr(first),
                                        stream_ptr()), "dr_ffm_gather_fwd")
    return inter, first


def ffm_gather_bwd(ids, row_base, table, F, k, d_inter, d_rows=None):
    """d_rows [B, F * F * k] of dr_ffm_gather_bwd, from the table and d_inter: what emb_pool_bwd takes as d_concat with D = F * k."""
    F, k, ids, row_base = _ffm_gather_args(ids, row_base, table, F, k)
    B = ids.shape[0]
    d_inter = _vec_arg("ffm", d_inter, B, "d_inter")
    d_rows, ld_d = _rows_arg("ffm", d_rows, F * F * k, "d_rows (F * F * k columns)", ((F, F, k), (F, F * k)), rows=B, device=ids.device)
    if B == 0:
        return d_rows
    _status(lib().dr_ffm_gather_bwd(ptr(ids), B, F, ptr(row_base), ptr(table), k, ptr(d_inter), ptr(d_rows), ld_d, stream_ptr()),
                "dr_ffm_gather_bwd")
    return d_rows


# ---- NFM: the Bi-Interaction pooling (csrc/bi_interaction.hip) ----------------------------------------------------------------------------
def _bi_dims(F, D):
    """validates the domain of dr_bi_interact_*; returns (F, D) as ints"""
    F, D = int(F), _slab_width("bi_interaction", D, "the row width D")
    if not 1 <= F <= 1024:
        raise ValueError("bi_interaction: needs 1 <= F <= 1024 fields, got F = %d" % F)
    return F, D


def _bi_gather_args(ids, row_base, table, F, D, lin_w=None, lin_bias=None):
    F, D = _bi_dims(F, D)
    ids = _ids_arg("bi_interaction", ids, "ids", F)
    row_base = _vec_arg("bi_interaction", row_base, F, "row_base", torch.int64)
    _table_arg("bi_interaction", table, "table", D)
    lin_w = _dense_arg(lin_w, "bi_interaction: lin_w", numel=table.shape[0])
    lin_bias = _dense_arg(lin_bias, "bi_interaction: lin_bias", numel=1)
    return F, D, ids, row_base, lin_w, lin_bias


def bi_interaction_fwd(rows, F, D, out=None):
    """out [B, D] of dr_bi_interact_fwd: 0.5 ((sum_f e_f)^2 - sum_f e_f^2) over the F rows of every example.  rows: [B, F, D] contiguous,
    or [B, F * D] with any row stride that is a multiple of 4 (the slab's concat, in place).  out: a buffer to overwrite."""
    F, D = _bi_dims(F, D)
    rows, ld = _rows_arg("bi_interaction", rows, F * D, "rows", ((F, D),))
    B = rows.shape[0]
    out, ld_out = _rows_arg("bi_interaction", out, D, "out", rows=B, device=rows.device)
    if B == 0:
        return out
    _status(lib().dr_bi_interact_fwd(ptr(rows), ld, B, F, D, ptr(out), ld_out, stream_ptr()), "dr_bi_interact_fwd")
    return out


def bi_interaction_bwd(rows, F, D, d_out, d_rows=None):
    """d_rows [B, F * D] of dr_bi_interact_bwd: d_rows[b, f, :] = d_out[b, :] * (sum_g e_g - e_f).  d_rows: a buffer to overwrite (only
    its first F * D columns are written)."""
    F, D = _bi_dims(F, D)
    rows, ld = _rows_arg("bi_interaction", rows, F * D, "rows", ((F, D),))
    B = rows.shape[0]
    d_out, ld_do = _rows_arg("bi_interaction", d_out, D, "d_out", rows=B, device=rows.device)
    d_rows, ld_d = _rows_arg("bi_interaction", d_rows, F * D, "d_rows", ((F, D),), rows=B, device=rows.device)
    if B == 0:
        return d_rows
    _status(lib().dr_bi_interact_bwd(ptr(rows), ld, ptr(d_out), ld_do, B, F, D, ptr(d_rows), ld_d, stream_ptr()), "dr_bi_interact_bwd")
    return d_rows


def bi_interaction_gather_fwd(ids, row_base, table, F, D, lin_w=None, lin_bias=None, out=None):
    """(out [B, D], first_order [B] | None) of dr_bi_interact_gather_fwd for single-valued fields: the rows table[row_base[f] + ids[b, f]]
    are read from the table and written nowhere; an id < 0 is a row of zeros.  first_order = lin_bias + sum_f lin_w[row] when lin_w is
    given."""
    F, D, ids, row_base, lin_w, lin_bias = _bi_gather_args(ids, row_base, table, F, D, lin_w, lin_bias)
    B = ids.shape[0]
    out, ld_out = _rows_arg("bi_interaction", out, D, "out", rows=B, device=ids.device)
    first = torch.empty((B,), dtype=torch.float32, device=ids.device) if lin_w is not None else None
    if B == 0:
        return out, first
    _status(lib().dr_bi_interact_gather_fwd(ptr(ids), B, F, ptr(row_base), ptr(table), D, ptr(lin_w), ptr(lin_bias), ptr(out), ld_out,
                                                ptr(first), stream_ptr()), "dr_bi_interact_gather_fwd")
    return out, first


def bi_interaction_gather_bwd(ids, row_base, table, F, D, d_out, d_rows=None):
    """d_rows [B, F * D] of dr_bi_interact_gather_bwd, from the table and d_out: what emb_pool_bwd takes as d_concat."""
    F, D, ids, row_base, _, _ = _bi_gather_args(ids, row_base, table, F, D)
    B = ids.shape[0]
    d_out, ld_do = _rows_arg("bi_interaction", d_out, D, "d_out", rows=B, device=ids.device)
    d_rows, ld_d = _rows_arg("bi_interaction", d_rows, F * D, "d_rows", ((F, D),), rows=B, device=ids.device)
    if B == 0:
        return d_rows
    _status(lib().dr_bi_interact_gather_bwd(ptr(ids), B, F, ptr(row_base), ptr(table), D, ptr(d_out), ld_do, ptr(d_rows), ld_d,
                                                stream_ptr()), "dr_bi_interact_gather_bwd")
    return d_rows


# ---- LS-PLM: the bag sum and the mixture head (csrc/lsplm.hip) ----------------------------------------------------------------------------
def _lsplm_dims(F, m):
    """validates the domain of dr_lsplm_*; returns (F, m) as ints"""
    F, m = int(F), int(m)
    if m % 2 != 0 or not 2 <= m <= 128:
        raise ValueError("lsplm: the number of regions m must be even and in [2, 128], got %d" % m)
    if not 1 <= F <= 1024:
        raise ValueError("lsplm: needs 1 <= F <= 1024 fields, got F = %d" % F)
    return F, m


def _lsplm_pool_args(ids, F, col_start, row_base, table, m, bias):
    """validates the inputs of the pooling; returns (F, m, ids, C, col_start, row_base, bias)"""
    F, m = _lsplm_dims(F, m)
    ids = _ids_arg("lsplm", ids, "ids")
    C = int(ids.shape[1])
    if col_start is None:
        if C != F:
            raise ValueError("lsplm: without col_start every field is single-valued and ids must be [B, %d], got %s" % (F, tuple(ids.shape)))
    else:
        col_start = _vec_arg("lsplm", col_start, F + 1, "col_start", torch.int32)
        if C < F:
            raise ValueError("lsplm: ids [B, C] needs C >= F = %d columns, got C = %d" % (F, C))
    row_base = _vec_arg("lsplm", row_base, F, "row_base", torch.int64)
    _table_arg("lsplm", table, "table", 2 * m)
    bias = _dense_arg(bias, "lsplm: bias", numel=2 * m)
    if bias is None:
        raise ValueError("lsplm: bias [%d] is required" % (2 * m))
    return F, m, ids, C, col_start, row_base, bias


def lsplm_fwd(ids, F, col_start, row_base, table, m, bias, want_z=True, z=None):
    """(p [B], q [B], z [B, 2 m] | None) of dr_lsplm_fwd: z = bias + the sum over the fields of the mean-pooled rows (K3's pooling; ids
    [B, C] with col_start int32 [F + 1], or col_start None and ids [B, F]), p = sum_i softmax(z[:m])_i sigmoid(z[m + i]) and q = 1 - p
    computed without the subtraction.  z: a buffer to overwrite."""
    F, m, ids, C, col_start, row_base, bias = _lsplm_pool_args(ids, F, col_start, row_base, table, m, bias)
    B = ids.shape[0]
    ld_z = 0
    if want_z or z is not None:
        z, ld_z = _rows_arg("lsplm", z, 2 * m, "z", rows=B, device=ids.device)
    p = torch.empty((B,), dtype=torch.float32, device=ids.device)
    q = torch.empty((B,), dtype=torch.float32, device=ids.device)
    if B == 0:
        return p, q, z
    _status(lib().dr_lsplm_fwd(ptr(ids), B, F, C, ptr(col_start), ptr(row_base), ptr(table), m, ptr(bias), ptr(z), ld_z, ptr(p), ptr(q),
                               stream_ptr()), "dr_lsplm_fwd")
    return p, q, z


def lsplm_bwd(z, F, m, d_p, d_z=None, d_rows=None):
    """(d_z [B, 2 m], d_rows [B, F * 2 m]) of dr_lsplm_bwd from the z that lsplm_fwd stored: d_z = d_p [pi (sg - p) ; pi sg (1 - sg)],
    d_rows = F copies of it (emb_pool_bwd's d_concat with D = 2 m).  d_z, d_rows: buffers to overwrite."""
    F, m = _lsplm_dims(F, m)
    ld_z = _row_pitch("lsplm", z, 2 * m, "z")
    B = z.shape[0]
    d_p = _vec_arg("lsplm", d_p, B, "d_p", none_ok=True)
    if d_p is None:
        raise ValueError("lsplm: d_p [%d] is required" % B)
    d_z, ld_dz = _rows_arg("lsplm", d_z, 2 * m, "d_z", rows=B, device=z.device)
    d_rows, ld_d = _rows_arg("lsplm", d_rows, F * 2 * m, "d_rows", rows=B, device=z.device)
    if B == 0:
        return d_z, d_rows
    _status(lib().dr_lsplm_bwd(ptr(z), ld_z, ptr(d_p), B, F, m, ptr(d_z), ld_dz, ptr(d_rows), ld_d, stream_ptr()), "dr_lsplm_bwd")
    return d_z, d_rows


def lsplm_loss_fwd(ids, F, col_start, row_base, table, m, bias, labels, sample_weight=None, row_scale=1.0, d_z=None, d_rows=None):
    """(p, q, loss [B], d_z [B, 2 m], d_rows [B, F * 2 m]) of dr_lsplm_loss_fwd, the one-pass training form: loss = -wt (y log p +
    (1 - y) log q) and the gradient of row_scale * loss with respect to z, bit for bit what lsplm_fwd + lsplm_bwd give for d_p =
    (row_scale * wt) * (-y / p + (1 - y) / q)."""
    F, m, ids, C, col_start, row_base, bias = _lsplm_pool_args(ids, F, col_start, row_base, table, m, bias)
    B = ids.shape[0]
    labels = _vec_arg("lsplm", labels, B, "labels", none_ok=True)
    if labels is None:
        raise ValueError("lsplm: labels [%d] are required" % B)
    sample_weight = _vec_arg("lsplm", sample_weight, B, "sample_weight", none_ok=True)
    d_z, ld_dz = _rows_arg("lsplm", d_z, 2 * m, "d_z", rows=B, device=ids.device)
    d_rows, ld_d = _rows_arg("lsplm", d_rows, F * 2 * m, "d_rows", rows=B, device=ids.device)
    p, q, loss = (torch.empty((B,), dtype=torch.float32, device=ids.device) for _ in range(3))
    if B == 0:
        return p, q, loss, d_z, d_rows
    _status(lib().dr_lsplm_loss_fwd(ptr(ids), B, F, C, ptr(col_start), ptr(row_base), ptr(table), m, ptr(bias), ptr(labels),
                                    ptr(sample_weight), float(row_scale), ptr(p), ptr(q), ptr(loss), ptr(d_z), ld_dz, ptr(d_rows), ld_d,
                                    stream_ptr()), "dr_lsplm_loss_fwd")
    return p, q, loss, d_z, d_rows


def lsplm_bias_grad(d_z, m):
    """d_bias [2 m] of dr_lsplm_bias_grad: the column sum of d_z [B, 2 m] in a fixed order (two stages, no float atomics)"""
    _, m = _lsplm_dims(1, m)
    ld = _row_pitch("lsplm", d_z, 2 * m, "d_z")
    B = d_z.shape[0]
    d_bias = torch.empty((2 * m,), dtype=torch.float32, device=d_z.device)
    nbytes = int(lib().dr_lsplm_bias_grad_workspace_bytes(B, m))
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=d_z.device)
    _status(lib().dr_lsplm_bias_grad(ptr(d_z), ld, B, m, ptr(d_bias), ptr(ws), ws.numel() * 4, stream_ptr()), "dr_lsplm_bias_grad")
    return d_bias


# ---- skip-gram with negative sampling (csrc/sgns.hip) and the samplers around it (csrc/sampling.hip) -----------------------------------
SGNS_SKIP_EQUAL = 1     # DR_SGNS_SKIP_EQUAL


def _sgns_args(in_table, out_table, centers, contexts, negatives):
    """validates the domain of dr_sgns_*; returns (B, K, D, centers, contexts, negatives) with the ids contiguous"""
    _table_arg("sgns", in_table, "in_table")
    _table_arg("sgns", out_table, "out_table")
    D = in_table.shape[1]
    if out_table.shape[1] != D:
        raise ValueError("sgns: in_table and out_table must share D, got %d and %d" % (D, out_table.shape[1]))
    _slab_width("sgns", D)
    if centers.dtype != torch.int64 or centers.dim() != 1:
        raise ValueError("sgns: centers must be int64 [B], got %s %s" % (centers.dtype, tuple(centers.shape)))
    B = centers.shape[0]
    if contexts.dtype != torch.int64 or tuple(contexts.shape) != (B,):
        raise ValueError("sgns: contexts must be int64 [%d], got %s %s" % (B, contexts.dtype, tuple(contexts.shape)))
    if negatives is None:
        negatives = torch.empty((B, 0), dtype=torch.int64, device=centers.device)
    negatives = _ids_arg("sgns", negatives, "negatives", rows=B)
    K = negatives.shape[1]
    if K > 63:
        raise ValueError("sgns: at most 63 negatives per example (ids [B, 1 + K] go through K4, F <= 64), got K = %d" % K)
    return B, K, D, centers.contiguous(), contexts.contiguous(), negatives


def sgns_fwd(in_table, out_table, centers, contexts, negatives=None, sample_weight=None, skip_equal=True, want_scores=False,
             row_scale=None, d_center=None, d_ctx=None):
    """(loss_rows [B], coeff [B, 1 + K], scores [B, 1 + K] | None, d_center | None, d_ctx | None) of dr_sgns_fwd.  centers, contexts
    int64 [B], negatives int64 [B, K] (None: K = 0); an id < 0 skips its slot (centers / contexts: the example), and with skip_equal a
    negative equal to the example's context is skipped too.  row_scale (a number) asks for the one-pass training form: d_center [B, D]
    and d_ctx [B, (1 + K) D], the gradient rows of row_scale * loss_rows, are written in the same pass (into the buffers given, else
    fresh ones) -- what K4 takes as d_concat for ids [B, 1] and [B, 1 + K]."""
    B, K, D, centers, contexts, negatives = _sgns_args(in_table, out_table, centers, contexts, negatives)
    dev = centers.device
    sample_weight = _vec_arg("sgns", sample_weight, B, "sample_weight", none_ok=True)
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    coeff = torch.empty((B, 1 + K), dtype=torch.float32, device=dev)
    scores = torch.empty((B, 1 + K), dtype=torch.float32, device=dev) if want_scores else None
    ld_dc = ld_dx = 0
    if row_scale is not None:
        d_center, ld_dc = _rows_arg("sgns", d_center, D, "d_center", rows=B, device=dev)
        d_ctx, ld_dx = _rows_arg("sgns", d_ctx, (1 + K) * D, "d_ctx", ((1 + K, D),), rows=B, device=dev)
    elif d_center is not None or d_ctx is not None:
        raise ValueError("sgns: gradient buffers are written only with a row_scale")
    if B == 0:
        return loss, coeff, scores, d_center, d_ctx
    _status(lib().dr_sgns_fwd(ptr(in_table), ptr(out_table), D, ptr(centers), ptr(contexts), ptr(negatives) if K else None, B, K,
                              ptr(sample_weight), SGNS_SKIP_EQUAL if skip_equal else 0, float(row_scale or 0.0), ptr(loss), ptr(coeff),
                              ptr(scores), ptr(d_center), ld_dc, ptr(d_ctx), ld_dx, stream_ptr()), "dr_sgns_fwd")
    return loss, coeff, scores, d_center, d_ctx


def sgns_bwd(in_table, out_table, centers, contexts, negatives, coeff, d_loss, skip_equal=True, d_center=None, d_ctx=None):
    """(d_center [B, D], d_ctx [B, (1 + K) D]) of dr_sgns_bwd: the gradient rows of sum_b d_loss[b] * loss_rows[b] from the forward's
    coeff, the rows gathered again.  Same ids and skip_equal as the forward."""
    B, K, D, centers, contexts, negatives = _sgns_args(in_table, out_table, centers, contexts, negatives)
    if coeff.dtype != torch.float32 or tuple(coeff.shape) != (B, 1 + K):
        raise ValueError("sgns: coeff must be fp32 [%d, %d], got %s %s" % (B, 1 + K, coeff.dtype, tuple(coeff.shape)))
    coeff = coeff.contiguous()
    d_loss = _vec_arg("sgns", d_loss, B, "d_loss")
    d_center, ld_dc = _rows_arg("sgns", d_center, D, "d_center", rows=B, device=centers.device)
    d_ctx, ld_dx = _rows_arg("sgns", d_ctx, (1 + K) * D, "d_ctx", ((1 + K, D),), rows=B, device=centers.device)
    if B == 0:
        return d_center, d_ctx
    _status(lib().dr_sgns_bwd(ptr(in_table), ptr(out_table), D, ptr(centers), ptr(contexts), ptr(negatives) if K else None, B, K,
                              SGNS_SKIP_EQUAL if skip_equal else 0, ptr(coeff), ptr(d_loss), ptr(d_center), ld_dc, ptr(d_ctx), ld_dx,
                              stream_ptr()), "dr_sgns_bwd")
    return d_center, d_ctx


def alias_table(weights):
    """(prob float32 [V], alias int32 [V]) of Vose's alias method for the distribution weights / sum(weights), NumPy on the host, built
    once: a draw picks a slot uniformly and returns it with probability prob[slot], else alias[slot].  word2vec's negative distribution
    is alias_table(counts ** 0.75).  An entry of weight 0 has prob 0 and is nobody's alias: it is never drawn."""
    import numpy as np
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    V = w.size
    if V < 1 or V >= 2 ** 31:
        raise ValueError("alias_table: needs 1 <= V < 2^31 weights, got %d" % V)
    if not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
        raise ValueError("alias_table: weights must be finite, >= 0 and not all zero")
    p = w * (V / w.sum())
    prob = np.ones(V, dtype=np.float64)
    alias = np.arange(V, dtype=np.int32)
    small = np.flatnonzero(p < 1.0).tolist()
    large = np.flatnonzero(p >= 1.0).tolist()
    while small and large:
        s, l = small.pop(), large.pop()
        prob[s], alias[s] = p[s], l
        p[l] = (p[l] + p[s]) - 1.0
        (small if p[l] < 1.0 else large).append(l)
    return prob.astype(np.float32), alias            # what is left on either list has p = 1 up to rounding: prob 1, its own alias


def alias_sample(prob, alias, n, seed, offset=0, out=None):
    """n int64 draws of dr_alias_sample from the table (prob fp32 [V], alias int32 [V], on the device): element i depends on
    (seed, offset + i) alone, so consecutive calls with a running offset continue one stream."""
    if prob.dtype != torch.float32 or alias.dtype != torch.int32 or prob.dim() != 1 or prob.shape != alias.shape or prob.numel() < 1:
        raise ValueError("alias_sample: prob fp32 [V] and alias int32 [V], V >= 1, got %s %s and %s %s"
                         % (prob.dtype, tuple(prob.shape), alias.dtype, tuple(alias.shape)))
    n = int(n)
    if n < 0 or int(offset) < 0:
        raise ValueError("alias_sample: n and offset must be >= 0")
    prob, alias = prob.contiguous(), alias.contiguous()
    if out is None:
        out = torch.empty((n,), dtype=torch.int64, device=prob.device)
    elif out.dtype != torch.int64 or out.numel() != n or not out.is_contiguous():
        raise ValueError("alias_sample: out must be contiguous int64 with %d elements" % n)
    if n == 0:
        return out
    _status(lib().dr_alias_sample(ptr(prob), ptr(alias), prob.numel(), n, int(seed) & (2 ** 64 - 1), int(offset), ptr(out), stream_ptr()),
            "dr_alias_sample")
    return out


def random_walk(row_ptr, col, n_rows, starts, length, seed):
    """walks int64 [W, length] of dr_random_walk over the CSR graph (row_ptr int64 [n_rows + 1], col int32): uniform next neighbours from
    starts [W]; a walk that reaches a node without neighbours, or starts outside [0, n_rows), continues as -1."""
    n_rows, L = int(n_rows), int(length)
    if row_ptr.dtype != torch.int64 or row_ptr.dim() != 1 or row_ptr.numel() != n_rows + 1 or col.dtype != torch.int32 or col.dim() != 1:
        raise ValueError("random_walk: row_ptr int64 [n_rows + 1] and col int32 [nnz], got %s %s and %s %s"
                         % (row_ptr.dtype, tuple(row_ptr.shape), col.dtype, tuple(col.shape)))
    if starts.dtype != torch.int64 or starts.dim() != 1:
        raise ValueError("random_walk: starts must be int64 [W], got %s %s" % (starts.dtype, tuple(starts.shape)))
    if L < 1:
        raise ValueError("random_walk: a walk has at least its start, got length %d" % L)
    row_ptr, col, starts = row_ptr.contiguous(), col.contiguous(), starts.contiguous()
    W = starts.numel()
    walks = torch.empty((W, L), dtype=torch.int64, device=starts.device)
    if W == 0:
        return walks
    _status(lib().dr_random_walk(ptr(row_ptr), ptr(col) if col.numel() else None, n_rows, ptr(starts), W, L, int(seed) & (2 ** 64 - 1),
                                 ptr(walks), stream_ptr()), "dr_random_walk")
    return walks


def random_walk_weighted(row_ptr, col, cum, n_rows, starts, length, seed):
    """walks int64 [W, length] of dr_random_walk_weighted: random_walk with the next neighbour drawn in proportion to integer edge
    weights, given as cum int64 [nnz], their inclusive prefix sums over the whole col array.  Every row's total must stay below 2^32:
    the caller checks that once per graph (the kernel cannot)."""
    n_rows, L = int(n_rows), int(length)
    if row_ptr.dtype != torch.int64 or row_ptr.dim() != 1 or row_ptr.numel() != n_rows + 1 or col.dtype != torch.int32 or col.dim() != 1:
        raise ValueError("random_walk_weighted: row_ptr int64 [n_rows + 1] and col int32 [nnz], got %s %s and %s %s"
                         % (row_ptr.dtype, tuple(row_ptr.shape), col.dtype, tuple(col.shape)))
    if cum.dtype != torch.int64 or cum.shape != col.shape:
        raise ValueError("random_walk_weighted: cum must be int64 [nnz = %d], got %s %s" % (col.numel(), cum.dtype, tuple(cum.shape)))
    if starts.dtype != torch.int64 or starts.dim() != 1:
        raise ValueError("random_walk_weighted: starts must be int64 [W], got %s %s" % (starts.dtype, tuple(starts.shape)))
    if L < 1:
        raise ValueError("random_walk_weighted: a walk has at least its start, got length %d" % L)
    row_ptr, col, cum, starts = row_ptr.contiguous(), col.contiguous(), cum.contiguous(), starts.contiguous()
    W = starts.numel()
    walks = torch.empty((W, L), dtype=torch.int64, device=starts.device)
    if W == 0:
        return walks
    some = col.numel() > 0
    _status(lib().dr_random_walk_weighted(ptr(row_ptr), ptr(col) if some else None, ptr(cum) if some else None, n_rows, ptr(starts), W, L,
                                          int(seed) & (2 ** 64 - 1), ptr(walks), stream_ptr()), "dr_random_walk_weighted")
    return walks


# ---- skip-gram with side information (csrc/eges.hip) ----------------------------------------------------------------------------------------
def _eges_side_args(side_table, row_base, side_ids, att, att_ids):
    """validates the gather side of dr_eges_*; returns (B, S, D, row_base, side_ids, att, ld_att, att_ids), ids contiguous"""
    _table_arg("eges", side_table, "side_table")
    D = _slab_width("eges", side_table.shape[1])
    side_ids = _ids_arg("eges", side_ids, "side_ids")
    B, S = side_ids.shape
    if not 1 <= S <= 16:
        raise ValueError("eges: 1 <= S <= 16 fields, got %d" % S)
    _one_device("eges", "side_ids", side_ids.device, side_table=side_table, att=att, att_ids=att_ids if att is not None else None)
    if row_base.dtype != torch.int64 or tuple(row_base.shape) != (S,) or row_base.device != side_ids.device:
        raise ValueError("eges: row_base must be int64 [%d] on the ids' device, got %s %s" % (S, row_base.dtype, tuple(row_base.shape)))
    ld_att = 0
    if att is not None:
        if att.dtype != torch.float32 or att.dim() != 2 or att.shape[1] < S or att.stride(1) != 1 or (att.shape[0] > 1 and att.stride(0) < S):
            raise ValueError("eges: att must be fp32 [R_att, >= %d] with unit column stride, got %s %s" % (S, att.dtype, tuple(att.shape)))
        if att_ids is None or att_ids.dtype != torch.int64 or tuple(att_ids.shape) != (B,):
            raise ValueError("eges: att needs att_ids int64 [%d]" % B)
        ld_att = att.stride(0) if att.shape[0] > 1 else att.shape[1]
        att_ids = att_ids.contiguous()
    else:
        att_ids = None
    return B, S, D, row_base.contiguous(), side_ids, att, ld_att, att_ids


def _eges_slot_args(out_table, contexts, negatives, B, D):
    """validates the slot side of dr_eges_fwd / _bwd; returns (P, K, contexts [B, P], negatives [B, K]) contiguous"""
    _table_arg("eges", out_table, "out_table", D)
    if contexts.dtype == torch.int64 and contexts.dim() == 1:
        contexts = contexts.reshape(-1, 1)
    contexts = _ids_arg("eges", contexts, "contexts", rows=B)
    P = contexts.shape[1]
    if not 1 <= P <= 4:
        raise ValueError("eges: 1 <= P <= 4 positives per example, got %d" % P)
    if negatives is None:
        negatives = torch.empty((B, 0), dtype=torch.int64, device=contexts.device)
    negatives = _ids_arg("eges", negatives, "negatives", rows=B)
    K = negatives.shape[1]
    if P + K > 64:
        raise ValueError("eges: at most 64 slots per example (ids [B, P + K] go through K4, F <= 64), got P + K = %d" % (P + K))
    return P, K, contexts, negatives


def _eges_grad_buffers(B, S, J, D, d_side, d_att, d_ctx, device):
    """(d_side [B, S D], its pitch, d_att [B, pad4(S)], its width, d_ctx [B, J D], its pitch): the caller's buffers, checked, or fresh"""
    ld_da = _pad4(S)
    if d_att is None:
        d_att = torch.empty((B, ld_da), dtype=torch.float32, device=device)
    if d_att.dtype != torch.float32 or tuple(d_att.shape) != (B, ld_da) or not d_att.is_contiguous():
        raise ValueError("eges: d_att must be contiguous fp32 [%d, %d] (S rounded up to a multiple of 4), got %s %s"
                         % (B, ld_da, d_att.dtype, tuple(d_att.shape)))
    d_side, ld_ds = _rows_arg("eges", d_side, S * D, "d_side", rows=B, device=device)
    d_ctx, ld_dx = _rows_arg("eges", d_ctx, J * D, "d_ctx", rows=B, device=device)
    return d_side, ld_ds, d_att, ld_da, d_ctx, ld_dx


def eges_fwd(side_table, row_base, side_ids, att, att_ids, out_table, contexts, negatives=None, sample_weight=None, skip_equal=True,
             want_scores=False, row_scale=None, d_side=None, d_att=None, d_ctx=None):
    """(loss_rows [B], coeff [B, P + K], alpha [B, S], scores | None, d_side | None, d_att | None, d_ctx | None) of dr_eges_fwd: SGNS
    whose centre is the softmax(att[att_ids[b], :S])-weighted sum of the rows side_table[row_base[s] + side_ids[b, s]] of the fields
    that are present (side_ids >= 0); att None or att_ids[b] < 0: their plain average.  contexts int64 [B, P] (or [B]) are the
    positives, negatives int64 [B, K].  row_scale (a number) asks for the one-pass training form: d_side [B, S D], d_att [B, pad4(S)]
    and d_ctx [B, (P + K) D], the gradient rows of row_scale * loss_rows, written in the same pass -- what K4 takes as d_concat for
    the ids (side_ids with row_base), att_ids [B, 1] and [contexts | negatives]."""
    B, S, D, row_base, side_ids, att, ld_att, att_ids = _eges_side_args(side_table, row_base, side_ids, att, att_ids)
    P, K, contexts, negatives = _eges_slot_args(out_table, contexts, negatives, B, D)
    dev = side_ids.device
    _one_device("eges", "side_ids", dev, out_table=out_table, contexts=contexts, negatives=negatives, sample_weight=sample_weight,
                d_side=d_side, d_att=d_att, d_ctx=d_ctx)
    sample_weight = _vec_arg("eges", sample_weight, B, "sample_weight", none_ok=True)
    J = P + K
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    coeff = torch.empty((B, J), dtype=torch.float32, device=dev)
    alpha = torch.empty((B, S), dtype=torch.float32, device=dev)
    scores = torch.empty((B, J), dtype=torch.float32, device=dev) if want_scores else None
    ld_ds = ld_da = ld_dx = 0
    if row_scale is not None:
        d_side, ld_ds, d_att, ld_da, d_ctx, ld_dx = _eges_grad_buffers(B, S, J, D, d_side, d_att, d_ctx, dev)
    elif d_side is not None or d_att is not None or d_ctx is not None:
        raise ValueError("eges: gradient buffers are written only with a row_scale")
    if B == 0:
        return loss, coeff, alpha, scores, d_side, d_att, d_ctx
    _status(lib().dr_eges_fwd(ptr(side_table), D, ptr(row_base), ptr(side_ids), S, ptr(att), ld_att, ptr(att_ids), ptr(out_table),
                              ptr(contexts), P, ptr(negatives) if K else None, K, B, ptr(sample_weight),
                              SGNS_SKIP_EQUAL if skip_equal else 0, float(row_scale or 0.0), ptr(loss), ptr(coeff), ptr(alpha),
                              ptr(scores), ptr(d_side), ld_ds, ptr(d_att), ld_da, ptr(d_ctx), ld_dx, stream_ptr()), "dr_eges_fwd")
    return loss, coeff, alpha, scores, d_side, d_att, d_ctx


def eges_bwd(side_table, row_base, side_ids, att, att_ids, out_table, contexts, negatives, coeff, alpha, d_loss, skip_equal=True,
             d_side=None, d_att=None, d_ctx=None):
    """(d_side [B, S D], d_att [B, pad4(S)], d_ctx [B, (P + K) D]) of dr_eges_bwd: the gradient rows of sum_b d_loss[b] * loss_rows[b]
    from the forward's coeff and alpha, the rows gathered again.  Same ids, att / att_ids and skip_equal as the forward."""
    B, S, D, row_base, side_ids, att, _, att_ids = _eges_side_args(side_table, row_base, side_ids, att, att_ids)
    P, K, contexts, negatives = _eges_slot_args(out_table, contexts, negatives, B, D)
    _one_device("eges", "side_ids", side_ids.device, out_table=out_table, contexts=contexts, negatives=negatives, coeff=coeff, alpha=alpha,
                d_loss=d_loss, d_side=d_side, d_att=d_att, d_ctx=d_ctx)
    J = P + K
    if coeff.dtype != torch.float32 or tuple(coeff.shape) != (B, J):
        raise ValueError("eges: coeff must be fp32 [%d, %d], got %s %s" % (B, J, coeff.dtype, tuple(coeff.shape)))
    if alpha.dtype != torch.float32 or tuple(alpha.shape) != (B, S):
        raise ValueError("eges: alpha must be fp32 [%d, %d], got %s %s" % (B, S, alpha.dtype, tuple(alpha.shape)))
    coeff, alpha = coeff.contiguous(), alpha.contiguous()
    d_loss = _vec_arg("eges", d_loss, B, "d_loss")
    d_side, ld_ds, d_att, ld_da, d_ctx, ld_dx = _eges_grad_buffers(B, S, J, D, d_side, d_att, d_ctx, side_ids.device)
    if B == 0:
        return d_side, d_att, d_ctx
    _status(lib().dr_eges_bwd(ptr(side_table), D, ptr(row_base), ptr(side_ids), S, ptr(att), ptr(att_ids), ptr(out_table), ptr(contexts),
                              P, ptr(negatives) if K else None, K, B, SGNS_SKIP_EQUAL if skip_equal else 0, ptr(coeff), ptr(alpha),
                              ptr(d_loss), ptr(d_side), ld_ds, ptr(d_att), ld_da, ptr(d_ctx), ld_dx, stream_ptr()), "dr_eges_bwd")
    return d_side, d_att, d_ctx


def eges_embed(side_table, row_base, side_ids, att=None, att_ids=None, out=None):
    """out [n, D] of dr_eges_embed: the aggregated vector of every row of side_ids [n, S] alone; a row with no field present is +0.0"""
    n, S, D, row_base, side_ids, att, ld_att, att_ids = _eges_side_args(side_table, row_base, side_ids, att, att_ids)
    _one_device("eges", "side_ids", side_ids.device, out=out)
    out, ld_out = _rows_arg("eges", out, D, "out", rows=n, device=side_ids.device)
    if n == 0:
        return out
    _status(lib().dr_eges_embed(ptr(side_table), D, ptr(row_base), ptr(side_ids), S, ptr(att), ld_att, ptr(att_ids), n, ptr(out), ld_out,
                                stream_ptr()), "dr_eges_embed")
    return out


# ---- sampled graph blocks: GraphSAGE / PinSage (csrc/neighbor_sample.hip) ----------------------------------------------------------------
SAMPLE_LONG_ROW = 512      # DR_SAMPLE_LONG_ROW: a row with more edges is selected by a whole block (radix select), a shorter one by a wave
SAMPLE_MAX_FANOUT = 64     # the largest fanout of dr_neighbor_sample / dr_block_csr and the largest T of dr_walk_neighbors
WALK_MAX_VISITS = 1024     # dr_walk_neighbors: R (L - 1) at most


def _fanout_arg(family, what, fanout):
    fanout = int(fanout)
    if not 1 <= fanout <= SAMPLE_MAX_FANOUT:
        raise ValueError("%s: %s must be in [1, %d], got %d" % (family, what, SAMPLE_MAX_FANOUT, fanout))
    return fanout


def neighbor_sample(row_ptr, col, n_rows, nodes, fanout, seed):
    """(nbr int64 [n, fanout], cnt int32 [n]) of dr_neighbor_sample over the CSR graph (row_ptr int64 [n_rows + 1], col int32 [nnz]):
    up to `fanout` neighbours of every node of nodes int64 [n], uniformly without replacement, in CSR order, -1 to the end of the row.
    A node outside [0, n_rows) (-1 is the padding of a node list) has none.  The sample of a node depends on (seed, node) alone."""
    n_rows = int(n_rows)
    fanout = _fanout_arg("neighbor_sample", "fanout", fanout)
    row_ptr = _dense_arg(row_ptr, "neighbor_sample: row_ptr", torch.int64, shape=(n_rows + 1,))
    if col.dim() != 1:
        raise ValueError("neighbor_sample: col must be int32 [nnz], got %s %s" % (col.dtype, tuple(col.shape)))
    col = _dense_arg(col, "neighbor_sample: col", torch.int32)
    if nodes.dim() != 1:
        raise ValueError("neighbor_sample: nodes must be int64 [n], got %s %s" % (nodes.dtype, tuple(nodes.shape)))
    nodes = _dense_arg(nodes, "neighbor_sample: nodes", torch.int64)
    _one_device("neighbor_sample", "the call's first tensor", row_ptr.device, col=col, nodes=nodes)
    n = nodes.numel()
    nbr = torch.empty((n, fanout), dtype=torch.int64, device=nodes.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=nodes.device)
    if n == 0:
        return nbr, cnt
    _status(lib().dr_neighbor_sample(ptr(row_ptr), ptr(col) if col.numel() else None, n_rows, ptr(nodes), n, fanout,
                                     int(seed) & (2 ** 64 - 1), ptr(nbr), ptr(cnt), stream_ptr()), "dr_neighbor_sample")
    return nbr, cnt


def walk_neighbors(walks, num_neighbors):
    """(nbr int64 [n, T], weight fp32 [n, T], cnt int32 [n]) of dr_walk_neighbors: walks int64 [n, R, L] holds R walks of L nodes from
    each of n starts (random_walk over the starts repeated R times, viewed [n, R, L]); the T = num_neighbors most visited ids of each
    start, by (visits descending, id ascending), with their visit counts as weights; -1 / 0 to the end of a row."""
    T = _fanout_arg("walk_neighbors", "num_neighbors", num_neighbors)
    if walks.dim() != 3:
        raise ValueError("walk_neighbors: walks must be int64 [n, R, L], got %s %s" % (walks.dtype, tuple(walks.shape)))
    walks = _dense_arg(walks, "walk_neighbors: walks", torch.int64)
    n, R, L = walks.shape
    if R < 1 or L < 1 or R * (L - 1) > WALK_MAX_VISITS:
        raise ValueError("walk_neighbors: walks [n, R, L] needs R >= 1, L >= 1 and R (L - 1) <= %d, got R = %d, L = %d" % (WALK_MAX_VISITS, R, L))
    nbr = torch.empty((n, T), dtype=torch.int64, device=walks.device)
    weight = torch.empty((n, T), dtype=torch.float32, device=walks.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=walks.device)
    if n == 0:
        return nbr, weight, cnt
    _status(lib().dr_walk_neighbors(ptr(walks), n, R, L, T, ptr(nbr), ptr(weight), ptr(cnt), stream_ptr()), "dr_walk_neighbors")
    return nbr, weight, cnt


def frontier_build(dst, nbr, id_bound=0):
    """(src int64 [n_dst + m], counts int64 [2] on the device, local int32 like nbr) of dr_frontier_build: dst int64 [n_dst] is a node
    list (valid ids first, -1 padding after them), nbr int64 (any shape, m elements, -1 = none) the neighbours sampled for it.
    src = dst's valid prefix, then the ids of nbr that dst does not hold in ascending order, then -1; counts = (valid dst entries, valid
    src entries); local = where each nbr entry sits in src (-1 for none).  id_bound > 0 promises ids < id_bound (fewer sort passes).
    Nothing is read back: src is the next layer's dst."""
    if dst.dim() != 1:
        raise ValueError("frontier_build: dst must be int64 [n_dst], got %s %s" % (dst.dtype, tuple(dst.shape)))
    dst = _dense_arg(dst, "frontier_build: dst", torch.int64)
    nbr = _dense_arg(nbr, "frontier_build: nbr", torch.int64)
    _one_device("frontier_build", "the call's first tensor", dst.device, nbr=nbr)
    n_dst, m = dst.numel(), nbr.numel()
    if n_dst + m >= 2 ** 31:
        raise ValueError("frontier_build: dst and nbr together must stay below 2^31 entries, got %d" % (n_dst + m))
    dev = dst.device
    src = torch.empty((n_dst + m,), dtype=torch.int64, device=dev)
    counts = torch.zeros((2,), dtype=torch.int64, device=dev)
    local = torch.empty(nbr.shape, dtype=torch.int32, device=dev)
    if n_dst + m == 0:
        return src, counts, local
    ws = torch.empty(max(1, lib().dr_frontier_workspace_bytes(n_dst, m)), dtype=torch.uint8, device=dev)
    _status(lib().dr_frontier_build(ptr(dst) if n_dst else None, n_dst, ptr(nbr) if m else None, m, int(id_bound), ptr(src), ptr(counts),
                                    ptr(local) if m else None, ptr(ws), ws.numel(), stream_ptr()), "dr_frontier_build")
    return src, counts, local


def block_csr(cnt, local, weight=None, add_self=False, n_valid=None):
    """(row_ptr int64 [n_dst + 1], col int32, val fp32, both [n_dst (fanout + add_self)]) of dr_block_csr: the CSR of a sampled block
    from cnt int32 [n_dst] and local int32 [n_dst, fanout] (frontier_build's), rows normalised to sum 1 (the mean; with weight fp32
    [n_dst, fanout] the weighted mean; add_self puts the row's own index first at weight 1).  n_valid: a one-element int64 device tensor,
    the number of rows that are not padding (rows beyond it are empty); None: all.  Only the first row_ptr[n_dst] entries of col / val
    are written."""
    if local.dim() != 2:
        raise ValueError("block_csr: local must be int32 [n_dst, fanout], got %s %s" % (local.dtype, tuple(local.shape)))
    n_dst, fanout = local.shape
    fanout = _fanout_arg("block_csr", "fanout (local.shape[1])", fanout)
    local = _dense_arg(local, "block_csr: local", torch.int32)
    cnt = _dense_arg(cnt, "block_csr: cnt", torch.int32, shape=(n_dst,))
    weight = _dense_arg(weight, "block_csr: weight", torch.float32, shape=(n_dst, fanout))
    n_valid = _dense_arg(n_valid, "block_csr: n_valid", torch.int64, numel=1)
    dev = local.device
    _one_device("block_csr", "the call's first tensor", dev, cnt=cnt, weight=weight, n_valid=n_valid)
    extra = 1 if add_self else 0
    row_ptr = torch.zeros((n_dst + 1,), dtype=torch.int64, device=dev)
    col = torch.empty((max(1, n_dst * (fanout + extra)),), dtype=torch.int32, device=dev)
    val = torch.empty((max(1, n_dst * (fanout + extra)),), dtype=torch.float32, device=dev)
    if n_dst == 0:
        return row_ptr, col[:0], val[:0]
    ws = torch.empty(max(1, lib().dr_block_csr_workspace_bytes(n_dst)), dtype=torch.uint8, device=dev)
    _status(lib().dr_block_csr(ptr(cnt), ptr(local), ptr(weight), n_dst, fanout, extra, ptr(n_valid), ptr(row_ptr), ptr(col), ptr(val),
                               ptr(ws), ws.numel(), stream_ptr()), "dr_block_csr")
    return row_ptr, col, val


# ---- sampled softmax (csrc/sampled_softmax.hip): YoutubeNet's training loss ------------------------------------------------------------
SAMPLED_SOFTMAX_TILE = 64           # DR_SAMPLED_SOFTMAX_TILE: rows / columns of a tile
SAMPLED_SOFTMAX_COL_GROUP = 128     # DR_SAMPLED_SOFTMAX_COL_GROUP: a column segment has at least this many columns ...
SAMPLED_SOFTMAX_MAX_GROUPS = 8      # DR_SAMPLED_SOFTMAX_MAX_GROUPS: ... and there are at most this many
SAMPLED_SOFTMAX_SPLIT_TILES = 128   # DR_SAMPLED_SOFTMAX_SPLIT_TILES: up to this many row tiles every segment has a block of its own
SAMPLED_SOFTMAX_ROW_CHUNK = 128     # DR_SAMPLED_SOFTMAX_ROW_CHUNK: a d_sampled partial covers at least this many rows ...
SAMPLED_SOFTMAX_MAX_CHUNKS = 64     # DR_SAMPLED_SOFTMAX_MAX_CHUNKS: ... and there are at most this many


def sampled_softmax_col_groups(B, S, D):
    """blocks per row tile of the row-owning kernels (1, or the number of column segments): dr_sampled_softmax_col_groups"""
    n = lib().dr_sampled_softmax_col_groups(int(B), int(S), int(D))
    if n < 0:
        _status(n, "dr_sampled_softmax_col_groups")
    return n


def sampled_softmax_row_chunks(B, S, D):
    """number of d_sampled partials of the column-owning sweep: dr_sampled_softmax_row_chunks"""
    n = lib().dr_sampled_softmax_row_chunks(int(B), int(S), int(D))
    if n < 0:
        _status(n, "dr_sampled_softmax_row_chunks")
    return n


def sampled_softmax_workspace_bytes(B, S, D):
    """dr_sampled_softmax_workspace_bytes: host arithmetic, no device"""
    n = lib().dr_sampled_softmax_workspace_bytes(int(B), int(S), int(D))
    if n < 0:
        _status(n, "dr_sampled_softmax_workspace_bytes")
    return n


def sampled_softmax_workspace(B, S, D, device):
    return torch.empty(max(16, sampled_softmax_workspace_bytes(B, S, D)), dtype=torch.uint8, device=device)


def _ssm_args(u, table, labels, sampled, log_q_true, log_q_sampled, sample_weight):
    """validates the domain of dr_sampled_softmax_*; returns (B, S, V, D, ld_u, labels, sampled, log_q_true, log_q_sampled, sample_weight)"""
    _table_arg("sampled_softmax", table, "table")
    V, D = table.shape
    _slab_width("sampled_softmax", D)
    if not 1 <= V < 2 ** 31:
        raise ValueError("sampled_softmax: needs 1 <= V < 2^31 classes, got %d" % V)
    ld_u = _row_pitch("sampled_softmax", u, D, "u")
    B = u.shape[0]
    labels = _vec_arg("sampled_softmax", labels, B, "labels", torch.int64)
    if sampled.dtype != torch.int64 or sampled.dim() != 1:
        raise ValueError("sampled_softmax: sampled must be int64 [S], got %s %s" % (sampled.dtype, tuple(sampled.shape)))
    S = sampled.shape[0]
    if not 1 <= S < 2 ** 31:
        raise ValueError("sampled_softmax: needs 1 <= S < 2^31 sampled classes, got %d" % S)
    _one_device("sampled_softmax", "the table", table.device, u=u, labels=labels, sampled=sampled, log_q_true=log_q_true,
                log_q_sampled=log_q_sampled, sample_weight=sample_weight)
    return (B, S, V, D, ld_u, labels, sampled.contiguous(), _vec_arg("sampled_softmax", log_q_true, B, "log_q_true", none_ok=True),
            _vec_arg("sampled_softmax", log_q_sampled, S, "log_q_sampled", none_ok=True),
            _vec_arg("sampled_softmax", sample_weight, B, "sample_weight", none_ok=True))


def sampled_softmax_fwd(u, table, labels, sampled, log_q_true=None, log_q_sampled=None, sample_weight=None, remove_accidental_hits=True,
                        want_scores=False, workspace=None):
    """(true_logit [B], row_lse [B], row_loss [B], scores [B, S] | None) of dr_sampled_softmax_fwd: tf.nn.sampled_softmax_loss with
    num_true = 1 and no bias.  u fp32 [B, D], possibly a view with a row pitch (a multiple of 4); table contiguous fp32 [V, D]; labels
    int64 [B] (< 0: a padding row, loss 0); sampled int64 [S] shared by the batch (< 0: the column is left out).  Labels and sampled
    ids must be < V: not checked on the device.  want_scores is for tests and diagnosis: the only [B, S] tensor of the family."""
    B, S, V, D, ld_u, labels, sampled, log_q_true, log_q_sampled, sample_weight = _ssm_args(u, table, labels, sampled, log_q_true,
                                                                                             log_q_sampled, sample_weight)
    dev = table.device
    true_logit = torch.empty((B,), dtype=torch.float32, device=dev)
    row_lse = torch.empty((B,), dtype=torch.float32, device=dev)
    row_loss = torch.empty((B,), dtype=torch.float32, device=dev)
    scores = torch.empty((B, S), dtype=torch.float32, device=dev) if want_scores else None
    if B == 0:
        return true_logit, row_lse, row_loss, scores
    if workspace is None:
        workspace = sampled_softmax_workspace(B, S, D, dev)
    _status(lib().dr_sampled_softmax_fwd(ptr(u), ld_u, ptr(table), V, D, ptr(labels), B, ptr(sampled), S, ptr(log_q_true),
                                         ptr(log_q_sampled), ptr(sample_weight), 1 if remove_accidental_hits else 0, ptr(true_logit),
                                         ptr(row_lse), ptr(row_loss), ptr(scores), ptr(workspace), workspace.numel(), stream_ptr()),
            "dr_sampled_softmax_fwd")
    return true_logit, row_lse, row_loss, scores


def sampled_softmax_bwd(u, table, labels, sampled, true_logit, row_lse, log_q_sampled=None, sample_weight=None,
                        remove_accidental_hits=True, row_scale=1.0, d_u=None, workspace=None):
    """(d_u [B, D], d_true [B, D], d_sampled [S, D]) of dr_sampled_softmax_bwd: the gradients of row_scale * sum_i row_loss[i] from the
    forward's true_logit and row_lse, the scores recomputed.  d_true with ids labels [B, 1] and d_sampled with ids sampled [S, 1] are
    what K4 takes; d_u may be given as a view with a row pitch and is written at that pitch."""
    B, S, V, D, ld_u, labels, sampled, _, log_q_sampled, sample_weight = _ssm_args(u, table, labels, sampled, None, log_q_sampled,
                                                                                  sample_weight)
    dev = table.device
    true_logit = _vec_arg("sampled_softmax", true_logit, B, "true_logit", none_ok=True)
    row_lse = _vec_arg("sampled_softmax", row_lse, B, "row_lse", none_ok=True)
    d_u, ld_du = _rows_arg("sampled_softmax", d_u, D, "d_u", rows=B, device=dev)
    d_true = torch.empty((B, D), dtype=torch.float32, device=dev)
    d_sampled = torch.empty((S, D), dtype=torch.float32, device=dev)
    if B == 0:
        return d_u, d_true, d_sampled.zero_()
    if workspace is None:
        workspace = sampled_softmax_workspace(B, S, D, dev)
    _status(lib().dr_sampled_softmax_bwd(ptr(u), ld_u, ptr(table), V, D, ptr(labels), B, ptr(sampled), S, ptr(log_q_sampled),
                                         ptr(sample_weight), 1 if remove_accidental_hits else 0, float(row_scale), ptr(true_logit),
                                         ptr(row_lse), ptr(d_u), ld_du, ptr(d_true), ptr(d_sampled), ptr(workspace), workspace.numel(),
                                         stream_ptr()), "dr_sampled_softmax_bwd")
    return d_u, d_true, d_sampled


# ---- margin ranking loss with hard-negative mining (csrc/margin_rank.hip): EBR's training loss ----------------------------------------
MARGIN_RANK_TILE = 64               # DR_MARGIN_RANK_TILE: rows / columns of a tile
MARGIN_RANK_COL_GROUP = 128         # DR_MARGIN_RANK_COL_GROUP: a column segment has at least this many columns ...
MARGIN_RANK_MAX_GROUPS = 8          # DR_MARGIN_RANK_MAX_GROUPS: ... and there are at most this many
MARGIN_RANK_SPLIT_TILES = 128       # DR_MARGIN_RANK_SPLIT_TILES: up to this many row tiles every segment has a block of its own
MARGIN_RANK_ROW_CHUNK = 128         # DR_MARGIN_RANK_ROW_CHUNK: a d_neg partial covers at least this many rows ...
MARGIN_RANK_MAX_CHUNKS = 64         # DR_MARGIN_RANK_MAX_CHUNKS: ... and there are at most this many
MARGIN_RANK_MAX_HARD = 8            # DR_MARGIN_RANK_MAX_HARD: the longest hard-negative list
MARGIN_RANK_EPS = 1e-12             # tf.math.l2_normalize's epsilon
MARGIN_RANK_METRICS = {"dot": 0, "cosine": 1}


def _mr_plan(fn, name, B, S, D):
    n = fn(int(B), int(S), int(D))
    if n < 0:
        _status(n, name)
    return n


def margin_rank_col_groups(B, S, D):
    """blocks per row tile of the row-owning kernels (1, or the number of column segments): dr_margin_rank_col_groups"""
    return _mr_plan(lib().dr_margin_rank_col_groups, "dr_margin_rank_col_groups", B, S, D)


def margin_rank_col_segments(B, S, D):
    """number of column segments, a function of S alone: dr_margin_rank_col_segments"""
    return _mr_plan(lib().dr_margin_rank_col_segments, "dr_margin_rank_col_segments", B, S, D)


def margin_rank_row_chunks(B, S, D):
    """number of d_neg partials of the column-owning sweep: dr_margin_rank_row_chunks"""
    return _mr_plan(lib().dr_margin_rank_row_chunks, "dr_margin_rank_row_chunks", B, S, D)


def margin_rank_workspace_bytes(B, S, D, num_hard=0):
    """dr_margin_rank_workspace_bytes: host arithmetic, no device"""
    n = lib().dr_margin_rank_workspace_bytes(int(B), int(S), int(D), int(num_hard))
    if n < 0:
        _status(n, "dr_margin_rank_workspace_bytes")
    return n


def margin_rank_workspace(B, S, D, num_hard, device):
    return torch.empty(max(16, margin_rank_workspace_bytes(B, S, D, num_hard)), dtype=torch.uint8, device=device)


def margin_rank_options(D, metric, num_hard):
    """the host-side domain of the options, shared with the EBR model: (metric code, num_hard); ValueError otherwise"""
    _slab_width("margin_rank", D)
    if metric not in MARGIN_RANK_METRICS:
        raise ValueError("margin_rank: metric must be one of %s, got %r" % (sorted(MARGIN_RANK_METRICS), metric))
    if int(num_hard) != num_hard or not 0 <= int(num_hard) <= MARGIN_RANK_MAX_HARD:
        raise ValueError("margin_rank: num_hard must be an integer in [0, %d], got %r" % (MARGIN_RANK_MAX_HARD, num_hard))
    return MARGIN_RANK_METRICS[metric], int(num_hard)


def _mr_args(q, pos, neg, pos_ids, neg_ids, sample_weight, metric, num_hard):
    """validates the domain of dr_margin_rank_*; returns (B, S, D, ld_q, ld_p, ld_n, neg, in_batch, pos_ids, neg_ids, sample_weight,
    metric code, num_hard)"""
    if q.dim() != 2:
        raise ValueError("margin_rank: q must be fp32 [B, D], got %s" % (tuple(q.shape),))
    B, D = q.shape
    code, K = margin_rank_options(D, metric, num_hard)
    ld_q = _row_pitch("margin_rank", q, D, "q")
    ld_p = _row_pitch("margin_rank", pos, D, "pos")
    if pos.shape[0] != B:
        raise ValueError("margin_rank: pos must have %d rows, got %d" % (B, pos.shape[0]))
    in_batch = neg is None
    if in_batch:
        neg, neg_ids = pos, (pos_ids if neg_ids is None else neg_ids)
    ld_n = _row_pitch("margin_rank", neg, D, "neg")
    S = neg.shape[0]
    if not in_batch and not 1 <= S < 2 ** 31:
        raise ValueError("margin_rank: needs 1 <= S < 2^31 negatives, got %d" % S)
    dev = q.device
    _one_device("margin_rank", "q", dev, pos=pos, neg=neg)
    return (B, S, D, ld_q, ld_p, ld_n, neg, in_batch, _vec_arg("margin_rank", pos_ids, B, "pos_ids", torch.int64, none_ok=True, device=dev),
            _vec_arg("margin_rank", neg_ids, S, "neg_ids", torch.int64, none_ok=True, device=dev),
            _vec_arg("margin_rank", sample_weight, B, "sample_weight", torch.float32, none_ok=True, device=dev), code, K)


def margin_rank_fwd(q, pos, neg=None, pos_ids=None, neg_ids=None, sample_weight=None, margin=0.2, metric="cosine", num_hard=0,
                    want_scores=False, workspace=None):
    """(pos_score [B], row_loss [B], row_active int32 [B], hard_idx int32 [B, num_hard] | None, scores [B, S] | None) of
    dr_margin_rank_fwd: loss_i = w_i sum_{j in N(i)} max(0, margin - s(q_i, pos_i) + s(q_i, neg_j)), s the cosine (or the dot product),
    N(i) the kept negatives of row i or its num_hard highest-scoring ones.  q, pos fp32 [B, D] and neg fp32 [S, D], each possibly a view
    with a row pitch (a multiple of 4); neg=None is in-batch: the negatives of row i are the pos rows of the other rows (and neg_ids
    defaults to pos_ids).  pos_ids int64 [B] (< 0: a padding row, loss 0), neg_ids int64 [S] (< 0: the negative is left out and never
    read); with both given a negative whose id equals the row's pos id is left out.  want_scores is for tests and diagnosis: the only
    [B, S] tensor of the family."""
    B, S, D, ld_q, ld_p, ld_n, neg, in_batch, pos_ids, neg_ids, sample_weight, code, K = _mr_args(q, pos, neg, pos_ids, neg_ids,
                                                                                                 sample_weight, metric, num_hard)
    dev = q.device
    pos_score = torch.empty((B,), dtype=torch.float32, device=dev)
    row_loss = torch.empty((B,), dtype=torch.float32, device=dev)
    row_active = torch.empty((B,), dtype=torch.int32, device=dev)
    hard_idx = torch.empty((B, K), dtype=torch.int32, device=dev) if K > 0 else None
    scores = torch.empty((B, S), dtype=torch.float32, device=dev) if want_scores else None
    if B == 0:
        return pos_score, row_loss, row_active, hard_idx, scores
    if workspace is None:
        workspace = margin_rank_workspace(B, S, D, K, dev)
    _status(lib().dr_margin_rank_fwd(ptr(q), ld_q, ptr(pos), ld_p, ptr(neg), ld_n, D, B, S, ptr(pos_ids), ptr(neg_ids),
                                     ptr(sample_weight), float(margin), code, 1 if in_batch else 0, K, MARGIN_RANK_EPS, ptr(pos_score),
                                     ptr(row_loss), ptr(row_active), ptr(hard_idx), ptr(scores), ptr(workspace), workspace.numel(),
                                     stream_ptr()), "dr_margin_rank_fwd")
    return pos_score, row_loss, row_active, hard_idx, scores


def margin_rank_bwd(q, pos, neg, pos_score, hard_idx, pos_ids=None, neg_ids=None, sample_weight=None, margin=0.2, metric="cosine",
                    num_hard=0, row_scale=1.0, d_q=None, workspace=None):
    """(d_q [B, D], d_pos [B, D], d_neg [S, D]) of dr_margin_rank_bwd: the gradients of row_scale * sum_i row_loss[i] with respect to
    the raw rows (the normalisation differentiated inside) from the forward's pos_score and hard_idx, the scores recomputed.  neg=None
    is in-batch: d_neg [B, D] is then the part that reaches pos as the other rows' negative, and the caller adds d_pos + d_neg.  d_q may
    be given as a view with a row pitch and is written at that pitch."""
    B, S, D, ld_q, ld_p, ld_n, neg, in_batch, pos_ids, neg_ids, sample_weight, code, K = _mr_args(q, pos, neg, pos_ids, neg_ids,
                                                                                                 sample_weight, metric, num_hard)
    dev = q.device
    pos_score = _vec_arg("margin_rank", pos_score, B, "pos_score", torch.float32, none_ok=True, device=dev)
    if K > 0:
        if hard_idx is None:
            raise ValueError("margin_rank: num_hard = %d needs the forward's hard_idx" % K)
        hard_idx = _vec_arg("margin_rank", hard_idx, B * K, "hard_idx", torch.int32, none_ok=True, device=dev)
    else:
        hard_idx = None
    d_q, ld_dq = _rows_arg("margin_rank", d_q, D, "d_q", rows=B, device=dev)
    d_pos = torch.empty((B, D), dtype=torch.float32, device=dev)
    d_neg = torch.empty((S, D), dtype=torch.float32, device=dev)
    if B == 0:
        return d_q, d_pos, d_neg.zero_()
    if workspace is None:
        workspace = margin_rank_workspace(B, S, D, K, dev)
    _status(lib().dr_margin_rank_bwd(ptr(q), ld_q, ptr(pos), ld_p, ptr(neg), ld_n, D, B, S, ptr(pos_ids), ptr(neg_ids),
                                     ptr(sample_weight), float(margin), code, 1 if in_batch else 0, K, MARGIN_RANK_EPS, float(row_scale),
                                     ptr(pos_score), ptr(hard_idx), ptr(d_q), ld_dq, ptr(d_pos), ptr(d_neg), ptr(workspace),
                                     workspace.numel(), stream_ptr()), "dr_margin_rank_bwd")
    return d_q, d_pos, d_neg


# ---- BERT (csrc/bert.hip) -----------------------------------------------------------------------------------------------------------------
SOFTMAX_CE_IDS_LDS_COLS = 32768     # DR_SOFTMAX_CE_IDS_LDS_COLS: rows up to this width are staged in LDS
MLM_MAX_LENGTH = 512                # dr_mlm_mask: one wave per sequence
MLM_MAX_PREDICTIONS = 128


def _bert_arg(t, what, dtype, shape=None):
    """an argument the BERT kernels address densely and never copy: another dtype, shape or a view is a ValueError naming it"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)) or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor%s, got %s" % (
            what, dtype, " of shape %s" % (tuple(shape),) if shape is not None else "",
            "%s %s with strides %s" % (t.dtype, tuple(t.shape), tuple(t.stride())) if isinstance(t, torch.Tensor) else type(t).__name__))
    return t


def gelu_fwd(z, out=None):
    """h [M, N] = z * Phi(z), the exact (erf) GELU of dr_gelu_fwd; z may be a view with a row pitch and is left as it is"""
    ld_z = _pitched("gelu_fwd", z, "z")
    M, N = z.shape
    if out is None:
        out = torch.empty((M, _pad4(N)), dtype=torch.float32, device=z.device)[:, :N]
    ld_h = _pitched("gelu_fwd", out, "out")
    if tuple(out.shape) != (M, N):
        raise ValueError("gelu_fwd: out must be %s, got %s" % ((M, N), tuple(out.shape)))
    check(lib().dr_gelu_fwd(ptr(z), ld_z, M, N, ptr(out), ld_h, stream_ptr()), "dr_gelu_fwd")
    return out


def gelu_bwd_(z, dy):
    """in place: dy *= Phi(z) + z phi(z), the GELU's derivative through the saved pre-activation z"""
    ld_z = _pitched("gelu_bwd_", z, "z")
    ld_dy = _pitched("gelu_bwd_", dy, "dy")
    if z.shape != dy.shape:
        raise ValueError("gelu_bwd_: z %s and dy %s differ in shape" % (tuple(z.shape), tuple(dy.shape)))
    check(lib().dr_gelu_bwd(ptr(z), ld_z, ptr(dy), ld_dy, z.shape[0], z.shape[1], stream_ptr()), "dr_gelu_bwd")
    return dy


def _bert_embed_args(ids, segment, tok, pos, seg, gamma, beta, rate):
    if not isinstance(ids, torch.Tensor) or ids.dim() != 2:
        raise ValueError("bert_embed: ids must be an int64 [B, L] tensor")
    B, L = ids.shape
    _bert_arg(ids, "bert_embed: ids", torch.int64)
    _bert_arg(segment, "bert_embed: segment", torch.int64, (B, L))
    if not isinstance(tok, torch.Tensor) or tok.dim() != 2:
        raise ValueError("bert_embed: tok must be an fp32 [V, D] tensor")
    V, D = tok.shape
    _bert_arg(tok, "bert_embed: tok", torch.float32)
    if not isinstance(pos, torch.Tensor) or pos.dim() != 2 or not isinstance(seg, torch.Tensor) or seg.dim() != 2:
        raise ValueError("bert_embed: pos must be [max_position, D] and seg [T, D]")
    _bert_arg(pos, "bert_embed: pos", torch.float32, (pos.shape[0], D))
    _bert_arg(seg, "bert_embed: seg", torch.float32, (seg.shape[0], D))
    _bert_arg(gamma, "bert_embed: gamma", torch.float32, (D,))
    if beta is not None:
        _bert_arg(beta, "bert_embed: beta", torch.float32, (D,))
    if D % 4 != 0 or D < 4 or D > 1024 or L > pos.shape[0] or V < 1 or seg.shape[0] < 1:
        raise ValueError("bert_embed: D %d must be a multiple of 4 in [4, 1024] and L %d <= max_position %d" % (D, L, pos.shape[0]))
    if not 0.0 <= float(rate) < 1.0:
        raise ValueError("bert_embed: rate must be in [0, 1), got %r" % (rate,))
    return B, L, V, D, pos.shape[0], seg.shape[0]


def bert_embed_fwd(ids, segment, tok, pos, seg, gamma, beta, eps=1e-12, rate=0.0, seed=0):
    """(out [B, L, D], stats [B * L, 2]) of dr_bert_embed_fwd: dropout(LayerNorm(tok[ids] + pos[l] + seg[segment])); ids, segment int64
    [B, L], tok [V, D], pos [max_position, D], seg [T, D]; an id or segment out of range reads as a zero row"""
    B, L, V, D, P, T = _bert_embed_args(ids, segment, tok, pos, seg, gamma, beta, rate)
    out = torch.empty((B, L, D), dtype=torch.float32, device=tok.device)
    stats = torch.empty((B * L, 2), dtype=torch.float32, device=tok.device)
    if B * L > 0:
        _status(lib().dr_bert_embed_fwd(ptr(ids), ptr(segment), B * L, L, ptr(tok), V, ptr(pos), P, ptr(seg), T, ptr(gamma), ptr(beta), D,
                                        float(eps), float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out), D, ptr(stats), stream_ptr()),
                "dr_bert_embed_fwd")
    return out, stats


def bert_embed_bwd(ids, segment, tok, pos, seg, gamma, stats, d_out, d_tok, rate=0.0, seed=0):
    """(d_s [B * L, D], d_gamma [D], d_beta [D], d_pos [L, D], d_seg [T, D]) of dr_bert_embed_bwd, and d_tok [V, D] += the rows of d_s
    summed per id in ascending position order.  Everything is summed in a fixed order (deterministic)."""
    B, L, V, D, P, T = _bert_embed_args(ids, segment, tok, pos, seg, gamma, None, rate)
    N = B * L
    _bert_arg(stats, "bert_embed_bwd: stats", torch.float32, (N, 2))
    _bert_arg(d_tok, "bert_embed_bwd: d_tok", torch.float32, (V, D))
    if not isinstance(d_out, torch.Tensor) or d_out.dtype != torch.float32 or d_out.numel() != N * D:
        raise ValueError("bert_embed_bwd: d_out must be fp32 with %d elements" % (N * D))
    d_out = d_out.reshape(N, D)
    ld_do = _pitched("bert_embed_bwd", d_out, "d_out") if N > 0 else D
    dev = tok.device
    d_s = torch.empty((N, D), dtype=torch.float32, device=dev)
    d_gamma = torch.zeros(D, dtype=torch.float32, device=dev)
    d_beta = torch.zeros(D, dtype=torch.float32, device=dev)
    d_pos = torch.zeros((L, D), dtype=torch.float32, device=dev)
    d_seg = torch.zeros((T, D), dtype=torch.float32, device=dev)
    if N == 0:
        return d_s, d_gamma, d_beta, d_pos, d_seg
    sorted_ids, order = torch.sort(ids.reshape(-1), stable=True)     # plumbing: the order of the row owners' sums
    nb = lib().dr_bert_embed_bwd_workspace_bytes(N, L, D, T)
    ws = torch.empty(max(1, nb // 4), dtype=torch.float32, device=dev)
    _status(lib().dr_bert_embed_bwd(ptr(ids), ptr(segment), ptr(sorted_ids), ptr(order), N, L, ptr(tok), V, ptr(pos), ptr(seg), T,
                                    ptr(gamma), ptr(stats), D, ptr(d_out), ld_do, float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(d_s),
                                    ptr(d_gamma), ptr(d_beta), ptr(d_tok), ptr(d_pos), ptr(d_seg), ptr(ws), ws.numel() * 4, stream_ptr()),
            "dr_bert_embed_bwd")
    return d_s, d_gamma, d_beta, d_pos, d_seg


def softmax_ce_ids(logits, labels, bias=None, weight=None, smoothing=0.0, row_scale=1.0, denom=None, denom_eps=0.0, row_loss=None,
                   _path=0):
    """row_loss [M] of dr_softmax_ce_ids; logits [M, C] (a row pitch is honoured) are OVERWRITTEN with the gradient
    row_scale * w / (denom + denom_eps) * (softmax(logits + bias) - (1 - smoothing) * onehot(labels) - smoothing / C).  labels int64 [M],
    a negative one marks a padding row (loss 0, a zero gradient row, its logits never read); denom is a one-element DEVICE tensor.
    _path (tests only): 1 forces the kernel that stages the row in LDS, 2 the one that re-reads it from memory."""
    ld = _pitched("softmax_ce_ids", logits, "logits")
    M, C = logits.shape
    _bert_arg(labels, "softmax_ce_ids: labels", torch.int64, (M,))
    if bias is not None:
        _bert_arg(bias, "softmax_ce_ids: bias", torch.float32, (C,))
    if weight is not None:
        _bert_arg(weight, "softmax_ce_ids: weight", torch.float32, (M,))
    if denom is not None:
        _bert_arg(denom, "softmax_ce_ids: denom", torch.float32)
        if denom.numel() != 1:
            raise ValueError("softmax_ce_ids: denom must hold one element, got %s" % (tuple(denom.shape),))
    if not 0.0 <= float(smoothing) < 1.0:
        raise ValueError("softmax_ce_ids: smoothing must be in [0, 1), got %r" % (smoothing,))
    if row_loss is None:
        row_loss = torch.empty(M, dtype=torch.float32, device=logits.device)
    else:
        _bert_arg(row_loss, "softmax_ce_ids: row_loss", torch.float32, (M,))
    _status(lib().dr_softmax_ce_ids(ptr(logits), ld, ptr(bias), ptr(labels), ptr(weight), M, C, float(smoothing), float(row_scale),
                                    ptr(denom), float(denom_eps), ptr(row_loss), int(_path), stream_ptr()), "dr_softmax_ce_ids")
    return row_loss


def colsum_add_workspace(M, C, device):
    return torch.empty(max(1, lib().dr_colsum_add_workspace_bytes(int(M), int(C)) // 4), dtype=torch.float32, device=device)


def colsum_add(g, dst, workspace=None):
    """dst [C] += the column sums of g [M, C] (a row pitch is honoured), in a fixed order: dr_colsum_add"""
    ld = _pitched("colsum_add", g, "g")
    M, C = g.shape
    _bert_arg(dst, "colsum_add: dst", torch.float32, (C,))
    if workspace is None or workspace.numel() * 4 < lib().dr_colsum_add_workspace_bytes(M, C):
        workspace = colsum_add_workspace(M, C, g.device)
    _status(lib().dr_colsum_add(ptr(g), ld, M, C, ptr(dst), ptr(workspace), workspace.numel() * 4, stream_ptr()), "dr_colsum_add")
    return dst


def mlm_prob_q16(prob):
    """round(prob * 65536): the fixed-point masking probability dr_mlm_mask takes"""
    if not 0.0 <= float(prob) <= 1.0:
        raise ValueError("mlm_mask: prob must be in [0, 1], got %r" % (prob,))
    return int(round(float(prob) * 65536))


def mlm_mask(ids, vocab_size, num_special, mask_id, prob=0.15, max_predictions=20, seed=0):
    """(out_ids [B, L], positions int32 [B, P], labels int64 [B, P]) of dr_mlm_mask: BERT's dynamic masking on the device, a function of
    (seed, ids) alone.  Positions holding an id >= num_special are candidates; positions / labels are -1 beyond a row's count."""
    if not isinstance(ids, torch.Tensor) or ids.dim() != 2:
        raise ValueError("mlm_mask: ids must be an int64 [B, L] tensor")
    _bert_arg(ids, "mlm_mask: ids", torch.int64)
    B, L = ids.shape
    P = int(max_predictions)
    if L > MLM_MAX_LENGTH or L < 1 or not 1 <= P <= MLM_MAX_PREDICTIONS:
        raise ValueError("mlm_mask: 1 <= L <= %d and 1 <= max_predictions <= %d, got L %d, max_predictions %d"
                         % (MLM_MAX_LENGTH, MLM_MAX_PREDICTIONS, L, P))
    if not 0 <= int(num_special) < int(vocab_size):
        raise ValueError("mlm_mask: 0 <= num_special < vocab_size, got %r, %r" % (num_special, vocab_size))
    out_ids = torch.empty_like(ids)
    positions = torch.empty((B, P), dtype=torch.int32, device=ids.device)
    labels = torch.empty((B, P), dtype=torch.int64, device=ids.device)
    _status(lib().dr_mlm_mask(ptr(ids), B, L, int(vocab_size), int(num_special), int(mask_id), mlm_prob_q16(prob), P,
                              int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out_ids), ptr(positions), ptr(labels), stream_ptr()), "dr_mlm_mask")
    return out_ids, positions, labels


# ---- IntentGC: the vector-wise convolution over typed blocks (csrc/intent_conv.hip) -------------------------------------------------------
INTENT_MAX_TYPES = 7        # R, the neighbour types of a typed block
INTENT_MAX_FILTERS = 16     # L, the local filters of a layer


_INTENT_ROWS = dict(mult4=True, aligned=True, tight_row=True)     # how dr_intent_* take h, out and the gradients (_pitched's policy)


def _intent_dims(R, D, L, act):
    """validates the domain of dr_intent_*; returns (R, D, L, act) as ints"""
    R, D, L = int(R), _slab_width("intent_conv", D, "the row width D"), int(L)
    if not 1 <= R <= INTENT_MAX_TYPES:
        raise ValueError("intent_conv: needs 1 <= R <= %d neighbour types, got R = %d" % (INTENT_MAX_TYPES, R))
    if not 1 <= L <= INTENT_MAX_FILTERS:
        raise ValueError("intent_conv: needs 1 <= L <= %d filters, got L = %d" % (INTENT_MAX_FILTERS, L))
    if act not in (0, 1):
        raise ValueError("intent_conv: act must be 0 (linear) or 1 (relu), got %r" % (act,))
    return R, D, L, int(act)


def _intent_filters(W, theta, R=None):
    """(W [L, R + 1], theta [L], R, L) dense fp32"""
    if W.dim() != 2 or W.shape[1] < 2 or (R is not None and W.shape[1] != int(R) + 1):
        raise ValueError("intent_conv: W must be fp32 [L, R + 1]%s, got %s" % ("" if R is None else " with R = %d" % int(R), tuple(W.shape)))
    L, R = int(W.shape[0]), int(W.shape[1]) - 1
    W = _dense_arg(W, "intent_conv: W")
    theta = _dense_arg(theta, "intent_conv: theta", numel=L)
    if theta is None:
        raise ValueError("intent_conv: theta [%d] is required" % L)
    return W, theta, R, L


def _intent_agg(agg, n_dst, R, D, what):
    """agg / d_agg as the kernels address it: fp32 [n_dst, R, D] (or [n_dst * R, D]) contiguous, 16-byte aligned"""
    if agg.dtype != torch.float32 or tuple(agg.shape) not in ((n_dst, R, D), (n_dst * R, D)):
        raise ValueError("intent_conv: %s must be fp32 [%d, %d, %d], got %s %s" % (what, n_dst, R, D, agg.dtype, tuple(agg.shape)))
    if not agg.is_contiguous() or agg.data_ptr() % 16 != 0:
        raise ValueError("intent_conv: %s must be contiguous and 16-byte aligned, got strides %s" % (what, tuple(agg.stride())))
    return agg


def intent_conv_fwd(row_ptr, col, val, n_dst, R, h, W, theta, act=1, want_agg=False, out=None):
    """(out [n_dst, D], agg [n_dst, R, D] | None) of dr_intent_conv_fwd over a typed block's CSR (row_ptr int64 [n_dst R + 1], col
    int32, val fp32; virtual row v R + r holds the type-(r + 1) neighbours of destination v): a_0 = h[v], a_r the rows' sums, p_i =
    sum_r W[i, r] a_r, out = act(sum_i theta_i relu(p_i)).  h fp32 [n_src, D] (its first n_dst rows are the destinations; a view with a
    row pitch is read in place).  want_agg stores the aggregates for intent_conv_bwd.  out: a buffer to overwrite."""
    n_dst = int(n_dst)
    W, theta, R, L = _intent_filters(W, theta, R)
    if h.dim() != 2:
        raise ValueError("intent_conv: h must be fp32 [n_src, D], got %s" % (tuple(h.shape),))
    R, D, L, act = _intent_dims(R, h.shape[1], L, act)
    ld_h = _pitched("intent_conv", h, "h", D, n_dst, min_rows=True, **_INTENT_ROWS)
    row_ptr = _dense_arg(row_ptr, "intent_conv: row_ptr", torch.int64, shape=(n_dst * R + 1,))
    col = _dense_arg(col, "intent_conv: col", torch.int32)
    val = _dense_arg(val, "intent_conv: val", torch.float32, numel=col.numel())
    if out is None:
        out = torch.empty((n_dst, D), dtype=torch.float32, device=h.device)
    ld_out = _pitched("intent_conv", out, "out", D, n_dst, **_INTENT_ROWS)
    agg = torch.empty((n_dst, R, D), dtype=torch.float32, device=h.device) if want_agg else None
    if n_dst == 0:
        return out, agg
    _status(lib().dr_intent_conv_fwd(ptr(row_ptr), ptr(col) if col.numel() else None, ptr(val) if val.numel() else None, n_dst, R, ptr(h),
                                     ld_h, D, ptr(W), ptr(theta), L, act, ptr(out), ld_out, ptr(agg), stream_ptr()), "dr_intent_conv_fwd")
    return out, agg


def intent_mix_fwd(h_self, agg, W, theta, act=1, out=None):
    """out [n_dst, D] of dr_intent_mix_fwd: intent_conv_fwd's filters on aggregates that already exist (agg fp32 [n_dst, R, D], e.g.
    adj.spmm(h) of a typed adjacency viewed so) and the destinations' own rows h_self [n_dst, D]; the same bits as the gathered form
    gives from the same aggregates."""
    W, theta, R, L = _intent_filters(W, theta)
    if h_self.dim() != 2:
        raise ValueError("intent_conv: h_self must be fp32 [n_dst, D], got %s" % (tuple(h_self.shape),))
    n_dst = int(h_self.shape[0])
    R, D, L, act = _intent_dims(R, h_self.shape[1], L, act)
    ld_h = _pitched("intent_conv", h_self, "h_self", D, n_dst, **_INTENT_ROWS)
    agg = _intent_agg(agg, n_dst, R, D, "agg")
    if out is None:
        out = torch.empty((n_dst, D), dtype=torch.float32, device=h_self.device)
    ld_out = _pitched("intent_conv", out, "out", D, n_dst, **_INTENT_ROWS)
    if n_dst == 0:
        return out
    _status(lib().dr_intent_mix_fwd(ptr(h_self), ld_h, ptr(agg), n_dst, R, D, ptr(W), ptr(theta), L, act, ptr(out), ld_out, stream_ptr()),
            "dr_intent_mix_fwd")
    return out


def intent_conv_bwd_workspace(n_dst, D, R, L, device):
    n = lib().dr_intent_conv_bwd_workspace_bytes(int(n_dst), int(D), int(R), int(L))
    if n < 0:
        raise ValueError("intent_conv: (n_dst, D, R, L) = %s is outside the kernel's domain" % ((n_dst, D, R, L),))
    return torch.empty((max(4, n) // 4,), dtype=torch.float32, device=device)


def intent_conv_bwd(h_self, agg, d_out, W, theta, act=1, out=None, d_self=None, workspace=None):
    """(d_self [n_dst, D], d_agg [n_dst, R, D], d_W [L, R + 1], d_theta [L]) of dr_intent_conv_bwd from the destinations' rows, the
    aggregates the forward stored, d_out [n_dst, D] and optionally the forward's out (otherwise recomputed).  d_self: a buffer to
    overwrite, e.g. the top rows of the source gradient; d_agg goes through the transposed block (adj.transpose().spmm) to the rest."""
    W, theta, R, L = _intent_filters(W, theta)
    if h_self.dim() != 2:
        raise ValueError("intent_conv: h_self must be fp32 [n_dst, D], got %s" % (tuple(h_self.shape),))
    n_dst = int(h_self.shape[0])
    R, D, L, act = _intent_dims(R, h_self.shape[1], L, act)
    ld_h = _pitched("intent_conv", h_self, "h_self", D, n_dst, **_INTENT_ROWS)
    agg = _intent_agg(agg, n_dst, R, D, "agg")
    ld_do = _pitched("intent_conv", d_out, "d_out", D, n_dst, **_INTENT_ROWS)
    ld_out = _pitched("intent_conv", out, "out", D, n_dst, **_INTENT_ROWS) if out is not None else 0
    dev = h_self.device
    if d_self is None:
        d_self = torch.empty((n_dst, D), dtype=torch.float32, device=dev)
    ld_ds = _pitched("intent_conv", d_self, "d_self", D, n_dst, **_INTENT_ROWS)
    d_agg = torch.empty((n_dst, R, D), dtype=torch.float32, device=dev)
    d_W = torch.zeros((L, R + 1), dtype=torch.float32, device=dev)
    d_theta = torch.zeros((L,), dtype=torch.float32, device=dev)
    if n_dst == 0:
        return d_self, d_agg, d_W, d_theta
    if workspace is None:
        workspace = intent_conv_bwd_workspace(n_dst, D, R, L, dev)
    _status(lib().dr_intent_conv_bwd(ptr(h_self), ld_h, ptr(agg), ptr(d_out), ld_do, ptr(out), ld_out, ptr(W), ptr(theta), n_dst, R, D, L,
                                     act, ptr(d_self), ld_ds, ptr(d_agg), ptr(d_W), ptr(d_theta), ptr(workspace), workspace.numel() * 4,
                                     stream_ptr()), "dr_intent_conv_bwd")
    return d_self, d_agg, d_W, d_theta
