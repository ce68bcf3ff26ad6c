"""Float64 restatement of FFM (Juan et al. 2016) in plain torch ops, written out pair by pair.  tests/test_gpu_ffm.py compares the kernels
(csrc/ffm.hip) and the model against it; tests/test_ffm_cpu.py checks it against hand-written cases, the FM limit and float64 autograd.

A [B, F, F, k]: A[b, i, j, :] is the factor of example b's feature of field i towards field j (block j of field i's table row).  The
diagonal blocks A[b, i, i, :] take no part: they are never touched here, so whatever they hold (NaN included) reaches nothing."""
import torch


def interaction(A):
    """inter [B] = sum_{i = 1 .. F-1} sum_{j < i} sum_c A[b, i, j, c] * A[b, j, i, c]"""
    B, F = A.shape[0], A.shape[1]
    inter = torch.zeros(B, dtype=A.dtype)
    for i in range(1, F):
        for j in range(i):
            inter = inter + (A[:, i, j] * A[:, j, i]).sum(-1)
    return inter


def interaction_backward(A, d_inter):
    """d_rows [B, F, F, k]: d_rows[b, i, j, :] = d_inter[b] * A[b, j, i, :] for j != i, zeros on the diagonal"""
    F = A.shape[1]
    d = torch.zeros_like(A)
    for i in range(F):
        for j in range(F):
            if i != j:
                d[:, i, j] = d_inter[:, None] * A[:, j, i]
    return d


def abs_sum(A):
    """sum_{j < i, c} |A[b, i, j, c]| |A[b, j, i, c]|: what the forward's error bound multiplies"""
    F = A.shape[1]
    s = torch.zeros(A.shape[0], dtype=A.dtype)
    for i in range(1, F):
        for j in range(i):
            s = s + (A[:, i, j].abs() * A[:, j, i].abs()).sum(-1)
    return s


def gather(table, ids, row_base, F, k):
    """A [B, F, F, k] from table [R, F * k], ids [B, F] (an id < 0 is a row of zeros) and row_base [F]"""
    rows = table[(ids.clamp_min(0) + row_base[None, :])]                  # [B, F, F * k]
    rows = torch.where((ids >= 0)[:, :, None], rows, torch.zeros_like(rows))
    return rows.reshape(ids.shape[0], F, F, k)


def first_order(lin_w, lin_bias, ids, row_base):
    """lin_bias + sum_f lin_w[row_base[f] + ids[b, f]], missing ids skipped"""
    w = lin_w[(ids.clamp_min(0) + row_base[None, :])]
    return lin_bias.reshape(()) + torch.where(ids >= 0, w, torch.zeros_like(w)).sum(-1)


def ffm_logits(A, first):
    """logit [B] = first_order + inter"""
    return first + interaction(A)
