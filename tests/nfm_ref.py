"""Restatement of NFM (He & Chua 2017) in plain torch ops, in the dtype of its arguments (float64 as the reference, float32 to measure what
rounding alone does to it).  tests/test_gpu_nfm.py compares the kernels (csrc/bi_interaction.hip) and the model against it;
tests/test_nfm_cpu.py checks its closed-form backward against autograd and the derived error bounds against its own float32 run.

rows [B, F, D]: rows[b, f] is the row of example b's field f (the mean of its bag, zeros when the bag is empty)."""
import torch

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def gather(table, ids, row_base):
    """rows [B, F, D] from table [R, D], ids [B, F] (an id < 0 is a row of zeros) and row_base [F]"""
    rows = table[(ids.clamp_min(0) + row_base[None, :])]
    return torch.where((ids >= 0)[:, :, None], rows, torch.zeros_like(rows))


def pool(table, bags, row_base):
    """rows [B, F, D] from bags = [ids [B, n_f] per field]: the mean over the valid ids, zeros for an empty bag (K3's pooling)"""
    out = []
    for f, ids in enumerate(bags):
        r = table[ids.clamp_min(0) + row_base[f]]                          # [B, n_f, D]
        valid = (ids >= 0)
        s = torch.where(valid[:, :, None], r, torch.zeros_like(r)).sum(1)
        cnt = valid.sum(1).clamp_min(1).to(table.dtype)
        out.append(s / cnt[:, None])
    return torch.stack(out, 1)


def first_order(lin_w, lin_bias, bags, row_base):
    """lin_bias + sum over every valid id of lin_w[row]"""
    fo = lin_bias.reshape(()).expand(bags[0].shape[0]).clone()
    for f, ids in enumerate(bags):
        w = lin_w[ids.clamp_min(0) + row_base[f]]
        fo = fo + torch.where(ids >= 0, w, torch.zeros_like(w)).sum(1)
    return fo


def bi_forward(rows):
    """[B, D] = 0.5 ((sum_f e_f)^2 - sum_f e_f^2)"""
    s = rows.sum(1)
    return 0.5 * (s * s - (rows * rows).sum(1))


def bi_pairs(rows):
    """the same vector written out pair by pair: sum_{i < j} e_i * e_j"""
    F = rows.shape[1]
    out = torch.zeros_like(rows[:, 0])
    for i in range(F):
        for j in range(i + 1, F):
            out = out + rows[:, i] * rows[:, j]
    return out


def bi_backward(rows, d_out):
    """d_rows [B, F, D] = d_out * (s - e_f), the closed form"""
    s = rows.sum(1, keepdim=True)
    return d_out[:, None, :] * (s - rows)


def fwd_bound(rows):
    """|out - exact| <= 0.5 gamma(2 F + 2) ((sum_f |e_f|)^2 + sum_f e_f^2) per element, any order, with or without FMA"""
    F = rows.shape[1]
    a = rows.abs().sum(1)
    return 0.5 * gamma(2 * F + 2) * (a * a + (rows * rows).sum(1))


def bwd_bound(rows, d_out):
    """|d_rows - exact| <= gamma(F + 2) |d_out| (sum_g |e_g| + |e_f|)"""
    F = rows.shape[1]
    a = rows.abs().sum(1, keepdim=True)
    return gamma(F + 2) * d_out.abs()[:, None, :] * (a + rows.abs())


def first_order_bound(lin_w, lin_bias, bags, row_base):
    """FFM's bound: gamma(n) (|bias| + sum |w|) for a sum of n + 1 terms in any order"""
    n = sum(int(b.shape[1]) for b in bags)
    return gamma(n + 1) * first_order(lin_w.abs(), lin_bias.abs(), bags, row_base)


ACTS = {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "linear": lambda x: x, None: lambda x: x}


def tower(bi, first, kernels, biases, w_out, activation="relu"):
    """logits [B, 1] = first + Dense(1, no bias)(MLP(bi))"""
    h = bi
    for W, b in zip(kernels, biases):
        h = ACTS[activation](h @ W + b)
    return first[:, None] + h @ w_out


def logits(params, bags, row_base, activation="relu"):
    rows = pool(params["table"], bags, row_base)
    return tower(bi_forward(rows), first_order(params["lin_w"], params["lin_bias"], bags, row_base), params["kernels"], params["biases"],
                 params["w_out"], activation)


def cast(params, dtype):
    return {k: [t.detach().to(dtype).clone() for t in v] if isinstance(v, list) else v.detach().to(dtype).clone()
            for k, v in params.items()}


def train_step(params, bags, row_base, labels, lr, activation="relu"):
    """one SGD step on the mean sigmoid cross-entropy with autograd in the parameters' dtype: (new params, loss)"""
    p = cast(params, params["table"].dtype)
    leaves = [p["table"], p["lin_w"], p["lin_bias"], p["w_out"]] + p["kernels"] + p["biases"]
    for t in leaves:
        t.requires_grad_()
    x = logits(p, bags, row_base, activation)[:, 0]
    y = labels.to(x.dtype)
    loss = (x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))).mean()
    loss.backward()
    new = {k: [(t - lr * t.grad).detach() for t in v] if isinstance(v, list) else (v - lr * v.grad).detach() for k, v in p.items()}
    return new, loss.detach()


# ---- the cases both test files use ---------------------------------------------------------------------------------------------------------
SHAPES = [(3, 1, 4), (2, 2, 4), (4, 3, 8), (3, 7, 12), (70, 5, 20), (130, 4, 4), (5, 26, 64), (2, 39, 16), (2, 2, 256), (1, 64, 4),
          (2, 1024, 4)]
ROWS_PER_FIELD = 5


def make_case(B, F, D, grid=False, seed=0):
    """float64 inputs of one shape: a 5-row-per-field table, ids repeated inside the batch and one id of -1, d_out, lin_w, lin_bias.
    grid: every entry an integer in {-3 .. 3}, where fp32 arithmetic of any order is exact"""
    g = torch.Generator().manual_seed(977 * seed + 31 * B + 7 * F + D)
    R = ROWS_PER_FIELD * F
    if grid:
        table = torch.randint(-3, 4, (R, D), generator=g).double()
        d_out = torch.randint(-3, 4, (B, D), generator=g).double()
        lin_w = torch.randint(-3, 4, (R,), generator=g).double()
        lin_bias = torch.tensor([2.0], dtype=torch.float64)
    else:
        table = torch.randn(R, D, generator=g, dtype=torch.float64).float().double()       # fp32-representable
        d_out = torch.randn(B, D, generator=g, dtype=torch.float64).float().double()
        lin_w = torch.randn(R, generator=g, dtype=torch.float64).float().double()
        lin_bias = torch.tensor([0.25], dtype=torch.float64)
    ids = torch.randint(0, 3, (B, F), generator=g)                                         # rows 3 and 4 of every field stay unreferenced
    ids[B // 2, F // 2] = -1
    row_base = ROWS_PER_FIELD * torch.arange(F)
    return {"shape": (B, F, D), "table": table, "ids": ids, "row_base": row_base, "d_out": d_out, "lin_w": lin_w, "lin_bias": lin_bias}
