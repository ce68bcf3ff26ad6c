"""Restatement of LS-PLM (Gai et al. 2017) in plain torch ops, in the dtype of its arguments (float64 as the reference, float32 to measure
what rounding alone does to it).  tests/test_gpu_lsplm.py compares the kernels (csrc/lsplm.hip) and the model against it;
tests/test_lsplm_cpu.py checks its closed-form backward against autograd and runs the XOR task the mixture exists for.

A table row is [u (m) | w (m)].  bags = [ids [B, n_f] per field]; an id < 0 is dropped, an empty bag adds nothing.  m = 1 is the plain
logistic model: the softmax over one region is 1."""
import math

import torch

U = 2.0 ** -24


def pool(table, bias, bags, row_base):
    """z [B, 2 m] = bias + sum_f mean over the valid ids of field f's bag of table[row_base[f] + id]"""
    z = bias[None, :].expand(bags[0].shape[0], -1).clone()
    for f, ids in enumerate(bags):
        r = table[ids.clamp_min(0) + row_base[f]]
        valid = ids >= 0
        s = torch.where(valid[:, :, None], r, torch.zeros_like(r)).sum(1)
        z = z + s / valid.sum(1).clamp_min(1).to(table.dtype)[:, None]
    return z


def head(z):
    """(p, q, pi, sg): p = sum_i softmax(z[:m])_i sigmoid(z[m + i]), q = sum_i pi_i sigmoid(-z[m + i])"""
    m = z.shape[1] // 2
    pi = torch.softmax(z[:, :m], 1)
    sg, sn = torch.sigmoid(z[:, m:]), torch.sigmoid(-z[:, m:])
    return (pi * sg).sum(1), (pi * sn).sum(1), pi, sg


def dz_closed_form(z, d_p):
    """d_z = d_p [pi (sg - p) ; pi sg (1 - sg)]"""
    p, _, pi, sg = head(z)
    return d_p[:, None] * torch.cat([pi * (sg - p[:, None]), pi * sg * (1 - sg)], 1)


def loss_rows(p, q, y, wt=None):
    """-wt (y log p + (1 - y) log q); a term whose coefficient is exactly 0 is not evaluated"""
    one = torch.ones_like(p)
    t = torch.where(y != 0, y * torch.log(torch.where(y != 0, p, one)), torch.zeros_like(p)) + \
        torch.where(y != 1, (1 - y) * torch.log(torch.where(y != 1, q, one)), torch.zeros_like(p))
    return -t if wt is None else -wt * t


def dp_of_loss(p, q, y, wt=None, row_scale=1.0):
    """d (row_scale loss_b) / d p_b = (row_scale wt) (-y / p + (1 - y) / q), with q = 1 - p"""
    one = torch.ones_like(p)
    c = torch.where(y != 0, -y / torch.where(y != 0, p, one), torch.zeros_like(p)) + \
        torch.where(y != 1, (1 - y) / torch.where(y != 1, q, one), torch.zeros_like(p))
    w = torch.full_like(p, row_scale) if wt is None else row_scale * wt
    return w * c


def train_step(table, bias, bags, row_base, labels, lr, wt=None):
    """one SGD step on the mean loss with autograd in the table's dtype: (new table, new bias, mean loss)"""
    t, b = table.detach().clone().requires_grad_(), bias.detach().clone().requires_grad_()
    p, q, _, _ = head(pool(t, b, bags, row_base))
    y = labels.to(t.dtype)
    loss = loss_rows(p, q, y, None if wt is None else wt.to(t.dtype)).mean()
    loss.backward()
    return (t - lr * t.grad).detach(), (b - lr * b.grad).detach(), loss.detach()


def xor_batch(seed, step, B):
    g = torch.Generator().manual_seed(1000 * seed + step)
    ab = torch.randint(0, 2, (B, 2), generator=g)
    return ab, (ab[:, 0] ^ ab[:, 1]).to(torch.float64)


XOR_POINTS = torch.tensor([[0, 0], [0, 1], [1, 0], [1, 1]])
XOR_ROW_BASE = torch.tensor([0, 2])


def xor_init(m, seed, sigma=0.5):
    """table [4, 2 m] float64 (two binary fields, two rows each), truncated normal at 2 sigma; bias zeros"""
    g = torch.Generator().manual_seed(seed)
    t = torch.empty(4, 2 * m, dtype=torch.float64)
    torch.nn.init.trunc_normal_(t, 0.0, sigma, -2 * sigma, 2 * sigma, generator=g)
    return t, torch.zeros(2 * m, dtype=torch.float64)


def xor_population_loss(table, bias):
    """the mean loss over the four points (a, b) with label a xor b"""
    y = (XOR_POINTS[:, 0] ^ XOR_POINTS[:, 1]).to(table.dtype)
    p, q, _, _ = head(pool(table, bias, [XOR_POINTS[:, :1], XOR_POINTS[:, 1:]], XOR_ROW_BASE))
    return loss_rows(p, q, y).mean().item()


def xor_run(m, seed, steps=300, B=256, lr=1.0, sigma=0.5):
    """SGD on the XOR stream in float64; the loss on the four-point population at the end"""
    table, bias = xor_init(m, seed, sigma)
    for s in range(steps):
        ab, y = xor_batch(seed, s, B)
        table, bias, _ = train_step(table, bias, [ab[:, :1], ab[:, 1:]], XOR_ROW_BASE, y, lr)
    return xor_population_loss(table, bias)


LN2 = math.log(2.0)


# ---- the cases both test files use ---------------------------------------------------------------------------------------------------------
SHAPES = [(3, 1, 2), (2, 2, 2), (4, 3, 6), (5, 39, 12), (70, 5, 10), (2, 2, 128), (3, 26, 4), (130, 4, 2)]
ROWS_PER_FIELD = 5
BAG_SIZES = (0, 1, 2, 4)
BAG_WIDTH = 4


def make_case(B, F, m, bags=False, grid=False, seed=0):
    """float64 inputs of one shape: a 5-row-per-field table [R, 2 m], bias, labels in {0, 1}, weights, d_p, and ids: single-valued
    [B, F] with one id of -1, or (bags) [B, 4 F] where every bag holds 0, 1, 2 or 4 valid ids padded with -1.  Rows 3 and 4 of every
    field stay unreferenced.  Entries are scaled by 1 / sqrt(F) so that p and q stay inside [1e-4, 1 - 1e-4]; grid: integers in
    {-3 .. 3}, where the pooling is exact in fp32 for these bag sizes"""
    g = torch.Generator().manual_seed(613 * seed + 31 * B + 7 * F + m + (1 if bags else 0))
    R, W = ROWS_PER_FIELD * F, 2 * m
    if grid:
        table = torch.randint(-3, 4, (R, W), generator=g).double()
        bias = torch.randint(-3, 4, (W,), generator=g).double()
    else:
        table = (torch.randn(R, W, generator=g, dtype=torch.float64) / math.sqrt(F)).float().double()
        bias = (0.1 * torch.randn(W, generator=g, dtype=torch.float64)).float().double()
    if bags:
        ids = torch.randint(0, 3, (B, F, BAG_WIDTH), generator=g)
        n = torch.tensor(BAG_SIZES)[torch.randint(0, len(BAG_SIZES), (B, F), generator=g)]
        n[0, 0] = 0
        n[B - 1, F - 1] = 4
        ids = torch.where(torch.arange(BAG_WIDTH)[None, None, :] < n[:, :, None], ids, torch.full_like(ids, -1))
        fields = [ids[:, f, :] for f in range(F)]
        col_start = (BAG_WIDTH * torch.arange(F + 1)).to(torch.int32)
        flat = ids.reshape(B, F * BAG_WIDTH)
    else:
        flat = torch.randint(0, 3, (B, F), generator=g)
        flat[B // 2, F // 2] = -1
        fields = [flat[:, f:f + 1] for f in range(F)]
        col_start = None
    labels = torch.randint(0, 2, (B,), generator=g).double()
    wt = (0.5 + torch.rand(B, generator=g, dtype=torch.float64)).float().double()
    d_p = torch.randn(B, generator=g, dtype=torch.float64).float().double()
    return {"shape": (B, F, m), "table": table, "bias": bias, "ids": flat, "fields": fields, "col_start": col_start,
            "row_base": ROWS_PER_FIELD * torch.arange(F), "labels": labels, "wt": wt, "d_p": d_p}
