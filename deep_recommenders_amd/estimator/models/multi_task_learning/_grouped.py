"""G parallel dense stacks of one shape (MMoE's experts and task towers, ESMM's two towers) run as grouped launches.

Storage: the first layer of a stack over a SHARED input is one concatenated kernel [K, G*N0] (+ bias [G*N0]) and runs as one
dr_linear_fwd; every other layer is [G, K_i, N_i] (+ [G, N_i]) and runs as one dr_linear_*_grouped launch whose groups read and
write the [B, G*N] row layout of the layer before.  The TF variables (`<scope>/dense{,_1,...}/{kernel,bias}`) are views of these
buffers: column slices of the concatenated kernel, slabs of the grouped ones."""
import torch

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops

ACT_CODES = {"relu": 1, "sigmoid": 2, "tanh": 3}


def act_code(activation):
    if activation is None:
        return 0
    name = activation if isinstance(activation, str) else getattr(activation, "__name__", "")
    if name not in ACT_CODES:
        raise ValueError("activation must be relu / sigmoid / tanh / None, got {!r}".format(activation))
    return ACT_CODES[name]


class GroupedStack:
    """Parameters and launches of G stacks `in_dim -> units[0] -> ... -> units[-1]`; hidden layers (all but the last) take `act`
    and dropout.  shared_input: the first layer reads one [B, in_dim] input (concatenated kernel); otherwise group g reads
    columns g*in_dim .. of a [B, G*in_dim] input."""

    def __init__(self, G, in_dim, units, act, dropout, shared_input, device):
        self.G, self.units, self.act, self.dropout, self.shared = G, list(units), act, dropout, shared_input
        self.dims = [in_dim] + self.units
        self.W, self.b = [], []
        for i, n in enumerate(self.units):
            k = self.dims[i]
            if i == 0 and shared_input:
                W = torch.empty((k, G * n), dtype=torch.float32, device=device)
                b = torch.zeros(G * n, dtype=torch.float32, device=device)
            else:
                W = torch.empty((G, k, n), dtype=torch.float32, device=device)
                b = torch.zeros((G, n), dtype=torch.float32, device=device)
            self.W.append(W)
            self.b.append(b)
        self.views = None

    def make_views(self):
        """[(layer, group, kernel view, bias view)] in layer-major order; every view shares storage with the buffers"""
        out = []
        for i, n in enumerate(self.units):
            for g in range(self.G):
                if i == 0 and self.shared:
                    out.append((i, g, self.W[i][:, g * n:(g + 1) * n], self.b[i][g * n:(g + 1) * n]))
                else:
                    out.append((i, g, self.W[i][g], self.b[i][g]))
        return out

    def init_glorot(self, kernels):
        for W in kernels:                  # [TF] B8 per TF variable (fan_in, fan_out of that layer)
            L.glorot_uniform_(W)

    # ---- forward --------------------------------------------------------------------------------------------------------------
    def forward(self, x, seed_fn=None):
        """x [B, in_dim] (shared) or [B, G*in_dim] -> (y [B, G*units[-1]], saved)"""
        B, G = x.shape[0], self.G
        n_layers = len(self.units)
        ins, acts_out, masks = [x], [], []
        h = x
        for i, n in enumerate(self.units):
            k = self.dims[i]
            last = i == n_layers - 1
            act = 0 if last else self.act
            y = torch.empty((B, G * n), dtype=torch.float32, device=x.device)
            if i == 0 and self.shared:
                ops.linear_fwd(h, self.W[0], self.b[0], 1 if act == 1 else 0, out=y)
            else:
                ops.linear_fwd_grouped(h, h.stride(0), k, self.W[i], n, k * n, self.b[i], n, B, k, n, G, 1 if act == 1 else 0,
                                       y, G * n, n)
            if act in (2, 3):
                ops.act_fwd_(y, act)
            acts_out.append(y)
            mask = None
            if not last and self.dropout is not None:
                y, mask = ops.dropout_fwd(y, self.dropout, seed_fn())      # rows keep their own pitch
            masks.append(mask)
            if not last:
                ins.append(y)
            h = y
        return h, (ins, acts_out, masks)

    # ---- backward -------------------------------------------------------------------------------------------------------------
    def backward(self, d_y, saved, need_dx):
        """d_y [B, G*units[-1]] -> (gW list, gb list, d_x or None).  Gradient buffers have the shape of the parameter buffers."""
        ins, acts_out, masks = saved
        B, G = d_y.shape[0], self.G
        n_layers = len(self.units)
        gW = [None] * n_layers
        gb = [None] * n_layers
        dy = d_y
        for i in range(n_layers - 1, -1, -1):
            k, n = self.dims[i], self.units[i]
            last = i == n_layers - 1
            if not last:
                # dy is the gradient of this hidden layer's (dropped-out) output, relu' already folded in by the dx above
                if masks[i] is not None:
                    dy = ops.dropout_bwd(dy, masks[i], self.dropout)
                if self.act in (2, 3):
                    ops.act_bwd_(acts_out[i], dy, self.act)
            x = ins[i]
            gW[i] = torch.zeros_like(self.W[i])
            gb[i] = torch.zeros_like(self.b[i])
            if i == 0 and self.shared:
                ws = ops.linear_bwd_dw_workspace(B, k, G * n, x.device)
                ops.linear_bwd_dw(x, dy, 1.0, gW[i], gb[i], workspace=ws)
            else:
                ws = ops.linear_bwd_dw_grouped_workspace(B, k, n, G, x.device)
                ops.linear_bwd_dw_grouped(x, x.stride(0), k, dy, dy.stride(0), n, B, k, n, G, 1.0, gW[i], n, k * n, gb[i], n,
                                          workspace=ws)
            if i == 0 and not need_dx:
                dy = None
                break
            relu_src = ins[i] if (i > 0 and self.act == 1) else None
            if i == 0 and self.shared:
                dy = ops.linear_bwd_dx(dy, self.W[0])
            else:
                dx = torch.empty((B, G * k), dtype=torch.float32, device=dy.device)
                ops.linear_bwd_dx_grouped(dy, dy.stride(0), n, self.W[i], n, k * n, B, k, n, G, relu_src,
                                          relu_src.stride(0) if relu_src is not None else 0, k, False, dx, G * k, k)
                dy = dx
        return gW, gb, dy


def grad_views(stack, gW, gb, active):
    """per-(layer, group) gradients as views of the gradient buffers, None for groups outside `active`"""
    out = []
    for i, n in enumerate(stack.units):
        for g in range(stack.G):
            if g not in active:
                out += [None, None]
            elif i == 0 and stack.shared:
                out += [gW[i][:, g * n:(g + 1) * n], gb[i][g * n:(g + 1) * n]]
            else:
                out += [gW[i][g], gb[i][g]]
    return out


def check_views(params, views):
    for p, v in zip(params, views):
        if p.data_ptr() != v.data_ptr() or p.stride() != v.stride():
            raise RuntimeError("a multi-task parameter no longer aliases its grouped buffer (was .data replaced?); copy values in "
                               "place (import_variables / p.data.copy_) instead")
