"""LS-PLM (Gai et al., Alibaba 2017, "Learning Piece-wise Linear Models from Large Scale Data for Ad Click Prediction"), also known as
MLR.  The reference's README lists it among its ranking models and ships no code for it; the model here follows the paper's eq. 2 with a
softmax gate and logistic experts:

    p(y = 1 | x) = sum_i softmax_i(u . x) * sigmoid(w_i . x)       over sparse x, i = 1 .. m regions

Every feature holds one row [u (m) | w (m)] of an EmbeddingSlab; the bag sum of the rows and the m-way head are one fused kernel
(csrc/lsplm.hip), and training is one pass: dr_lsplm_loss_fwd writes the loss and the rows' gradient, K4 applies it.

OUT OF SCOPE: the paper's L1 + L2,1 regulariser and its quasi-Newton (LBFGS / OWLQN-style) solver.  `train_step` is plain SGD on the
log-loss.  The package adds no torch.autograd.Function for this model; nothing here records an autograd graph."""
from typing import Dict

import torch
from torch import nn

from deep_recommenders_amd import feature_column as fc
from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops


class LSPLM(nn.Module):
    """LSPLM(indicator_columns, num_regions=12, initializer=None).call(inputs) -> prob [B, 1].

    `indicator_columns` name the categorical columns (the sparse x); multi-valued columns are mean-pooled as the slab pools them.  One
    EmbeddingSlab holds the rows, 2 * num_regions wide: the first half is the gate u, the second the expert w.  `bias` [2 m] (zeros) is
    the constant feature's row.  Rows are truncated normal with sigma = 0.5 unless `initializer(rows)` is given: all-equal gate rows
    would never separate the regions (every region would receive the same gradient).  num_regions must be even, in [2, 128].

    `call`, `predict` and `loss(inputs, labels)` return values.  `train_step(inputs, labels, lr)` is one SGD step on the mean log-loss."""

    def __init__(self, indicator_columns, num_regions: int = 12, initializer=None, device="cuda", **kwargs):
        super().__init__()
        if indicator_columns is None or len(indicator_columns) == 0:
            raise ValueError("LSPLM needs the indicator columns that name its sparse features")
        if int(num_regions) != num_regions or int(num_regions) % 2 != 0 or not 2 <= int(num_regions) <= 128:
            raise ValueError("`num_regions` should be an even integer in [2, 128]. Got {!r}".format(num_regions))
        if len(indicator_columns) > 1024:
            raise ValueError("LSPLM takes up to 1024 fields, got {}".format(len(indicator_columns)))
        self._indicator_columns = indicator_columns
        self._kwargs = kwargs
        self.m = int(num_regions)
        init = initializer if initializer is not None else (lambda rows: L.truncated_normal_(rows, 0.5))
        wide = [fc.embedding_column(c.categorical_column, 2 * self.m, initializer=init) for c in indicator_columns]
        self.slab = L.EmbeddingSlab(wide, device=device)
        self.F = len(self.slab.keys)
        self.bias = nn.Parameter(torch.zeros(2 * self.m, dtype=torch.float32, device=device))
        self._plan = None

    def _ids(self, inputs: Dict[str, object]):
        for key in self.slab.keys:
            if key not in inputs:
                raise ValueError("LSPLM needs every field in `inputs`: {!r} is missing".format(key))
        return self.slab.transform(inputs, self.slab.keys)

    def _vec(self, v, B, what):
        if v is None:
            return None
        v = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
        if v.numel() != B:
            raise ValueError("LSPLM: `{}` needs one value per example ({}), got {}".format(what, B, v.numel()))
        return v.to(self.bias.device)

    def call(self, inputs, **kwargs):
        ids, col_start, row_base = self._ids(inputs)
        p, _, _ = ops.lsplm_fwd(ids, self.F, col_start, row_base, self.slab.table.data, self.m, self.bias.data, want_z=False)
        return p.reshape(-1, 1)

    forward = call

    def predict(self, inputs):
        return self.call(inputs).cpu().numpy()

    def loss(self, inputs, labels, sample_weight=None):
        """the mean over the batch of -wt (y log p + (1 - y) log q), a value"""
        ids, col_start, row_base = self._ids(inputs)
        B = ids.shape[0]
        _, _, rows, _, _ = ops.lsplm_loss_fwd(ids, self.F, col_start, row_base, self.slab.table.data, self.m, self.bias.data,
                                              self._vec(labels, B, "labels"), self._vec(sample_weight, B, "sample_weight"), 1.0 / max(B, 1))
        return ops.reduce_sum(rows, alpha=1.0 / max(B, 1)).reshape(())

    def train_step(self, inputs, labels, lr, sample_weight=None, deterministic=False):
        """one SGD step on the mean loss: dr_lsplm_loss_fwd with row_scale = 1 / B, K4 with scale = -lr on the table, bias -= lr *
        colsum(d_z) (fixed-order reduction).  deterministic=True takes the sorted K4 (emb_sort_slots / emb_pool_bwd_sorted), whose
        slot plan is [B, F]: single-valued inputs only.  Returns the mean loss [] as the step found it."""
        ids, col_start, row_base = self._ids(inputs)
        if deterministic and (col_start is not None or self.F > 64):
            raise ValueError("LSPLM.train_step(deterministic=True) needs single-valued inputs and at most 64 fields: the slot plan is "
                             "[B, F]")
        B, F, W = ids.shape[0], self.F, 2 * self.m
        table = self.slab.table.data
        _, _, rows, d_z, d_rows = ops.lsplm_loss_fwd(ids, F, col_start, row_base, table, self.m, self.bias.data,
                                                     self._vec(labels, B, "labels"), self._vec(sample_weight, B, "sample_weight"),
                                                     1.0 / max(B, 1))
        loss = ops.reduce_sum(rows, alpha=1.0 / max(B, 1)).reshape(())
        if B == 0:
            return loss
        if deterministic:
            self._plan = L.sgns_apply_rows(table, ids, d_rows, -float(lr), plan=self._plan if self._plan is not None else
                                           ops.SortPlan(B * F, ids.device), row_base=row_base)
        else:
            if col_start is None:
                col_start = torch.arange(F + 1, dtype=torch.int32, device=ids.device)
            ops.emb_pool_bwd(ids, F, col_start, row_base, W, d_rows, None, None, None, -float(lr), table, None, None)
        ops.axpy(-float(lr), ops.lsplm_bias_grad(d_z, self.m), self.bias.data)
        return loss

    def get_config(self):
        config = {"num_regions": self.m}
        return {**self._kwargs, **config}
