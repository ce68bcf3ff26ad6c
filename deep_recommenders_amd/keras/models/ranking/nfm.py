"""NFM (He & Chua, SIGIR 2017, "Neural Factorization Machines for Sparse Predictive Analytics").  The reference's README lists NFM among
its ranking models and ships no code for it; the model here follows the paper and is built like ffm.py: one EmbeddingSlab for the tables
and the linear term, and the paper's Bi-Interaction pooling as one fused kernel each way (csrc/bi_interaction.hip).  For single-valued
fields the pooled vector is computed straight from the table rows (dr_bi_interact_gather_fwd) and the gathered rows are never written.

The package adds no torch.autograd.Function for it: `train_step` drives the kernels explicitly, as YoutubeNet, EBR and GraphSAGE do.
Batch normalisation inside the tower (the paper's optional BN) is not here."""
from typing import Dict

import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import losses
from deep_recommenders_amd import ops


class BiInteraction(nn.Module):
    """BiInteraction().call(rows) -> [B, D] = 0.5 ((sum_f e_f)^2 - sum_f e_f^2), the sum over the pairs of fields of e_i * e_j.

    rows [B, F, D] or [B, F * D] (then `num_fields` names F).  `call` returns a VALUE: no autograd graph is recorded, the transpose is
    explicit: `backward(rows, d_out) -> d_rows` = d_out * (sum_g e_g - e_f), with the sum recomputed.  No [B, F, D] square is built."""

    def __init__(self, **kwargs):
        super().__init__()
        self._kwargs = kwargs

    @staticmethod
    def _shape(rows, num_fields):
        rows = torch.as_tensor(rows, dtype=torch.float32)
        if rows.dim() == 3:
            F, D = int(rows.shape[1]), int(rows.shape[2])
        elif rows.dim() == 2:
            if num_fields is None or int(num_fields) < 1 or rows.shape[1] % int(num_fields) != 0 or rows.shape[1] == 0:
                raise ValueError("`rows` [B, F * D] needs `num_fields` = F dividing its width. Got shape {} and num_fields = {!r}"
                                 .format(tuple(rows.shape), num_fields))
            F = int(num_fields)
            D = int(rows.shape[1]) // F
        else:
            raise ValueError("`rows` dim should be 2 or 3. Got `rows` dim = {}".format(rows.dim()))
        ops._bi_dims(F, D)                                     # the kernel's domain, checked before anything moves to the device
        return rows, F, D

    def call(self, rows, num_fields=None, **kwargs):
        rows, F, D = self._shape(rows, num_fields)
        rows = rows.detach().cuda()
        return ops.bi_interaction_fwd(rows if rows.dim() == 2 else rows.contiguous(), F, D)

    forward = call

    def backward(self, rows, d_out, num_fields=None):
        rows, F, D = self._shape(rows, num_fields)
        rows = rows.detach().cuda()
        d_out = torch.as_tensor(d_out, dtype=torch.float32).detach().cuda()
        d_rows = ops.bi_interaction_bwd(rows if rows.dim() == 2 else rows.contiguous(), F, D, d_out)
        return d_rows.view(-1, F, D) if rows.dim() == 3 else d_rows

    def get_config(self):
        return dict(self._kwargs)


class NFM(nn.Module):
    """NFM(indicator_columns, embedding_columns, dnn_units_size, activation="relu", dropout=0.0, bi_dropout=0.0).call(inputs)
    -> prob = sigmoid(first_order + Dense(1, use_bias=False)(MLP(dropout(BiInteraction(embeddings))))).

    One EmbeddingSlab holds the tables and the linear term with the model's only output bias.  The fields are numbered in the order of
    `embedding_columns` (= `model.slab.keys`).  The tower's kernels are glorot-uniform, its biases zero; `bi_dropout` is applied to the
    pooled vector and `dropout` after every hidden layer while `model.training` (layers.dropout, a fresh mask per call).  Multi-valued
    fields are mean-pooled by the slab and the pooled row is the field's row; a missing id is a row of zeros.

    `logits`, `call` and `predict` run the forward kernels and return values as far as the slab is concerned: GRADIENTS REACH THE DENSE
    PARAMETERS THROUGH AUTOGRAD BUT DO NOT REACH THE SLAB (table, lin_w, lin_bias).  `train_step` is the way to train: it runs the
    backward kernels explicitly and honours `model.slab.sparse_lr` (None: dense .grad on the slab's parameters for any torch
    optimizer; a value: fused SGD in place)."""

    def __init__(self, indicator_columns, embedding_columns, dnn_units_size, activation="relu", dropout: float = 0.0,
                 bi_dropout: float = 0.0, device="cuda", **kwargs):
        super().__init__()
        if indicator_columns is None or len(indicator_columns) == 0:
            raise ValueError("NFM needs the indicator columns of its linear term")
        if activation not in ops.ACT_CODES:
            raise ValueError("activation must be one of {}, got {!r}".format(sorted(k for k in ops.ACT_CODES if k), activation))
        if dnn_units_size is None or len(dnn_units_size) == 0 or any(int(u) < 1 for u in dnn_units_size):
            raise ValueError("`dnn_units_size` should name at least one hidden layer of positive width. Got {!r}".format(dnn_units_size))
        for name, rate in (("dropout", dropout), ("bi_dropout", bi_dropout)):
            if not 0.0 <= float(rate) < 1.0:
                raise ValueError("`{}` should be in [0, 1). Got {!r}".format(name, rate))
        if len(embedding_columns) > 1024:
            raise ValueError("NFM takes up to 1024 fields, got {}".format(len(embedding_columns)))
        self._indicator_columns = indicator_columns
        self._embedding_columns = embedding_columns
        self._dnn_units_size = [int(u) for u in dnn_units_size]
        self._activation = activation
        self._dropout, self._bi_dropout = float(dropout), float(bi_dropout)
        self._dropout_calls = 0
        self._kwargs = kwargs
        self.slab = L.EmbeddingSlab(embedding_columns, indicator_columns, device=device)
        self.F, self.D = len(self.slab.keys), self.slab.D
        self.interaction = BiInteraction()
        self.kernels, self.biases = nn.ParameterList(), nn.ParameterList()
        d = self.D
        for u in self._dnn_units_size:
            self.kernels.append(self._kernel(d, u, device))
            self.biases.append(nn.Parameter(torch.zeros(u, dtype=torch.float32, device=device)))
            d = u
        self.w_out = self._kernel(d, 1, device)

    @staticmethod
    def _kernel(rows, cols, device):
        W = torch.empty((rows, cols), dtype=torch.float32, device=device)
        L.glorot_uniform_(W)
        return nn.Parameter(W)

    # ---- the slab's side: values, no graph --------------------------------------------------------------------------------------------
    def _gathered(self, inputs: Dict[str, object]):
        """(bi [B, D], first_order [B], state) by the forward kernels; `state` is what the backward needs.  The slab's autograd graph is
        recorded only on the rows path (multi-valued fields), where K3 writes `concat` and train_step differentiates through it."""
        for key in self.slab.keys:
            if key not in inputs:
                raise ValueError("NFM needs every field in `inputs`: {!r} is missing".format(key))
        slab, F, D = self.slab, self.F, self.D
        ids, col_start, row_base = slab.transform(inputs, slab.keys)
        if col_start is None:                                  # every field single-valued: straight from the table
            bi, first = ops.bi_interaction_gather_fwd(ids, row_base, slab.table.data, F, D, slab.lin_w.data, slab.lin_bias.data)
            return bi, first, ("gather", ids, row_base)
        concat, first, _ = slab(inputs, slab.keys, second_order=False)         # [B, F * D]: the pooled rows, field-major
        bi = ops.bi_interaction_fwd(concat.detach(), F, D)                     # read in place
        return bi, first.detach(), ("rows", concat, first)

    # ---- the tower: autograd over existing Functions -------------------------------------------------------------------------------------
    def _drop(self, x, rate):
        if rate > 0.0 and self.training:
            self._dropout_calls += 1
            return L.dropout(x, rate, self._dropout_calls)
        return x

    def _tower(self, bi, first):
        act = ops.ACT_CODES[self._activation]
        h = self._drop(bi, self._bi_dropout)
        for W, b in zip(self.kernels, self.biases):
            h = self._drop(L.mlp(h, [W], [b], [act]), self._dropout)
        return first.reshape(-1, 1) + L.mlp(h, [self.w_out], [None], [0])

    def logits(self, inputs):
        if torch.is_grad_enabled():
            with torch.no_grad():
                bi, first, _ = self._gathered(inputs)
        else:
            bi, first, _ = self._gathered(inputs)
        return self._tower(bi, first)

    def call(self, inputs, **kwargs):
        return losses.sigmoid(self.logits(inputs))

    forward = call

    def predict(self, inputs):
        with torch.no_grad():
            return self.call(inputs).cpu().numpy()

    # ---- training --------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _accumulate(param, grad):
        param.grad = grad if param.grad is None else param.grad + grad

    def _loss(self, logits, labels, sample_weight):
        """the package's sigmoid cross-entropy, mean over the batch; with `sample_weight` sum_b w_b loss_b / B, taken as the two-class
        softmax cross-entropy of the logits [0, x], which is the same function of x"""
        B = logits.shape[0]
        y = torch.as_tensor(labels, dtype=torch.float32).to(logits.device).reshape(B, 1)
        if sample_weight is None:
            return losses.sigmoid_cross_entropy(y, logits)
        w = torch.as_tensor(sample_weight, dtype=torch.float32).to(logits.device).reshape(B) / B
        two = torch.cat([torch.zeros_like(logits), logits], dim=1)
        return losses._SoftmaxCEFn.apply(two.contiguous(), torch.cat([1.0 - y, y], dim=1).contiguous(), w.contiguous()).reshape(())

    def train_step(self, inputs, labels, optimizer=None, sample_weight=None):
        """one step: the gather (or K3 + rows) forward, the tower and the sigmoid cross-entropy under autograd with the pooled vector and
        the first-order term as leaves, dr_bi_interact_*_bwd on the pooled vector's gradient, then K4 (one dr_emb_pool_bwd call on the
        gather path, K3's own backward on the rows path).  `slab.sparse_lr` None fills table.grad, lin_w.grad and lin_bias.grad densely;
        a value applies fused SGD in place.  optimizer.step() if one is given.  Returns the mean loss [] as the step found it."""
        slab, F, D = self.slab, self.F, self.D
        if optimizer is not None:
            optimizer.zero_grad(set_to_none=True)
        bi, first, state = self._gathered(inputs)
        bi, first = bi.requires_grad_(), first.requires_grad_()
        loss = self._loss(self._tower(bi, first), labels, sample_weight)
        loss.backward()
        if state[0] == "gather":
            _, ids, row_base = state
            d_rows = ops.bi_interaction_gather_bwd(ids, row_base, slab.table.data, F, D, bi.grad)
            col_start = torch.arange(F + 1, dtype=torch.int32, device=ids.device)
            d_first = first.grad.contiguous()
            if slab.sparse_lr is None:
                g_table, g_lin = L._param_grad(slab.table), L._param_grad(slab.lin_w)
                g_bias = torch.zeros(1, dtype=torch.float32, device=ids.device)
                ops.emb_pool_bwd(ids, F, col_start, row_base, D, d_rows, None, None, d_first, 1.0, g_table, g_lin, g_bias)
                self._accumulate(slab.table, g_table)
                self._accumulate(slab.lin_w, g_lin)
                self._accumulate(slab.lin_bias, g_bias)
            else:
                ops.emb_pool_bwd(ids, F, col_start, row_base, D, d_rows, None, None, d_first, -float(slab.sparse_lr), slab.table.data,
                                 slab.lin_w.data, slab.lin_bias.data)
        else:
            _, concat, first_graph = state
            d_rows = ops.bi_interaction_bwd(concat.detach(), F, D, bi.grad)
            torch.autograd.backward([concat, first_graph], [d_rows, first.grad])     # K4, with sparse_lr as the slab applies it
        if optimizer is not None:
            optimizer.step()
        return loss.detach()

    def get_config(self):
        config = {"dnn_units_size": self._dnn_units_size, "activation": self._activation, "dropout": self._dropout,
                  "bi_dropout": self._bi_dropout}
        return {**self._kwargs, **config}
