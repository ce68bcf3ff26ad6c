"""PNN (Qu et al., ICDM 2016, "Product-based Neural Networks for User Response Prediction").  The reference's README lists PNN among its
ranking models and ships no code for it; the model here follows the paper and is built like dlrm.py: one EmbeddingSlab for the tables,
Dense layers on layers.mlp, the inner products on DotInteraction, and the outer-product layer as fused kernels each way
(dr_pnn_outer_fwd / dr_pnn_outer_bwd, csrc/pnn_outer.hip)."""
from typing import Dict

import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import losses
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.ranking.dlrm import DotInteraction


class OuterProduct(nn.Module):
    """OuterProduct(units)(embeddings, addend=None) -> [B, units].

    embeddings [B, F, D].  With u = sum_i e_i (the paper's superposition, eq. 15-16) the output is
    l_p[n] = sum_{d,e} u_d u_e W[d * D + e, n] (+ addend[n]): the flattened outer product u u^T times W [D * D, units], the full square in
    row-major order.  W is glorot-uniform and created on the first call.  The [B, D * D] matrix is never built."""

    def __init__(self, units: int, **kwargs):
        super().__init__()
        if int(units) != units or not 1 <= int(units) <= 4096:
            raise ValueError("`units` should be an integer in [1, 4096]. Got {!r}".format(units))
        self._units = int(units)
        self._kwargs = kwargs
        self.built = False

    def build(self, input_shape, device="cuda"):
        if len(input_shape) != 3:
            raise ValueError("`embeddings` dim should be 3. Got `embeddings` dim = {}".format(len(input_shape)))
        D = int(input_shape[2])
        W = torch.empty((D * D, self._units), dtype=torch.float32, device=device)
        L.glorot_uniform_(W)
        self.W = nn.Parameter(W)
        self.built = True

    def call(self, embeddings, addend=None, **kwargs):
        embeddings = torch.as_tensor(embeddings, dtype=torch.float32)
        if embeddings.dim() != 3:
            raise ValueError("`embeddings` dim should be 3. Got `embeddings` dim = {}".format(embeddings.dim()))
        embeddings = embeddings.cuda()
        if not self.built:
            self.build(tuple(embeddings.shape), embeddings.device)
        if addend is not None:
            addend = torch.as_tensor(addend, dtype=torch.float32).cuda()
            if addend.dim() != 2 or addend.shape[1] != self._units:
                raise ValueError("`addend` should be [B, {}]. Got shape = {}".format(self._units, tuple(addend.shape)))
        return L.pnn_outer(embeddings, self.W, addend)

    forward = call

    def get_config(self):
        config = {"units": self._units}
        return {**self._kwargs, **config}


class PNN(nn.Module):
    """PNN(embedding_columns, dnn_units_size, use_inner=True, use_outer=False, self_interaction=False, activation="relu").call(inputs)
    -> prob = sigmoid(Dense(1)(Dense(u, act) ... (l1))) with the paper's product layer

        l1 = act(z W_z + [use_inner: DotInteraction(self_interaction)(E) W_in] + [use_outer: OuterProduct(D1)(E)] + b1)

    over z = the concatenated embeddings and D1 = dnn_units_size[0]; the remaining sizes are plain Dense layers.  use_inner alone is
    IPNN, use_outer alone OPNN, both PNN*.  Kernels are glorot-uniform, biases zero.  One EmbeddingSlab holds the tables (no linear
    term); `model.slab.sparse_lr = lr` applies fused SGD to the looked-up rows."""

    def __init__(self, embedding_columns, dnn_units_size, use_inner: bool = True, use_outer: bool = False, self_interaction: bool = False,
                 activation="relu", device="cuda", **kwargs):
        super().__init__()
        if activation not in ops.ACT_CODES:
            raise ValueError("activation must be one of {}, got {!r}".format(sorted(k for k in ops.ACT_CODES if k), activation))
        if not use_inner and not use_outer:
            raise ValueError("PNN needs a product layer: at least one of `use_inner` and `use_outer`")
        if dnn_units_size is None or len(dnn_units_size) == 0:
            raise ValueError("`dnn_units_size` should name at least the width of the product layer")
        self._embedding_columns = embedding_columns
        self._dnn_units_size = [int(u) for u in dnn_units_size]
        self._use_inner, self._use_outer = bool(use_inner), bool(use_outer)
        self._activation = activation
        self._kwargs = kwargs
        self.slab = L.EmbeddingSlab(embedding_columns, device=device)
        if self._use_outer and self.slab.D > 128:
            raise ValueError("the outer-product layer takes embedding dimensions up to 128, got {}".format(self.slab.D))
        self.interaction = DotInteraction(self_interaction)
        self.outer = OuterProduct(self._dnn_units_size[0]) if self._use_outer else None
        self.w_z = None
        self.w_inner = None
        self.kernels, self.biases = nn.ParameterList(), nn.ParameterList()
        self._built = False

    @staticmethod
    def _kernel(rows, cols, device):
        W = torch.empty((rows, cols), dtype=torch.float32, device=device)
        L.glorot_uniform_(W)
        return nn.Parameter(W)

    def _build(self, num_fields, device):
        D, D1 = self.slab.D, self._dnn_units_size[0]
        self.w_z = self._kernel(num_fields * D, D1, device)
        if self._use_inner:
            width = ops.dot_interact_width(num_fields, D, False, self.interaction._self_interaction)
            self.w_inner = self._kernel(width, D1, device)
        self.b1 = nn.Parameter(torch.zeros(D1, dtype=torch.float32, device=device))
        d = D1
        for u in self._dnn_units_size[1:] + [1]:
            self.kernels.append(self._kernel(d, u, device))
            self.biases.append(nn.Parameter(torch.zeros(u, dtype=torch.float32, device=device)))
            d = u
        self._built = True

    def _field_keys(self, inputs: Dict[str, object]):
        return [k for k in inputs.keys() if k in self.slab.columns]

    def logits(self, inputs):
        keys = self._field_keys(inputs)
        F, D = len(keys), self.slab.D
        act = ops.ACT_CODES[self._activation]
        concat, _, _ = self.slab(inputs, keys, second_order=False)   # [B, F * D]: the gathered rows, field-major
        if not self._built:
            self._build(F, concat.device)
        z = concat[:, :F * D]
        e = z.reshape(-1, F, D)                                      # the same rows viewed per field, read in place
        pre = L.mlp(z, [self.w_z], [self.b1], [0])
        if self._use_inner:
            pre = pre + L.mlp(self.interaction(e), [self.w_inner], [None], [0])
        if self._use_outer:
            pre = self.outer(e, pre)                                 # l_z + l_inner + b1 ride in as the kernel's addend
        l1 = L.activation(pre, act)
        return L.mlp(l1, list(self.kernels), list(self.biases), [act] * (len(self.kernels) - 1) + [0])

    def call(self, inputs, **kwargs):
        return losses.sigmoid(self.logits(inputs))

    forward = call

    def predict(self, inputs):
        with torch.no_grad():
            return self.call(inputs).cpu().numpy()

    def get_config(self):
        config = {"dnn_units_size": self._dnn_units_size, "use_inner": self._use_inner, "use_outer": self._use_outer,
                  "self_interaction": self.interaction._self_interaction, "activation": self._activation}
        return {**self._kwargs, **config}
