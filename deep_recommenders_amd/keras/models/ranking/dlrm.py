"""DLRM (Naumov et al. 2019, "Deep Learning Recommendation Model for Personalization and Recommendation Systems").  The reference's
README lists DLRM among the models it plans and ships no code for it; the model here follows the paper and is built like xdeepfm.py:
one EmbeddingSlab for the tables, Dense towers on layers.mlp, and the paper's pairwise dot interaction as one fused kernel each way
(dr_dot_interact_fwd / dr_dot_interact_bwd, csrc/dot_interact.hip)."""
from typing import Dict, Optional

import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import losses
from deep_recommenders_amd import ops


class DotInteraction(nn.Module):
    """DotInteraction(self_interaction=False)(embeddings, dense=None) -> [B, c0 + P].

    embeddings [B, F, D]; dense [B, D] or None.  With T = [dense; the F embeddings] (N rows) the output is dense itself in the first
    c0 = D columns (c0 = 0 without it) followed by the row-major lower triangle of T T^T: <t_i, t_j> for j < i, or j <= i with
    self_interaction, the order of the DLRM paper's code.  The [B, N, N] matrix is never built."""

    def __init__(self, self_interaction: bool = False, **kwargs):
        super().__init__()
        self._self_interaction = bool(self_interaction)
        self._kwargs = kwargs

    def call(self, embeddings, dense=None, **kwargs):
        embeddings = torch.as_tensor(embeddings, dtype=torch.float32)
        if embeddings.dim() != 3:
            raise ValueError("`embeddings` dim should be 3. Got `embeddings` dim = {}".format(embeddings.dim()))
        embeddings = embeddings.cuda()
        if dense is not None:
            dense = torch.as_tensor(dense, dtype=torch.float32).cuda()
            if dense.dim() != 2 or dense.shape[1] != embeddings.shape[2]:
                raise ValueError("`dense` should be [B, {}]. Got shape = {}".format(embeddings.shape[2], tuple(dense.shape)))
        return L.dot_interaction(dense, embeddings, self._self_interaction)

    forward = call

    def get_config(self):
        config = {"self_interaction": self._self_interaction}
        return {**self._kwargs, **config}


class DLRM(nn.Module):
    """DLRM(embedding_columns, bottom_units_size, top_units_size, dense_features_key, activation="relu", self_interaction=False).call(inputs)
    -> prob = sigmoid(top(DotInteraction(embeddings, bottom(dense)))).

    bottom: Sequential(Dense(u, act) for u in bottom_units_size) on the float [B, Nd] feature `dense_features_key`; its last width must
    equal the embedding dimension.  top: Sequential(Dense(u, act) for u in top_units_size, Dense(1)).  Kernels are glorot-uniform, biases
    zero.  One EmbeddingSlab holds the tables (no linear term); `model.slab.sparse_lr = lr` applies fused SGD to the looked-up rows.
    `dense_features_key=None`: the embedding-only variant, without the bottom tower."""

    def __init__(self, embedding_columns, bottom_units_size, top_units_size, dense_features_key: Optional[str], activation="relu",
                 self_interaction: bool = False, device="cuda", **kwargs):
        super().__init__()
        if activation not in ops.ACT_CODES:
            raise ValueError("activation must be one of {}, got {!r}".format(sorted(k for k in ops.ACT_CODES if k), activation))
        self._embedding_columns = embedding_columns
        self._bottom_units_size = [] if dense_features_key is None else [int(u) for u in bottom_units_size]
        self._top_units_size = [int(u) for u in top_units_size]
        self._activation = activation
        self._dense_key = dense_features_key
        self._kwargs = kwargs
        self.slab = L.EmbeddingSlab(embedding_columns, device=device)
        if dense_features_key is not None and (len(self._bottom_units_size) == 0 or self._bottom_units_size[-1] != self.slab.D):
            raise ValueError("the bottom tower's output is interacted with the embeddings: the last of `bottom_units_size` must equal the "
                             "embedding dimension {}, got {!r}".format(self.slab.D, list(bottom_units_size)))
        self.interaction = DotInteraction(self_interaction)
        self.bottom_kernels, self.bottom_biases = nn.ParameterList(), nn.ParameterList()
        self.top_kernels, self.top_biases = nn.ParameterList(), nn.ParameterList()
        self._built = False

    @staticmethod
    def _tower(in_dim, units, kernels, biases, device):
        d = in_dim
        for u in units:                                          # glorot-uniform kernel, zero bias, as DeepFM's
            W = torch.empty((d, u), dtype=torch.float32, device=device)
            L.glorot_uniform_(W)
            kernels.append(nn.Parameter(W))
            biases.append(nn.Parameter(torch.zeros(u, dtype=torch.float32, device=device)))
            d = u

    def _build(self, num_dense, num_fields, device):
        if self._dense_key is not None:
            self._tower(num_dense, self._bottom_units_size, self.bottom_kernels, self.bottom_biases, device)
        width = ops.dot_interact_width(num_fields, self.slab.D, self._dense_key is not None, self.interaction._self_interaction)
        self._tower(width, self._top_units_size + [1], self.top_kernels, self.top_biases, device)
        self._built = True

    def _field_keys(self, inputs: Dict[str, object]):
        return [k for k in inputs.keys() if k in self.slab.columns]

    def logits(self, inputs):
        keys = self._field_keys(inputs)
        F, D = len(keys), self.slab.D
        act = ops.ACT_CODES[self._activation]
        x = None
        if self._dense_key is not None:
            x = torch.as_tensor(inputs[self._dense_key], dtype=torch.float32).to(self.slab.table.device)
        concat, _, _ = self.slab(inputs, keys, second_order=False)   # [B, F * D]: the gathered rows, field-major
        if not self._built:
            self._build(0 if x is None else x.shape[1], F, concat.device)
        bottom = None
        if x is not None:
            bottom = L.mlp(x, list(self.bottom_kernels), list(self.bottom_biases), [act] * len(self.bottom_kernels))
        z = self.interaction(concat.reshape(-1, F, D), bottom)       # the same rows viewed per field, read in place
        return L.mlp(z, list(self.top_kernels), list(self.top_biases), [act] * len(self._top_units_size) + [0])

    def call(self, inputs, **kwargs):
        return losses.sigmoid(self.logits(inputs))

    forward = call

    def predict(self, inputs):
        with torch.no_grad():
            return self.call(inputs).cpu().numpy()

    def get_config(self):
        config = {"bottom_units_size": self._bottom_units_size, "top_units_size": self._top_units_size,
                  "dense_features_key": self._dense_key, "activation": self._activation,
                  "self_interaction": self.interaction._self_interaction}
        return {**self._kwargs, **config}
