"""AFM (Xiao et al., IJCAI 2017, "Attentional Factorization Machines: Learning the Weight of Feature Interactions via Attention
Networks").  The reference's README lists AFM among its ranking models and ships no code for it; the model here follows the paper and is
built like xdeepfm.py: one EmbeddingSlab for the tables and the linear term, and the paper's attention-based pooling of the pairwise
products as one fused kernel each way (dr_afm_pool_fwd / dr_afm_pool_bwd, csrc/afm_pool.hip)."""
from typing import Dict

import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import losses


class AttentionalPooling(nn.Module):
    """AttentionalPooling(attention_factor)(embeddings, want_attention=False) -> [B, D]  (or ([B, D], [B, P]) with want_attention).

    embeddings [B, F, D].  For every pair of fields (i, j), j < i, numbered q = i (i - 1) / 2 + j as DotInteraction numbers them:
    p_q = e_i * e_j, s_q = h^T relu(W^T p_q + b), a = softmax over the P = F (F - 1) / 2 pairs, output = sum_q a_q p_q (the paper's
    eq. 4-5 before the projection).  W [D, attention_factor] and h [attention_factor] are glorot-uniform, b zeros; they are created on
    the first call.  Neither the pair products [B, P, D] nor the hidden layer [B, P, attention_factor] is ever built; the attention
    weights are returned on request and carry no gradient."""

    def __init__(self, attention_factor: int = 8, **kwargs):
        super().__init__()
        if int(attention_factor) != attention_factor or not 1 <= int(attention_factor) <= 128:
            raise ValueError("`attention_factor` should be an integer in [1, 128]. Got {!r}".format(attention_factor))
        self._attention_factor = int(attention_factor)
        self._kwargs = kwargs
        self.built = False

    def build(self, input_shape, device="cuda"):
        if len(input_shape) != 3:
            raise ValueError("`embeddings` dim should be 3. Got `embeddings` dim = {}".format(len(input_shape)))
        D, A = int(input_shape[2]), self._attention_factor
        W = torch.empty((D, A), dtype=torch.float32, device=device)
        L.glorot_uniform_(W)
        h = torch.empty((A, 1), dtype=torch.float32, device=device)
        L.glorot_uniform_(h)
        self.W = nn.Parameter(W)
        self.b = nn.Parameter(torch.zeros(A, dtype=torch.float32, device=device))
        self.h = nn.Parameter(h.reshape(A))
        self.built = True

    def call(self, embeddings, want_attention: bool = False, **kwargs):
        embeddings = torch.as_tensor(embeddings, dtype=torch.float32)
        if embeddings.dim() != 3:
            raise ValueError("`embeddings` dim should be 3. Got `embeddings` dim = {}".format(embeddings.dim()))
        embeddings = embeddings.cuda()
        if not self.built:
            self.build(tuple(embeddings.shape), embeddings.device)
        out, attn = L.afm_pooling(embeddings, self.W, self.b, self.h, want_attention)
        return (out, attn) if want_attention else out

    forward = call

    def get_config(self):
        config = {"attention_factor": self._attention_factor}
        return {**self._kwargs, **config}


class AFM(nn.Module):
    """AFM(indicator_columns, embedding_columns, attention_factor=8, dropout=0.0).call(inputs)
    -> prob = sigmoid(linear(indicator) + Dense(1, use_bias=False)(dropout(AttentionalPooling(stacked embeddings)))).

    One EmbeddingSlab holds the tables and the linear term with the model's only output bias; the projection `w_out` [D, 1] is
    glorot-uniform (the paper's p).  `dropout` is applied to the pooled vector while `model.training` (layers.dropout, a fresh mask per
    call); `model.slab.sparse_lr = lr` applies fused SGD to the looked-up rows.  `attention(inputs)` returns the [B, P] weights."""

    def __init__(self, indicator_columns, embedding_columns, attention_factor: int = 8, dropout: float = 0.0, device="cuda", **kwargs):
        super().__init__()
        if indicator_columns is None or len(indicator_columns) == 0:
            raise ValueError("AFM needs the indicator columns of its linear term")
        if len(embedding_columns) < 2:
            raise ValueError("AFM pools pairs of fields: at least 2 embedding columns are required, got {}".format(len(embedding_columns)))
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError("`dropout` should be in [0, 1). Got {!r}".format(dropout))
        self._indicator_columns = indicator_columns
        self._embedding_columns = embedding_columns
        self._dropout = float(dropout)
        self._dropout_calls = 0
        self._kwargs = kwargs
        self.slab = L.EmbeddingSlab(embedding_columns, indicator_columns, device=device)
        self.pooling = AttentionalPooling(attention_factor)
        w = torch.empty((self.slab.D, 1), dtype=torch.float32, device=device)
        L.glorot_uniform_(w)
        self.w_out = nn.Parameter(w)

    def _field_keys(self, inputs: Dict[str, object]):
        return [k for k in inputs.keys() if k in self.slab.columns]

    def _pooled(self, inputs, want_attention):
        keys = self._field_keys(inputs)
        F, D = len(keys), self.slab.D
        concat, linear, _ = self.slab(inputs, keys, second_order=False)   # [B, F * D]: the gathered rows, field-major
        e = concat[:, :F * D].reshape(-1, F, D)                           # the same rows viewed per field, read in place
        return linear, self.pooling(e, want_attention)

    def logits(self, inputs):
        linear, pooled = self._pooled(inputs, False)
        if self._dropout > 0.0 and self.training:
            self._dropout_calls += 1
            pooled = L.dropout(pooled, self._dropout, self._dropout_calls)
        return linear.reshape(-1, 1) + L.mlp(pooled, [self.w_out], [None], [0])

    def attention(self, inputs):
        with torch.no_grad():
            return self._pooled(inputs, True)[1][1]

    def call(self, inputs, **kwargs):
        return losses.sigmoid(self.logits(inputs))

    forward = call

    def predict(self, inputs):
        with torch.no_grad():
            return self.call(inputs).cpu().numpy()

    def get_config(self):
        config = {"attention_factor": self.pooling._attention_factor, "dropout": self._dropout}
        return {**self._kwargs, **config}
