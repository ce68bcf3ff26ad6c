"""Embedding, ScaledDotProductAttention and MultiHeadAttention -- the constructor / call surface of the reference's
keras/models/nlp/multi_head_attention.py on the fused attention kernels (dr_attn_fwd / dr_attn_bwd).

Inputs are lists as in the reference: [queries, keys, values, masks] with masking, [queries, keys, values] without; `masks` is a
[batch, key length] boolean tensor, True at padded keys.  The semantics the kernels reproduce: scores
divided by sqrt(head width) after the product; the padding mask ADDS -2^32 + 1 in fp32, so a row whose keys are all padded attends
uniformly; the future mask REPLACES the entries above the diagonal; queries at padded positions are not masked; dropout on the
softmax output is always on (K.dropout has no training switch) and draws a fresh counter-based mask on every call
(`seed` offsets the stream; `last_seed` is the seed the latest call used).  MultiHeadAttention has three bias-free projections
and no output projection; the heads are column blocks of the projected tensors, never split or concatenated."""
import torch
from torch import nn

from deep_recommenders_amd import layers as L

MASKING_NUM = -2 ** 32 + 1


def _f32(x):
    x = torch.as_tensor(x)
    x = x if x.dtype == torch.float32 else x.to(torch.float32)
    return x if x.is_cuda else x.cuda()


def _check_rate(rate):
    if not 0.0 <= float(rate) < 1.0:
        raise ValueError("dropout rate must be in [0, 1), got {}".format(rate))
    return float(rate)


class _Seeded(nn.Module):
    """the counter-based dropout stream of a layer: call n of a layer with seed s uses s * 1000003 + n"""

    def _init_seed(self, kwargs):
        self.seed = int(kwargs.get("seed", 0))
        self._calls = 0
        self.last_seed = None

    def _next_seed(self):
        self._calls += 1
        self.last_seed = (self.seed * 1000003 + self._calls) & 0xFFFFFFFFFFFFFFFF
        return self.last_seed

    def reset_calls(self):
        self._calls = 0


class Embedding(nn.Module):
    def __init__(self, vocab_size, model_dim, **kwargs):
        super().__init__()
        self._vocab_size = vocab_size
        self._model_dim = model_dim
        self._kwargs = kwargs
        self.built = False

    def build(self, device="cuda"):
        w = torch.empty((self._vocab_size, self._model_dim), dtype=torch.float32, device=device)
        self.embeddings = nn.Parameter(L.glorot_uniform_(w))
        self.built = True

    def call(self, inputs, **kwargs):
        ids = torch.as_tensor(inputs)
        ids = ids if ids.is_cuda else ids.cuda()
        if not self.built:
            self.build(ids.device)
        return L.token_embedding(self.embeddings, ids)            # gather * sqrt(model_dim)

    forward = call

    def get_config(self):
        return {**self._kwargs, "vocab_size": self._vocab_size, "model_dim": self._model_dim}


class ScaledDotProductAttention(_Seeded):
    """One head per batch row, as the reference's layer: [queries, keys, values(, masks)] with queries [N, Lq, d]; `masks` [B, Lk]
    is tiled over N // B head-major groups (rows h * B + b), as K.tile does."""

    def __init__(self, masking=True, future=False, dropout_rate=0., **kwargs):
        super().__init__()
        self._masking = masking
        self._future = future
        self._dropout_rate = _check_rate(dropout_rate)
        self._masking_num = MASKING_NUM
        self._init_seed(kwargs)
        self._kwargs = kwargs

    def call(self, inputs, **kwargs):
        if self._masking:
            if len(inputs) != 4:
                raise ValueError("with masking the inputs are [queries, keys, values, masks]")
            queries, keys, values, masks = inputs
        else:
            if len(inputs) != 3:
                raise ValueError("without masking the inputs are [queries, keys, values]")
            queries, keys, values = inputs
            masks = None
        queries, keys, values = _f32(queries), _f32(keys), _f32(values)
        if masks is not None:
            masks = torch.as_tensor(masks).to(device=queries.device, dtype=torch.bool)
            masks = masks.repeat(queries.shape[0] // masks.shape[0], 1)
        return L.attention(queries, keys, values, 1, masks, self._future, self._dropout_rate, self._next_seed())

    forward = call

    def get_config(self):
        return {**self._kwargs, "masking": self._masking, "future": self._future, "dropout_rate": self._dropout_rate}


class MultiHeadAttention(_Seeded):
    def __init__(self, n_heads, head_dim, dropout_rate=.1, masking=True, future=False, trainable=True, **kwargs):
        super().__init__()
        self._n_heads = n_heads
        self._head_dim = head_dim
        self._dropout_rate = _check_rate(dropout_rate)
        self._masking = masking
        self._future = future
        self._trainable = trainable
        self._init_seed(kwargs)
        self._kwargs = kwargs
        self.built = False

    def build(self, input_shape, device="cuda"):
        """input_shape: the shapes of [queries, keys, values]"""
        width = self._n_heads * self._head_dim
        for name, shape in zip(("_weights_queries", "_weights_keys", "_weights_values"), input_shape):
            w = torch.empty((int(shape[-1]), width), dtype=torch.float32, device=device)
            setattr(self, name, nn.Parameter(L.glorot_uniform_(w), requires_grad=bool(self._trainable)))
        self.built = True

    def call(self, inputs, **kwargs):
        if self._masking:
            if len(inputs) != 4:
                raise ValueError("with masking the inputs are [queries, keys, values, masks]")
            queries, keys, values, masks = inputs
            masks = torch.as_tensor(masks)
        else:
            if len(inputs) != 3:
                raise ValueError("without masking the inputs are [queries, keys, values]")
            queries, keys, values = inputs
            masks = None
        queries, keys, values = _f32(queries), _f32(keys), _f32(values)
        if not self.built:
            self.build([queries.shape, keys.shape, values.shape], queries.device)
        if masks is not None:
            masks = masks.to(device=queries.device, dtype=torch.bool)

        def project(x, w):
            b, l, d = x.shape
            return L.mlp(x.reshape(b * l, d), [w], [None], [0]).reshape(b, l, w.shape[1])

        q = project(queries, self._weights_queries)
        k = project(keys, self._weights_keys)
        v = project(values, self._weights_values)
        return L.attention(q, k, v, self._n_heads, masks, self._future, self._dropout_rate, self._next_seed())

    forward = call

    def get_config(self):
        return {**self._kwargs, "n_heads": self._n_heads, "head_dim": self._head_dim, "dropout_rate": self._dropout_rate,
                "masking": self._masking, "future": self._future, "trainable": self._trainable}
