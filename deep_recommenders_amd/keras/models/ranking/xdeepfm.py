"""xDeepFM.  The Compressed Interaction Network layer `CIN` has the constructor / call / get_config surface of the reference's
keras/models/ranking/xdeepfm.py:9-117 and is backed by dr_cin_fwd / dr_cin_bwd (deep_recommenders_amd/csrc/cin.hip).  The reference
stops at the layer; `CINNetwork` (the stack with the paper's sum pooling and direct connection) and `XDeepFM` (linear + CIN + DNN,
Lian et al. 2018, eq. 9) complete the model on dr_cin_pool_fwd / dr_cin_pool_bwd (csrc/cin_pool.hip), built like deepfm.py."""
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import losses
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.ranking.dcn import _init


class _CinFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, x, W, bias, act):
        x0, x, W = L._rows(x0, dense=True), L._rows(x, dense=True), L._rows(W, dense=True)
        out = ops.cin_fwd(x0, x, W, bias, act)
        ctx.act = act
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x0, x, W, out)
        return out

    @staticmethod
    @L._needed_only
    def backward(ctx, d_out):
        x0, x, W, out = ctx.saved_tensors
        d_x0, d_x, dW, dbias = ops.cin_bwd(x0, x, W, ctx.act, out, L._rows(d_out, dense=True), want_bias=ctx.has_bias)
        return d_x0, d_x, dW, dbias, None


class CIN(nn.Module):
    """CIN(feature_map=3, use_bias=False, activation="sigmoid", kernel_init="truncated_normal", kernel_regu=None,
    bias_init="zeros", bias_regu=None)((x0, x)) -> [B, feature_map, D]   (xdeepfm.py:71-96)."""

    def __init__(self, feature_map: Optional[int] = 3, use_bias: bool = False, activation="sigmoid",
                 kernel_init="truncated_normal", kernel_regu=None, bias_init="zeros", bias_regu=None, **kwargs):
        super().__init__()
        self._feature_map = feature_map
        self._use_bias = use_bias
        if activation is not None and not callable(activation) and activation not in ops.ACT_CODES:
            raise ValueError("unknown activation {!r}; supported: {}".format(activation, sorted(k for k in ops.ACT_CODES if k)))
        self._activation = activation
        self._kernel_init, self._kernel_regu = kernel_init, kernel_regu
        self._bias_init, self._bias_regu = bias_init, bias_regu
        if kernel_regu is not None or bias_regu is not None:
            raise NotImplementedError("regularizers are not used by any reference model/test")
        self._kwargs = kwargs
        self.built = False

    def build(self, input_shape, device="cuda"):
        if not isinstance(input_shape, tuple):                                      # xdeepfm.py:41-44
            raise ValueError("`CIN` layer's inputs type should be `tuple`."
                             "Got `CIN` layer's inputs type = `{}`".format(type(input_shape)))
        if len(input_shape) != 2:                                                   # :46-48
            raise ValueError("`CIN` Layer inputs tuple length should be 2."
                             "Got `length` = {}".format(len(input_shape)))
        x0_shape, x_shape = input_shape
        self._x0_fields, self._x_fields = int(x0_shape[1]), int(x_shape[1])
        # conv1d kernel [1, H0 * Hk, feature_map] (:54-60), stored without the leading width-1 axis
        self.kernel = nn.Parameter(_init(self._kernel_init, (self._x0_fields * self._x_fields, self._feature_map), device))
        self.bias = nn.Parameter(_init(self._bias_init, (self._feature_map,), device)) if self._use_bias is True else None
        self.built = True

    def call(self, inputs: Tuple[torch.Tensor, torch.Tensor], **kwargs):
        if not isinstance(inputs, tuple):
            raise ValueError("`CIN` layer's inputs type should be `tuple`."
                             "Got `CIN` layer's inputs type = `{}`".format(type(inputs)))
        if len(inputs) != 2:
            raise ValueError("`CIN` Layer inputs tuple length should be 2."
                             "Got `length` = {}".format(len(inputs)))
        x0, x = (torch.as_tensor(t, dtype=torch.float32).cuda() for t in inputs)
        if x0.dim() != 3 or x.dim() != 3:                                           # :75-80
            raise ValueError("`x0` and `x` dim should be 3."
                             "Got `x0` dim = {}, `x` dim = {}".format(x0.dim(), x.dim()))
        if not self.built:
            self.build((tuple(x0.shape), tuple(x.shape)), x0.device)
        if callable(self._activation):                                              # a user-supplied layer: linear kernel + it
            return self._activation(_CinFn.apply(x0, x, self.kernel, self.bias, 0))
        return _CinFn.apply(x0, x, self.kernel, self.bias, ops.ACT_CODES[self._activation])

    forward = call

    def get_config(self):
        config = {
            "feature_map": self._feature_map,
            "use_bias": self._use_bias,
            "activation": self._activation,
            "kernel_init": self._kernel_init,
            "kernel_regu": self._kernel_regu,
            "bias_init": self._bias_init,
            "bias_regu": self._bias_regu,
        }
        return {**self._kwargs, **config}


class CINNetwork(nn.Module):
    """CINNetwork(layer_sizes, activation=None, use_bias=False, kernel_init="truncated_normal", bias_init="zeros")(x0) -> [B, sum sizes].

    x_k = CIN(layer_sizes[k])((x0, x_{k-1})) with x_0 = x0 [B, F, D]; every layer is sum-pooled over D and the pooled vectors are
    concatenated (the paper's direct connection: every layer's whole output feeds both the next layer and the output unit, no
    split-half).  The default activation is linear, which the paper found best; the last layer's [B, Hk, D] output is never written
    when the activation is linear.  One autograd node for the whole stack (layers.cin_stack)."""

    def __init__(self, layer_sizes: Sequence[int], activation=None, use_bias: bool = False, kernel_init="truncated_normal",
                 bias_init="zeros", **kwargs):
        super().__init__()
        sizes = [int(s) for s in layer_sizes]
        if len(sizes) == 0 or any(s <= 0 for s in sizes):
            raise ValueError("`layer_sizes` must hold at least one positive size. Got {!r}".format(layer_sizes))
        if activation not in ops.ACT_CODES:
            raise ValueError("unknown activation {!r}; supported: {}".format(activation, sorted(k for k in ops.ACT_CODES if k)))
        self._layer_sizes = sizes
        self._activation = activation
        self._use_bias = use_bias
        self._kernel_init, self._bias_init = kernel_init, bias_init
        self._kwargs = kwargs
        self.kernels = nn.ParameterList()
        self.biases = nn.ParameterList()
        self.built = False

    @property
    def output_dim(self):
        return sum(self._layer_sizes)

    def build(self, input_shape, device="cuda"):
        if len(input_shape) != 3:
            raise ValueError("`x0` dim should be 3. Got `x0` dim = {}".format(len(input_shape)))
        h0 = hk = int(input_shape[1])
        for size in self._layer_sizes:
            self.kernels.append(nn.Parameter(_init(self._kernel_init, (h0 * hk, size), device)))
            if self._use_bias is True:
                self.biases.append(nn.Parameter(_init(self._bias_init, (size,), device)))
            hk = size
        self.built = True

    def call(self, x0, **kwargs):
        x0 = torch.as_tensor(x0, dtype=torch.float32)
        if x0.dim() != 3:
            raise ValueError("`x0` dim should be 3. Got `x0` dim = {}".format(x0.dim()))
        x0 = x0.cuda()
        if not self.built:
            self.build(tuple(x0.shape), x0.device)
        biases = list(self.biases) if self._use_bias is True else [None] * len(self.kernels)
        return L.cin_stack(x0, list(self.kernels), biases, ops.ACT_CODES[self._activation])

    forward = call

    def get_config(self):
        config = {
            "layer_sizes": self._layer_sizes,
            "activation": self._activation,
            "use_bias": self._use_bias,
            "kernel_init": self._kernel_init,
            "bias_init": self._bias_init,
        }
        return {**self._kwargs, **config}


class XDeepFM(nn.Module):
    """XDeepFM(indicator_columns, embedding_columns, cin_layer_sizes, dnn_units_size, cin_activation=None, dnn_activation="relu").call(inputs)
    -> prob = sigmoid(linear(indicator) + CINNetwork(stacked embeddings) w_cin + Sequential(Dense(u, act)..., Dense(1))(concat embeddings)).

    One EmbeddingSlab holds the tables and the linear term with the model's only output bias; `w_cin` [sum sizes, 1] is glorot-uniform
    and has no bias of its own.  `dense_features_key`: as in DeepFM, a float [B, Nd] feature appended to the DNN input only."""

    def __init__(self, indicator_columns, embedding_columns, cin_layer_sizes, dnn_units_size, cin_activation=None, dnn_activation="relu",
                 dense_features_key: Optional[str] = None, device="cuda", **kwargs):
        super().__init__()
        if dnn_activation not in ops.ACT_CODES:
            raise ValueError("dnn_activation must be one of {}, got {!r}".format(sorted(k for k in ops.ACT_CODES if k), dnn_activation))
        if indicator_columns is None or len(indicator_columns) == 0:
            raise ValueError("XDeepFM needs the indicator columns of its linear term")
        self._indicator_columns = indicator_columns
        self._embedding_columns = embedding_columns
        self._dnn_units_size = list(dnn_units_size)
        self._dnn_activation = dnn_activation
        self._dense_key = dense_features_key
        self._kwargs = kwargs
        self.slab = L.EmbeddingSlab(embedding_columns, indicator_columns, device=device)
        self.cin = CINNetwork(cin_layer_sizes, activation=cin_activation)
        w = torch.empty((self.cin.output_dim, 1), dtype=torch.float32, device=device)
        L.glorot_uniform_(w)
        self.w_cin = nn.Parameter(w)
        self.dnn_kernels = nn.ParameterList()
        self.dnn_biases = nn.ParameterList()
        self._dnn_built = False

    def _build_dnn(self, in_dim, device):
        d = in_dim
        for u in self._dnn_units_size + [1]:                     # glorot-uniform kernel, zero bias, as DeepFM's
            W = torch.empty((d, u), dtype=torch.float32, device=device)
            L.glorot_uniform_(W)
            self.dnn_kernels.append(nn.Parameter(W))
            self.dnn_biases.append(nn.Parameter(torch.zeros(u, dtype=torch.float32, device=device)))
            d = u
        self._dnn_built = True

    def _field_keys(self, inputs: Dict[str, object]):
        return [k for k in inputs.keys() if k in self.slab.columns]

    def logits(self, inputs):
        keys = self._field_keys(inputs)
        F, D = len(keys), self.slab.D
        FD = F * D
        dense = None
        in_dim = FD
        if self._dense_key is not None:
            dense = torch.as_tensor(inputs[self._dense_key], dtype=torch.float32).to(self.slab.table.device)
            in_dim = FD + dense.shape[1]
        concat, linear, _ = self.slab(inputs, keys, ld_concat=L._pad4(in_dim), second_order=False)
        if dense is not None:
            concat.data[:, FD:in_dim].copy_(dense)                 # layout only: append to the DNN input
        if not self._dnn_built:
            self._build_dnn(in_dim, concat.device)
        x0 = concat[:, :FD].reshape(-1, F, D)                      # the same gathered rows, viewed per field
        cin_out = L.mlp(self.cin(x0), [self.w_cin], [None], [0])
        acts = [ops.ACT_CODES[self._dnn_activation]] * len(self._dnn_units_size) + [0]
        dnn_out = L.mlp(concat[:, :in_dim], list(self.dnn_kernels), list(self.dnn_biases), acts)
        return linear.reshape(-1, 1) + cin_out + dnn_out

    def call(self, inputs, **kwargs):
        return losses.sigmoid(self.logits(inputs))

    forward = call

    def predict(self, inputs):
        with torch.no_grad():
            return self.call(inputs).cpu().numpy()

    def get_config(self):
        config = {"cin_layer_sizes": self.cin._layer_sizes, "cin_activation": self.cin._activation,
                  "dnn_units_size": self._dnn_units_size, "dnn_activation": self._dnn_activation}
        return {**self._kwargs, **config}
