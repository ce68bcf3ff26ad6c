"""GCN -- same constructor / call / get_config surface as the reference's keras/models/retrieval/gcn.py:8-70:
out = act(Dense(adj @ features)) (+ features when residual).

The aggregation runs first and the Dense layer second, as in the reference (gcn.py:44-52).  A sparse adjacency (SparseAdjacency,
a torch sparse tensor, a scipy sparse matrix or (indices, values, shape)) goes through dr_csr_spmm, a dense one through the GEMM.
Build a SparseAdjacency once per graph and pass it to every layer: its plan and transpose are then made once.  The Dense layer is the
MFMA GEMM path (deep_recommenders_amd.layers.mlp): relu fused in its epilogue, sigmoid / tanh through dr_act_fwd, softmax through
dr_softmax_rows_fwd (whose output lets losses.categorical_crossentropy work on the logits, as Keras does)."""
import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd.keras.models.ranking.dcn import _init

_ACTS = {"relu": 1, "linear": 0, None: 0, "sigmoid": 2, "tanh": 3, "softmax": 0}


class GCN(nn.Module):
    def __init__(self, units: int, residual=False, use_bias=False, activation="relu", kernel_initializer="truncated_normal",
                 kernel_regularizer=None, bias_initializer="zeros", bias_regularizer=None, **kwargs):
        super().__init__()
        self._units = units
        self._residual = residual
        self._use_bias = use_bias
        if activation not in _ACTS:
            raise NotImplementedError("GCN activation %r: relu, sigmoid, tanh, softmax and linear are provided" % (activation,))
        self._kernel_activation = activation
        self._kernel_initializer = kernel_initializer
        self._kernel_regularizer = kernel_regularizer
        self._bias_initializer = bias_initializer
        self._bias_regularizer = bias_regularizer
        if kernel_regularizer is not None or bias_regularizer is not None:
            raise NotImplementedError("regularizers are not used by any reference model/test")
        self._kwargs = kwargs
        self.built = False

    def build(self, in_dim, device="cuda"):
        self.kernel = nn.Parameter(_init(self._kernel_initializer, (in_dim, self._units), device))          # gcn.py:32-40 Dense
        self.bias = nn.Parameter(_init(self._bias_initializer, (self._units,), device)) if self._use_bias else None
        self.built = True

    def call(self, features, adj, **kwargs):
        x = torch.as_tensor(features, dtype=torch.float32)
        x = x.cuda() if not x.is_cuda else x
        if not self.built:
            self.build(x.shape[1], x.device)
        sparse = L.as_adjacency(adj, device=x.device)
        if sparse is not None:
            agg = L.aggregate(sparse, x)                                                    # gcn.py:44-46
        else:
            a = torch.as_tensor(adj, dtype=torch.float32)
            agg = L.aggregate(a.cuda() if not a.is_cuda else a, x)                          # :47-48
        act = self._kernel_activation
        out = L.mlp(agg, [self.kernel], [self.bias], [_ACTS[act]])                          # :50
        if act == "softmax":
            out = L.softmax_rows(out)
        if self._residual is True:
            out = L._AddFn.apply(out, x)                                                    # :52-53
        return out

    forward = call

    def get_config(self):
        # the reference's keys; it leaves `residual` out (gcn.py:57-66), and so does this
        config = {
            "units": self._units,
            "use_bias": self._use_bias,
            "activation": self._kernel_activation,
            "kernel_initializer": self._kernel_initializer,
            "kernel_regularizer": self._kernel_regularizer,
            "bias_initializer": self._bias_initializer,
            "bias_regularizer": self._bias_regularizer,
        }
        return {**self._kwargs, **config}
