"""GraphSAGE (Hamilton, Ying & Leskovec, NeurIPS 2017) and PinSage (Ying et al., KDD 2018) -- the reference's README lists both under
retrieval and ships no code; the surface follows its GCN (keras/models/retrieval/gcn.py): a layer class with build / call / get_config.

A mini-batch of seed nodes is expanded on the device into one block per layer (deep_recommenders_amd.layers.sample_blocks:
dr_neighbor_sample or dr_random_walk + dr_walk_neighbors, dr_frontier_build, dr_block_csr).  A block is a SparseAdjacency
[n_dst, n_src] whose rows sum to 1 and whose first n_dst source nodes are its destinations, so everything after the sampling is what
GCN runs on: layers.aggregate (dr_csr_spmm, backward on the device-built transpose), layers.mlp (the MFMA GEMM path), the residual's
add kernel, dr_act_fwd and dr_softmax_rows_fwd.

  mean  h'_v = act(h_v W_self + mean_{u in S(v)} h_u W_neigh + b)        two products and an add: no concatenated activations
  gcn   h'_v = act(mean_{u in S(v) + {v}} h_u W + b)                      one product on a block built with add_self
  neighbor_units = m:  the aggregated rows are relu(h_u Q + q) (PinSage's Q) instead of h_u

Waiting for an entry of the autograd table (tests/layer_autograd_cases.py) and therefore not here: the max-pool and LSTM aggregators,
PinSage's row normalisation and max-margin loss, GraphSAGE's unsupervised loss."""
import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.ranking.dcn import _init
from deep_recommenders_amd.keras.models.retrieval.gcn import _ACTS

_AGGREGATORS = ("mean", "gcn")


class SAGEConv(nn.Module):
    def __init__(self, units: int, aggregator="mean", neighbor_units=None, activation="relu", use_bias=True,
                 kernel_initializer="truncated_normal", bias_initializer="zeros", **kwargs):
        super().__init__()
        if aggregator not in _AGGREGATORS:
            raise NotImplementedError("SAGEConv aggregator %r: mean and gcn are provided (max-pool and LSTM wait for an autograd table "
                                      "entry)" % (aggregator,))
        if activation not in _ACTS:
            raise NotImplementedError("SAGEConv activation %r: relu, sigmoid, tanh, softmax and linear are provided" % (activation,))
        if neighbor_units is not None and int(neighbor_units) < 1:
            raise ValueError("SAGEConv: neighbor_units must be >= 1 or None, got %r" % (neighbor_units,))
        self._units = int(units)
        self._aggregator = aggregator
        self._neighbor_units = None if neighbor_units is None else int(neighbor_units)
        self._kernel_activation = activation
        self._use_bias = use_bias
        self._kernel_initializer = kernel_initializer
        self._bias_initializer = bias_initializer
        self._kwargs = kwargs
        self.built = False

    def build(self, in_dim, device="cuda"):
        agg_dim = in_dim
        self.neighbor_kernel = self.neighbor_bias = None
        if self._neighbor_units is not None:
            self.neighbor_kernel = nn.Parameter(_init(self._kernel_initializer, (in_dim, self._neighbor_units), device))
            self.neighbor_bias = nn.Parameter(_init(self._bias_initializer, (self._neighbor_units,), device))
            agg_dim = self._neighbor_units
        self.kernel = nn.Parameter(_init(self._kernel_initializer, (agg_dim, self._units), device))     # W_neigh; the gcn aggregator's W
        self.self_kernel = None
        if self._aggregator == "mean":
            self.self_kernel = nn.Parameter(_init(self._kernel_initializer, (in_dim, self._units), device))
        self.bias = nn.Parameter(_init(self._bias_initializer, (self._units,), device)) if self._use_bias else None
        self.built = True

    def call(self, h, block, **kwargs):
        """h [n_src, in_dim] fp32, the rows of block.src_ids; returns [n_dst, units]"""
        if h.shape[0] != block.n_src:
            raise ValueError("SAGEConv: the block has %d source nodes, h has %d rows" % (block.n_src, h.shape[0]))
        if not self.built:
            self.build(h.shape[1], h.device)
        act = self._kernel_activation
        q = h if self.neighbor_kernel is None else L.mlp(h, [self.neighbor_kernel], [self.neighbor_bias], [_ACTS["relu"]])
        agg = L.aggregate(block.adj, q)
        if self._aggregator == "gcn":
            out = L.mlp(agg, [self.kernel], [self.bias], [_ACTS[act]])
        else:
            out = L.mlp(h[:block.n_dst], [self.self_kernel], [self.bias], [0])
            out = L._AddFn.apply(out, L.mlp(agg, [self.kernel], [None], [0]))
            out = L.activation(out, _ACTS[act])
        if act == "softmax":
            out = L.softmax_rows(out)
        return out

    forward = call

    def get_config(self):
        config = {
            "units": self._units,
            "aggregator": self._aggregator,
            "neighbor_units": self._neighbor_units,
            "use_bias": self._use_bias,
            "activation": self._kernel_activation,
            "kernel_initializer": self._kernel_initializer,
            "bias_initializer": self._bias_initializer,
        }
        return {**self._kwargs, **config}


def pad_feature_columns(features):
    """features [N, D] with zero columns added up to the next width gather_feature_rows reads well: a multiple of 4 up to 256, of 256
    beyond.  Done once per graph, on the host or the device; a zero column changes no output (its weight row gets no gradient)."""
    D = features.shape[1]
    width = -(-D // 4) * 4 if D <= 256 else -(-D // 256) * 256
    if width == D:
        return features
    out = features.new_zeros((features.shape[0], width))
    out[:, :D] = features
    return out


def gather_feature_rows(features, ids):
    """features[ids] on dr_rows_gather, which reads rows of up to 256 floats: a wider contiguous row is read as D / c pieces of the
    largest c <= 256 that divides D (a view of the matrix; the piece indices are an integer expression on ids)."""
    if not features.is_contiguous():
        raise ValueError("GraphSAGE: features must be contiguous (dr_rows_gather addresses them as dense rows)")
    N, D = features.shape
    if D % 4 != 0:
        raise ValueError("GraphSAGE: the feature width must be a multiple of 4, got %d; pad_feature_columns() pads a matrix once" % D)
    c = next(w for w in range(min(D, 256), 0, -4) if D % w == 0)
    if c == D:
        return ops.rows_gather(ids, features)[0]
    pieces = D // c
    rows = (ids[:, None] * pieces + torch.arange(pieces, device=ids.device)).reshape(-1)
    return ops.rows_gather(rows, features.view(N * pieces, c))[0].view(ids.numel(), D)


class GraphSAGE(nn.Module):
    """len(fanouts) SAGEConv layers of units_list[k] units over blocks of fanouts[k] sampled neighbours; with num_classes a Dense +
    softmax head on the seeds' rows (losses.categorical_crossentropy applies as in the GCN example), otherwise the seeds' embeddings.

    call(features, adjacency, seeds, seed): features fp32 [N, D] on the device, contiguous, D a multiple of 4 (pad_feature_columns;
    inputs: their rows are read with dr_rows_gather, no gradient and no transpose is made for them), adjacency a
    layers.SparseAdjacency of the whole graph, seeds int64 [B], seed the sampling seed of this step.  The blocks of the last call stay
    in `self.blocks`."""

    def __init__(self, units_list, fanouts, aggregator="mean", num_classes=None, neighbor_units=None, importance=None,
                 activation="relu", use_bias=True):
        super().__init__()
        units_list, fanouts = [int(u) for u in units_list], [int(f) for f in fanouts]
        if not units_list or len(units_list) != len(fanouts):
            raise ValueError("GraphSAGE: one fanout per layer, got units_list %s and fanouts %s" % (units_list, fanouts))
        for f in fanouts:
            if not 1 <= f <= ops.SAMPLE_MAX_FANOUT:
                raise ValueError("GraphSAGE: every fanout must be in [1, %d], got %s" % (ops.SAMPLE_MAX_FANOUT, fanouts))
        self._units_list, self._fanouts, self._aggregator = units_list, fanouts, aggregator
        self._num_classes = None if num_classes is None else int(num_classes)
        self._neighbor_units, self._importance = neighbor_units, None if importance is None else dict(importance)
        self.convs = nn.ModuleList([SAGEConv(u, aggregator=aggregator, neighbor_units=neighbor_units, activation=activation,
                                             use_bias=use_bias) for u in units_list])
        self.head_kernel = self.head_bias = None
        self.blocks = None
        self.built = False

    def build(self, device="cuda"):
        if self._num_classes is not None:
            self.head_kernel = nn.Parameter(_init("truncated_normal", (self._units_list[-1], self._num_classes), device))
            self.head_bias = nn.Parameter(_init("zeros", (self._num_classes,), device))
        self.built = True

    def call(self, features, adjacency, seeds, seed=0, **kwargs):
        if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2:
            raise ValueError("GraphSAGE: features must be an fp32 [N, D] tensor on the device")
        adj = L.as_adjacency(adjacency, device=features.device)
        if adj is None:
            raise TypeError("GraphSAGE: adjacency must be sparse (a layers.SparseAdjacency, built once per graph)")
        if not self.built:
            self.build(features.device)
        self.blocks = L.sample_blocks(adj, seeds, self._fanouts, seed, importance=self._importance, add_self=self._aggregator == "gcn")
        h = gather_feature_rows(features.detach(), self.blocks[0].src_ids)
        for conv, block in zip(self.convs, self.blocks):
            h = conv(h, block)
        if self.head_kernel is not None:
            h = L.softmax_rows(L.mlp(h, [self.head_kernel], [self.head_bias], [0]))
        return h

    forward = call

    def get_config(self):
        return {"units_list": self._units_list, "fanouts": self._fanouts, "aggregator": self._aggregator, "num_classes": self._num_classes,
                "neighbor_units": self._neighbor_units, "importance": self._importance}


class PinSage(GraphSAGE):
    """GraphSAGE over importance neighbours: a node's neighbourhood is the fanouts[k] most visited nodes of num_walks random walks of
    walk_length nodes from it, aggregated with their visit counts as weights after the Dense + relu `Q` (neighbor_units wide)."""

    def __init__(self, units_list, fanouts, num_walks=16, walk_length=3, neighbor_units=None, num_classes=None, aggregator="mean",
                 activation="relu", use_bias=True):
        if neighbor_units is None:
            neighbor_units = int(list(units_list)[0])
        super().__init__(units_list, fanouts, aggregator=aggregator, num_classes=num_classes, neighbor_units=neighbor_units,
                         importance=dict(num_walks=int(num_walks), walk_length=int(walk_length)), activation=activation, use_bias=use_bias)
