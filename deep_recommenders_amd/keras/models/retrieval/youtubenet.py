"""YoutubeNet: the candidate-generation network of Covington et al., "Deep Neural Networks for YouTube Recommendations", RecSys 2016.
The reference's README lists it among its retrieval models and ships no code for it.

A user tower -- mean-pooled bags of watch / search ids from one EmbeddingSlab (K3), numeric features such as the example age, a ReLU
tower (layers.mlp) -- produces u [B, D]; training is a softmax over num_classes videos with num_sampled negatives that the whole
batch shares, importance-corrected: tf.nn.sampled_softmax_loss, here dr_sampled_softmax_fwd / _bwd (csrc/sampled_softmax.hip).  The
negatives come from dr_alias_sample, the class table is updated through K4 (layers.sgns_apply_rows) and served through
BruteForce / ops.topk_mips.  The class table is separate from the input video embeddings, as in the paper; there is no per-class
bias (the paper's softmax has none)."""
import math

import numpy as np
import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.retrieval.factorized_top_k import BruteForce

_ACT = {"relu": 1, None: 0, "linear": 0, "sigmoid": 2, "tanh": 3}
_P_FLOOR = 1e-30        # a class of count 0 is never drawn; as a label its log Q stays finite


def log_uniform_probabilities(num_classes):
    """float64 [V]: TensorFlow's log-uniform (Zipfian) candidate sampler, p(c) = log((c + 2) / (c + 1)) / log(V + 1)"""
    c = np.arange(int(num_classes), dtype=np.float64)
    return np.log((c + 2.0) / (c + 1.0)) / math.log(int(num_classes) + 1.0)


def expected_counts(p, num_sampled):
    """float64 [V]: Q(c) = S p(c), the expected count of class c among S draws with replacement (TensorFlow's unique=False form)"""
    return float(num_sampled) * np.asarray(p, dtype=np.float64)


class YoutubeNet(nn.Module):
    """YoutubeNet(embedding_columns, num_classes, dnn_units_size, num_sampled, class_counts=None, dense_features_key=None,
    activation="relu", remove_accidental_hits=True, deterministic=False, seed=0).call(inputs) -> user vectors [B, D].

    embedding_columns: the tower's categorical inputs, all of one dimension; a multi-valued column (watch history, search tokens) is
    a mean-pooled bag.  slab.sparse_lr set: the fused SGD on the slab, as in DLRM.  dense_features_key: a float [B, Nd] feature joined
    to the pooled embeddings (dr_gather_cols, as InputLayer joins numeric columns).  dnn_units_size: the tower, glorot-uniform
    kernels and zero biases, `activation` on every layer; its last entry is the dimension D of class_table [num_classes, D]
    (truncated normal, sigma = 1 / sqrt(D)).  class_counts [num_classes]: the sampler's distribution (None: TensorFlow's log-uniform
    one, which expects the classes ordered by falling frequency); a class of count 0 is never drawn.  The num_sampled negatives
    are drawn once per step for the whole batch, with replacement, from (seed, running offset); log Q = log(num_sampled * p) is one
    fp32 [num_classes] device vector built once in float64.  deterministic=True keeps two slot plans and takes the sorted K4 for the
    class table: with the kernels' fixed summation order the class table, the tower and the loss curve are bit-reproducible.  The
    slab's own K4 stays the atomic form (its bags are multi-valued, the sorted K4 takes single-valued fields): slab rows that several
    slots of a batch share are summed in arrival order.  Labels < 0 are padding rows; labels and sampled ids must be < num_classes."""

    def __init__(self, embedding_columns, num_classes, dnn_units_size, num_sampled, class_counts=None, dense_features_key=None,
                 activation="relu", remove_accidental_hits=True, deterministic=False, seed=0, device="cuda"):
        super().__init__()
        V, S = int(num_classes), int(num_sampled)
        units = [int(n) for n in dnn_units_size]
        if not 1 <= V < 2 ** 31:
            raise ValueError("YoutubeNet: needs 1 <= num_classes < 2^31, got %d" % V)
        if not 1 <= S < 2 ** 31:
            raise ValueError("YoutubeNet: num_sampled must be >= 1 (and < 2^31), got %d" % S)
        if len(units) == 0 or min(units) < 1:
            raise ValueError("YoutubeNet: dnn_units_size needs at least one positive width, got %r" % (list(dnn_units_size),))
        D = units[-1]
        if D % 4 != 0:
            raise ValueError("YoutubeNet: the tower's last width is the class dimension and must be a multiple of 4, got %d" % D)
        if not 4 <= D <= 256:
            raise ValueError("YoutubeNet: the class dimension (last entry of dnn_units_size) must lie in [4, 256], got %d" % D)
        if activation not in _ACT:
            raise ValueError("YoutubeNet: activation must be one of %s, got %r" % (sorted(k for k in _ACT if k), activation))
        if class_counts is None:
            p = log_uniform_probabilities(V)
        else:
            counts = np.asarray(class_counts, dtype=np.float64).reshape(-1)
            if counts.size != V:
                raise ValueError("YoutubeNet: class_counts must have num_classes = %d entries, got %d" % (V, counts.size))
            if not np.isfinite(counts).all() or (counts < 0).any() or not counts.sum() > 0:
                raise ValueError("YoutubeNet: class_counts must be finite, >= 0 and not all zero")
            p = counts / counts.sum()
        self.num_classes, self.num_sampled, self.embedding_dim = V, S, D
        self._units, self._activation, self._dense_key = units, activation, dense_features_key
        self._has_counts = class_counts is not None
        self.remove_accidental_hits, self.deterministic, self.seed = bool(remove_accidental_hits), bool(deterministic), int(seed)
        # everything above is host arithmetic: the argument errors come before anything touches the device
        self.slab = L.EmbeddingSlab(embedding_columns, device=device)
        self.class_table = nn.Parameter(L.truncated_normal_(torch.empty((V, D), dtype=torch.float32, device=device), 1.0 / math.sqrt(D)))
        prob, alias = ops.alias_table(p)
        log_q = np.log(expected_counts(np.maximum(p, _P_FLOOR), S)).astype(np.float32)
        self.register_buffer("alias_prob", torch.from_numpy(prob).to(device), persistent=False)
        self.register_buffer("alias_index", torch.from_numpy(alias).to(device), persistent=False)
        self.register_buffer("log_q", torch.from_numpy(log_q).to(device), persistent=False)
        self.dnn_kernels = nn.ParameterList()
        self.dnn_biases = nn.ParameterList()
        self._dnn_built = False
        self._maps = None
        self.draw_offset = 0                # elements drawn so far: the next call continues the stream
        self._plans = None
        self._scratch = None
        self._serving = {}                  # k -> BruteForce over the class table as the last step left it

    # ---- the user tower ------------------------------------------------------------------------------------------------------------
    def build(self, dense_width=0):
        """creates the tower's parameters for `dense_width` numeric inputs (call() does it on the first batch otherwise)"""
        if self._dnn_built:
            return self
        dev = self.slab.table.device
        d = len(self.slab.keys) * self.slab.D + int(dense_width)
        for n in self._units:                                       # glorot-uniform kernel, zero bias
            self.dnn_kernels.append(nn.Parameter(L.glorot_uniform_(torch.empty((d, n), dtype=torch.float32, device=dev))))
            self.dnn_biases.append(nn.Parameter(torch.zeros(n, dtype=torch.float32, device=dev)))
            d = n
        self._dnn_built = True
        return self

    def call(self, inputs, **kwargs):
        """user vectors [B, D], differentiable"""
        keys = self.slab.keys
        FD = len(keys) * self.slab.D
        concat, _, _ = self.slab(inputs, keys, second_order=False)
        x = concat[:, :FD]
        if self._dense_key is not None:
            dev = self.slab.table.device
            num = torch.as_tensor(inputs[self._dense_key], dtype=torch.float32).to(dev)
            num = num.reshape(num.shape[0], -1)
            Nd = num.shape[1]
            if self._maps is None or self._maps[2] != Nd:
                col_map = torch.tensor([-i - 1 for i in range(FD)] + list(range(Nd)), dtype=torch.int32, device=dev)
                emb_map = torch.arange(FD, dtype=torch.int32, device=dev)
                self._maps = (col_map, emb_map, Nd)
            self.build(Nd)
            x = L._GatherColsFn.apply(num, x, self._maps[0], self._maps[1], FD + Nd)
        else:
            self.build(0)
        acts = [_ACT[self._activation]] * len(self._units)
        return L.mlp(x, list(self.dnn_kernels), list(self.dnn_biases), acts)

    forward = call

    # ---- the sampler ---------------------------------------------------------------------------------------------------------------
    def sample(self):
        """int64 [num_sampled] from the alias table, with replacement, advancing the running offset: one draw per step for the batch"""
        s = ops.alias_sample(self.alias_prob, self.alias_index, self.num_sampled, self.seed, self.draw_offset)
        self.draw_offset += self.num_sampled
        return s

    def _labels(self, labels):
        return torch.as_tensor(labels, dtype=torch.int64).to(self.class_table.device).reshape(-1).contiguous()

    def _log_q(self, labels, sampled):
        """the per-step [B] and [S] gathers of log Q (plumbing; an id < 0 reads entry 0, the kernel never uses it)"""
        return self.log_q[labels.clamp(min=0)], self.log_q[sampled.clamp(min=0)]

    @staticmethod
    def _valid(labels):
        """the number of rows with a label, at least 1: ONE host read per call"""
        return max(1, int((labels >= 0).sum().item()))

    def plans(self, B):
        """the two slot plans of the sorted K4 (ids labels [B, 1] and sampled [S, 1]), None unless deterministic"""
        if not self.deterministic:
            return None
        n = max(B, self.num_sampled)
        if self._plans is None or self._plans[0].n < B:
            dev = self.class_table.device
            self._plans = (ops.SortPlan(B, dev), ops.SortPlan(self.num_sampled, dev))
            self._scratch = torch.empty((n, self.embedding_dim), dtype=torch.float32, device=dev)
        return self._plans

    # ---- loss and step -------------------------------------------------------------------------------------------------------------
    def loss(self, inputs, labels, sampled=None):
        """mean sampled-softmax loss over the rows with a label >= 0, as a value (no gradient)"""
        labels = self._labels(labels)
        sampled = self.sample() if sampled is None else sampled
        with torch.no_grad():
            u = self.call(inputs)
            lq_t, lq_s = self._log_q(labels, sampled)
            _, _, rows, _ = ops.sampled_softmax_fwd(u, self.class_table.data, labels, sampled, lq_t, lq_s, None,
                                                    self.remove_accidental_hits)
            return ops.reduce_sum(rows, alpha=1.0 / self._valid(labels)).reshape(())

    def train_step(self, inputs, labels, lr, optimizer=None, sampled=None):
        """one step: the forward and backward kernels, -lr times d_true and d_sampled applied to the class table through K4 (both
        buffers are complete before the table changes), u.backward(d_u) for the tower and the slab, optimizer.step() if one is
        given.  Returns the mean loss [] of the batch as the step found it."""
        labels = self._labels(labels)
        sampled = self.sample() if sampled is None else sampled
        B, S = labels.shape[0], sampled.shape[0]
        inv = 1.0 / self._valid(labels)
        if optimizer is not None:
            optimizer.zero_grad(set_to_none=True)
        u = self.call(inputs)
        lq_t, lq_s = self._log_q(labels, sampled)
        rows, d_u, d_true, d_sampled = L.sampled_softmax(u, self.class_table.data, labels, sampled, lq_t, lq_s, None,
                                                         self.remove_accidental_hits, row_scale=inv)
        plans = self.plans(B)
        plan_t, plan_s = plans if plans is not None else (None, None)
        L.sgns_apply_rows(self.class_table.data, labels.reshape(B, 1), d_true, -float(lr), plan_t, self._scratch)
        L.sgns_apply_rows(self.class_table.data, sampled.reshape(S, 1), d_sampled, -float(lr), plan_s, self._scratch)
        self._serving.clear()
        u.backward(d_u)
        if optimizer is not None:
            optimizer.step()
        return ops.reduce_sum(rows, alpha=inv).reshape(())

    # ---- serving -------------------------------------------------------------------------------------------------------------------
    def index(self, k=10):
        """a BruteForce index over the class table as it is now (rebuilt after a train_step)"""
        if int(k) not in self._serving:
            self._serving.clear()
            self._serving[int(k)] = BruteForce(k=int(k)).index(self.class_table.data)
        return self._serving[int(k)]

    def top_k(self, inputs, k=10):
        """(scores [B, k], class ids [B, k]) of the k best classes by u . class_table[c]"""
        with torch.no_grad():
            return self.index(k).call(self.call(inputs), k)

    def get_config(self):
        return {"num_classes": self.num_classes, "dnn_units_size": list(self._units), "num_sampled": self.num_sampled,
                "class_counts": self._has_counts, "dense_features_key": self._dense_key, "activation": self._activation,
                "remove_accidental_hits": self.remove_accidental_hits, "deterministic": self.deterministic, "seed": self.seed}
