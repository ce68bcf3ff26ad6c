"""EBR: the two-tower model of Huang et al., "Embedding-based Retrieval in Facebook Search", KDD 2020.  The reference's README lists it
among its retrieval models and ships no code for it.

A query tower and a document tower, each YoutubeNet's kind of tower -- mean-pooled bags of hashed text n-gram ids and single-valued ids
(location, social context) from one EmbeddingSlab per side, optional numeric features, a layers.mlp stack -- produce q and d [B, D].
Training is the paper's triplet loss on cosine similarities, L = sum_j max(0, margin - cos(q_i, d_i) + cos(q_i, d_j)), with the other
documents of the batch as negatives ("random negatives" come for free), optionally over each query's num_hard_negatives highest-scoring
in-batch negatives (the paper's online hard-negative mining): dr_margin_rank_fwd / _bwd (csrc/margin_rank.hip), which fold the L2
normalisation in and return gradients with respect to the raw tower outputs.  Serving goes through the indices the package has:
BruteForce, Faiss (IVF-Flat on csrc/ivf.hip) or FaissIVFPQ (the paper's IVF-PQ, csrc/ivf_pq.hip), the two IVF kinds with normalize=True.
Not built: offline hard-negative mining from an index, the embedding ensemble."""
import contextlib

import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.retrieval.factorized_top_k import BruteForce, Faiss, FaissIVFPQ

_ACT = {"relu": 1, None: 0, "linear": 0, "sigmoid": 2, "tanh": 3}


@contextlib.contextmanager
def _seeded(device, seed):
    """torch's generators set to `seed` inside the block and put back after it: the initialisers draw from them"""
    dev = torch.device(device)
    with torch.random.fork_rng(devices=[dev] if dev.type == "cuda" else []):
        torch.manual_seed(int(seed))
        yield


class _Tower(nn.Module):
    """one side: EmbeddingSlab (a multi-valued column is a mean-pooled bag; slab.sparse_lr set: the fused SGD on the slab), an optional
    float [B, Nd] feature joined to the pooled embeddings, glorot-uniform kernels and zero biases with `activation` on every layer"""

    def __init__(self, columns, units, activation, dense_key, device, seed):
        super().__init__()
        self._seed = int(seed)
        with _seeded(device, self._seed):
            self.slab = L.EmbeddingSlab(columns, device=device)
        self._units, self._activation, self._dense_key = units, activation, dense_key
        self.dnn_kernels = nn.ParameterList()
        self.dnn_biases = nn.ParameterList()
        self._built = False
        self._maps = None

    def build(self, dense_width=0):
        if self._built:
            return self
        dev = self.slab.table.device
        d = len(self.slab.keys) * self.slab.D + int(dense_width)
        with _seeded(dev, self._seed + 1):
            for n in self._units:
                self.dnn_kernels.append(nn.Parameter(L.glorot_uniform_(torch.empty((d, n), dtype=torch.float32, device=dev))))
                self.dnn_biases.append(nn.Parameter(torch.zeros(n, dtype=torch.float32, device=dev)))
                d = n
        self._built = True
        return self

    def forward(self, inputs):
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
        return L.mlp(x, list(self.dnn_kernels), list(self.dnn_biases), [_ACT[self._activation]] * len(self._units))


class EBR(nn.Module):
    """EBR(query_columns, document_columns, dnn_units_size, margin=0.2, num_hard_negatives=0, metric="cosine", activation="relu", seed=0).

    query_columns / document_columns: each side's categorical inputs, all of one dimension per side.  dnn_units_size: both towers; its
    last entry is the embedding dimension D (a multiple of 4 in [4, 256]).  query_dense_key / document_dense_key: a float [B, Nd]
    feature of that side.  metric "cosine" (the paper's) or "dot".  num_hard_negatives in [0, 8]: 0 takes every other document of the
    batch as a negative, k > 0 each query's k highest-scoring ones.  document_ids int64 [B] given to loss() / train_step(): a row with
    id < 0 is padding, and a document that occurs twice in the batch is no negative of the rows it is the positive of."""

    def __init__(self, query_columns, document_columns, dnn_units_size, margin=0.2, num_hard_negatives=0, metric="cosine",
                 activation="relu", seed=0, device="cuda", query_dense_key=None, document_dense_key=None):
        super().__init__()
        units = [int(n) for n in dnn_units_size]
        if len(units) == 0 or min(units) < 1:
            raise ValueError("EBR: dnn_units_size needs at least one positive width, got %r" % (list(dnn_units_size),))
        D = units[-1]
        if D % 4 != 0:
            raise ValueError("EBR: the towers' last width is the embedding dimension and must be a multiple of 4, got %d" % D)
        if not 4 <= D <= 256:
            raise ValueError("EBR: the embedding dimension (last entry of dnn_units_size) must lie in [4, 256], got %d" % D)
        if metric not in ops.MARGIN_RANK_METRICS:
            raise ValueError("EBR: metric must be one of %s, got %r" % (sorted(ops.MARGIN_RANK_METRICS), metric))
        if int(num_hard_negatives) != num_hard_negatives or not 0 <= int(num_hard_negatives) <= ops.MARGIN_RANK_MAX_HARD:
            raise ValueError("EBR: num_hard_negatives must be an integer in [0, %d], got %r" % (ops.MARGIN_RANK_MAX_HARD, num_hard_negatives))
        if activation not in _ACT:
            raise ValueError("EBR: activation must be one of %s, got %r" % (sorted(k for k in _ACT if k), activation))
        if len(query_columns) == 0 or len(document_columns) == 0:
            raise ValueError("EBR: each tower needs at least one embedding column")
        self.embedding_dim, self.margin, self.metric = D, float(margin), metric
        self.num_hard_negatives, self.seed = int(num_hard_negatives), int(seed)
        self._units, self._activation = units, activation
        self._dense_keys = (query_dense_key, document_dense_key)
        self._columns = tuple([{"key": c.categorical_column.key, "num_buckets": int(c.categorical_column.num_buckets),
                                "dimension": int(c.dimension)} for c in cols] for cols in (query_columns, document_columns))
        # everything above is host arithmetic: the argument errors come before anything touches the device
        self.query_tower = _Tower(query_columns, units, activation, query_dense_key, device, 2 * self.seed)
        self.document_tower = _Tower(document_columns, units, activation, document_dense_key, device, 2 * self.seed + 1000003)
        self.active_fraction = None         # of the last train_step: active (query, negative) pairs / pairs the loss ran over
        self._serving = None

    def build(self, query_dense_width=0, document_dense_width=0):
        """creates the towers' parameters (the first batch does it otherwise)"""
        self.query_tower.build(query_dense_width)
        self.document_tower.build(document_dense_width)
        return self

    # ---- the towers ------------------------------------------------------------------------------------------------------------------
    def query_vectors(self, inputs):
        """raw query embeddings [B, D], differentiable (the loss and the indices normalise)"""
        return self.query_tower(inputs)

    def document_vectors(self, inputs):
        """raw document embeddings [B, D], differentiable"""
        return self.document_tower(inputs)

    def call(self, inputs, **kwargs):
        return self.query_vectors(inputs)

    forward = call

    def _ids(self, document_ids):
        if document_ids is None:
            return None
        return torch.as_tensor(document_ids, dtype=torch.int64).to(self.query_tower.slab.table.device).reshape(-1).contiguous()

    def _weight(self, sample_weight):
        if sample_weight is None:
            return None
        return torch.as_tensor(sample_weight, dtype=torch.float32).to(self.query_tower.slab.table.device).reshape(-1).contiguous()

    @staticmethod
    def _valid(ids, B):
        """the number of rows that are no padding, at least 1: ONE host read per call (none without ids)"""
        return max(1, B if ids is None else int((ids >= 0).sum().item()))

    # ---- loss and step ---------------------------------------------------------------------------------------------------------------
    def loss(self, query_inputs, document_inputs, document_ids=None, sample_weight=None):
        """mean in-batch triplet loss over the rows that are no padding, as a value (no gradient)"""
        ids, w = self._ids(document_ids), self._weight(sample_weight)
        with torch.no_grad():
            q, d = self.query_vectors(query_inputs), self.document_vectors(document_inputs)
            _, rows, _, _, _ = ops.margin_rank_fwd(q, d, None, ids, None, w, self.margin, self.metric, self.num_hard_negatives)
            return ops.reduce_sum(rows, alpha=1.0 / self._valid(ids, q.shape[0])).reshape(())

    def train_step(self, query_inputs, document_inputs, optimizer=None, document_ids=None, sample_weight=None):
        """one step: both towers, the forward and backward kernels, torch.autograd.backward([q, d], [d_q, d_d]) for the towers and the
        slabs, optimizer.step() if one is given.  Returns the mean loss [] of the batch as the step found it; active_fraction is set."""
        ids, w = self._ids(document_ids), self._weight(sample_weight)
        if optimizer is not None:
            optimizer.zero_grad(set_to_none=True)
        q, d = self.query_vectors(query_inputs), self.document_vectors(document_inputs)
        B = q.shape[0]
        n_valid = self._valid(ids, B)
        inv = 1.0 / n_valid
        rows, active, d_q, d_d, _ = L.margin_rank(q, d, None, ids, None, w, self.margin, self.metric, self.num_hard_negatives, row_scale=inv)
        self._serving = None
        torch.autograd.backward([q, d], [d_q, d_d])
        if optimizer is not None:
            optimizer.step()
        per_row = self.num_hard_negatives if self.num_hard_negatives > 0 else max(1, B - 1)
        self.active_fraction = ops.reduce_sum(active.to(torch.float32), alpha=1.0 / (n_valid * min(per_row, max(1, B - 1)))).reshape(())
        return ops.reduce_sum(rows, alpha=inv).reshape(())

    # ---- serving ---------------------------------------------------------------------------------------------------------------------
    def _unit(self, x):
        x = x.contiguous()
        return ops.rows_scale(x, ops.rowdot(x, x), mode=1) if self.metric == "cosine" else x

    def index(self, document_inputs, identifiers=None, k=10, kind="brute_force", **faiss_kwargs):
        """indexes the documents' vectors as the towers are now: "brute_force" (exact; unit vectors for the cosine), "faiss"
        (IVF-Flat, normalize=True for the cosine; nlist, nprobe, niter, seed as Faiss takes them) or "ivfpq" (IVF-PQ, normalize=True
        for the cosine; nlist, nprobe, m, refine, niter, pq_niter, seed as FaissIVFPQ takes them)"""
        if kind not in ("brute_force", "faiss", "ivfpq"):
            raise ValueError("EBR: kind must be 'brute_force', 'faiss' or 'ivfpq', got %r" % (kind,))
        with torch.no_grad():
            d = self.document_vectors(document_inputs)
            if kind == "ivfpq":
                self._serving = (FaissIVFPQ(k=int(k), normalize=self.metric == "cosine", **faiss_kwargs).index(d.contiguous(), identifiers),
                                 kind)
            elif kind == "faiss":
                self._serving = (Faiss(k=int(k), normalize=self.metric == "cosine", **faiss_kwargs).index(d.contiguous(), identifiers), kind)
            else:
                self._serving = (BruteForce(k=int(k)).index(self._unit(d), identifiers), kind)
        return self._serving[0]

    def top_k(self, query_inputs, k=10):
        """(scores [B, k], identifiers [B, k]) of the k best indexed documents by the model's metric"""
        if self._serving is None:
            raise ValueError("EBR: index() must be called first (and again after a train_step)")
        with torch.no_grad():
            q = self.query_vectors(query_inputs)
            idx, kind = self._serving
            return idx.call(q.contiguous() if kind in ("faiss", "ivfpq") else self._unit(q), int(k))

    def get_config(self):
        """the constructor's arguments; the columns as (key, num_buckets, dimension) records, enough to rebuild identity / hashed
        embedding columns of the same shape (an initializer given to a column is not recorded)"""
        return {"query_columns": [dict(c) for c in self._columns[0]], "document_columns": [dict(c) for c in self._columns[1]],
                "dnn_units_size": list(self._units), "margin": self.margin, "num_hard_negatives": self.num_hard_negatives,
                "metric": self.metric, "activation": self._activation, "seed": self.seed,
                "query_dense_key": self._dense_keys[0], "document_dense_key": self._dense_keys[1]}
