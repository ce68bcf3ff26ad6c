"""EGES (Wang et al., KDD 2018, "Billion-scale Commodity Embedding for E-commerce Recommendation in Alibaba"): DeepWalk over a weighted
item graph built from sessions, the centre's vector a softmax-weighted sum of the item's own row and the rows of its side features,
with attention logits of the item's own.  The reference's README lists the model and ships no code for it.

The step runs on dr_random_walk_weighted (the walks), dr_alias_sample (the negatives), dr_eges_fwd (every row read once: loss and the
three gradient-row buffers) and K4 on the three tables.  A cold item -- side features only, field 0 missing -- gets the average of
its side rows from dr_eges_embed: that is what embeddings() serves an index from."""
import math

import numpy as np
import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.retrieval.skipgram import _SEED_STRIDE


def graph_from_sessions(sessions, num_items):
    """(indices [E, 2], values [E], (num_items, num_items)): every consecutive pair (a, b) of a session is a directed edge a -> b of
    weight 1, duplicates included -- SparseAdjacency sums them into the co-occurrence counts.  Host only."""
    num_items = int(num_items)
    src, dst = [], []
    for s in sessions:
        s = np.asarray(s, dtype=np.int64).reshape(-1)
        if s.size and (s.min() < 0 or s.max() >= num_items):
            raise ValueError("graph_from_sessions: item ids must lie in [0, %d)" % num_items)
        src.append(s[:-1])
        dst.append(s[1:])
    src = np.concatenate(src) if src else np.zeros(0, dtype=np.int64)
    dst = np.concatenate(dst) if dst else np.zeros(0, dtype=np.int64)
    return np.stack([src, dst], axis=1), np.ones(src.size, dtype=np.float32), (num_items, num_items)


def _cumulative_weights(adj):
    """cum int64 [nnz] on the adjacency's device and the weighted out-degree [n] (float64, host); refuses values that are no
    non-negative integers and rows whose total reaches 2^32 (the walk's draw is a 32-bit product)"""
    val = adj.val.cpu().numpy().astype(np.float64)
    if not np.isfinite(val).all() or (val < 0).any() or (val != np.floor(val)).any():
        raise ValueError("EGES: the adjacency's values must be non-negative integers (co-occurrence counts)")
    cum = np.cumsum(val.astype(np.int64))
    row_ptr = adj.row_ptr.cpu().numpy()
    padded = np.concatenate([np.zeros(1, dtype=np.int64), cum])
    totals = padded[row_ptr[1:]] - padded[row_ptr[:-1]]
    if totals.size and totals.max() >= 2 ** 32:
        raise ValueError("EGES: a node's edge weights sum to %d; the walk needs every total below 2^32" % int(totals.max()))
    return torch.from_numpy(cum).to(adj.row_ptr.device), totals.astype(np.float64)


class EGES(nn.Module):
    """Field 0 of an item is the item itself, fields 1 .. n its side features: item_side_ids int64 [num_items, n], -1 for an unknown
    feature, feature f in [0, side_sizes[f]).  One side_table of num_items + sum(side_sizes) rows with row_base (the slab's layout),
    att [num_items, S rounded up to a multiple of 4] starting at zero (uniform weights), out_table [num_items, D].  The walks run over
    `adjacency` (non-negative integer weights, e.g. graph_from_sessions); negatives follow weighted out-degree ** 0.75 unless `counts`
    is given.  deterministic=True takes the sorted K4 on all three tables."""

    def __init__(self, num_items, side_sizes, item_side_ids, embedding_dim, adjacency, walk_length, window, num_negatives=5,
                 counts=None, device="cuda", seed=0, skip_equal=True, deterministic=False):
        super().__init__()
        num_items, D, K = int(num_items), int(embedding_dim), int(num_negatives)
        side_sizes = [int(n) for n in side_sizes]
        S = 1 + len(side_sizes)
        if num_items < 1 or num_items >= 2 ** 31:
            raise ValueError("EGES: needs 1 <= num_items < 2^31, got %d" % num_items)
        if D % 4 != 0 or not 4 <= D <= 256:
            raise ValueError("EGES: embedding_dim must be a multiple of 4 in [4, 256], got %d" % D)
        if not 0 <= K <= 63:
            raise ValueError("EGES: num_negatives must lie in [0, 63], got %d" % K)
        if S > 16 or any(n < 1 for n in side_sizes):
            raise ValueError("EGES: at most 15 side features, each with at least one value")
        item_side_ids = torch.as_tensor(item_side_ids, dtype=torch.int64).reshape(num_items, S - 1)
        for f, n in enumerate(side_sizes):
            if int(item_side_ids[:, f].max()) >= n:
                raise ValueError("EGES: side feature %d has ids >= its size %d" % (f, n))
        if int(walk_length) < 2 or int(window) < 1:
            raise ValueError("EGES: needs walk_length >= 2 and window >= 1")
        adj = L.as_adjacency(adjacency, device=device)
        if adj is None:
            raise TypeError("EGES: the adjacency must be sparse (a SparseAdjacency or what it accepts)")
        if adj.shape != (num_items, num_items):
            raise ValueError("EGES: the adjacency must be [num_items, num_items], got %s" % (adj.shape,))
        cum, out_weight = _cumulative_weights(adj)
        self.num_items, self.embedding_dim, self.num_negatives, self.num_fields = num_items, D, K, S
        self.skip_equal, self.deterministic, self.seed = bool(skip_equal), bool(deterministic), int(seed)
        self.adjacency, self.walk_length, self.window = adj, int(walk_length), int(window)
        rows = num_items + sum(side_sizes)
        sigma = 1.0 / math.sqrt(D)
        self.side_table = nn.Parameter(L.truncated_normal_(torch.empty((rows, D), dtype=torch.float32, device=device), sigma))
        self.att = nn.Parameter(torch.zeros((num_items, ops._pad4(S)), dtype=torch.float32, device=device))
        self.out_table = nn.Parameter(L.truncated_normal_(torch.empty((num_items, D), dtype=torch.float32, device=device), sigma))
        base = np.concatenate([[0], np.cumsum([num_items] + side_sizes[:-1])]).astype(np.int64) if side_sizes else np.zeros(1, np.int64)
        self.register_buffer("row_base", torch.from_numpy(base).to(device), persistent=False)
        fields = torch.cat([torch.arange(num_items, dtype=torch.int64)[:, None], item_side_ids.clamp_min(-1)], dim=1)
        self.register_buffer("item_fields", fields.to(device), persistent=False)
        self.register_buffer("cum", cum, persistent=False)
        if counts is None:
            counts = out_weight if out_weight.sum() > 0 else None
        if counts is None:
            prob, alias = np.ones(num_items, dtype=np.float32), np.arange(num_items, dtype=np.int32)
        else:
            counts = np.asarray(counts, dtype=np.float64).reshape(-1)
            if counts.size != num_items:
                raise ValueError("EGES: counts must have num_items = %d entries, got %d" % (num_items, counts.size))
            prob, alias = ops.alias_table(counts ** 0.75)
        self.register_buffer("alias_prob", torch.from_numpy(prob).to(device), persistent=False)
        self.register_buffer("alias_index", torch.from_numpy(alias).to(device), persistent=False)
        self.draw_offset = 0
        self.walk_calls = 0
        self._plans = None
        self._scratch = None

    # ---- sampling, as DeepWalk ---------------------------------------------------------------------------------------------------------
    def walks(self, starts):
        """int64 [W, walk_length] weighted walks; every call walks with a seed of its own"""
        seed = (self.seed + 1 + self.walk_calls * _SEED_STRIDE) & (2 ** 64 - 1)
        self.walk_calls += 1
        return ops.random_walk_weighted(self.adjacency.row_ptr, self.adjacency.col, self.cum, self.num_items, starts, self.walk_length, seed)

    def walk_batch(self, starts):
        """(centers, contexts) of one walk per start: skipgram_pairs(walks(starts), window), -1 where there is no pair"""
        return L.skipgram_pairs(self.walks(starts), self.window)

    def sample_negatives(self, batch_size):
        """int64 [batch_size, num_negatives] from the alias table, advancing the running offset"""
        n = int(batch_size) * self.num_negatives
        neg = ops.alias_sample(self.alias_prob, self.alias_index, n, self.seed, self.draw_offset)
        self.draw_offset += n
        return neg.reshape(int(batch_size), self.num_negatives)

    # ---- the step -----------------------------------------------------------------------------------------------------------------------
    def fields_of(self, centers):
        """side_ids int64 [B, S] of the centres: item_fields[centers], a row of -1 for a centre < 0"""
        ok = centers >= 0
        rows = self.item_fields[centers.clamp_min(0)]
        return torch.where(ok[:, None], rows, torch.full_like(rows, -1))

    def plans(self, B):
        """the three slot plans of the sorted K4 (ids [B, S], [B, 1] and [B, 1 + K]), None unless deterministic"""
        if not self.deterministic:
            return None
        S, F, dev = self.num_fields, 1 + self.num_negatives, self.side_table.device
        if self._plans is None or self._plans[0].n < B * S or self._plans[1].n < B or self._plans[2].n < B * F:
            self._plans = (ops.SortPlan(B * S, dev), ops.SortPlan(B, dev), ops.SortPlan(B * F, dev))
            self._scratch = (torch.empty((B * S, self.embedding_dim), dtype=torch.float32, device=dev),
                             torch.empty((B, self.att.shape[1]), dtype=torch.float32, device=dev),
                             torch.empty((B * F, self.embedding_dim), dtype=torch.float32, device=dev))
        return self._plans

    @staticmethod
    def _valid(centers, contexts):
        return max(1, int(((centers >= 0) & (contexts >= 0)).sum().item()))

    def _ids(self, centers, contexts, negatives):
        centers, contexts = centers.reshape(-1), contexts.reshape(-1)
        if negatives is None:
            negatives = self.sample_negatives(centers.shape[0])
        return centers, contexts, negatives

    def loss(self, centers, contexts, negatives=None):
        """mean loss over the valid pairs, differentiable (layers.eges_loss: .grad buffers for any torch optimizer)"""
        centers, contexts, negatives = self._ids(centers, contexts, negatives)
        rows = L.eges_loss(self.side_table, self.row_base, self.fields_of(centers), self.att, centers, self.out_table,
                           contexts.reshape(-1, 1), negatives, None, self.skip_equal, None, self.plans(centers.shape[0]))
        return rows.sum() / self._valid(centers, contexts)

    forward = loss

    def train_step(self, centers, contexts, lr, negatives=None):
        """one SGD step in one pass over the rows: dr_eges_fwd writes the loss and the gradient rows of the mean loss, K4 applies -lr
        times them to side_table, att and out_table (all three buffers are complete before any table changes).  Returns the mean
        loss [] of the batch as the step found it."""
        centers, contexts, negatives = self._ids(centers, contexts, negatives)
        B = centers.shape[0]
        inv = 1.0 / self._valid(centers, contexts)
        plans = self.plans(B)
        side_ids = self.fields_of(centers)
        loss, _, _, _, d_side, d_att, d_ctx = ops.eges_fwd(self.side_table.data, self.row_base, side_ids, self.att.data, centers,
                                                           self.out_table.data, contexts.reshape(B, 1), negatives, None,
                                                           self.skip_equal, row_scale=inv)
        ids_out = torch.cat([contexts.reshape(B, 1), negatives], dim=1)
        p = plans if plans is not None else (None, None, None)
        sc = self._scratch if plans is not None else (None, None, None)
        L.sgns_apply_rows(self.side_table.data, side_ids, d_side, -float(lr), p[0], sc[0], row_base=self.row_base)
        L.sgns_apply_rows(self.att.data, centers.reshape(B, 1), d_att, -float(lr), p[1], sc[1])
        L.sgns_apply_rows(self.out_table.data, ids_out, d_ctx, -float(lr), p[2], sc[2])
        return ops.reduce_sum(loss, alpha=inv).reshape(())

    def embeddings(self, side_ids=None):
        """H [num_items, D] for all items, or [n, D] for the given side_ids [n, S] rows (field 0 the item id, -1 for a cold item, whose
        vector is then the average of its side rows), through dr_eges_embed"""
        if side_ids is None:
            side_ids = self.item_fields
        side_ids = side_ids.to(self.side_table.device)
        return ops.eges_embed(self.side_table.data, self.row_base, side_ids, self.att.data, side_ids[:, 0].contiguous())
