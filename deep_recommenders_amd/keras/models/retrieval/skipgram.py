"""Skip-gram with negative sampling: SkipGram (= Item2Vec; Word2Vec in keras/models/nlp/word2vec.py) and DeepWalk.  The reference's
README lists Word2Vec, Item2Vec and DeepWalk and ships no code for them; the models are Mikolov et al. 2013, Barkan & Koenigstein 2016
and Perozzi et al. 2014 with the negative-sampling objective.

The whole step runs on three kernel families: dr_alias_sample draws the negatives, dr_sgns_fwd reads the 2 + K rows of every pair once
and writes the loss and both gradient-row buffers, K4 (dr_emb_pool_bwd, or dr_emb_pool_bwd_sorted with `deterministic=True`) applies
them to the two tables.  Pairs with a center or context of -1 (what layers.skipgram_pairs writes for padding and window edges) are
skipped by the kernel; nothing is compacted."""
import math

import numpy as np
import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops

_SEED_STRIDE = 0x9E3779B97F4A7C15        # one walk batch per seed: seed + call * odd constant (mod 2^64)


class SkipGram(nn.Module):
    """in_table / out_table [num_items, embedding_dim], both truncated normal with sigma = 1 / sqrt(D) (as the slab); `counts` [num_items]
    gives the negative distribution counts ** 0.75 (None: uniform).  Negatives are drawn from (seed, running offset): the same seed
    and the same calls give the same run.  deterministic=True keeps two slot plans and takes the sorted K4, whose sums over the slots
    of a shared row have a fixed order: the tables are then bit-reproducible too."""

    def __init__(self, num_items, embedding_dim, num_negatives=5, counts=None, device="cuda", seed=0, skip_equal=True,
                 deterministic=False):
        super().__init__()
        num_items, D, K = int(num_items), int(embedding_dim), int(num_negatives)
        if num_items < 1 or num_items >= 2 ** 31:
            raise ValueError("SkipGram: needs 1 <= num_items < 2^31, got %d" % num_items)
        if D % 4 != 0 or not 4 <= D <= 256:
            raise ValueError("SkipGram: embedding_dim must be a multiple of 4 in [4, 256], got %d" % D)
        if not 0 <= K <= 63:
            raise ValueError("SkipGram: num_negatives must lie in [0, 63], got %d" % K)
        self.num_items, self.embedding_dim, self.num_negatives = num_items, D, K
        self.skip_equal, self.deterministic, self.seed = bool(skip_equal), bool(deterministic), int(seed)
        self.in_table = nn.Parameter(L.truncated_normal_(torch.empty((num_items, D), dtype=torch.float32, device=device), 1.0 / math.sqrt(D)))
        self.out_table = nn.Parameter(L.truncated_normal_(torch.empty((num_items, D), dtype=torch.float32, device=device), 1.0 / math.sqrt(D)))
        if counts is None:
            prob, alias = np.ones(num_items, dtype=np.float32), np.arange(num_items, dtype=np.int32)
        else:
            counts = np.asarray(counts, dtype=np.float64).reshape(-1)
            if counts.size != num_items:
                raise ValueError("SkipGram: counts must have num_items = %d entries, got %d" % (num_items, counts.size))
            prob, alias = ops.alias_table(counts ** 0.75)
        self.register_buffer("alias_prob", torch.from_numpy(prob).to(device), persistent=False)
        self.register_buffer("alias_index", torch.from_numpy(alias).to(device), persistent=False)
        self.draw_offset = 0                # elements drawn so far: the next call continues the stream
        self._plans = None
        self._scratch = None

    def embeddings(self):
        return self.in_table

    def sample_negatives(self, batch_size):
        """int64 [batch_size, num_negatives] from the alias table, advancing the running offset"""
        n = int(batch_size) * self.num_negatives
        neg = ops.alias_sample(self.alias_prob, self.alias_index, n, self.seed, self.draw_offset)
        self.draw_offset += n
        return neg.reshape(int(batch_size), self.num_negatives)

    def plans(self, B):
        """the two slot plans of the sorted K4 (ids [B, 1] and [B, 1 + K]), None unless deterministic"""
        if not self.deterministic:
            return None
        F = 1 + self.num_negatives
        if self._plans is None or self._plans[1].n < B * F:
            self._plans = (ops.SortPlan(B, self.in_table.device), ops.SortPlan(B * F, self.in_table.device))
            self._scratch = torch.empty((B * F, self.embedding_dim), dtype=torch.float32, device=self.in_table.device)
        return self._plans

    @staticmethod
    def _valid(centers, contexts):
        """the number of pairs the kernel does not skip, at least 1: ONE host read per call -- row_scale and K4's scale are scalar
        arguments of their launches"""
        return max(1, int(((centers >= 0) & (contexts >= 0)).sum().item()))

    def _ids(self, centers, contexts, negatives):
        centers, contexts = centers.reshape(-1), contexts.reshape(-1)
        if negatives is None:
            negatives = self.sample_negatives(centers.shape[0])
        return centers, contexts, negatives

    def loss(self, centers, contexts, negatives=None):
        """mean SGNS loss over the valid pairs, differentiable (layers.sgns_loss: .grad buffers for any torch optimizer)"""
        centers, contexts, negatives = self._ids(centers, contexts, negatives)
        rows = L.sgns_loss(self.in_table, self.out_table, centers, contexts, negatives, None, self.skip_equal, None,
                           self.plans(centers.shape[0]))
        return rows.sum() / self._valid(centers, contexts)

    forward = loss

    def train_step(self, centers, contexts, lr, negatives=None):
        """one SGD step in one pass over the rows: dr_sgns_fwd writes the loss and the gradient rows of the mean loss, K4 applies
        -lr times them to both tables (both buffers are complete before either table changes).  Returns the mean loss [] of the
        batch as the step found it."""
        centers, contexts, negatives = self._ids(centers, contexts, negatives)
        B, K, D = centers.shape[0], negatives.shape[1], self.embedding_dim
        inv = 1.0 / self._valid(centers, contexts)
        plans = self.plans(B)
        loss, _, _, d_center, d_ctx = ops.sgns_fwd(self.in_table.data, self.out_table.data, centers, contexts, negatives, None,
                                                   self.skip_equal, row_scale=inv)
        ids_out = torch.cat([contexts.reshape(B, 1), negatives], dim=1)
        plan_in, plan_out = plans if plans is not None else (None, None)
        L.sgns_apply_rows(self.in_table.data, centers.reshape(B, 1), d_center, -float(lr), plan_in, self._scratch)
        L.sgns_apply_rows(self.out_table.data, ids_out, d_ctx, -float(lr), plan_out, self._scratch)
        return ops.reduce_sum(loss, alpha=inv).reshape(())


Item2Vec = SkipGram


class DeepWalk(SkipGram):
    """SkipGram over the nodes of a graph, its sentences uniform random walks (dr_random_walk on the adjacency's device CSR).  The
    negatives follow degree ** 0.75, the walk's stationary distribution standing in for the corpus counts."""

    def __init__(self, adjacency, embedding_dim, walk_length, window, num_negatives=5, device="cuda", seed=0, **kwargs):
        adj = L.as_adjacency(adjacency, device=device)
        if adj is None:
            raise TypeError("DeepWalk: the adjacency must be sparse (a SparseAdjacency or what it accepts)")
        if adj.shape[0] != adj.shape[1]:
            raise ValueError("DeepWalk: the adjacency must be square, got %s" % (adj.shape,))
        if int(walk_length) < 2 or int(window) < 1:
            raise ValueError("DeepWalk: needs walk_length >= 2 and window >= 1")
        degree = np.diff(adj.row_ptr.cpu().numpy()).astype(np.float64)
        super().__init__(adj.shape[0], embedding_dim, num_negatives, counts=degree if degree.sum() > 0 else None, device=device,
                         seed=seed, **kwargs)
        self.adjacency, self.walk_length, self.window = adj, int(walk_length), int(window)
        self.walk_calls = 0

    def walks(self, starts):
        """int64 [W, walk_length]; every call walks with a seed of its own"""
        seed = (self.seed + 1 + self.walk_calls * _SEED_STRIDE) & (2 ** 64 - 1)
        self.walk_calls += 1
        return ops.random_walk(self.adjacency.row_ptr, self.adjacency.col, self.num_items, starts, self.walk_length, seed)

    def walk_batch(self, starts):
        """(centers, contexts) of one walk per start: skipgram_pairs(random_walk(starts), window), -1 where there is no pair"""
        return L.skipgram_pairs(self.walks(starts), self.window)
