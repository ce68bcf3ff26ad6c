"""Airbnb's listing embeddings (Grbovic & Cheng, KDD 2018, "Real-time Personalization using Embeddings for Search Ranking at Airbnb"):
skip-gram over click sessions with the session's booked listing as a second positive of every pair (the "global context"), and extra
negatives drawn from the centre's own market.  The reference's README lists the model and ships no code for it.

The step is dr_eges_fwd with one field, no attention and two positives [context, booked] -- with booked = -1 everywhere it is
SkipGram's step bit for bit.  The market negatives come from dr_random_walk with L = 2 over a CSR whose rows are the markets and whose
columns are their listings: a walk that starts at market_of[centre] steps to a uniform member of that market."""
import numpy as np
import torch

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.retrieval.skipgram import SkipGram, _SEED_STRIDE


class Airbnb(SkipGram):
    """SkipGram over num_listings with market_of int64 [num_listings] (each listing's market, >= 0).  Every example has num_negatives
    draws from the alias table followed by num_market_negatives uniform members of the centre's market."""

    def __init__(self, num_listings, embedding_dim, market_of, num_negatives=5, num_market_negatives=5, counts=None, device="cuda",
                 seed=0, skip_equal=True, deterministic=False):
        Km = int(num_market_negatives)
        if Km < 0 or 2 + int(num_negatives) + Km > 64:
            raise ValueError("Airbnb: 2 positives + num_negatives + num_market_negatives must be <= 64")
        super().__init__(num_listings, embedding_dim, num_negatives, counts=counts, device=device, seed=seed, skip_equal=skip_equal,
                         deterministic=deterministic)
        market_of = np.asarray(market_of, dtype=np.int64).reshape(-1)
        if market_of.size != self.num_items or (market_of.size and market_of.min() < 0):
            raise ValueError("Airbnb: market_of needs one market >= 0 per listing")
        self.num_market_negatives = Km
        self.num_markets = int(market_of.max()) + 1 if market_of.size else 0
        order = np.argsort(market_of, kind="stable")
        row_ptr = np.concatenate([[0], np.cumsum(np.bincount(market_of, minlength=self.num_markets))]).astype(np.int64)
        self.register_buffer("market_of", torch.from_numpy(market_of).to(device), persistent=False)
        self.register_buffer("market_ptr", torch.from_numpy(row_ptr).to(device), persistent=False)
        self.register_buffer("market_listings", torch.from_numpy(order.astype(np.int32)).to(device), persistent=False)
        self.register_buffer("row_base", torch.zeros(1, dtype=torch.int64, device=device), persistent=False)
        self.market_calls = 0

    def sample_market_negatives(self, centers):
        """int64 [B, num_market_negatives]: uniform members of market_of[centers[b]]; -1 for a centre < 0"""
        B, Km = centers.shape[0], self.num_market_negatives
        if Km == 0:
            return torch.empty((B, 0), dtype=torch.int64, device=centers.device)
        market = torch.where(centers >= 0, self.market_of[centers.clamp_min(0)], torch.full_like(centers, -1))
        seed = (self.seed + 2 + self.market_calls * _SEED_STRIDE) & (2 ** 64 - 1)
        self.market_calls += 1
        starts = market[:, None].expand(B, Km).reshape(-1)
        walks = ops.random_walk(self.market_ptr, self.market_listings, self.num_markets, starts, 2, seed)
        return walks[:, 1].reshape(B, Km)

    def plans(self, B):
        """the two slot plans of the sorted K4 (ids [B, 1] and [B, 2 + K + Km]), None unless deterministic"""
        if not self.deterministic:
            return None
        F = 2 + self.num_negatives + self.num_market_negatives
        if self._plans is None or self._plans[1].n < B * F:
            self._plans = (ops.SortPlan(B, self.in_table.device), ops.SortPlan(B * F, self.in_table.device))
            self._scratch = torch.empty((B * F, self.embedding_dim), dtype=torch.float32, device=self.in_table.device)
        return self._plans

    def _slots(self, centers, contexts, booked, negatives):
        centers, contexts, booked = centers.reshape(-1), contexts.reshape(-1), booked.reshape(-1)
        if negatives is None:
            negatives = torch.cat([self.sample_negatives(centers.shape[0]), self.sample_market_negatives(centers)], dim=1)
        return centers, contexts, torch.stack([contexts, booked], dim=1), negatives

    def loss(self, centers, contexts, booked, negatives=None):
        """mean loss over the valid pairs, differentiable (layers.eges_loss)"""
        centers, contexts, positives, negatives = self._slots(centers, contexts, booked, negatives)
        plans = self.plans(centers.shape[0])                                       # (in, out); there is no attention table to plan for
        rows = L.eges_loss(self.in_table, self.row_base, centers.reshape(-1, 1), None, None, self.out_table, positives, negatives, None,
                           self.skip_equal, None, None if plans is None else (plans[0], None, plans[1]))
        return rows.sum() / self._valid(centers, contexts)

    forward = loss

    def train_step(self, centers, contexts, booked, lr, negatives=None):
        """one SGD step: positives [context, booked] (booked int64 [B], -1 for a session without a booking), negatives int64
        [B, num_negatives + num_market_negatives] or None to draw them.  Returns the mean loss [] of the batch as the step found it."""
        centers, contexts, positives, negatives = self._slots(centers, contexts, booked, negatives)
        B = centers.shape[0]
        inv = 1.0 / self._valid(centers, contexts)
        plans = self.plans(B)
        side_ids = centers.reshape(B, 1)
        loss, _, _, _, d_side, _, d_ctx = ops.eges_fwd(self.in_table.data, self.row_base, side_ids, None, None, self.out_table.data,
                                                       positives, negatives, None, self.skip_equal, row_scale=inv)
        ids_out = torch.cat([positives, negatives], dim=1)
        plan_in, plan_out = plans if plans is not None else (None, None)
        L.sgns_apply_rows(self.in_table.data, side_ids, d_side, -float(lr), plan_in, self._scratch)
        L.sgns_apply_rows(self.out_table.data, ids_out, d_ctx, -float(lr), plan_out, self._scratch)
        return ops.reduce_sum(loss, alpha=inv).reshape(())
