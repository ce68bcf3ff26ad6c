"""EGES on synthetic sessions, Keras style, on the MI355X hot path: DeepWalk over the weighted item graph of the sessions, the centre's
vector an attention-weighted sum of the item's own row and its side feature's row (Wang et al., KDD 2018; the reference lists EGES
and has no code for it).

    data      `--items` items in blocks of `--block` (the generator of the Item2Vec example: a session is `--length` items of ONE block,
              one in ten replaced by any item); the block is the item's side feature.  A share `--cold` of the items is held out of
              every session: they have no edge, are never a centre, and their own rows are never trained
    graph     graph_from_sessions: consecutive items -> directed edges, duplicates summed into weights
    step      EGES.walk_batch (dr_random_walk_weighted + skipgram_pairs) and EGES.train_step (dr_alias_sample, dr_eges_fwd in its
              one-pass form, K4 on side_table, att and out_table)
    check     the loss on held-out walks before and after, and the fraction of items whose nearest neighbour by cosine of
              embeddings() lies in the item's own block -- for warm items by their full fields, for cold items by their side feature
              alone (field 0 = -1: the cold-start rule)

  python examples/train_eges_on_synthetic_keras.py [--steps 300] [--items 2000] [--block 100] [--cold 0.1] [--seed 0]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import ops  # noqa: E402
from deep_recommenders_amd.keras.models.retrieval import EGES, graph_from_sessions  # noqa: E402
from deep_recommenders_amd.keras.models.retrieval.factorized_top_k import BruteForce  # noqa: E402


def sessions(rng, n, warm, items, block, length):
    """[n, length] int64 over the warm items: a block per session, warm items of it, one in ten from anywhere"""
    by_block = [warm[warm // block == k] for k in range(items // block)]
    out = np.empty((n, length), dtype=np.int64)
    for i, k in enumerate(rng.integers(0, items // block, size=n)):
        out[i] = rng.choice(by_block[k], size=length)
    noise = rng.random((n, length)) < 0.1
    out[noise] = rng.choice(warm, size=int(noise.sum()))
    return out


def own_block_fraction(emb, index_rows, query_rows, block):
    """share of query_rows whose nearest other row among index_rows (by cosine) lies in their own block"""
    emb = ops.rows_scale(emb.contiguous(), ops.rowdot(emb, emb), mode=1)           # x / |x|: inner product = cosine
    index = emb[index_rows].contiguous()
    _, ids = BruteForce(k=2).index(index)(emb[query_rows].contiguous())
    hit = index_rows[ids]                                                          # item numbers of the two best
    nearest = torch.where(hit[:, 0] == query_rows, hit[:, 1], hit[:, 0])           # the first hit may be the item itself
    return float(((nearest // block) == (query_rows // block)).float().mean())


def train_model(steps=300, items=2000, block=100, length=8, window=2, dim=32, negatives=5, walks=512, walk_length=8, pair_lr=0.025,
                cold=0.1, seed=0, verbose=True):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    is_cold = rng.random(items) < cold
    warm, cold_items = np.flatnonzero(~is_cold), np.flatnonzero(is_cold)
    graph = graph_from_sessions(sessions(rng, 8192, warm, items, block, length), items)
    side = (np.arange(items) // block).reshape(items, 1)
    model = EGES(items, [items // block], side, dim, graph, walk_length=walk_length, window=window, num_negatives=negatives, seed=seed)
    warm_t = torch.from_numpy(warm).cuda()
    cold_t = torch.from_numpy(cold_items).cuda()

    def fractions():
        fields = model.item_fields.clone()
        fields[cold_t, 0] = -1                                                     # a cold item is served from its side feature alone
        emb = model.embeddings(fields)
        return own_block_fraction(emb, warm_t, warm_t, block), own_block_fraction(emb, warm_t, cold_t, block)

    held_c, held_o = model.walk_batch(warm_t[torch.from_numpy(rng.integers(0, len(warm), size=2048)).cuda()])
    held_neg = model.sample_negatives(held_c.shape[0])
    before = float(model.train_step(held_c, held_o, 0.0, held_neg))               # lr 0: the loss, the tables untouched
    warm0, cold0 = fractions()
    for step in range(steps):
        starts = warm_t[torch.from_numpy(rng.integers(0, len(warm), size=walks)).cuda()]
        centers, contexts = model.walk_batch(starts)
        valid = int(((centers >= 0) & (contexts >= 0)).sum())
        loss = model.train_step(centers, contexts, pair_lr * valid)               # the mean loss divides every pair's step by `valid`
        if verbose and (step + 1) % 50 == 0:
            print("step %d/%d - loss: %.4f - pairs: %d of %d" % (step + 1, steps, float(loss), valid, centers.numel()))
    after = float(model.train_step(held_c, held_o, 0.0, held_neg))
    warm1, cold1 = fractions()
    print("EGES loss on held-out walks: {:.4f} -> {:.4f}".format(before, after))
    print("Warm items ({}) whose nearest neighbour lies in their own block: {:.4f} (untrained: {:.4f})".format(len(warm), warm1, warm0))
    print("Cold items ({}, side feature only) whose nearest warm neighbour lies in their own block: {:.4f} (untrained: {:.4f}, "
          "chance: {:.4f})".format(len(cold_items), cold1, cold0, block / items))
    return before, after, warm1, cold1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--cold", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    train_model(a.steps, a.items, a.block, cold=a.cold, seed=a.seed)


if __name__ == "__main__":
    main()
