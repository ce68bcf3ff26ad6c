"""Item2Vec on synthetic sessions, Keras style, on the MI355X hot path: skip-gram with negative sampling over item sessions (Barkan &
Koenigstein 2016; the reference lists Item2Vec and has no code for it).

    data      `--items` items in blocks of `--block`; a session is `--length` items of ONE block (one in ten replaced by any item),
              padded with -1 to show the kernel's skipping; seeded
    pairs     layers.skipgram_pairs(sessions, window): every (item, neighbour in the window), -1 where there is none
    step      SkipGram.train_step: negatives from counts ** 0.75 (dr_alias_sample), dr_sgns_fwd in its one-pass form, K4 on both tables
    check     the SGNS loss on held-out sessions before and after, and the fraction of items whose nearest neighbour by cosine of
              in_table (the BruteForce top-K over the normalised rows) lies in the item's own block

  python examples/train_item2vec_on_synthetic_keras.py [--steps 300] [--items 2000] [--block 100] [--seed 0]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import layers as L  # noqa: E402
from deep_recommenders_amd import ops  # noqa: E402
from deep_recommenders_amd.keras.models.retrieval import Item2Vec  # noqa: E402
from deep_recommenders_amd.keras.models.retrieval.factorized_top_k import BruteForce  # noqa: E402


def sessions(rng, n, items, block, length):
    """[n, length + 2] int64: a block per session, items of it, one in ten from anywhere, the last two positions padding"""
    base = rng.integers(0, items // block, size=(n, 1)) * block
    s = base + rng.integers(0, block, size=(n, length))
    noise = rng.random((n, length)) < 0.1
    s[noise] = rng.integers(0, items, size=int(noise.sum()))
    return torch.from_numpy(np.concatenate([s, np.full((n, 2), -1)], axis=1)).cuda()


def own_block_fraction(model, block):
    emb = model.embeddings().detach().contiguous()
    emb = ops.rows_scale(emb, ops.rowdot(emb, emb), mode=1)                        # x / |x|: inner product = cosine
    _, ids = BruteForce(k=2).index(emb)(emb)                                       # the first hit is the item itself
    item = torch.arange(emb.shape[0], device=emb.device)
    nearest = torch.where(ids[:, 0] == item, ids[:, 1], ids[:, 0])
    return float(((nearest // block) == (item // block)).float().mean())


def train_model(steps=300, items=2000, block=100, length=8, window=2, dim=32, negatives=5, batch=1024, pair_lr=0.025, seed=0, verbose=True):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    corpus = sessions(rng, 4096, items, block, length).cpu().numpy().reshape(-1)
    counts = np.bincount(corpus[corpus >= 0], minlength=items) + 1
    model = Item2Vec(items, dim, num_negatives=negatives, counts=counts, seed=seed)
    held_c, held_o = L.skipgram_pairs(sessions(rng, 2048, items, block, length), window)
    held_neg = model.sample_negatives(held_c.shape[0])
    before = float(model.train_step(held_c, held_o, 0.0, held_neg))               # lr 0: the loss, the tables untouched
    frac0 = own_block_fraction(model, block)
    for step in range(steps):
        centers, contexts = L.skipgram_pairs(sessions(rng, batch, items, block, length), window)
        valid = int(((centers >= 0) & (contexts >= 0)).sum())
        loss = model.train_step(centers, contexts, pair_lr * valid)               # the mean loss divides every pair's step by `valid`
        if verbose and (step + 1) % 50 == 0:
            print("step %d/%d - loss: %.4f - pairs: %d of %d" % (step + 1, steps, float(loss), valid, centers.numel()))
    after = float(model.train_step(held_c, held_o, 0.0, held_neg))
    frac = own_block_fraction(model, block)
    print("SGNS loss on held-out sessions: {:.4f} -> {:.4f}".format(before, after))
    print("Nearest neighbour in the item's own block: {:.4f} (untrained: {:.4f}, chance: {:.4f})".format(frac, frac0, (block - 1) / (items - 1)))
    return before, after, frac


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    train_model(a.steps, a.items, a.block, seed=a.seed)


if __name__ == "__main__":
    main()
