"""IntentGC on a seeded synthetic marketplace: users and items fall into taste blocks, a user clicks items of their own block, and each
side has two kinds of auxiliary nodes (users: search words and visited shops; items: brands and categories) that follow the blocks
with noise.  translate_relations turns each incidence matrix into a user-user or item-item relation (R = 2 per side), and the dual
IntentNet is trained with the triplet loss over negatives shared by the batch.

  python examples/train_intentgc_on_synthetic_keras.py [--users 2000] [--items 3000] [--steps 200] [--batch 256] [--negatives 64]
                                                       [--seed 0]

Prints the triplet loss on a fixed held-out batch and recall@10 of top_k over all items for the held-out clicks, before and after."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import optim  # noqa: E402
from deep_recommenders_amd.keras.models.retrieval import IntentGC, translate_relations  # noqa: E402


def _incidence(r, block, num_blocks, per_block, links, noise):
    """[N, num_blocks * per_block] 0/1: every node links to `links` auxiliary nodes, of its own block's group except with probability
    `noise`"""
    N, A = block.size, num_blocks * per_block
    B = np.zeros((N, A), dtype=np.float32)
    for v in range(N):
        for _ in range(links):
            g = r.randint(num_blocks) if r.rand() < noise else block[v]
            B[v, g * per_block + r.randint(per_block)] = 1.0
    return B


def make_data(num_users=2000, num_items=3000, num_blocks=8, feature_dim=16, seed=0):
    """a dict of host arrays: the blocks, the four incidence matrices, weakly informative features, the clicks split into train / held-out"""
    r = np.random.RandomState(seed)
    ub, ib = r.randint(num_blocks, size=num_users), r.randint(num_blocks, size=num_items)
    proto = r.standard_normal((num_blocks, feature_dim)).astype(np.float32)
    feat = lambda b: (0.5 * proto[b] + r.standard_normal((b.size, feature_dim))).astype(np.float32)
    by_block = [np.flatnonzero(ib == g) for g in range(num_blocks)]
    clicks = []
    for u in range(num_users):
        own = by_block[ub[u]]
        for _ in range(4):
            clicks.append((u, int(own[r.randint(own.size)]) if own.size and r.rand() < 0.9 else int(r.randint(num_items))))
    clicks = np.asarray(clicks, dtype=np.int64)
    r.shuffle(clicks)
    n_held = max(16, len(clicks) // 20)
    return dict(num_users=num_users, num_items=num_items, user_block=ub, item_block=ib, user_features=feat(ub), item_features=feat(ib),
                user_aux=[_incidence(r, ub, num_blocks, 6, 3, 0.2), _incidence(r, ub, num_blocks, 4, 2, 0.3)],
                item_aux=[_incidence(r, ib, num_blocks, 5, 2, 0.2), _incidence(r, ib, num_blocks, 3, 1, 0.1)],
                train=clicks[n_held:], held=clicks[:n_held])


def build_model(data, embedding_dim=32, num_filters=4, fanouts=(5, 3), dnn_units_size=(32, 16), top_k=10, seed=0):
    user_rel = [translate_relations(B, top_k) for B in data["user_aux"]]
    item_rel = [translate_relations(B, top_k) for B in data["item_aux"]]
    return IntentGC(user_rel, item_rel, torch.from_numpy(data["user_features"]).cuda(), torch.from_numpy(data["item_features"]).cuda(),
                    embedding_dim=embedding_dim, num_layers=len(fanouts), num_filters=num_filters, fanouts=fanouts,
                    dnn_units_size=dnn_units_size, margin=0.2, seed=seed)


def evaluate(model, data, negatives, k=10):
    """{"loss": the triplet loss of the held-out clicks against fixed negatives, "recall@k": the share of them in the user's top k}"""
    users, items = torch.from_numpy(data["held"][:, 0].copy()), torch.from_numpy(data["held"][:, 1].copy())
    with torch.no_grad():
        loss = model.loss(users, items, negatives, seed=10 ** 6).item()
        model.index(torch.arange(data["num_items"]), k=k, seed=10 ** 6)
        _, top = model.top_k(users, k=k, seed=10 ** 6)
    hit = (top.cpu() == items[:, None]).any(dim=1).float().mean().item()
    return {"loss": loss, "recall@%d" % k: hit}


def train_model(data, steps=200, batch=256, num_negatives=64, lr=0.01, seed=0, verbose=True):
    """returns (model, held-out figures before, after, the training loss of every step)"""
    model = build_model(data, seed=seed)
    opt = optim.Adam(model.parameters(), lr=lr)
    r = np.random.RandomState(seed + 1)
    eval_neg = torch.from_numpy(r.randint(data["num_items"], size=num_negatives).astype(np.int64))
    before = evaluate(model, data, eval_neg)
    train = data["train"]
    history = []
    for step in range(steps):
        rows = r.choice(len(train), size=min(batch, len(train)), replace=False)
        neg = r.randint(data["num_items"], size=num_negatives).astype(np.int64)
        loss = model.train_step(torch.from_numpy(train[rows, 0].copy()), torch.from_numpy(train[rows, 1].copy()), torch.from_numpy(neg),
                                optimizer=opt, seed=step + 1)            # a fresh neighbourhood sample every step
        history.append(loss.item())
        if verbose and (step % 20 == 0 or step == steps - 1):
            print("step %d/%d - loss: %.4f - active: %.3f" % (step + 1, steps, history[-1], model.active_fraction.item()))
    after = evaluate(model, data, eval_neg)
    if verbose:
        for name, f in (("before", before), ("after", after)):
            print("held-out %s: %s" % (name, ", ".join("%s %.4f" % kv for kv in sorted(f.items()))))
    return model, before, after, history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=2000)
    ap.add_argument("--items", type=int, default=3000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--negatives", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    data = make_data(args.users, args.items, seed=args.seed)
    train_model(data, steps=args.steps, batch=args.batch, num_negatives=args.negatives, seed=args.seed)


if __name__ == "__main__":
    main()
