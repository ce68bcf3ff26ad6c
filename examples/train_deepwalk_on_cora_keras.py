"""DeepWalk on Cora, Keras style, on the MI355X hot path: uniform random walks over the citation graph (dr_random_walk), skip-gram pairs
inside a window (layers.skipgram_pairs), negatives from degree ** 0.75 (dr_alias_sample), and the one-pass SGNS step (dr_sgns_fwd + K4 on
both tables).  The reference lists DeepWalk and has no code for it; the model is Perozzi et al. 2014 with the negative-sampling
objective.  No label is used in training: afterwards a logistic probe (one Dense layer on the frozen embeddings, trained on the 140
labelled nodes of the GCN example's split) says what the embeddings know about the classes.

  python examples/train_deepwalk_on_cora_keras.py [--data DIR] [--steps 300] [--seed 0]

--data DIR reads DIR/cora/cora.{content,cites}.  Without it a seeded Cora-shaped planted-partition graph is generated into a
temporary directory (deep_recommenders_amd.datasets.synthetic_cora), since the data is not shipped."""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import layers as L  # noqa: E402
from deep_recommenders_amd import losses, optim  # noqa: E402
from deep_recommenders_amd.datasets import Cora, synthetic_cora  # noqa: E402
from deep_recommenders_amd.keras.models.retrieval import DeepWalk  # noqa: E402


def probe_accuracy(emb, train, test, num_classes, steps=100):
    """test accuracy of softmax(emb W + b) after `steps` full-batch Adam steps on the training nodes; emb is not trained"""
    (train_labels, train_mask), (test_labels, test_mask) = train, test
    W = torch.nn.Parameter(torch.zeros((emb.shape[1], num_classes), device=emb.device))
    b = torch.nn.Parameter(torch.zeros(num_classes, device=emb.device))
    opt = optim.Adam([W, b], lr=0.05)
    y = torch.from_numpy(np.asarray(train_labels, dtype=np.float32)).to(emb.device)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        losses.categorical_crossentropy(y, L.softmax_rows(L.mlp(emb, [W], [b], [0])), sample_weight=train_mask).backward()
        opt.step()
    with torch.no_grad():
        pred = L.mlp(emb, [W], [b], [0]).cpu().numpy().argmax(1)
    hit = (pred == test_labels.argmax(1)).astype(np.float64)
    return float((hit * test_mask).sum() / max(test_mask.sum(), 1))


def train_model(data_dir, steps=300, seed=0, dim=64, walk_length=10, window=3, negatives=5, walks_per_step=512, pair_lr=0.025, verbose=True):
    np.random.seed(seed)
    torch.manual_seed(seed)
    cora = Cora(data_dir)
    ids, _, labels = cora.load_content()
    graph = cora.build_graph(ids)                               # symmetric, no self loops: the walk's graph (not the spectral one)
    train, _, test = cora.split_labels(labels)
    n = graph.shape[0]

    model = DeepWalk(L.SparseAdjacency(graph), dim, walk_length=walk_length, window=window, num_negatives=negatives, seed=seed)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    every = torch.arange(n, dtype=torch.int64, device="cuda")
    held_c, held_o = model.walk_batch(every)                    # one walk from every node, never trained on as a batch
    held_neg = model.sample_negatives(held_c.shape[0])
    before = float(model.train_step(held_c, held_o, 0.0, held_neg))               # lr 0: the loss, the tables untouched
    acc0 = probe_accuracy(model.embeddings().detach(), train, test, cora.num_classes)
    for step in range(steps):
        starts = torch.randint(0, n, (walks_per_step,), device="cuda", generator=gen)
        centers, contexts = model.walk_batch(starts)
        valid = int(((centers >= 0) & (contexts >= 0)).sum())
        loss = model.train_step(centers, contexts, pair_lr * valid)               # the mean loss divides every pair's step by `valid`
        if verbose and (step + 1) % 50 == 0:
            print("step %d/%d - loss: %.4f - pairs: %d" % (step + 1, steps, float(loss), valid))
    after = float(model.train_step(held_c, held_o, 0.0, held_neg))
    acc = probe_accuracy(model.embeddings().detach(), train, test, cora.num_classes)
    print("SGNS loss on held-out walks: {:.4f} -> {:.4f}".format(before, after))
    print("Probe Test Accuracy: {:.4f} (untrained embeddings: {:.4f})".format(acc, acc0))
    return before, after, acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help="directory holding cora/cora.content and cora/cora.cites")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.data is not None:
        train_model(a.data, a.steps, a.seed)
        return
    with tempfile.TemporaryDirectory() as tmp:
        train_model(synthetic_cora(tmp, seed=a.seed), a.steps, a.seed)


if __name__ == "__main__":
    main()
