"""YoutubeNet on a synthetic watch log, Keras style, on the MI355X hot path: the candidate-generation network of Covington et al.
(RecSys 2016; the reference lists YoutubeNet and has no code for it), trained with the sampled softmax.

    data      `--videos` videos in taste blocks of `--block`, popularity falling with the id inside the whole catalogue (the order
              the log-uniform sampler expects); a user belongs to one block, the history is `--history` watches from it (one in ten
              from anywhere, some positions padded with -1), the search tokens name the block, the label is the next watch; seeded,
              no file
    tower     one EmbeddingSlab over the history and search bags (mean-pooled), the example age joined as a numeric feature, a ReLU
              tower; slab.sparse_lr is the fused SGD on the slab, the tower's weights take torch SGD
    step      YoutubeNet.train_step: `--sampled` negatives per step for the whole batch (dr_alias_sample, log-uniform),
              dr_sampled_softmax_fwd / _bwd, K4 on the class table
    check     the FULL-softmax loss over all videos on held-out users and recall@10 of top_k, before and after

  python examples/train_youtubenet_on_synthetic_keras.py [--steps 300] [--videos 2000] [--block 50] [--sampled 200] [--seed 0]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import feature_column as fc  # noqa: E402
from deep_recommenders_amd import ops  # noqa: E402
from deep_recommenders_amd.keras.models.retrieval import YoutubeNet  # noqa: E402


def watch_log(rng, n, videos, block, history):
    """(inputs, labels): the users' blocks are interleaved over the catalogue (video v belongs to block v % n_blocks), so that every
    block has popular and rare videos and the label's popularity falls with its id"""
    n_blocks = videos // block
    user_block = rng.integers(0, n_blocks, size=n)
    rank = np.minimum((rng.pareto(1.0, size=(n, history + 1)) * 2).astype(np.int64), block - 1)      # popular ranks more often
    watched = rank * n_blocks + user_block[:, None]
    noise = rng.random((n, history + 1)) < 0.1
    watched[noise] = rng.integers(0, videos, size=int(noise.sum()))
    hist, labels = watched[:, :history].copy(), watched[:, history].copy()
    hist[:, 1:][rng.random((n, history - 1)) < 0.2] = -1
    inputs = {"history": torch.from_numpy(hist).cuda(), "search": torch.from_numpy(user_block[:, None].copy()).cuda(),
              "age": torch.from_numpy(rng.random((n, 1)).astype(np.float32)).cuda()}
    return inputs, torch.from_numpy(labels).cuda()


def evaluate(model, inputs, labels):
    """(full-softmax loss over all classes, recall@10): the softmax over the whole class table, which training never computes"""
    with torch.no_grad():
        u = model.call(inputs).contiguous()
        logits = ops.scores_nt(u, model.class_table.data).contiguous()
        onehot = torch.zeros_like(logits)
        onehot[torch.arange(labels.shape[0], device=labels.device), labels] = 1.0
        loss = float(ops.softmax_ce_rows(logits, onehot)) / labels.shape[0]
    _, ids = model.top_k(inputs, k=10)
    recall = float((ids == labels[:, None]).any(dim=1).float().mean())
    return loss, recall


def train_model(steps=300, videos=2000, block=50, history=8, dim=16, units=(64, 32), sampled=200, batch=1024, row_lr=0.125, tower_lr=0.5, seed=0,
                verbose=True):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    n_blocks = videos // block
    columns = [fc.embedding_column(fc.categorical_column_with_identity("history", videos), dim),
               fc.embedding_column(fc.categorical_column_with_identity("search", n_blocks), dim)]
    model = YoutubeNet(columns, videos, list(units), sampled, dense_features_key="age", seed=seed).build(1)
    model.slab.sparse_lr = row_lr * batch               # the mean loss divides every row's step by the batch
    opt = torch.optim.SGD(list(model.dnn_kernels) + list(model.dnn_biases), lr=tower_lr)
    held_in, held_lab = watch_log(rng, 4096, videos, block, history)
    loss0, recall0 = evaluate(model, held_in, held_lab)
    for step in range(steps):
        inputs, labels = watch_log(rng, batch, videos, block, history)
        loss = model.train_step(inputs, labels, row_lr * batch, optimizer=opt)
        if verbose and (step + 1) % 50 == 0:
            print("step %d/%d - sampled-softmax loss: %.4f" % (step + 1, steps, float(loss)))
    loss1, recall1 = evaluate(model, held_in, held_lab)
    print("Full-softmax loss on held-out users: {:.4f} -> {:.4f} (log V = {:.4f})".format(loss0, loss1, float(np.log(videos))))
    print("Recall@10 of top_k on held-out users: {:.4f} (untrained: {:.4f}, chance: {:.4f})".format(recall1, recall0, 10.0 / videos))
    return loss0, loss1, recall0, recall1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--videos", type=int, default=2000)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--sampled", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    train_model(a.steps, a.videos, a.block, sampled=a.sampled, seed=a.seed)


if __name__ == "__main__":
    main()
