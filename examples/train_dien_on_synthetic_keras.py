#!/usr/bin/env python
"""DIEN on a seeded synthetic behaviour-sequence set, Keras style, on the MI355X hot path.

    model     DIEN(num_items, embedding_dim, gru_units, dnn_units_size=(64, 32))  -- item table -> InterestExtractor (GRU) ->
              InterestEvolution (attention + AUGRU) -> Dense tower with Dice -> sigmoid
    loss      binary_crossentropy + aux_weight * model.auxiliary_loss, Adam
    metric    AUC() on a held-out part, after every epoch

The data.  Items belong to one of `--topics` topics (item id mod topics).  A user's history drifts: the topic of step t is the topic of
step t - 1 with probability 0.8, else a fresh one; the item is drawn from that topic.  The label says whether the candidate's topic
is the topic of the user's LAST THREE behaviours' majority -- the recent interest, not the whole history's: the histogram of a long
history says little about it, so a sum pooling of the behaviours cannot solve the task, while a recurrent state can.  Lengths are
uniform in [T / 4, T]; negatives for the auxiliary loss are uniform items.  Nothing is read from disk or downloaded.

    python examples/train_dien_on_synthetic_keras.py --epochs 3 --steps 60
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import losses, optim                                   # noqa: E402
from deep_recommenders_amd.keras.models.ranking import DIEN                       # noqa: E402
from deep_recommenders_amd.metrics import AUC                                     # noqa: E402


def synthetic_batches(steps, batch, T, num_items, topics, seed):
    rng = np.random.default_rng(seed)
    per_topic = num_items // topics
    for _ in range(steps):
        lengths = rng.integers(max(T // 4, 3), T + 1, size=batch)
        topic = np.empty((batch, T), dtype=np.int64)
        topic[:, 0] = rng.integers(0, topics, size=batch)
        for t in range(1, T):
            stay = rng.uniform(size=batch) < 0.8
            topic[:, t] = np.where(stay, topic[:, t - 1], rng.integers(0, topics, size=batch))
        behaviors = topic + topics * rng.integers(0, per_topic, size=(batch, T))              # item id mod topics == its topic
        last3 = np.stack([topic[np.arange(batch), lengths - 1 - k] for k in range(3)], axis=1)
        recent = np.where(last3[:, 1] == last3[:, 2], last3[:, 1], last3[:, 0])               # the majority, else the last
        positive = rng.uniform(size=batch) < 0.5
        cand_topic = np.where(positive, recent, (recent + rng.integers(1, topics, size=batch)) % topics)
        target = cand_topic + topics * rng.integers(0, per_topic, size=batch)
        negatives = rng.integers(0, num_items, size=(batch, T))
        yield behaviors, lengths, target, negatives, positive.astype(np.float32).reshape(batch, 1)


def run_epoch(model, optimizer, metric, batches, aux_weight):
    metric.reset_states()
    total, total_aux, n = 0.0, 0.0, 0
    for behaviors, lengths, target, negatives, y in batches:
        y = torch.from_numpy(y).cuda()
        if optimizer is not None:
            optimizer.zero_grad(set_to_none=True)
            prob = model(behaviors, lengths, target, negatives)
            loss = losses.binary_crossentropy(y, prob)
            aux = model.auxiliary_loss
            (loss + aux_weight * aux).backward()
            optimizer.step()
            total_aux += float(aux.detach())
        else:
            with torch.no_grad():
                prob = model(behaviors, lengths, target)
                loss = losses.binary_crossentropy(y, prob)
        metric.update_state(y, prob.detach())
        total += float(loss)
        n += 1
    return {"loss": total / max(n, 1), "aux": total_aux / max(n, 1), "auc": float(metric.result())}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--eval-steps", type=int, default=10)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--num-items", type=int, default=400)
    ap.add_argument("--topics", type=int, default=8)
    ap.add_argument("--dim", type=int, default=16, help="embedding_dim == gru_units")
    ap.add_argument("--aux-weight", type=float, default=1.0)
    ap.add_argument("--lr", type=float, default=0.005)
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args(argv)

    torch.manual_seed(a.seed)
    model = DIEN(a.num_items, a.dim, a.dim, dnn_units_size=(64, 32))
    metric = AUC()
    val = lambda: synthetic_batches(a.eval_steps, a.batch, a.seq_len, a.num_items, a.topics, a.seed)      # noqa: E731
    before = run_epoch(model, None, metric, val(), a.aux_weight)                  # also builds the layers' variables
    print("before training: val_loss: %.4f - val_auc: %.4f" % (before["loss"], before["auc"]), flush=True)
    optimizer = optim.Adam(list(model.parameters()), lr=a.lr)
    history = []
    for epoch in range(a.epochs):
        t0 = time.time()
        logs = run_epoch(model, optimizer, metric, synthetic_batches(a.steps, a.batch, a.seq_len, a.num_items, a.topics, a.seed + 1 + epoch),
                         a.aux_weight)
        v = run_epoch(model, None, metric, val(), a.aux_weight)
        logs.update(val_loss=v["loss"], val_auc=v["auc"])
        history.append(logs)
        print("Epoch %d/%d - %.1fs - " % (epoch + 1, a.epochs, time.time() - t0) + " - ".join("%s: %.4f" % kv for kv in logs.items()), flush=True)
    return before, history


if __name__ == "__main__":
    main()
