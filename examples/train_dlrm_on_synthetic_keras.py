#!/usr/bin/env python
"""DLRM on Criteo-shaped synthetic data, Keras style, on the MI355X hot path.

    columns   26 categorical_column_with_hash_bucket fields wrapped in embedding_column(dimension=D)
    model     DLRM(embedding_columns, bottom_units_size=[64, D], top_units_size=[64, 32], dense_features_key="dense")
    compile   loss binary_crossentropy, Adam with Keras' defaults, metrics AUC()
    fit       epochs of `steps` training steps and a validation pass after each (the loop of train_deepfm_on_movielens_keras.py)

The reference's README lists DLRM among its planned models and has neither the model nor an example of it; this script follows the
other Keras examples.  Data is SURVEY.md section 8d's Criteo-shaped recipe at a small size, seeded, nothing is downloaded: 26
single-valued int64 fields whose raw keys are Zipf(1.05)-distributed ranks scrambled into [0, 10^15) and hashed into `--buckets`
buckets each, 13 dense features log1p(|N(0, 1)|), and -- so that there is something to learn -- a label drawn from a planted logit: a
fixed random score per (field, key) for the most frequent keys plus a linear term of the dense features, shifted to a base rate of
about 0.25.

    python examples/train_dlrm_on_synthetic_keras.py --epochs 3 --steps 50
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from deep_recommenders_amd import feature_column as fc                            # noqa: E402
from deep_recommenders_amd import optim                                           # noqa: E402
from deep_recommenders_amd.keras.models.ranking import DLRM                       # noqa: E402
from deep_recommenders_amd.metrics import AUC                                     # noqa: E402
from train_deepfm_on_movielens_keras import run_epoch                             # noqa: E402

FIELDS, NUM_DENSE, HOT_KEYS = 26, 13, 1000


def build_columns(buckets, dimension):
    return [fc.embedding_column(fc.categorical_column_with_hash_bucket("C%d" % (i + 1), buckets, dtype=int), dimension)
            for i in range(FIELDS)]


class CriteoShaped:
    """the seeded generator: the planted scores are fixed by `seed`, the batches by the seed given to batches()"""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.key_score = rng.normal(0.0, 0.6, size=(FIELDS, HOT_KEYS))           # rarer keys score 0
        self.dense_w = rng.normal(0.0, 0.3, size=NUM_DENSE)
        self.salt = rng.integers(1, 10 ** 9, size=FIELDS)

    def batches(self, steps, batch, seed):
        rng = np.random.default_rng(seed)
        for _ in range(steps):
            rank = np.minimum(rng.zipf(1.05, size=(batch, FIELDS)), 10 ** 6) - 1  # 0 = the most frequent key of its field
            keys = (rank.astype(np.int64) * 2654435761 + self.salt) % (10 ** 15)  # raw keys below 10^15, one fixed key per rank
            dense = np.log1p(np.abs(rng.standard_normal((batch, NUM_DENSE)))).astype(np.float32)
            score = np.where(rank < HOT_KEYS, self.key_score[np.arange(FIELDS), np.minimum(rank, HOT_KEYS - 1)], 0.0).sum(1)
            logit = score + dense @ self.dense_w - 1.9
            labels = (rng.random(batch) < 1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
            features = {"C%d" % (i + 1): keys[:, i:i + 1] for i in range(FIELDS)}
            features["dense"] = dense
            yield features, labels.reshape(-1, 1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50, help="training steps per epoch")
    ap.add_argument("--eval-steps", type=int, default=10)
    ap.add_argument("--buckets", type=int, default=20000, help="hash buckets per field")
    ap.add_argument("--dimension", type=int, default=16)
    ap.add_argument("--self-interaction", action="store_true")
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args(argv)

    torch.manual_seed(a.seed)
    model = DLRM(build_columns(a.buckets, a.dimension), bottom_units_size=[64, a.dimension], top_units_size=[64, 32],
                 dense_features_key="dense", self_interaction=a.self_interaction)
    metrics = [AUC()]
    data = CriteoShaped(a.seed)
    val_batches = lambda: data.batches(a.eval_steps, a.batch, a.seed)                         # noqa: E731

    before = run_epoch(model, None, metrics, val_batches())                       # also builds the towers' variables
    print("before training: " + " - ".join("val_%s: %.4f" % (k, v) for k, v in before.items() if k != "examples"), flush=True)
    optimizer = optim.Adam(list(model.parameters()))                              # tf.keras.optimizers.Adam(): 0.001, 0.9, 0.999, 1e-7
    history = []
    for epoch in range(a.epochs):
        t0 = time.time()
        logs = run_epoch(model, optimizer, metrics, data.batches(a.steps, a.batch, a.seed + 1 + epoch))
        val = run_epoch(model, None, metrics, val_batches())
        logs.update({"val_" + k: v for k, v in val.items()})
        history.append(logs)
        print("Epoch %d/%d - %.1fs - " % (epoch + 1, a.epochs, time.time() - t0)
              + " - ".join("%s: %.4f" % (k, v) for k, v in logs.items() if not k.endswith("examples")), flush=True)
    return before, history


if __name__ == "__main__":
    main()
