#!/usr/bin/env python
"""NFM on MovieLens, Keras style, on the MI355X hot path -- examples/train_ffm_on_movielens_keras.py with the model exchanged:

    build_columns()  the six categorical columns of the FM / DeepFM examples, embedded with dimension 16
    model            NFM(indicator_columns, embedding_columns, dnn_units_size=[64, 32]): linear term + MLP over the Bi-Interaction vector
    compile          sigmoid cross-entropy, Adam with Keras' defaults, metrics AUC(), Precision(), Recall()
    fit              epochs of `steps_per_epoch` calls of model.train_step, a validation pass after each, EarlyStopping(patience=3) on
                     the validation loss

The reference lists NFM and has no code for it; the model is He & Chua 2017.  NFM has no autograd Function of its own: the training
pass calls `model.train_step(features, labels, optimizer)`, which runs the backward kernels explicitly.  `movie_genres` is multi-valued,
so this example takes the K3 + rows path; with single-valued fields only the gather path runs.  `--data movielens.tfrecords` reads the
reference's TFRecord file, without it the seeded MovieLens-shaped synthetic stream is used (nothing is downloaded).

    python examples/train_nfm_on_movielens_keras.py --epochs 3 --steps 100
"""
import argparse
import itertools
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from deep_recommenders_amd import optim                                           # noqa: E402
from deep_recommenders_amd.datasets import MovielensRanking                       # noqa: E402
from deep_recommenders_amd.keras.models.ranking import NFM                        # noqa: E402
from deep_recommenders_amd.metrics import AUC, Precision, Recall                  # noqa: E402
from train_deepfm_on_movielens_keras import run_epoch                             # noqa: E402
from train_fm_on_movielens_estimator import build_columns, synthetic_input_fn     # noqa: E402


def train_epoch(model, optimizer, batches):
    """one training pass by model.train_step; the loss is summed on the device and read once"""
    total, examples = None, 0
    for features, labels in batches:
        y = torch.as_tensor(labels, dtype=torch.float32).reshape(-1)
        loss = model.train_step(features, y, optimizer)
        total = loss * y.shape[0] if total is None else total + loss * y.shape[0]
        examples += y.shape[0]
    return {"loss": float(total) / examples if examples else float("nan"), "examples": examples}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help="movielens.tfrecords written by the reference's datasets/movielens.py")
    ap.add_argument("--batch", type=int, default=1024, help="MovielensRanking's default")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=None, help="training steps per epoch (with --data: train_steps_per_epoch; else 100)")
    ap.add_argument("--eval-steps", type=int, default=None, help="validation steps (with --data: test_steps; else 20)")
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--bi-dropout", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args(argv)

    torch.manual_seed(a.seed)
    indicator_columns, embedding_columns = build_columns()
    model = NFM(indicator_columns, embedding_columns, dnn_units_size=[64, 32], dropout=a.dropout, bi_dropout=a.bi_dropout)
    predict = lambda features: model(features).reshape(-1, 1)                     # noqa: E731  ([B, 1], as run_epoch pairs it with the labels)
    metrics = [AUC(), Precision(), Recall()]

    if a.data:
        movielens = MovielensRanking(epochs=a.epochs, batch_size=a.batch, filename=a.data)
        steps = a.steps or movielens.train_steps_per_epoch
        eval_steps = a.eval_steps or movielens.test_steps
        stream = movielens.training_input_fn                                      # `epochs` passes over the training part, as one stream
        train_batches = lambda epoch: itertools.islice(stream, steps)             # noqa: E731
        val_batches = lambda: itertools.islice(movielens.testing_input_fn, eval_steps)   # noqa: E731
    else:
        steps, eval_steps = a.steps or 100, a.eval_steps or 20
        print("no --data: training on the seeded MovieLens-shaped synthetic stream (%d steps of %d per epoch)" % (steps, a.batch))
        train_batches = lambda epoch: synthetic_input_fn(steps, a.batch, a.seed + 1 + epoch)      # noqa: E731
        val_batches = lambda: synthetic_input_fn(eval_steps, a.batch, a.seed)                     # noqa: E731

    model.eval()
    before = run_epoch(predict, None, metrics, val_batches())
    print("before training: " + " - ".join("val_%s: %.4f" % (k, v) for k, v in before.items() if k != "examples"), flush=True)
    optimizer = optim.Adam(list(model.parameters()))                              # tf.keras.optimizers.Adam(): 0.001, 0.9, 0.999, 1e-7
    best, wait, history = float("inf"), 0, []
    for epoch in range(a.epochs):
        t0 = time.time()
        model.train()
        logs = train_epoch(model, optimizer, train_batches(epoch))
        model.eval()
        val = run_epoch(predict, None, metrics, val_batches())
        logs.update({"val_" + k: v for k, v in val.items()})
        history.append(logs)
        print("Epoch %d/%d - %.1fs - " % (epoch + 1, a.epochs, time.time() - t0)
              + " - ".join("%s: %.4f" % (k, v) for k, v in logs.items() if not k.endswith("examples")), flush=True)
        if val["loss"] < best:                                                    # tf.keras.callbacks.EarlyStopping(patience=3)
            best, wait = val["loss"], 0
        else:
            wait += 1
            if wait >= 3:
                print("no improvement of val_loss for 3 epochs: stopping")
                break
    return before, history


if __name__ == "__main__":
    main()
