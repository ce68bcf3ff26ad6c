#!/usr/bin/env python
"""PNN on MovieLens, Keras style, on the MI355X hot path -- examples/train_deepfm_on_movielens_keras.py with the model exchanged:

    build_columns()  the six embedding columns of the FM / DeepFM examples (PNN has no linear term)
    model            PNN(embedding_columns, [64, 32], use_inner=True, use_outer=True)      (the paper's PNN*)
    compile          loss binary_crossentropy, Adam with Keras' defaults, metrics AUC(), Precision(), Recall()
    fit              epochs of `steps_per_epoch` training steps, a validation pass after each, EarlyStopping(patience=3) on the
                     validation loss

The reference lists PNN and has no code for it; the model (product layer over the concatenated embeddings, their pairwise inner products
and the outer product of their sum, then Dense layers) is Qu et al. 2016.  Data handling, the training loop and the device-resident
metrics are the DeepFM example's: `--data movielens.tfrecords` reads the reference's TFRecord file, without it the seeded
MovieLens-shaped synthetic stream is used (nothing is downloaded).  The validation AUC is printed before and after training.

    python examples/train_pnn_on_movielens_keras.py --epochs 3 --steps 100 [--no-inner | --no-outer]
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
from deep_recommenders_amd.keras.models.ranking import PNN                        # noqa: E402
from deep_recommenders_amd.metrics import AUC, Precision, Recall                  # noqa: E402
from train_deepfm_on_movielens_keras import run_epoch                             # noqa: E402
from train_fm_on_movielens_estimator import build_columns, synthetic_input_fn     # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help="movielens.tfrecords written by the reference's datasets/movielens.py")
    ap.add_argument("--batch", type=int, default=1024, help="MovielensRanking's default")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=None, help="training steps per epoch (with --data: train_steps_per_epoch; else 100)")
    ap.add_argument("--eval-steps", type=int, default=None, help="validation steps (with --data: test_steps; else 20)")
    ap.add_argument("--units", default="64,32", help="dnn_units_size: the product layer's width, then the Dense layers'")
    ap.add_argument("--no-inner", action="store_true", help="OPNN: without the inner products")
    ap.add_argument("--no-outer", action="store_true", help="IPNN: without the outer product")
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args(argv)

    torch.manual_seed(a.seed)
    _, embedding_columns = build_columns()
    model = PNN(embedding_columns, [int(u) for u in a.units.split(",")], use_inner=not a.no_inner, use_outer=not a.no_outer)
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
    before = run_epoch(model, None, metrics, val_batches())                       # also builds the layers' variables
    print("before training: " + " - ".join("val_%s: %.4f" % (k, v) for k, v in before.items() if k != "examples"), flush=True)
    optimizer = optim.Adam(list(model.parameters()))                              # tf.keras.optimizers.Adam(): 0.001, 0.9, 0.999, 1e-7
    best, wait, history = float("inf"), 0, []
    for epoch in range(a.epochs):
        t0 = time.time()
        model.train()
        logs = run_epoch(model, optimizer, metrics, train_batches(epoch))
        model.eval()
        val = run_epoch(model, None, metrics, val_batches())
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
    print("validation AUC: %.4f before training, %.4f after" % (before["auc"], history[-1]["val_auc"]))
    return before, history


if __name__ == "__main__":
    main()
