#!/usr/bin/env python
"""DeepFM on MovieLens, Keras style -- the runnable equivalent of the reference's examples/train_deepfm_on_movielens_keras.py on the
MI355X hot path:

    build_columns()  the six feature columns of :11-35 (shared with examples/train_fm_on_movielens_estimator.py)
    model            DeepFM(indicator_columns, embedding_columns, dnn_units_size=[256, 32])                              (:42)
    compile          loss binary_crossentropy, Adam with Keras' defaults, metrics AUC(), Precision(), Recall()          (:43-47)
    fit              epochs of `steps_per_epoch` training steps, a validation pass after each, EarlyStopping(patience=3) on the
                     validation loss                                                                                     (:49-54)

compile / fit are written out as the loop they stand for.  The metrics are device-resident streaming states
(deep_recommenders_amd.metrics): every batch's labels and probabilities stay on the device, update_state() enqueues one histogram
update per metric, and result() is read once per epoch.

Data: `--data movielens.tfrecords` reads the reference's TFRecord file through datasets.MovielensRanking.  Without it the seeded
MovieLens-shaped synthetic stream of the FM example is used (nothing is downloaded): fresh training batches every epoch, one fixed
validation stream.

    python examples/train_deepfm_on_movielens_keras.py --epochs 3 --steps 100
"""
import argparse
import itertools
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from deep_recommenders_amd import losses, optim                                   # noqa: E402
from deep_recommenders_amd.datasets import MovielensRanking                       # noqa: E402
from deep_recommenders_amd.keras.models.ranking import DeepFM                     # noqa: E402
from deep_recommenders_amd.metrics import AUC, Precision, Recall                  # noqa: E402
from train_fm_on_movielens_estimator import build_columns, synthetic_input_fn     # noqa: E402


def _labels(labels, device):
    return torch.as_tensor(labels, dtype=torch.float32).to(device)


def run_epoch(model, optimizer, metrics, batches):
    """One pass over `batches`: a training pass with an optimizer, an evaluation pass without.  The loss is summed on the device and
    the metrics are updated from device tensors; the host reads one loss and one result per metric when the pass is over."""
    for m in metrics:
        m.reset_states()
    total, examples = None, 0
    with torch.enable_grad() if optimizer is not None else torch.no_grad():
        for features, labels in batches:
            prob = model(features)                                                # [B, 1] probabilities (deepfm.py:47)
            y = _labels(labels, prob.device)
            loss = losses.binary_crossentropy(y, prob)
            if optimizer is not None:
                optimizer.zero_grad(set_to_none=True)
                loss.backward()
                optimizer.step()
            for m in metrics:
                m.update_state(y, prob)
            b = y.shape[0]
            total = loss.detach() * b if total is None else total + loss.detach() * b
            examples += b
    logs = {"loss": float(total) / examples if examples else float("nan"), "examples": examples}
    logs.update({m.name: m.result() for m in metrics})
    return logs


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help="movielens.tfrecords written by the reference's datasets/movielens.py")
    ap.add_argument("--batch", type=int, default=1024, help="MovielensRanking's default, which the reference script uses")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=None, help="training steps per epoch (with --data: train_steps_per_epoch; else 100)")
    ap.add_argument("--eval-steps", type=int, default=None, help="validation steps (with --data: test_steps; else 20)")
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args(argv)

    torch.manual_seed(a.seed)
    indicator_columns, embedding_columns = build_columns()
    model = DeepFM(indicator_columns, embedding_columns, dnn_units_size=[256, 32])
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

    before = run_epoch(model, None, metrics, val_batches())                       # also builds the DNN's variables
    print("before training: " + " - ".join("val_%s: %.4f" % (k, v) for k, v in before.items() if k != "examples"), flush=True)
    optimizer = optim.Adam(list(model.parameters()))                              # tf.keras.optimizers.Adam(): 0.001, 0.9, 0.999, 1e-7
    best, wait, history = float("inf"), 0, []
    for epoch in range(a.epochs):
        t0 = time.time()
        logs = run_epoch(model, optimizer, metrics, train_batches(epoch))
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
    return before, history


if __name__ == "__main__":
    main()
