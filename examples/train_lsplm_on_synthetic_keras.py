#!/usr/bin/env python
"""LS-PLM on a synthetic piece-wise linear stream, on the MI355X hot path.

    columns  `--fields` identity columns of `--buckets` ids each (single-valued), wrapped as indicator columns: the sparse x
    teacher  a fixed LS-PLM of `--teacher-regions` regions with large weights draws the labels: the click probability is piece-wise
             linear in x, which a plain logistic model cannot follow
    model    LSPLM(indicator_columns, num_regions): p = sum_i softmax_i(u . x) sigmoid(w_i . x)
    fit      plain SGD by model.train_step(features, labels, lr): one fused forward + loss + gradient kernel, K4, the bias update

The reference lists LS-PLM and has no code for it; the model is Gai et al. 2017 without the paper's L1 + L2,1 regulariser and its
quasi-Newton solver.  `--data file.npz` (arrays `ids` [N, F] int64 and `labels` [N]) trains on recorded examples instead; nothing is
downloaded.

    python examples/train_lsplm_on_synthetic_keras.py --epochs 5 --steps 200
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import feature_column as fc                            # noqa: E402
from deep_recommenders_amd.keras.models.ranking import LSPLM                      # noqa: E402
from deep_recommenders_amd.metrics import AUC                                     # noqa: E402


def teacher(fields, buckets, regions, seed=12345):
    """the "true" model: (gate [F, buckets, regions], expert [F, buckets, regions])"""
    world = np.random.default_rng(seed)
    return world.normal(0, 2.0, (fields, buckets, regions)), world.normal(0, 1.5, (fields, buckets, regions))


def synthetic_input_fn(steps, batch, seed, fields, buckets, world):
    gate, expert = world
    rng = np.random.default_rng(seed)
    f = np.arange(fields)[None, :]
    for _ in range(steps):
        ids = rng.integers(0, buckets, (batch, fields))
        u, w = gate[f, ids].sum(1), expert[f, ids].sum(1)
        pi = np.exp(u - u.max(1, keepdims=True))
        pi /= pi.sum(1, keepdims=True)
        p = (pi / (1.0 + np.exp(-w))).sum(1)
        yield ids, (rng.random(batch) < p).astype(np.float32)


def recorded_input_fn(ids, labels, batch, lo, hi):
    for s in range(lo, hi, batch):
        yield ids[s:min(s + batch, hi)], labels[s:min(s + batch, hi)].astype(np.float32)


def features_of(ids):
    t = torch.from_numpy(np.ascontiguousarray(ids))
    return {"f%d" % i: t[:, i:i + 1] for i in range(ids.shape[1])}


def evaluate(model, batches):
    auc, total, n = AUC(), 0.0, 0
    auc.reset_states()
    for ids, y in batches:
        feats, labels = features_of(ids), torch.from_numpy(y)
        total += model.loss(feats, labels).item() * len(y)
        auc.update_state(labels.cuda().reshape(-1, 1), model(feats))
        n += len(y)
    return {"loss": total / max(n, 1), "auc": auc.result()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help=".npz with `ids` [N, F] int64 and `labels` [N]; the last tenth is held out")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--eval-steps", type=int, default=20)
    ap.add_argument("--fields", type=int, default=8)
    ap.add_argument("--buckets", type=int, default=50)
    ap.add_argument("--regions", type=int, default=12, help="m, the model's regions")
    ap.add_argument("--teacher-regions", type=int, default=4)
    ap.add_argument("--lr", type=float, default=10.0, help="SGD on the MEAN loss: a row seen by B / buckets examples moves by about lr / buckets")
    ap.add_argument("--deterministic", action="store_true", help="the sorted K4: bit-reproducible on shared rows")
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args(argv)

    torch.manual_seed(a.seed)
    if a.data:
        rec = np.load(a.data)
        ids, labels = rec["ids"].astype(np.int64), rec["labels"].reshape(-1)
        fields, buckets, cut = ids.shape[1], int(ids.max()) + 1, len(ids) - len(ids) // 10
        train_batches = lambda epoch: recorded_input_fn(ids, labels, a.batch, 0, cut)              # noqa: E731
        val_batches = lambda: recorded_input_fn(ids, labels, a.batch, cut, len(ids))                # noqa: E731
    else:
        fields, buckets = a.fields, a.buckets
        world = teacher(fields, buckets, a.teacher_regions)
        print("no --data: training on the seeded synthetic stream (%d steps of %d per epoch, %d fields of %d ids, a teacher of %d regions)"
              % (a.steps, a.batch, fields, buckets, a.teacher_regions))
        train_batches = lambda epoch: synthetic_input_fn(a.steps, a.batch, a.seed + 1 + epoch, fields, buckets, world)   # noqa: E731
        val_batches = lambda: synthetic_input_fn(a.eval_steps, a.batch, a.seed, fields, buckets, world)                 # noqa: E731

    columns = [fc.indicator_column(fc.categorical_column_with_identity("f%d" % i, buckets)) for i in range(fields)]
    model = LSPLM(columns, num_regions=a.regions)
    before = evaluate(model, val_batches())
    print("before training: val_loss: %.4f - val_auc: %.4f" % (before["loss"], before["auc"]), flush=True)
    history = []
    for epoch in range(a.epochs):
        t0, total, n = time.time(), None, 0
        for ids_b, y in train_batches(epoch):
            loss = model.train_step(features_of(ids_b), torch.from_numpy(y), a.lr, deterministic=a.deterministic)
            total = loss * len(y) if total is None else total + loss * len(y)
            n += len(y)
        val = evaluate(model, val_batches())
        logs = {"loss": float(total) / max(n, 1), "val_loss": val["loss"], "val_auc": val["auc"]}
        history.append(logs)
        print("Epoch %d/%d - %.1fs - " % (epoch + 1, a.epochs, time.time() - t0) + " - ".join("%s: %.4f" % kv for kv in logs.items()),
              flush=True)
    return before, history


if __name__ == "__main__":
    main()
