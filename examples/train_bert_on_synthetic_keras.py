#!/usr/bin/env python
"""BERT pre-training (masked LM + next-sentence prediction) on a synthetic corpus, on the MI355X hot path.

    corpus   `--topics` topics, each owning a block of `--block` ordinary tokens; a sentence draws its tokens from ONE topic's block.
             An example is [CLS] A [SEP] B [SEP]: B continues A's topic (label 0, "is next") or comes from another topic (label 1)
    model    BERT(vocab, hidden, layers, heads, ...) + BertPretraining: the masked-LM head tied to the token table and the NSP head
    fit      BertPretraining.pretrain_step: dynamic masking on the device (dr_mlm_mask), the fused embedding kernel, the encoder on
             the attention / GEMM / GELU kernels, the chunked full-vocabulary cross-entropy, optim.Adam

A masked token can be predicted from its sentence's topic (loss log(block) at best, against log(vocab - 5) for the uniform guess) and
the two sentences' topics decide the NSP label.  Held-out masked-LM loss and NSP accuracy are printed before and after.  The reference
lists BERT and has no code for it.  `--data file.npz` (arrays `ids` [N, L] int64, `segments` [N, L] int64, `nsp` [N] int64, ids 0..4
being [PAD] [UNK] [CLS] [SEP] [MASK]) trains on recorded examples instead, the last tenth held out; nothing is downloaded and no
tokeniser is included.

    python examples/train_bert_on_synthetic_keras.py --epochs 3 --steps 100
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import optim                                           # noqa: E402
from deep_recommenders_amd.keras.models.nlp import BERT, BertPretraining          # noqa: E402

PAD, UNK, CLS, SEP, MASK, NUM_SPECIAL = 0, 1, 2, 3, 4, 5


def synthetic_input_fn(steps, batch, seed, length, topics, block):
    rng = np.random.default_rng(seed)
    la = (length - 3) // 2
    lb = length - 3 - la
    for _ in range(steps):
        ta = rng.integers(0, topics, batch)
        nsp = rng.integers(0, 2, batch)
        tb = np.where(nsp == 0, ta, (ta + 1 + rng.integers(0, topics - 1, batch)) % topics)
        a = NUM_SPECIAL + ta[:, None] * block + rng.integers(0, block, (batch, la))
        b = NUM_SPECIAL + tb[:, None] * block + rng.integers(0, block, (batch, lb))
        ids = np.concatenate([np.full((batch, 1), CLS), a, np.full((batch, 1), SEP), b, np.full((batch, 1), SEP)], axis=1)
        seg = np.concatenate([np.zeros((batch, la + 2), np.int64), np.ones((batch, lb + 1), np.int64)], axis=1)
        yield ids.astype(np.int64), seg, nsp.astype(np.int64)


def recorded_input_fn(ids, seg, nsp, batch, lo, hi):
    for s in range(lo, hi, batch):
        e = min(s + batch, hi)
        yield ids[s:e], seg[s:e], nsp[s:e]


def _cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def evaluate(head, batches, prob, max_predictions):
    """held-out masked-LM loss and NSP accuracy; the masks of the evaluation are seeded by the batch number"""
    mlm, hits, n = 0.0, 0, 0
    for k, (ids, seg, nsp) in enumerate(batches):
        ids_d, seg_d, nsp_d = _cuda(ids, seg, nsp)
        masked, positions, labels = head.mask(ids_d, prob, max_predictions, seed=10 ** 6 + k)
        loss, _ = head.losses(masked, seg_d, positions, labels, nsp_d)
        with torch.no_grad():
            seq, _ = head.bert(masked, seg_d)
            logits = head.nsp_logits(seq[:, 0, :].contiguous())
        mlm += float(loss) * len(nsp)
        hits += int((logits.argmax(1) == nsp_d).sum())
        n += len(nsp)
    return {"mlm_loss": mlm / max(n, 1), "nsp_acc": hits / max(n, 1)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help=".npz with `ids`, `segments` [N, L] int64 and `nsp` [N]; the last tenth is held out")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--eval-steps", type=int, default=10)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--topics", type=int, default=16)
    ap.add_argument("--block", type=int, default=8, help="ordinary tokens per topic")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--intermediate", type=int, default=256)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--prob", type=float, default=0.15)
    ap.add_argument("--max-predictions", type=int, default=5)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args(argv)

    torch.manual_seed(a.seed)
    if a.data:
        rec = np.load(a.data)
        ids, seg, nsp = rec["ids"].astype(np.int64), rec["segments"].astype(np.int64), rec["nsp"].astype(np.int64).reshape(-1)
        vocab, length, cut = int(ids.max()) + 1, ids.shape[1], len(ids) - len(ids) // 10
        train_batches = lambda epoch: recorded_input_fn(ids, seg, nsp, a.batch, 0, cut)                # noqa: E731
        val_batches = lambda: recorded_input_fn(ids, seg, nsp, a.batch, cut, len(ids))                  # noqa: E731
    else:
        vocab, length = NUM_SPECIAL + a.topics * a.block, a.length
        print("no --data: training on the seeded synthetic corpus (%d steps of %d per epoch, %d topics of %d tokens, length %d; "
              "uniform guess %.3f, topic known %.3f)" % (a.steps, a.batch, a.topics, a.block, length, np.log(vocab - NUM_SPECIAL),
                                                           np.log(a.block)))
        train_batches = lambda epoch: synthetic_input_fn(a.steps, a.batch, a.seed + 1 + epoch, length, a.topics, a.block)   # noqa: E731
        val_batches = lambda: synthetic_input_fn(a.eval_steps, a.batch, a.seed, length, a.topics, a.block)                 # noqa: E731

    bert = BERT(vocab, a.hidden, a.layers, a.heads, a.intermediate, max_position=max(length, 16), hidden_dropout=a.dropout,
                attention_dropout=a.dropout, seed=a.seed)
    head = BertPretraining(bert, NUM_SPECIAL, MASK)
    optimizer = optim.Adam(head.parameters(), lr=a.lr)
    before = evaluate(head, val_batches(), a.prob, a.max_predictions)
    print("before training: val_mlm_loss: %.4f - val_nsp_acc: %.4f" % (before["mlm_loss"], before["nsp_acc"]), flush=True)
    history = []
    for epoch in range(a.epochs):
        t0, mlm, nsp_l, n = time.time(), None, None, 0
        for ids_b, seg_b, nsp_b in train_batches(epoch):
            l1, l2 = head.pretrain_step(*_cuda(ids_b, seg_b, nsp_b), optimizer, prob=a.prob, max_predictions=a.max_predictions)
            mlm = l1 if mlm is None else mlm + l1
            nsp_l = l2 if nsp_l is None else nsp_l + l2
            n += 1
        val = evaluate(head, val_batches(), a.prob, a.max_predictions)
        logs = {"mlm_loss": float(mlm) / max(n, 1), "nsp_loss": float(nsp_l) / max(n, 1), "val_mlm_loss": val["mlm_loss"],
                "val_nsp_acc": val["nsp_acc"]}
        history.append(logs)
        print("Epoch %d/%d - %.1fs - " % (epoch + 1, a.epochs, time.time() - t0) + " - ".join("%s: %.4f" % kv for kv in logs.items()),
              flush=True)
    return before, history


if __name__ == "__main__":
    main()
