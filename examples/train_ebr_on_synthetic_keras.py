"""EBR on a synthetic search log, Keras style, on the MI355X hot path: the two-tower model of Huang et al. (KDD 2020; the reference
lists EBR and has no code for it), trained with the in-batch triplet loss on cosine similarities, with and without online
hard-negative mining.

    data      queries and documents in `--topics` topic blocks; a text is a bag of `--bag` hashed token ids drawn from the block's
              vocabulary, one in five a noise token from anywhere, some positions padded with -1; a query also carries the searcher's
              city and a document its own, equal for a matching pair four times in five; seeded, no file
    towers    per side one EmbeddingSlab over the token bag (mean-pooled) and the city, a ReLU tower; slab.sparse_lr is the fused SGD
              on the slabs, the towers' weights take torch SGD
    step      EBR.train_step: both towers, dr_margin_rank_fwd / _bwd over the batch's own documents as negatives (all of them, or each
              query's `--hard` highest-scoring ones), torch.autograd.backward([q, d], [d_q, d_d])
    check     on a held-out corpus: the in-batch triplet loss, the share of active (query, negative) pairs, and recall@10 of top_k
              (the query's own document among the 10 nearest of the corpus by cosine), before and after

    runs      one over all in-batch negatives; one that spends the second half of its steps on the mined negatives

  python examples/train_ebr_on_synthetic_keras.py [--steps 300] [--topics 500] [--hard 2] [--seed 0] [--all-lr 0.02 0.05] [--hard-lr 0.05 0.1]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import feature_column as fc  # noqa: E402
from deep_recommenders_amd import ops  # noqa: E402
from deep_recommenders_amd.keras.models.retrieval import EBR  # noqa: E402

CITIES = 20


def search_log(rng, n, topics, vocab, bag):
    """(query inputs, document inputs): pair i is a query and the document it was answered with, both from one topic block"""
    per = vocab // topics
    topic = rng.integers(0, topics, size=n)

    def text():
        tok = topic[:, None] * per + rng.integers(0, per, size=(n, bag))
        noise = rng.random((n, bag)) < 0.2
        tok[noise] = rng.integers(0, vocab, size=int(noise.sum()))
        tok[:, 1:][rng.random((n, bag - 1)) < 0.2] = -1
        return tok
    city = rng.integers(0, CITIES, size=(n, 1))
    doc_city = np.where(rng.random((n, 1)) < 0.8, city, rng.integers(0, CITIES, size=(n, 1)))
    q = {"query_tokens": torch.from_numpy(text()).cuda(), "query_city": torch.from_numpy(city).cuda()}
    d = {"doc_tokens": torch.from_numpy(text()).cuda(), "doc_city": torch.from_numpy(doc_city).cuda()}
    return q, d


def evaluate(model, q_in, d_in):
    """(held-out in-batch triplet loss, active fraction, recall@10 of the query's own document in the held-out corpus)"""
    n = q_in["query_tokens"].shape[0]
    with torch.no_grad():
        q, d = model.query_vectors(q_in), model.document_vectors(d_in)
        _, rows, active, _, _ = ops.margin_rank_fwd(q, d, None, margin=model.margin, metric=model.metric, num_hard=model.num_hard_negatives)
        per_row = model.num_hard_negatives if model.num_hard_negatives > 0 else n - 1
        loss, frac = float(rows.sum()) / n, float(active.sum()) / (n * per_row)
    model.index(d_in, k=10)
    _, ids = model.top_k(q_in, 10)
    recall = float((ids == torch.arange(n, device=ids.device)[:, None]).any(dim=1).float().mean())
    return loss, frac, recall


def train_model(steps=300, topics=500, vocab=5000, bag=6, dim=16, units=(64, 32), hard=0, batch=1024, all_lr=(0.02, 0.05), hard_lr=(0.05, 0.1),
                seed=0, verbose=True):
    """hard == 0: `steps` steps over all in-batch negatives.  hard > 0: the first half of the steps the same way, the second half over
    each query's `hard` highest-scoring negatives: hard negatives complement the random ones, as the paper finds.  The loss over all
    negatives is a sum of ~batch terms per row and takes the (row, tower) learning rates all_lr; the mined one has `hard` terms and
    takes hard_lr.  The cosine makes the loss invariant to the scale of the towers' outputs, so the outcome depends little on the
    rates (the same figures to within a few per cent from all_lr 5e-5 to 2e-2)."""
    rng = np.random.default_rng(seed)
    cols = lambda side: [fc.embedding_column(fc.categorical_column_with_identity(side + "_tokens", vocab), dim),      # noqa: E731
                         fc.embedding_column(fc.categorical_column_with_identity(side + "_city", CITIES), dim)]
    model = EBR(cols("query"), cols("doc"), list(units), margin=0.2, num_hard_negatives=0, seed=seed).build()
    dense = [p for t in (model.query_tower, model.document_tower) for p in list(t.dnn_kernels) + list(t.dnn_biases)]
    opt = torch.optim.SGD(dense, lr=all_lr[1])

    def rates(lr):
        for tower in (model.query_tower, model.document_tower):
            tower.slab.sparse_lr = lr[0] * batch            # the mean loss divides every row's step by the batch
        for group in opt.param_groups:
            group["lr"] = lr[1]
    rates(all_lr)
    held_q, held_d = search_log(rng, 2048, topics, vocab, bag)
    what = "all in-batch negatives" + (", then the %d hardest" % hard if hard else "")
    loss0, frac0, recall0 = evaluate(model, held_q, held_d)
    for step in range(steps):
        if hard and step == steps // 2:
            loss_h, frac_h, recall_h = evaluate(model, held_q, held_d)
            print("%s: after %d steps over all negatives: held-out triplet loss %.4f, recall@10 %.4f" % (what, step, loss_h, recall_h))
            model.num_hard_negatives = hard
            rates(hard_lr)
            loss_m, frac_m, _ = evaluate(model, held_q, held_d)
            print("%s: the mined loss at the switch: %.4f, active fraction %.3f" % (what, loss_m, frac_m))
        q_in, d_in = search_log(rng, batch, topics, vocab, bag)
        loss = model.train_step(q_in, d_in, optimizer=opt)
        if verbose and (step + 1) % 50 == 0:
            print("step %d/%d - triplet loss: %.4f - active fraction: %.3f" % (step + 1, steps, float(loss), float(model.active_fraction)))
    loss1, frac1, recall1 = evaluate(model, held_q, held_d)
    if hard:
        print("%s: held-out mined triplet loss %.4f -> %.4f, active fraction %.3f -> %.3f" % (what, loss_m, loss1, frac_m, frac1))
    else:
        print("%s: held-out triplet loss %.4f -> %.4f, active fraction %.3f -> %.3f" % (what, loss0, loss1, frac0, frac1))
    print("%s: recall@10 of top_k on the held-out corpus of 2048: %.4f (untrained: %.4f, chance: %.4f)" % (what, recall1, recall0, 10.0 / 2048))
    return loss0, loss1, recall0, recall1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--topics", type=int, default=500)
    ap.add_argument("--hard", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--all-lr", type=float, nargs=2, default=(0.02, 0.05), help="(row, tower) learning rates over all negatives")
    ap.add_argument("--hard-lr", type=float, nargs=2, default=(0.05, 0.1), help="(row, tower) learning rates over the mined negatives")
    a = ap.parse_args()
    train_model(a.steps, a.topics, hard=0, all_lr=tuple(a.all_lr), hard_lr=tuple(a.hard_lr), seed=a.seed)
    train_model(a.steps, a.topics, hard=a.hard, all_lr=tuple(a.all_lr), hard_lr=tuple(a.hard_lr), seed=a.seed)


if __name__ == "__main__":
    main()
