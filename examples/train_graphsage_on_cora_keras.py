"""Mini-batch node classification with GraphSAGE (or PinSage) on Cora: the graph and split of examples/train_gcn_on_cora_keras.py,
trained on batches of seed nodes whose neighbourhoods are sampled on the device each step instead of on the whole graph.

  python examples/train_graphsage_on_cora_keras.py [--data DIR] [--model sage|pinsage] [--aggregator mean|gcn] [--steps 200]
                                                   [--batch 64] [--fanouts 10,5] [--seed 0]

--data DIR reads DIR/cora/cora.{content,cites}.  Without it a seeded Cora-shaped planted-partition graph is generated into a
temporary directory (deep_recommenders_amd.datasets.synthetic_cora), since the data is not shipped.  Prints the accuracy on the nodes
outside the training set before and after training."""
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
from deep_recommenders_amd.keras.models.retrieval import GraphSAGE, PinSage  # noqa: E402
from deep_recommenders_amd.keras.models.retrieval.graphsage import pad_feature_columns  # noqa: E402


def build_model(kind, num_classes, fanouts, aggregator="mean", hidden=32):
    units = [hidden] * len(fanouts)
    if kind == "pinsage":
        return PinSage(units, fanouts, num_walks=16, walk_length=3, num_classes=num_classes, aggregator=aggregator)
    return GraphSAGE(units, fanouts, aggregator=aggregator, num_classes=num_classes)


def accuracy(model, feats, adj, nodes, labels, seed, batch=512):
    hit = 0
    with torch.no_grad():
        for i in range(0, len(nodes), batch):
            part = nodes[i:i + batch]
            pred = model(feats, adj, torch.from_numpy(part), seed).argmax(1).cpu().numpy()
            hit += int((pred == labels[part]).sum())
    return hit / max(len(nodes), 1)


def train_model(data_dir, kind="sage", aggregator="mean", steps=200, batch=64, fanouts=(10, 5), seed=0, verbose=True):
    """returns (accuracy before, accuracy after, the training loss of every step)"""
    np.random.seed(seed)
    torch.manual_seed(seed)
    cora = Cora(data_dir)
    ids, features, labels = cora.load_content()
    graph = cora.build_graph(ids)
    onehot = cora.encode_labels(labels).astype(np.float32)
    y = onehot.argmax(1)
    train_nodes = np.asarray(sorted(cora.sample_train_nodes(labels)), dtype=np.int64)
    rest = np.setdiff1d(np.arange(len(ids), dtype=np.int64), train_nodes)

    adj = L.SparseAdjacency(graph.tocsr())                      # the whole graph on the device once; every step samples from it
    feats = pad_feature_columns(torch.from_numpy(features.toarray().astype(np.float32))).cuda()    # 1433 -> 1536 columns, once
    targets = torch.from_numpy(onehot).cuda()
    model = build_model(kind, cora.num_classes, list(fanouts), aggregator)
    model(feats, adj, torch.from_numpy(train_nodes[:2]), 0)     # builds the variables
    opt = optim.Adam(model.parameters(), lr=0.01)
    before = accuracy(model, feats, adj, rest, y, seed=10 ** 6)
    r = np.random.RandomState(seed)
    history = []
    for step in range(steps):
        seeds = torch.from_numpy(np.sort(r.choice(train_nodes, size=min(batch, len(train_nodes)), replace=False)))
        opt.zero_grad(set_to_none=True)
        pred = model(feats, adj, seeds, seed=step + 1)          # a fresh neighbourhood sample every step
        loss = losses.categorical_crossentropy(targets[seeds.cuda()], pred)
        loss.backward()
        opt.step()
        history.append(loss.item())
        if verbose and (step % 20 == 0 or step == steps - 1):
            print("step %d/%d - loss: %.4f" % (step + 1, steps, history[-1]))
    after = accuracy(model, feats, adj, rest, y, seed=10 ** 6)
    print("Accuracy before: {:.4f}".format(before))
    print("Accuracy after: {:.4f}".format(after))
    return before, after, history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help="directory holding cora/cora.content and cora/cora.cites")
    ap.add_argument("--model", default="sage", choices=["sage", "pinsage"])
    ap.add_argument("--aggregator", default="mean", choices=["mean", "gcn"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--fanouts", default="10,5")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    fanouts = [int(f) for f in a.fanouts.split(",")]
    if a.data is not None:
        train_model(a.data, a.model, a.aggregator, a.steps, a.batch, fanouts, a.seed)
        return
    with tempfile.TemporaryDirectory() as tmp:
        train_model(synthetic_cora(tmp, seed=a.seed), a.model, a.aggregator, a.steps, a.batch, fanouts, a.seed)


if __name__ == "__main__":
    main()
