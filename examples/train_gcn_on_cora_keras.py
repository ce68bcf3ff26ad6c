"""examples/train_gcn_on_cora_keras.py of the reference on this package: GCN(32) -> GCN(7, softmax) over Cora's spectral graph,
Adam(0.01), full-batch epochs (up to 200) with the train mask as sample weights, early stopping on the validation loss (patience 3),
then the test loss and weighted accuracy.

  python examples/train_gcn_on_cora_keras.py [--data DIR] [--epochs 200] [--seed 0]

--data DIR reads DIR/cora/cora.{content,cites}.  Without it a seeded Cora-shaped planted-partition graph is generated into a
temporary directory (deep_recommenders_amd.datasets.synthetic_cora), since the data is not shipped."""
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
from deep_recommenders_amd.keras.models.retrieval import GCN  # noqa: E402


class Model(torch.nn.Module):
    def __init__(self, num_classes):
        super().__init__()
        self.g1 = GCN(32)
        self.g2 = GCN(num_classes, activation="softmax")

    def forward(self, graph, feats):
        return self.g2(self.g1(feats, graph), graph)


def weighted_acc(pred, labels, mask):
    hit = (pred.argmax(1) == labels.argmax(1)).astype(np.float64)
    w = mask.astype(np.float64)
    return float((hit * w).sum() / max(w.sum(), 1e-12))


def train_model(data_dir, epochs=200, seed=0, verbose=True):
    np.random.seed(seed)
    torch.manual_seed(seed)
    cora = Cora(data_dir)
    ids, features, labels = cora.load_content()
    graph = cora.build_graph(ids)
    spectral_graph = cora.spectral_graph(graph)
    train, valid, test = cora.split_labels(labels)

    adj = L.SparseAdjacency(spectral_graph)                     # the graph on the device once: plan and transpose are kept
    feats = torch.from_numpy(features.toarray().astype(np.float32)).cuda()
    model = Model(cora.num_classes)
    model(adj, feats)                                           # builds the variables
    opt = optim.Adam(model.parameters(), lr=0.01)

    def dev(a):
        return torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda()

    (train_labels, train_mask), (valid_labels, valid_mask), (test_labels, test_mask) = train, valid, test
    yt, wt, yv, wv = dev(train_labels), train_mask, dev(valid_labels), valid_mask
    best, wait, history = np.inf, 0, []
    for epoch in range(epochs):
        opt.zero_grad(set_to_none=True)
        loss = losses.categorical_crossentropy(yt, model(adj, feats), sample_weight=wt)
        loss.backward()
        opt.step()
        with torch.no_grad():
            pred = model(adj, feats)
            val_loss = losses.categorical_crossentropy(yv, pred, sample_weight=wv).item()
            p = pred.cpu().numpy()
        history.append((loss.item(), val_loss))
        if verbose:
            print("Epoch %d/%d - loss: %.4f - acc: %.4f - val_loss: %.4f - val_acc: %.4f" % (
                epoch + 1, epochs, history[-1][0], weighted_acc(p, train_labels, train_mask), val_loss,
                weighted_acc(p, valid_labels, valid_mask)))
        if val_loss < best:                                     # tf.keras.callbacks.EarlyStopping(patience=3), monitor val_loss
            best, wait = val_loss, 0
        else:
            wait += 1
            if wait >= 3:
                break
    with torch.no_grad():
        pred = model(adj, feats)
        test_loss = losses.categorical_crossentropy(dev(test_labels), pred, sample_weight=test_mask).item()
        test_acc = weighted_acc(pred.cpu().numpy(), test_labels, test_mask)
    print("Test Loss: {:.4f}".format(test_loss))
    print("Test Accuracy: {:.4f}".format(test_acc))
    return test_loss, test_acc, history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help="directory holding cora/cora.content and cora/cora.cites")
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.data is not None:
        train_model(a.data, a.epochs, a.seed)
        return
    with tempfile.TemporaryDirectory() as tmp:
        train_model(synthetic_cora(tmp, seed=a.seed), a.epochs, a.seed)


if __name__ == "__main__":
    main()
