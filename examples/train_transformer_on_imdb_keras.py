"""examples/train_transformer_on_imdb_keras.py of the reference on this package: Transformer(vocab 5000, model_dim 8, 2 heads, 2 + 2
stacks, feed-forward 50) -> GlobalAveragePooling1D -> Dense(2, softmax), categorical cross-entropy, Adam(beta_1 0.9, beta_2 0.98,
epsilon 1e-9), batches of 128, 20 % of the training set held out for validation, early stopping on the validation loss
(patience 3), then loss and accuracy on the test set.

As in the reference, the model is fed [x, (x == 0)]: the encoder sees the pre-padded token ids and the DECODER sees the padding
indicator as ids (0 / 1) -- kept as it is.  Dropout has no training switch there, so evaluation runs with dropout too.

  python examples/train_transformer_on_imdb_keras.py [--data imdb.npz] [--epochs 10] [--seed 0]

--data takes a local copy of Keras' imdb.npz (x_train / y_train / x_test / y_test; word indices get Keras' start / oov / offset
treatment, reviews of max_len words or more are dropped, the rest pre-padded).  Nothing is downloaded: without --data the script
trains on a seeded IMDB-shaped SYNTHETIC set -- pre-padded id sequences of random length whose label depends on the tokens (a
review of class c draws 70 % of its words from that class's half of the vocabulary) -- and says so."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import layers as L  # noqa: E402
from deep_recommenders_amd import losses, optim  # noqa: E402
from deep_recommenders_amd.keras.models.nlp import Transformer  # noqa: E402


def pad_sequences(seqs, maxlen):
    """tf.keras.preprocessing.sequence.pad_sequences defaults: pre-padding with 0, pre-truncation"""
    x = np.zeros((len(seqs), maxlen), dtype=np.int64)
    for i, s in enumerate(seqs):
        s = list(s)[-maxlen:]
        if s:
            x[i, maxlen - len(s):] = s
    return x


def synthetic_imdb(vocab_size, max_len, n_train, n_test, seed):
    rng = np.random.default_rng(seed)
    half = (vocab_size - 4) // 2

    def make(n):
        y = rng.integers(0, 2, size=n)
        seqs = []
        for c in y:
            length = int(rng.integers(max_len // 8, max_len))
            own = rng.random(length) < 0.7
            side = np.where(own, c, 1 - c)
            seqs.append([1] + list(4 + side * half + rng.integers(0, half, size=length))[:max_len - 1])
        return pad_sequences(seqs, max_len), np.eye(2, dtype=np.float32)[y]
    return make(n_train), make(n_test)


def load_imdb(path, vocab_size, max_len):
    def prepare(xs, ys):
        seqs, labels = [], []
        for x, y in zip(xs, ys):
            s = [1] + [w + 3 for w in x]                                   # start_char 1, index_from 3
            if len(s) < max_len:                                           # load_data(maxlen=...) drops the longer reviews
                seqs.append([w if w < vocab_size else 2 for w in s])       # oov_char 2
                labels.append(int(y))
        return pad_sequences(seqs, max_len), np.eye(2, dtype=np.float32)[np.asarray(labels)]
    with np.load(path, allow_pickle=True) as f:
        return prepare(f["x_train"], f["y_train"]), prepare(f["x_test"], f["y_test"])


class Model(torch.nn.Module):
    def __init__(self, vocab_size, model_dim=8, n_heads=2, encoder_stack=2, decoder_stack=2, ff_size=50, seed=0):
        super().__init__()
        self.transformer = Transformer(vocab_size, model_dim, n_heads=n_heads, encoder_stack=encoder_stack, decoder_stack=decoder_stack,
                                       feed_forward_size=ff_size, seed=seed)
        self.kernel = torch.nn.Parameter(L.glorot_uniform_(torch.empty((vocab_size, 2), dtype=torch.float32, device="cuda")))
        self.bias = torch.nn.Parameter(torch.zeros(2, dtype=torch.float32, device="cuda"))

    def forward(self, encoder_inputs, decoder_inputs):
        outputs = self.transformer(encoder_inputs, decoder_inputs)
        outputs = L.global_average_pooling_1d(outputs)
        return L.softmax_rows(L.mlp(outputs, [self.kernel], [self.bias], [0]))


def evaluate(model, x, y, batch_size):
    loss, hits = 0.0, 0
    with torch.no_grad():
        for i in range(0, len(x), batch_size):
            xb = torch.from_numpy(x[i:i + batch_size]).cuda()
            yb = torch.from_numpy(y[i:i + batch_size]).cuda()
            p = model(xb, xb == 0)
            loss += losses.categorical_crossentropy(yb, p).item() * len(xb)
            hits += int((p.argmax(1) == yb.argmax(1)).sum().item())
    return loss / max(len(x), 1), hits / max(len(x), 1)


def train_model(data=None, vocab_size=5000, max_len=128, batch_size=128, epochs=10, seed=0, train_samples=4096, test_samples=1024,
                verbose=True):
    np.random.seed(seed)
    torch.manual_seed(seed)
    if data is None:
        print("no --data: training on the seeded IMDB-shaped synthetic set (%d train / %d test sequences)" % (train_samples, test_samples))
        (x_train, y_train), (x_test, y_test) = synthetic_imdb(vocab_size, max_len, train_samples, test_samples, seed)
    else:
        (x_train, y_train), (x_test, y_test) = load_imdb(data, vocab_size, max_len)
    n_val = int(len(x_train) * 0.2)                                        # validation_split=0.2: the last fifth, before shuffling
    x_val, y_val = x_train[len(x_train) - n_val:], y_train[len(y_train) - n_val:]
    x_train, y_train = x_train[:len(x_train) - n_val], y_train[:len(y_train) - n_val]

    model = Model(vocab_size, seed=seed)
    model(torch.from_numpy(x_train[:2]).cuda(), torch.from_numpy(x_train[:2] == 0).cuda())       # builds the variables
    opt = optim.Adam(model.parameters(), beta_1=0.9, beta_2=0.98, epsilon=1e-9)
    rng = np.random.default_rng(seed)
    best, wait, history = np.inf, 0, []
    for epoch in range(epochs):
        t0 = time.time()
        order = rng.permutation(len(x_train))
        run_loss, run_hits, seen = 0.0, 0, 0
        for i in range(0, len(order), batch_size):
            idx = order[i:i + batch_size]
            xb = torch.from_numpy(x_train[idx]).cuda()
            yb = torch.from_numpy(y_train[idx]).cuda()
            opt.zero_grad(set_to_none=True)
            p = model(xb, xb == 0)
            loss = losses.categorical_crossentropy(yb, p)
            loss.backward()
            opt.step()
            run_loss += loss.item() * len(idx)
            run_hits += int((p.argmax(1) == yb.argmax(1)).sum().item())
            seen += len(idx)
        val_loss, val_acc = evaluate(model, x_val, y_val, batch_size)
        history.append((run_loss / seen, run_hits / seen, val_loss, val_acc))
        if verbose:
            print("Epoch %d/%d - %.1fs - loss: %.4f - accuracy: %.4f - val_loss: %.4f - val_accuracy: %.4f" % (
                (epoch + 1, epochs, time.time() - t0) + history[-1]), flush=True)
        if val_loss < best:                                                # tf.keras.callbacks.EarlyStopping(patience=3)
            best, wait = val_loss, 0
        else:
            wait += 1
            if wait >= 3:
                break
    test_loss, test_acc = evaluate(model, x_test, y_test, batch_size)
    print("loss on Test: %.4f" % test_loss)
    print("accu on Test: %.4f" % test_acc)
    return test_loss, test_acc, history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help="a local imdb.npz (Keras' file); without it a synthetic set is generated")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--train-samples", type=int, default=4096, help="size of the synthetic training set")
    ap.add_argument("--test-samples", type=int, default=1024)
    a = ap.parse_args()
    train_model(a.data, batch_size=a.batch_size, epochs=a.epochs, seed=a.seed, train_samples=a.train_samples, test_samples=a.test_samples)


if __name__ == "__main__":
    main()
