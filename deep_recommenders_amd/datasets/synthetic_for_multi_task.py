"""The synthetic two-task regression data of the MMoE paper (Ma et al., KDD 2018, section 3.2), with the interface of the reference's
deep_recommenders/datasets/synthetic_for_multi_task.py (SyntheticForMultiTask(num_examples, example_dim, c, p, m).input_fn).

Generator, for d = example_dim:
  u1 ~ N(0, I_d), centred and scaled to norm 1;  u2 ~ N(0, I_d) made orthogonal to u1 and scaled to norm 1
  w1 = c u1,  w2 = c (p u1 + sqrt(1 - p^2) u2)            (so cos(w1, w2) = p: the task correlation)
  alpha_i, beta_i ~ N(0, 1) for i < m;  x ~ N(0, I_d) per example
  y_k = w_k . x + sum_i sin(alpha_i w_k . x + beta_i) + N(0, 0.01^2)     k = 1, 2
Features are float32 columns "C0" .. "C{d-1}" of shape [b, 1]; labels "labels0", "labels1" of shape [b]."""
import numpy as np


def synthetic_data(num_examples, example_dim=100, c=0.3, p=0.8, m=5, rng=None):
    rng = np.random.RandomState() if rng is None else rng
    u1 = rng.normal(size=example_dim)
    u1 = (u1 - u1.mean()) / (u1.std() * np.sqrt(example_dim))
    u2 = rng.normal(size=example_dim)
    u2 -= u2.dot(u1) * u1
    u2 /= np.linalg.norm(u2)
    w1 = c * u1
    w2 = c * (p * u1 + np.sqrt(1.0 - p ** 2) * u2)
    alpha = rng.normal(size=m)
    beta = rng.normal(size=m)
    x = rng.normal(size=(num_examples, example_dim))
    labels = []
    for w in (w1, w2):
        wx = x @ w
        y = wx + np.sin(np.outer(wx, alpha) + beta).sum(axis=1) + rng.normal(size=num_examples, scale=0.01)
        labels.append(y.astype(np.float32))
    return x.astype(np.float32), tuple(labels)


class SyntheticForMultiTask:

    def __init__(self, num_examples, example_dim=100, c=0.3, p=0.8, m=5, seed=None):
        self._num_examples = int(num_examples)
        self._example_dim = int(example_dim)
        self._c, self._p, self._m = c, p, int(m)
        self._seed = seed

    def data(self):
        """(examples [N, d] float32, (labels0 [N], labels1 [N])) -- the same arrays for the same seed"""
        return synthetic_data(self._num_examples, self._example_dim, self._c, self._p, self._m, np.random.RandomState(self._seed))

    def input_fn(self, epochs=1, batch_size=512, buffer_size=512):
        """Iterator of (features, labels) batches in order, `epochs` passes, the last partial batch kept (the reference batches
        without drop_remainder).  buffer_size is the reference's prefetch depth and has no effect here."""
        x, (y0, y1) = self.data()
        d = self._example_dim

        def gen():
            n = x.shape[0]
            for _ in range(epochs):
                for s in range(0, n, batch_size):
                    xb = x[s:s + batch_size]
                    feats = {"C{}".format(i): xb[:, i:i + 1] for i in range(d)}
                    yield feats, {"labels0": y0[s:s + batch_size], "labels1": y1[s:s + batch_size]}
        return gen()
