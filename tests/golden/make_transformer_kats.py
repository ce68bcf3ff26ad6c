"""Writes tests/golden/transformer_kats.json: a small known-answer set for the Transformer package, computed here in numpy float64
and with Python integers, independently of tests/transformer_ref.py (torch) and of the kernels.

These are RESTATED SEMANTICS (scale after the product, the additive -2^32 + 1 padding mask as an fp32 add,
the replacing future mask, population-variance LayerNormalization with epsilon inside the root, the counter hash of the dropout
masks), not recorded TensorFlow output: TensorFlow is not available where this project is built.

  python tests/golden/make_transformer_kats.py"""
import json
import os

import numpy as np

M64 = (1 << 64) - 1


def mix32(seed, idx):
    z = (idx * 0x9E3779B97F4A7C15 + seed) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (z ^ (z >> 31)) >> 32


def attention(q, k, v, H, mask, future):
    B, Lq, W = q.shape
    Lk = k.shape[1]
    dh = W // H
    out = np.zeros((B, Lq, W))
    probs = np.zeros((B, H, Lq, Lk))
    for b in range(B):
        for h in range(H):
            sl = slice(h * dh, (h + 1) * dh)
            s = q[b, :, sl] @ k[b, :, sl].T / np.sqrt(dh)
            if mask is not None:
                added = (s.astype(np.float32) + np.float32(mask[b].astype(np.float32) * np.float32(-2 ** 32 + 1))[None, :]).astype(np.float64)
                s = np.where(mask[b][None, :], added, s)
            if future:
                s = np.where(np.triu(np.ones((Lq, Lk), dtype=bool), 1), float(np.float32(-2 ** 32 + 1)), s)
            e = np.exp(s - s.max(1, keepdims=True))
            p = e / e.sum(1, keepdims=True)
            probs[b, h] = p
            out[b, :, sl] = p @ v[b, :, sl]
    return out, probs


def main():
    rng = np.random.default_rng(20240611)
    kats = {"note": "restated semantics in numpy float64, not TensorFlow output; see make_transformer_kats.py"}
    kats["mix32"] = [{"seed": s, "idx": i, "hash": mix32(s, i)} for s, i in
                     [(0, 0), (1, 0), (0, 1), (12345, 67890), (M64, 1 << 40), (1000003, (1 << 33) + 7)]]
    cases = []
    for name, B, Lq, Lk, H, dh, masked, future, scale in [
            ("plain", 2, 3, 5, 2, 4, False, False, 1.0),
            ("padded", 2, 4, 4, 2, 4, True, False, 1.0),
            ("causal_prepadded", 2, 5, 5, 1, 4, True, True, 1.0),
            ("large_scores", 1, 3, 4, 1, 4, True, False, 16.0)]:
        # integers / 2 keep every product exact in fp32 and float64 alike
        q = rng.integers(-4, 5, size=(B, Lq, H * dh)) * (0.5 * scale)
        k = rng.integers(-4, 5, size=(B, Lk, H * dh)) * (0.5 * scale)
        v = rng.integers(-8, 9, size=(B, Lk, H * dh)) * 0.25
        mask = None
        if masked:
            mask = np.zeros((B, Lk), dtype=bool)
            mask[0, :2] = True                 # pre-padding: the first keys are padded
            if B > 1:
                mask[1, :] = name != "causal_prepadded"          # a fully padded row of keys
                mask[1, :3] = True
            if name == "large_scores":
                mask[0, :] = True
        out, probs = attention(q, k, v, H, mask, future)
        cases.append({"name": name, "n_heads": H, "future": future, "q": q.tolist(), "k": k.tolist(), "v": v.tolist(),
                      "mask": None if mask is None else mask.astype(int).tolist(), "out": out.tolist(), "probs": probs.tolist()})
    kats["attention"] = cases
    a = rng.integers(-6, 7, size=(3, 8)) * 0.5
    a[1, :] = 2.5                                                  # a constant row: variance 0, the epsilon path
    b = rng.integers(-6, 7, size=(3, 8)) * 0.25
    b[1, :] = -1.0
    gamma = rng.integers(1, 5, size=8) * 0.5
    beta = rng.integers(-3, 4, size=8) * 0.25
    s = a + b
    mean = s.mean(1, keepdims=True)
    var = ((s - mean) ** 2).mean(1, keepdims=True)
    kats["layer_norm"] = {"a": a.tolist(), "b": b.tolist(), "gamma": gamma.tolist(), "beta": beta.tolist(), "eps": 1e-8,
                          "y": (gamma * (s - mean) / np.sqrt(var + 1e-8) + beta).tolist()}
    kats["position_encoding"] = {"L": 4, "D": 6, "table": [[float(np.float32(np.sin(p / 10000 ** ((i - i % 2) / 6)) if i % 2 == 0 else
                                                                              np.cos(p / 10000 ** ((i - i % 2) / 6))))
                                                             for i in range(6)] for p in range(4)]}
    kats["noam"] = [{"model_dim": 8, "warmup_steps": 4000, "step": t,
                     "lr": 8 ** -0.5 * (4000 ** -1.5 if t == 0 else min(t ** -0.5, t * 4000 ** -1.5))} for t in (0, 1, 100, 4000, 10000)]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "transformer_kats.json")
    with open(path, "w") as f:
        json.dump(kats, f, indent=1)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
