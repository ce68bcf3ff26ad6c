"""Training-step time of the multi-task models: MMoE on the grouped / gate-mix kernels against the straightforward composition
(one L.mlp tower per expert and per task, torch softmax + bmm for the gates), both with the example's two-apply Adam recipe.

  python tools/bench_multitask.py [--steps 50] [--warmup 10]

Prints one JSON line: ms per training step (forward + both backwards + both Adam applies) for
  example  B = 512,    256 numeric columns,                        E = 2, T = 2, experts [64, 32],   towers [32, 10]
  scaled   B = 65536,  26 embedding columns (D = 16) + 13 numeric, E = 8, T = 2, experts [256, 128], towers [64]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deep_recommenders_amd import feature_column as fc  # noqa: E402
from deep_recommenders_amd import layers as L  # noqa: E402
from deep_recommenders_amd import losses, optim  # noqa: E402
from deep_recommenders_amd.estimator.models.multi_task_learning import MMoE  # noqa: E402

CONFIGS = {
    "example": dict(B=512, n_num=256, n_emb=0, D=16, vocab=0, E=2, T=2, experts=[64, 32], towers=[32, 10]),
    "scaled": dict(B=65536, n_num=13, n_emb=26, D=16, vocab=10000, E=8, T=2, experts=[256, 128], towers=[64]),
}


def columns(cfg):
    cols = [fc.numeric_column("I%d" % i) for i in range(cfg["n_num"])]
    cols += [fc.embedding_column(fc.categorical_column_with_identity("C%d" % i, cfg["vocab"]), cfg["D"]) for i in range(cfg["n_emb"])]
    return cols


def features(cfg, seed=0):
    r = np.random.RandomState(seed)
    f = {"I%d" % i: r.normal(size=(cfg["B"], 1)).astype(np.float32) for i in range(cfg["n_num"])}
    for i in range(cfg["n_emb"]):
        f["C%d" % i] = torch.from_numpy(r.randint(0, cfg["vocab"], size=(cfg["B"], 1))).cuda()
    labels = [torch.from_numpy(r.normal(size=(cfg["B"], 1)).astype(np.float32)).cuda() for _ in range(cfg["T"])]
    return f, labels


class Composed(torch.nn.Module):
    """the same MMoE as separate launches: L.mlp per expert / per gate / per tower, torch softmax + bmm for the mixture"""

    def __init__(self, model):
        super().__init__()
        self.m = model
        E, T = model.num_experts, model.num_tasks
        v = {n: model.variable(n).detach().clone().contiguous() for n in model.var_names if not n.startswith("input_layer/")}
        ne = len(model.experts.units)
        self.ex = [[(torch.nn.Parameter(v["mixture_of_experts/dense%s/kernel" % ("" if e * ne + i == 0 else "_%d" % (e * ne + i))]),
                     torch.nn.Parameter(v["mixture_of_experts/dense%s/bias" % ("" if e * ne + i == 0 else "_%d" % (e * ne + i))]))
                    for i in range(ne)] for e in range(E)]
        self.gates = [torch.nn.Parameter(v["multi_gate/dense%s/kernel" % ("" if t == 0 else "_%d" % t)]) for t in range(T)]
        nt = len(model.towers.units)
        self.tw = [[(torch.nn.Parameter(v["task%d/dense%s/kernel" % (t, "" if i == 0 else "_%d" % i)]),
                     torch.nn.Parameter(v["task%d/dense%s/bias" % (t, "" if i == 0 else "_%d" % i)])) for i in range(nt)]
                   for t in range(T)]
        self.plist = torch.nn.ParameterList([p for e in self.ex for wb in e for p in wb] + self.gates +
                                            [p for t in self.tw for wb in t for p in wb])

    def forward(self, feats):
        x = self.m.input_layer(feats)
        hs = []
        for layers in self.ex:
            n = len(layers)
            hs.append(L.mlp(x, [w for w, _ in layers], [b for _, b in layers], [1] * (n - 1) + [0]))
        moe = torch.stack(hs, 1)
        outs = []
        for t, layers in enumerate(self.tw):
            g = torch.softmax(L.mlp(x, [self.gates[t]], [None], [0]), 1)
            mix = torch.bmm(g.unsqueeze(1), moe).squeeze(1)
            n = len(layers)
            outs.append(L.mlp(mix, [w for w, _ in layers], [b for _, b in layers], [1] * (n - 1) + [0]))
        return outs


def step_fn(model, opt, feats, labels):
    outs = model(feats)
    params = [p for p in model.parameters() if p.requires_grad]
    grads = []
    for t, (o, y) in enumerate(zip(outs, labels)):
        loss = losses.mean_squared_error(y, o)
        grads.append(torch.autograd.grad(loss, params, retain_graph=t < len(outs) - 1, allow_unused=True))
    for g in grads:
        opt.apply_gradients(zip(g, params))


def time_steps(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--configs", default="example,scaled")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"metric": "multitask_train_step_ms", "device": torch.cuda.get_device_name(0)}
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        torch.manual_seed(0)
        feats, labels = features(cfg)
        m = MMoE(columns(cfg), num_tasks=cfg["T"], num_experts=cfg["E"], expert_hidden_units=cfg["experts"],
                 task_hidden_units=cfg["towers"])
        opt = optim.Adam(m.parameters(), lr=0.01, epsilon=1e-8, shared_step=True)
        grouped = time_steps(lambda: step_fn(m, opt, feats, labels), a.steps, a.warmup)
        c = Composed(m)
        opt_c = optim.Adam(c.parameters(), lr=0.01, epsilon=1e-8, shared_step=True)
        composed = time_steps(lambda: step_fn(c, opt_c, feats, labels), a.steps, a.warmup)
        out[name] = {"B": cfg["B"], "E": cfg["E"], "T": cfg["T"], "grouped_ms": round(grouped, 4), "composed_ms": round(composed, 4),
                     "speedup": round(composed / grouped, 3)}
        del m, c, opt, opt_c
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
