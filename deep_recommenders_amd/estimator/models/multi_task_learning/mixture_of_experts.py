"""Estimator-style MMoE -- same surface as the reference's estimator/models/multi_task_learning/mixture_of_experts.py:13-90.

    inputs = input_layer(features, columns)                                   (:61)
    expert e = dnn(inputs, expert_hidden_units)  for e < num_experts          (:63-70)
    gate t   = softmax(dense(inputs, num_experts, use_bias=False))            (:50-57, :72-77)
    task t   = dnn(sum_e gate_t[e] expert_e, task_hidden_units + [1])          (:79-88)

The dense part is a handful of launches: the experts' first layers as ONE dr_linear_fwd over their concatenated kernel, the gates
as one more, every deeper expert layer and every task-tower layer as one grouped launch, the gate softmax + mixture as one
dr_mmoe_gate_mix_fwd; the backward mirrors it.  Reference quirks kept: `num_experts` gates are built and indexed by task, so
num_tasks > num_experts raises IndexError and gates t >= num_tasks exist as variables but are never computed (no gradient);
batch_normalization=True raises TypeError; dropout draws on every call."""
import itertools

import numpy as np
import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops
from deep_recommenders_amd.estimator.models.feature_interaction.dnn import relu
from deep_recommenders_amd.estimator.models.multi_task_learning import _grouped as GR
from deep_recommenders_amd.estimator.models import variables as V

_seed_counter = itertools.count(1)


def _check_bn(flag):
    if flag is True:
        raise TypeError("batch_normalization() missing required arguments (the reference's dnn.py:23-24 "
                        "calls tf.nn.batch_normalization(x) and raises too)")


def _check_dropout(rate):
    if rate is not None and not (0.0 <= float(rate) < 1.0):
        raise ValueError("dropout rate must be in [0, 1), got {}".format(rate))
    return None if rate is None else float(rate)


class _MMoEFn(torch.autograd.Function):
    """x [B, K] -> T task outputs [B, 1].  params: every TF variable view (for autograd), in MMoE.params order."""

    @staticmethod
    def forward(ctx, model, x, *params):
        ctx.set_materialize_grads(False)
        x = L._rows(x)
        E, T, ne = model.num_experts, model.num_tasks, model.num_experts
        B = x.shape[0]
        seed = lambda: next(_seed_counter) * 1000003 + model.seed       # noqa: E731
        h, ex_saved = model.experts.forward(x, seed)                     # [B, E*U]
        U = model.experts.units[-1]
        logits = torch.empty((B, T * E), dtype=torch.float32, device=x.device)
        ops.linear_fwd(x, model.gates_w[:, :T * E], None, 0, out=logits)  # the first T of num_experts gates (ld = ne*E)
        p, mix = ops.mmoe_gate_mix_fwd(h, logits, E, T, U)
        y, tw_saved = model.towers.forward(mix, seed)                    # [B, T]
        ctx.model, ctx.ex_saved, ctx.tw_saved = model, ex_saved, tw_saved
        ctx.save_for_backward(x, h, p)
        ctx.ne = ne
        return tuple(y[:, t:t + 1] for t in range(T))

    @staticmethod
    @L._needed_only
    def backward(ctx, *d_outs):
        model = ctx.model
        x, h, p = ctx.saved_tensors
        E, T = model.num_experts, model.num_tasks
        B = x.shape[0]
        U = model.experts.units[-1]
        active = {t for t, d in enumerate(d_outs) if d is not None}
        if not active:
            return (None,) * (2 + len(model.params))
        d_y = torch.zeros((B, T), dtype=torch.float32, device=x.device)
        for t in active:
            d_y[:, t:t + 1].copy_(d_outs[t])
        tW, tb, d_mix = model.towers.backward(d_y, ctx.tw_saved, need_dx=True)
        d_h, d_l = ops.mmoe_gate_mix_bwd(h, p, d_mix, E, T, U)
        need_x = ctx.needs_input_grad[1]
        eW, eb, d_x = model.experts.backward(d_h, ctx.ex_saved, need_dx=need_x)
        g_gates = torch.zeros_like(model.gates_w)
        ops.linear_bwd_dw(x, d_l, 1.0, g_gates[:, :T * E], None, workspace=ops.linear_bwd_dw_workspace(B, x.shape[1], T * E, x.device))
        if need_x:
            ops.linear_bwd_dx(d_l, model.gates_w[:, :T * E], None, accumulate=True, out=d_x)
        grads = GR.grad_views(model.experts, eW, eb, set(range(E)))
        grads += [g_gates[:, t * E:(t + 1) * E] if t in active else None for t in range(T)]
        grads += GR.grad_views(model.towers, tW, tb, active)
        return (None, d_x if need_x else None, *grads)


class MMoE(nn.Module):

    def __init__(self, feature_columns, num_tasks, num_experts, expert_hidden_units, task_hidden_units, task_hidden_activation=relu,
                 task_batch_normalization=False, task_dropout=None, expert_hidden_activation=relu, expert_batch_normalization=False,
                 expert_dropout=None, device="cuda", seed=0):
        super().__init__()
        _check_bn(task_batch_normalization)
        _check_bn(expert_batch_normalization)
        if num_tasks > num_experts:     # mixture_of_experts.py:72-82 builds num_experts gates and indexes them by task
            raise IndexError("list index out of range (MMoE builds num_experts={} gates and indexes them by task; num_tasks={})"
                             .format(num_experts, num_tasks))
        if num_tasks < 1 or num_experts < 1 or len(expert_hidden_units) < 1:
            raise ValueError("MMoE needs at least one task, one expert and one expert layer")
        if num_experts > 64 or num_tasks > 16:
            raise ValueError("the gate-mix kernel covers num_experts <= 64 and num_tasks <= 16")
        self._columns = feature_columns
        self.num_tasks, self.num_experts = int(num_tasks), int(num_experts)
        self._expert_hidden_units = list(expert_hidden_units)
        self._task_hidden_units = list(task_hidden_units)
        self.seed = int(seed)
        self.input_layer = L.InputLayer(feature_columns, device=device)
        K, E, T = self.input_layer.K, self.num_experts, self.num_tasks
        self.experts = GR.GroupedStack(E, K, self._expert_hidden_units, GR.act_code(expert_hidden_activation),
                                       _check_dropout(expert_dropout), True, device)
        self.towers = GR.GroupedStack(T, self._expert_hidden_units[-1], self._task_hidden_units + [1],
                                      GR.act_code(task_hidden_activation), _check_dropout(task_dropout), False, device)
        self.gates_w = torch.empty((K, E * E), dtype=torch.float32, device=device)
        # TF variables, in the reference's creation order (expert 0's layers, expert 1's, ...; gates; task 0's tower, ...)
        self.var_names, views = [], []
        ex = {(i, g): (w, b) for i, g, w, b in self.experts.make_views()}
        for g in range(E):
            for i in range(len(self._expert_hidden_units)):
                j = g * len(self._expert_hidden_units) + i
                name = "mixture_of_experts/dense{}".format("" if j == 0 else "_%d" % j)
                self.var_names += [name + "/kernel", name + "/bias"]
                views += list(ex[(i, g)])
        for g in range(E):
            self.var_names.append("multi_gate/dense{}/kernel".format("" if g == 0 else "_%d" % g))
            views.append(self.gates_w[:, g * E:(g + 1) * E])
        tw = {(i, g): (w, b) for i, g, w, b in self.towers.make_views()}
        for t in range(T):
            for i in range(len(self.towers.units)):
                name = "task{}/dense{}".format(t, "" if i == 0 else "_%d" % i)
                self.var_names += [name + "/kernel", name + "/bias"]
                views += list(tw[(i, t)])
        for name, v in zip(self.var_names, views):
            if name.endswith("/kernel"):
                L.glorot_uniform_(v)                                      # [TF] B8: per variable (its own fan-in / fan-out)
        self.tf_vars = nn.ParameterDict()
        self._views = {}
        for name, v in zip(self.var_names, views):
            key = name.replace("/", "__")
            self.tf_vars[key] = nn.Parameter(v)                           # shares storage with the grouped buffer
            self._views[name] = v
        # the Function's parameter order: experts (layer-major), the first T gates, towers (layer-major)
        order = []
        for i in range(len(self._expert_hidden_units)):
            for g in range(E):
                j = g * len(self._expert_hidden_units) + i
                name = "mixture_of_experts/dense{}".format("" if j == 0 else "_%d" % j)
                order += [name + "/kernel", name + "/bias"]
        order += ["multi_gate/dense{}/kernel".format("" if t == 0 else "_%d" % t) for t in range(T)]
        for i in range(len(self.towers.units)):
            for t in range(T):
                name = "task{}/dense{}".format(t, "" if i == 0 else "_%d" % i)
                order += [name + "/kernel", name + "/bias"]
        self._order = order
        if self.input_layer.slab is not None:
            self.var_names += ["input_layer/%s_embedding/embedding_weights" % k for k in self.input_layer.emb_keys]

    @property
    def params(self):
        return [self.tf_vars[n.replace("/", "__")] for n in self._order]

    def __call__(self, *args, **kwargs):
        return self.call(*args, **kwargs)

    def call(self, features):
        x = self.input_layer(features)
        ps = self.params
        GR.check_views(ps, [self._views[n] for n in self._order])
        return list(_MMoEFn.apply(self, x, *ps))

    forward = call

    def export_variables(self):
        return V.export_named(self)

    def import_variables(self, variables, strict=True):
        return V.import_named(self, variables, strict)

    def variable(self, name):
        """the tensor behind a TF variable name"""
        if name.startswith("input_layer/"):
            key = name.split("/")[1][:-len("_embedding")]
            return self.input_layer.slab.embedding_weights(key)
        return self.tf_vars[name.replace("/", "__")]
