"""Estimator-style ESMM -- same surface as the reference's estimator/models/multi_task_learning/esmm.py:13-55:

    inputs = input_layer(features, columns)
    p_cvr = sigmoid(dnn(inputs, hidden_units + [1]))   in scope pCVR   (built first)
    p_ctr = sigmoid(dnn(inputs, hidden_units + [1]))   in scope pCTR
    p_ctcvr = p_ctr * p_cvr

The two towers are one GroupedStack (G = 2, group 0 = pCVR): their first layers as one dr_linear_fwd over the concatenated kernel,
every deeper layer as one grouped launch, the head (two sigmoids and the product) as dr_esmm_head_fwd; the backward mirrors it."""
import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops
from deep_recommenders_amd.estimator.models import variables as V
from deep_recommenders_amd.estimator.models.feature_interaction.dnn import relu
from deep_recommenders_amd.estimator.models.multi_task_learning import _grouped as GR
from deep_recommenders_amd.estimator.models.multi_task_learning.mixture_of_experts import _check_bn, _check_dropout, _seed_counter


class _ESMMFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, model, x, *params):
        ctx.set_materialize_grads(False)
        x = L._rows(x)
        seed = lambda: next(_seed_counter) * 1000003 + model.seed       # noqa: E731
        logits, saved = model.towers.forward(x, seed)                    # [B, 2] = (cvr, ctr)
        p_cvr, p_ctr, p_ctcvr = ops.esmm_head_fwd(logits)
        ctx.model, ctx.saved = model, saved
        ctx.save_for_backward(x, p_cvr, p_ctr)
        return p_cvr.reshape(-1, 1), p_ctr.reshape(-1, 1), p_ctcvr.reshape(-1, 1)

    @staticmethod
    @L._needed_only
    def backward(ctx, d_cvr, d_ctr, d_ctcvr):
        model = ctx.model
        x, p_cvr, p_ctr = ctx.saved_tensors
        active = set()
        if d_cvr is not None or d_ctcvr is not None:
            active.add(0)
        if d_ctr is not None or d_ctcvr is not None:
            active.add(1)
        if not active:
            return (None,) * (2 + len(model.params))
        d_logits = ops.esmm_head_bwd(p_cvr, p_ctr, d_cvr, d_ctr, d_ctcvr)
        need_x = ctx.needs_input_grad[1]
        gW, gb, d_x = model.towers.backward(d_logits, ctx.saved, need_dx=need_x)
        return (None, d_x if need_x else None, *GR.grad_views(model.towers, gW, gb, active))


class ESMM(nn.Module):

    def __init__(self, feature_columns, hidden_units, activation=relu, batch_normalization=False, dropout=None, device="cuda", seed=0,
                 **kwargs):
        super().__init__()
        _check_bn(batch_normalization)
        self._columns = feature_columns
        self._hidden_units = list(hidden_units)
        self._configs = kwargs
        self.seed = int(seed)
        self.input_layer = L.InputLayer(feature_columns, device=device)
        self.towers = GR.GroupedStack(2, self.input_layer.K, self._hidden_units + [1], GR.act_code(activation), _check_dropout(dropout),
                                      True, device)
        vs = {(i, g): (w, b) for i, g, w, b in self.towers.make_views()}
        self.var_names, self._order, self._views = [], [], {}
        for g, scope in enumerate(("pCVR", "pCTR")):
            for i in range(len(self.towers.units)):
                name = "{}/dense{}".format(scope, "" if i == 0 else "_%d" % i)
                self.var_names += [name + "/kernel", name + "/bias"]
                self._views[name + "/kernel"], self._views[name + "/bias"] = vs[(i, g)]
                L.glorot_uniform_(vs[(i, g)][0])
        for i in range(len(self.towers.units)):
            for scope in ("pCVR", "pCTR"):
                name = "{}/dense{}".format(scope, "" if i == 0 else "_%d" % i)
                self._order += [name + "/kernel", name + "/bias"]
        self.tf_vars = nn.ParameterDict({n.replace("/", "__"): nn.Parameter(self._views[n]) for n in self.var_names})
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
        return _ESMMFn.apply(self, x, *ps)

    forward = call

    def export_variables(self):
        return V.export_named(self)

    def import_variables(self, variables, strict=True):
        return V.import_named(self, variables, strict)

    def variable(self, name):
        if name.startswith("input_layer/"):
            return self.input_layer.slab.embedding_weights(name.split("/")[1][:-len("_embedding")])
        return self.tf_vars[name.replace("/", "__")]
