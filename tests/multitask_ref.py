"""Plain-torch restatements of the multi-task models (MMoE, ESMM) and of the gate softmax + mixture, in the dtype of the tensors handed
in.  No GPU and no package kernel is used here: tests/test_gpu_multitask.py checks the kernels and the models against it, and
tests/layer_autograd_cases.py differentiates it for the autograd Functions of the two models."""
import numpy as np
import torch

_ACT = {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}


def _gate_mix_ref(h, l, E, T, U):
    B = h.shape[0]
    p = torch.softmax(l.reshape(B, T, E), dim=2)
    out = torch.einsum("bte,beu->btu", p, h.reshape(B, E, U)).reshape(B, T * U)
    return p.reshape(B, T * E), out


def _ref_dnn(x, V, scope, names, act):
    n = len(names)
    for i, nm in enumerate(names):
        x = x @ V[scope + "/" + nm + "/kernel"] + V[scope + "/" + nm + "/bias"]
        if i < n - 1:
            x = _ACT[act](x)
    return x


def _dense_names(start, count):
    return ["dense" if j == 0 else "dense_%d" % j for j in range(start, start + count)]


def _ref_input(features, columns, V):
    from deep_recommenders_amd import feature_column as fc
    layout, _ = fc.input_layer_layout(columns)
    blocks = []
    for name, c, off, w in layout:
        if isinstance(c, fc.NumericColumn):
            blocks.append(torch.as_tensor(np.asarray(features[c.key], np.float32)).double().reshape(-1, w))
        else:
            ids = torch.as_tensor(np.asarray(features[c.categorical_column.key])).reshape(-1)
            blocks.append(V["input_layer/%s_embedding/embedding_weights" % c.categorical_column.key][ids])
    return torch.cat(blocks, 1)


def _ref_mmoe_x(x, V, E, T, eu, tu, act_e="relu", act_t="relu"):
    """the T task outputs from the input layer's output x [B, K]"""
    experts = [_ref_dnn(x, V, "mixture_of_experts", _dense_names(e * len(eu), len(eu)), act_e) for e in range(E)]
    moe = torch.stack(experts, 1)
    outs = []
    for t in range(T):
        gate = torch.softmax(x @ V["multi_gate/" + _dense_names(t, 1)[0] + "/kernel"], 1)
        mix = (gate.unsqueeze(1) @ moe).squeeze(1)
        outs.append(_ref_dnn(mix, V, "task%d" % t, _dense_names(0, len(tu) + 1), act_t))
    return outs


def _ref_mmoe(features, columns, V, E, T, eu, tu, act_e="relu", act_t="relu"):
    return _ref_mmoe_x(_ref_input(features, columns, V), V, E, T, eu, tu, act_e, act_t)


def _ref_esmm_x(x, V, n_layers, act="relu"):
    """(p_cvr, p_ctr, p_ctcvr) from the input layer's output x [B, K]; n_layers dense layers per tower, the last one the logit"""
    cvr = torch.sigmoid(_ref_dnn(x, V, "pCVR", _dense_names(0, n_layers), act))
    ctr = torch.sigmoid(_ref_dnn(x, V, "pCTR", _dense_names(0, n_layers), act))
    return cvr, ctr, ctr * cvr
