"""DIN -- the reference's keras/models/ranking/din.py with the same constructor / call / get_config surfaces:

  * ActivationUnit (din.py:8-88): Dense(1)(Dense(units, activation)(concat([x, y, interacter([x, y])], axis=1))).  The concat
    (+ Subtract / Multiply interaction) is one kernel (dr_din_concat_fwd), the two Dense layers are the MFMA GEMM path
    (deep_recommenders_amd.layers.mlp); the activation is relu / linear / sigmoid / tanh or a Dice instance (Dense -> dr_dice -> Dense).
  * Dice (din.py:88-130): literally the reference's arithmetic -- the standard deviation, which it names "var", gets another square
    root.  One deliberate deviation, in the gradient only: where a row is constant (always for a single feature) the term through the
    standard deviation is taken as zero; TensorFlow returns NaN there, which a dead unit row with a zero bias would feed into training.
  * InterestPooling: what the unit exists for -- every key of a behaviour sequence scored against the candidate and the sequence summed
    with those scores -- as one fused kernel (dr_din_pool_fwd) that never builds the [B * T, 3D] pair matrix.  No softmax over the
    sequence, as in the paper."""
import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.ranking.dcn import _init


class Subtract:
    """keras.layers.Subtract restricted to what ActivationUnit feeds it: [x, y] -> x - y (tests/keras/test_din.py:33)."""
    mode = 1

    def __call__(self, inputs):
        x, y = inputs
        return _DinConcatFn.apply(x, y, 1)[:, 2 * x.shape[1]:]


class Multiply:
    """keras.layers.Multiply: [x, y] -> x * y."""
    mode = 2

    def __call__(self, inputs):
        x, y = inputs
        return _DinConcatFn.apply(x, y, 2)[:, 2 * x.shape[1]:]


class _DinConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, mode):
        x, y = L._rows(x, dense=True), L._rows(y, dense=True)
        ctx.mode = mode
        ctx.save_for_backward(x, y)
        return ops.din_concat_fwd(x, y, mode)

    @staticmethod
    @L._needed_only
    def backward(ctx, d_out):
        x, y = ctx.saved_tensors
        d_x, d_y = ops.din_concat_bwd(x, y, ctx.mode, L._rows(d_out))
        return d_x, d_y, None


class Dice(nn.Module):
    """Dice (din.py:88-130): y = where(prelu(x) > 0, p, 1 - p) * prelu(x) with p = sigmoid((x - mean) / sqrt(std + epsilon)) over
    axis 1 of [M, N] and Keras PReLU's per-feature alpha [N].  Builds on the first call.  The gradient at a constant row takes the
    term through the standard deviation as zero (TensorFlow: NaN)."""

    def __init__(self, epsilon=1e-8, alpha_initializer="zeros", alpha_regularizer=None, **kwargs):
        super().__init__()
        self._epsilon = epsilon
        self._alpha_initializer = alpha_initializer
        self._alpha_regularizer = alpha_regularizer
        if alpha_regularizer is not None:
            raise NotImplementedError("regularizers are not used by any reference model/test")
        self._kwargs = kwargs
        self.built = False

    def build(self, n_features, device="cuda"):
        self.alpha = nn.Parameter(_init(self._alpha_initializer, (n_features,), device))    # PReLU's alpha, din.py:104-107
        self.built = True

    def call(self, inputs, **kwargs):
        x = torch.as_tensor(inputs, dtype=torch.float32).cuda()
        if x.dim() != 2:
            raise ValueError("Dice is called on [M, N]")
        if not self.built:
            self.build(x.shape[1], x.device)
        return L.dice(x, self.alpha, self._epsilon)

    forward = call

    def get_config(self):
        config = {
            "epsilon": self._epsilon,
            "alpha_initializer": self._alpha_initializer,
            "alpha_regularizer": self._alpha_regularizer,
        }
        return {**self._kwargs, **config}


_ACT_CODES = {None: 0, "linear": 0, "relu": 1, "sigmoid": 2, "tanh": 3}


def _act_code(activation):
    if isinstance(activation, Dice):
        return 4
    if not (activation is None or isinstance(activation, str)) or activation not in _ACT_CODES:
        raise NotImplementedError("activation %r: the kernels provide relu / linear / sigmoid / tanh or a Dice instance" % (activation,))
    return _ACT_CODES[activation]


class ActivationUnit(nn.Module):
    def __init__(self, units, interacter=None, use_bias=True, activation="relu", kernel_init="truncated_normal",
                 kernel_regu=None, bias_init="zeros", bias_regu=None, **kwargs):
        super().__init__()
        self._kernel_units = units
        self._interacter = interacter
        self._use_bias = use_bias
        self._act_code = _act_code(activation)
        self.dice = activation if isinstance(activation, Dice) else None       # its alpha is a parameter of this unit
        self._kernel_activation = None if self.dice is not None else activation
        self._kernel_init, self._kernel_regu = kernel_init, kernel_regu
        self._bias_init, self._bias_regu = bias_init, bias_regu
        if kernel_regu is not None or bias_regu is not None:
            raise NotImplementedError("regularizers are not used by any reference model/test")
        self._kwargs = kwargs
        self.built = False

    def build(self, in_dim, device="cuda"):
        u = self._kernel_units
        self.dense_kernel_w = nn.Parameter(_init(self._kernel_init, (in_dim, u), device))       # din.py:37-45
        self.dense_output_w = nn.Parameter(_init(self._kernel_init, (u, 1), device))            # :46-54
        self.dense_kernel_b = nn.Parameter(_init(self._bias_init, (u,), device)) if self._use_bias else None
        self.dense_output_b = nn.Parameter(_init(self._bias_init, (1,), device)) if self._use_bias else None
        self.built = True

    def call(self, x_embeddings, y_embeddings=None, **kwargs):
        x = torch.as_tensor(x_embeddings, dtype=torch.float32).cuda()
        y = x if y_embeddings is None else torch.as_tensor(y_embeddings, dtype=torch.float32).cuda()      # din.py:59-60
        mode = getattr(self._interacter, "mode", None) if self._interacter is not None else 0
        if mode is not None:
            h = _DinConcatFn.apply(x, y, mode)                                                           # :62-66 in one pass
        else:   # a user-supplied interacter: its output is appended as a third column block
            h = torch.cat([_DinConcatFn.apply(x, y, 0), self._interacter([x, y])], dim=1)
        if not self.built:
            self.build(h.shape[1], h.device)
        if self.dice is not None:
            hidden = self.dice(L.mlp(h, [self.dense_kernel_w], [self.dense_kernel_b], [0]))
            return L.mlp(hidden, [self.dense_output_w], [self.dense_output_b], [0])
        return L.mlp(h, [self.dense_kernel_w, self.dense_output_w], [self.dense_kernel_b, self.dense_output_b],
                     [self._act_code, 0])                                                                # :68-69

    forward = call

    def get_config(self):
        config = {
            "units": self._kernel_units,
            "interacter": self._interacter,
            "use_bias": self._use_bias,
            "activation": self.dice if self.dice is not None else self._kernel_activation,
            "kernel_init": self._kernel_init,
            "kernel_regu": self._kernel_regu,
            "bias_init": self._bias_init,
            "bias_regu": self._bias_regu,
        }
        return {**self._kwargs, **config}


class InterestPooling(nn.Module):
    """DIN's local activation unit applied over a behaviour sequence, fused:

        score[b, t] = mask[b, t] ? ActivationUnit(query[b], keys[b, t]) : 0          out[b] = sum over valid t of score[b, t] keys[b, t]

    Constructor and parameter names are ActivationUnit's (the two are interchangeable on shared parameters).  Called as
    (query [B, D], keys [B, T, D], mask=None, lengths=None, return_scores=False); mask [B, T] is nonzero / True at valid positions,
    lengths [B] is turned into the mask t < lengths[b].  Masked positions are skipped, not multiplied by zero: whatever the keys
    hold there reaches neither the output nor any gradient.  There is no softmax over t.  Domain of the kernels: D % 4 == 0,
    4 <= D <= 128, 1 <= units <= 128, T >= 1 -- a ValueError outside it, there is no composed fallback."""

    def __init__(self, units, interacter=None, use_bias=True, activation="relu", kernel_init="truncated_normal",
                 kernel_regu=None, bias_init="zeros", bias_regu=None, **kwargs):
        super().__init__()
        self._kernel_units = units
        self._interacter = interacter
        self._use_bias = use_bias
        self._act_code = _act_code(activation)
        self.dice = activation if isinstance(activation, Dice) else None
        self._kernel_activation = None if self.dice is not None else activation
        self._kernel_init, self._kernel_regu = kernel_init, kernel_regu
        self._bias_init, self._bias_regu = bias_init, bias_regu
        if kernel_regu is not None or bias_regu is not None:
            raise NotImplementedError("regularizers are not used by any reference model/test")
        if interacter is not None and getattr(interacter, "mode", None) not in (1, 2):
            raise NotImplementedError("InterestPooling folds the interacter into the kernel: Subtract() / Multiply() (an object with "
                                      "mode 1 / 2) or None")
        self._mode = 0 if interacter is None else interacter.mode
        self._kwargs = kwargs
        self.built = False

    build = ActivationUnit.build

    def call(self, query, keys, mask=None, lengths=None, return_scores=False, **kwargs):
        q = torch.as_tensor(query, dtype=torch.float32).cuda()
        k = torch.as_tensor(keys, dtype=torch.float32).cuda()
        if k.dim() != 3 or q.dim() != 2:
            raise ValueError("InterestPooling is called on query [B, D] and keys [B, T, D]")
        B, T, D = k.shape
        if lengths is not None:
            if mask is not None:
                raise ValueError("give mask or lengths, not both")
            lengths = torch.as_tensor(lengths).to(k.device)
            mask = torch.arange(T, device=k.device).unsqueeze(0) < lengths.reshape(B, 1)           # plumbing: [B, T] bool
        elif mask is not None:
            mask = torch.as_tensor(mask).to(k.device)
            if mask.dtype not in (torch.bool, torch.uint8):
                mask = mask != 0
        if not self.built:
            self.build((2 if self._mode == 0 else 3) * D, k.device)
        if self.dice is not None and not self.dice.built:
            self.dice.build(self._kernel_units, k.device)
        out, scores = L.din_interest_pooling(q, k, mask, self.dense_kernel_w, self.dense_kernel_b, self.dense_output_w, self.dense_output_b,
                                             self._mode, self._act_code, self.dice.alpha if self.dice is not None else None,
                                             self.dice._epsilon if self.dice is not None else 1e-8)
        return (out, scores) if return_scores else out

    forward = call
    get_config = ActivationUnit.get_config
