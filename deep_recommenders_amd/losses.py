"""Sigmoid + the three binary losses the reference's examples use, as autograd functions over the K11
kernels.  Reference call sites (reference root): examples/train_fm_on_movielens_estimator.py:46
(tf.losses.sigmoid_cross_entropy), examples/train_deepfm_on_movielens_estimator.py:47 (tf.losses.log_loss),
examples/train_deepfm_on_movielens_keras.py:43 (tf.keras.losses.binary_crossentropy)."""
import numpy as np
import torch

from . import ops
from .layers import _needed_only, _rows


class _SigmoidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = ops.sigmoid_fwd(_rows(x, dense=True))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @_needed_only
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.sigmoid_bwd(y, _rows(dy, dense=True))


class _LogitLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, mode):
        loss, _, g = ops.bce_fwd_bwd(logits, labels, mode, want_prob=False, want_grad=True)
        ctx.save_for_backward(g)
        ctx.shape = logits.shape
        return loss.reshape(())

    @staticmethod
    @_needed_only
    def backward(ctx, d_loss):
        (g,) = ctx.saved_tensors
        return (g * d_loss).reshape(ctx.shape) if ctx.needs_input_grad[0] else None, None, None


class _ProbLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prob, labels, mode):
        loss, g = ops.bce_prob_fwd_bwd(prob, labels, mode)
        ctx.save_for_backward(g)
        ctx.shape = prob.shape
        return loss.reshape(())

    @staticmethod
    @_needed_only
    def backward(ctx, d_loss):
        (g,) = ctx.saved_tensors
        return (g * d_loss).reshape(ctx.shape) if ctx.needs_input_grad[0] else None, None, None


def sigmoid(x: torch.Tensor) -> torch.Tensor:
    return _SigmoidFn.apply(x)


def sigmoid_cross_entropy(labels, logits):
    """tf.losses.sigmoid_cross_entropy(labels, logits): mean over all elements ([TF] B9)."""
    return _LogitLossFn.apply(logits.contiguous(), labels.to(torch.float32).contiguous(), ops.LOSS_SIGMOID_CE)


def log_loss(labels, predictions):
    """tf.losses.log_loss(labels, predictions) on probabilities, eps = 1e-7 ([TF] B10)."""
    return _ProbLossFn.apply(predictions.contiguous(), labels.to(torch.float32).contiguous(), ops.LOSS_LOG_LOSS)


def binary_crossentropy(y_true, y_pred):
    """tf.keras.losses.binary_crossentropy on probabilities, mean over the batch ([TF] B11)."""
    return _ProbLossFn.apply(y_pred.contiguous(), y_true.to(torch.float32).contiguous(), ops.LOSS_KERAS_BCE)


class _MseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, predictions, labels):
        loss, d = ops.mse_fwd_bwd(predictions, labels)
        ctx.save_for_backward(d)
        ctx.shape = predictions.shape
        return loss

    @staticmethod
    @_needed_only
    def backward(ctx, d_loss):
        (d,) = ctx.saved_tensors
        return (d * d_loss.reshape(1, -1)).reshape(ctx.shape) if ctx.needs_input_grad[0] else None, None


def mean_squared_error(labels, predictions):
    """tf.losses.mean_squared_error(labels, predictions) with unit weights (SUM_BY_NONZERO_WEIGHTS = the mean over the batch),
    examples/train_mmoe_on_synthetic_estimator.py:39-40.  predictions [B, 1] (or [B, T]: T losses in one launch, returned [T])."""
    p = predictions if predictions.dim() == 2 else predictions.reshape(-1, 1)
    y = torch.as_tensor(labels, dtype=torch.float32, device=p.device).reshape(p.shape)
    loss = _MseFn.apply(_rows(p), _rows(y))
    return loss.reshape(()) if p.shape[1] == 1 else loss


class _SoftmaxCEFn(torch.autograd.Function):
    """sum_r w_r * CE(softmax(logits_r), y_r) on dr_softmax_ce_rows; the gradient goes to the logits directly"""

    @staticmethod
    def forward(ctx, logits, labels, weights):
        loss = ops.softmax_ce_rows(logits, labels, 1.0, weights)
        ctx.save_for_backward(ops.softmax_ce_rows_bwd(logits, labels, 1.0, weights, 1.0))
        return loss

    @staticmethod
    @_needed_only
    def backward(ctx, d_loss):
        (g,) = ctx.saved_tensors
        return g * d_loss if ctx.needs_input_grad[0] else None, None, None


class _CceProbFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prob, labels, weights):
        row, g = ops.cce_prob_rows(prob, labels, weights)
        ctx.save_for_backward(g)
        return ops.reduce_sum(row).reshape(())

    @staticmethod
    @_needed_only
    def backward(ctx, d_loss):
        (g,) = ctx.saved_tensors
        return g * d_loss if ctx.needs_input_grad[0] else None, None, None


def categorical_crossentropy(y_true, y_pred, sample_weight=None):
    """tf.keras.losses.categorical_crossentropy under compile/fit (examples/train_gcn_on_cora_keras.py:28-31): the weighted per-row
    cross-entropies summed and divided by the number of rows, every row counted (SUM_OVER_BATCH_SIZE; sample_weight is the train
    mask there).  When y_pred is the output of a softmax layer of this package (GCN(activation="softmax")) the loss is computed from
    that layer's logits, unclipped, and the gradient goes straight to them -- what Keras' backend does for a Softmax op.  Any other
    probability tensor takes Keras' formula: p / sum(p), clipped to [1e-7, 1 - 1e-7]."""
    logits = getattr(y_pred, "_dr_logits", None)
    p = logits if logits is not None else y_pred
    B = p.shape[0]
    y = torch.as_tensor(y_true, dtype=torch.float32)
    y = (y.cuda() if not y.is_cuda else y).reshape(p.shape).contiguous()
    if sample_weight is None:
        w = torch.full((B,), 1.0 / B, dtype=torch.float32, device=y.device)
    else:
        w = torch.as_tensor(np.asarray(sample_weight, dtype=np.float64).reshape(-1) / B if not isinstance(sample_weight, torch.Tensor)
                            else sample_weight.detach().to(torch.float64).reshape(-1).cpu().numpy() / B)
        w = w.to(torch.float32).to(y.device)
    if logits is not None:
        return _SoftmaxCEFn.apply(logits.contiguous(), y, w)
    return _CceProbFn.apply(_rows(y_pred), y, w)
