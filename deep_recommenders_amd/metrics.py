"""Streaming evaluation metrics with the reference scripts' TensorFlow semantics, on a device-resident confusion histogram.

Reference call sites (reference root): examples/train_deepfm_on_movielens_keras.py:45-47 (tf.keras.metrics.AUC / Precision / Recall),
examples/train_{fm,fnn,wdl,deepfm}_on_movielens_estimator.py (tf.metrics.auc).

State: hist [2, T + 1] fp64 on the device; hist[label != 0][b] is the weight of the examples whose prediction exceeds exactly b of
the T ascending thresholds (ops.confusion_hist_update, one call per batch, nothing waits for the device).  result() copies the state
to the host once and evaluates the closed forms below in fp64.  The confusion vectors TensorFlow keeps are suffix sums of the rows:
tp[t] = sum_{b > t} hist[1][b], fp[t] = sum_{b > t} hist[0][b], fn[t] = sum_{b <= t} hist[1][b], tn[t] = sum_{b <= t} hist[0][b].
"""
import numpy as np
import torch

from . import ops
from ._lib import lib

_EPSILON = 1e-7            # K.epsilon() / tf.metrics' kepsilon: how far the end thresholds lie outside [0, 1]


def _div(a, b):
    """a / b, 0 where b == 0 (tf.math.divide_no_nan)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.divide(a, b, out=np.zeros(np.broadcast(a, b).shape, dtype=np.float64), where=b != 0)


def auc_thresholds(num_thresholds=200, thresholds=None):
    """[0 - 1e-7, 1 / (T - 1), ..., (T - 2) / (T - 1), 1 + 1e-7] as fp32, or the given values (each in [0, 1]) sorted between the same
    two ends"""
    if thresholds is not None:
        inner = sorted(float(t) for t in np.asarray(thresholds, dtype=np.float64).reshape(-1))
        if any(not (0.0 <= t <= 1.0) for t in inner):
            raise ValueError("thresholds must lie in [0, 1], got %r" % (thresholds,))
    else:
        if int(num_thresholds) != num_thresholds or num_thresholds < 2:
            raise ValueError("num_thresholds must be an integer >= 2, got %r" % (num_thresholds,))
        T = int(num_thresholds)
        inner = [(i + 1) * 1.0 / (T - 1) for i in range(T - 2)]
    return np.asarray([0.0 - _EPSILON] + inner + [1.0 + _EPSILON], dtype=np.float32)


def confusion_from_hist(hist):
    """hist [2, T + 1] -> (tp, fp, tn, fn), fp64 [T] each.  fn and tn are taken as the prefix sums sum_{b <= t} hist[r][b] -- the
    same numbers as (row total - tp) and (row total - fp), without the cancellation where almost everything lies above a threshold"""
    hist = np.asarray(hist, dtype=np.float64)
    above = np.cumsum(hist[:, ::-1], axis=1)[:, ::-1]          # above[r][b] = sum_{b' >= b} hist[r][b']
    below = np.cumsum(hist, axis=1)                            # below[r][b] = sum_{b' <= b} hist[r][b']
    return above[1, 1:], above[0, 1:], below[0, :-1], below[1, :-1]


def _interpolate_pr_auc(tp, fp, fn):
    """Davis & Goadrich's interpolation of the PR curve between thresholds, as Keras (AUC.interpolate_pr_auc) and TF1
    (careful_interpolation) write it"""
    dtp = tp[:-1] - tp[1:]
    p = tp + fp
    slope = _div(dtp, np.maximum(p[:-1] - p[1:], 0))
    intercept = tp[1:] - slope * p[1:]
    both = (p[:-1] > 0) & (p[1:] > 0)
    ratio = np.where(both, _div(p[:-1], np.maximum(p[1:], 0)), 1.0)
    return float(np.sum(_div(slope * (dtp + intercept * np.log(ratio)), np.maximum(tp[1:] + fn[1:], 0))))


def _riemann(x, y, method):
    if method in ("interpolation", "trapezoidal", "careful_interpolation"):
        heights = (y[:-1] + y[1:]) / 2.0
    elif method == "minoring":
        heights = np.minimum(y[:-1], y[1:])
    else:
        heights = np.maximum(y[:-1], y[1:])
    return float(np.sum((x[:-1] - x[1:]) * heights))


def keras_auc_value(tp, fp, tn, fn, curve="ROC", summation_method="interpolation"):
    """tf.keras.metrics.AUC.result()"""
    if curve == "PR" and summation_method == "interpolation":
        return _interpolate_pr_auc(tp, fp, fn)
    recall = _div(tp, tp + fn)
    if curve == "ROC":
        x, y = _div(fp, fp + tn), recall
    else:
        x, y = recall, _div(tp, tp + fp)
    return _riemann(x, y, summation_method)


def tf1_auc_value(tp, fp, tn, fn, curve="ROC", summation_method="trapezoidal"):
    """tf.metrics.auc's value tensor (epsilon 1e-6 in the rates)"""
    eps = 1.0e-6
    if curve == "PR" and summation_method == "careful_interpolation":
        return _interpolate_pr_auc(tp, fp, fn)
    rec = (tp + eps) / (tp + fn + eps)
    if curve == "ROC":
        x, y = fp / (fp + tn + eps), rec
    else:
        x, y = rec, (tp + eps) / (tp + fp + eps)
    return _riemann(x, y, summation_method)


class _ConfusionMetric:
    """update_state / result / reset_states over one confusion histogram.  `thresholds`: ascending fp32, compared on the device."""

    def __init__(self, thresholds, name, from_logits=False):
        self.name = name
        self._from_logits = bool(from_logits)
        self._thr = np.ascontiguousarray(thresholds, dtype=np.float32)
        if self._thr.size > ops.CONFUSION_HIST_MAX_THRESHOLDS:
            raise ValueError("at most %d thresholds are supported, got %d" % (ops.CONFUSION_HIST_MAX_THRESHOLDS, self._thr.size))
        # the state: a host array until the first update (so that the closed forms can be used and tested without a device), a
        # device tensor from then on
        self._hist = np.zeros((2, self._thr.size + 1), dtype=np.float64)
        self._thr_dev = None
        self._ws = None

    def _to_device(self, device):
        if not isinstance(self._hist, torch.Tensor):
            self._hist = torch.from_numpy(self._hist).to(device)
            self._thr_dev = torch.from_numpy(self._thr).to(device)

    @staticmethod
    def _flat(t, device=None):
        t = torch.as_tensor(t).detach()
        if not t.is_cuda:
            t = t.cuda() if device is None else t.to(device)
        return t.to(torch.float32).reshape(-1)

    def update_state(self, y_true, y_pred, sample_weight=None):
        """Adds a batch: any shapes with equal element counts; sample_weight broadcasts against y_pred.  Enqueues kernel work on the
        current stream and returns -- no .item(), no copy to the host."""
        pred = self._flat(y_pred)
        labels = self._flat(y_true, pred.device)
        if labels.numel() != pred.numel():
            raise ValueError("y_true and y_pred hold %d and %d elements" % (labels.numel(), pred.numel()))
        weights = None
        if sample_weight is not None:
            w = torch.as_tensor(sample_weight).detach().to(pred.device).to(torch.float32)
            if w.numel() != pred.numel():
                shape = tuple(torch.as_tensor(y_pred).shape)
                w = torch.broadcast_to(w.reshape(w.shape + (1,) * (len(shape) - w.dim())), shape)
            weights = w.reshape(-1)
        n = pred.numel()
        if n == 0:
            return
        self._to_device(pred.device)
        need = lib().dr_confusion_hist_workspace_bytes(n, self._thr.size)
        if self._ws is None or self._ws.numel() * 8 < need or self._ws.device != pred.device:
            self._ws = ops.confusion_hist_workspace(n, self._thr.size, pred.device)
        ops.confusion_hist_update(pred, labels, self._thr_dev, self._hist, weights, self._from_logits, self._ws)

    def histogram(self):
        """The state on the host, fp64 [2, T + 1] (one device-to-host copy of at most 64 KB)."""
        if isinstance(self._hist, torch.Tensor):
            return self._hist.cpu().numpy()
        return self._hist.copy()

    def load_histogram(self, hist):
        """Replaces the state (restoring an evaluation, or stating counters directly)."""
        hist = np.array(hist, dtype=np.float64)
        if hist.shape != (2, self._thr.size + 1):
            raise ValueError("expected a [2, %d] histogram, got %r" % (self._thr.size + 1, hist.shape))
        if isinstance(self._hist, torch.Tensor):
            self._hist.copy_(torch.from_numpy(hist))
        else:
            self._hist = hist

    def reset_states(self):
        if isinstance(self._hist, torch.Tensor):
            self._hist.zero_()
        else:
            self._hist[:] = 0.0

    reset_state = reset_states

    def _confusion(self):
        return confusion_from_hist(self.histogram())

    true_positives = property(lambda self: self._confusion()[0])
    false_positives = property(lambda self: self._confusion()[1])
    true_negatives = property(lambda self: self._confusion()[2])
    false_negatives = property(lambda self: self._confusion()[3])


class AUC(_ConfusionMetric):
    """tf.keras.metrics.AUC(num_thresholds=200, curve="ROC", summation_method="interpolation", name="auc", thresholds=None,
    from_logits=False).  multi_label / label_weights are not implemented (no reference script uses them)."""

    def __init__(self, num_thresholds=200, curve="ROC", summation_method="interpolation", name="auc", thresholds=None,
                 multi_label=False, num_labels=None, label_weights=None, from_logits=False):
        if multi_label or label_weights is not None:
            raise NotImplementedError("AUC(multi_label / label_weights) is not implemented")
        if curve not in ("ROC", "PR"):
            raise ValueError("curve must be 'ROC' or 'PR', got %r" % (curve,))
        if summation_method not in ("interpolation", "minoring", "majoring"):
            raise ValueError("summation_method must be 'interpolation', 'minoring' or 'majoring', got %r" % (summation_method,))
        super().__init__(auc_thresholds(num_thresholds, thresholds), name, from_logits)
        self.num_thresholds = self._thr.size
        self.curve, self.summation_method = curve, summation_method

    @property
    def thresholds(self):
        return [float(t) for t in self._thr[1:-1]]

    def result(self):
        return keras_auc_value(*self._confusion(), curve=self.curve, summation_method=self.summation_method)


class StreamingAUC(_ConfusionMetric):
    """tf.metrics.auc(labels, predictions, num_thresholds=200, curve="ROC", summation_method="trapezoidal"): the estimator scripts'
    metric.  Same state and thresholds as AUC; the rates carry TF1's epsilon of 1e-6."""

    def __init__(self, num_thresholds=200, curve="ROC", summation_method="trapezoidal", name="auc"):
        if curve not in ("ROC", "PR"):
            raise ValueError("curve must be 'ROC' or 'PR', got %r" % (curve,))
        if summation_method not in ("trapezoidal", "careful_interpolation", "minoring", "majoring"):
            raise ValueError("summation_method must be 'trapezoidal', 'careful_interpolation', 'minoring' or 'majoring', got %r"
                             % (summation_method,))
        super().__init__(auc_thresholds(num_thresholds), name)
        self.num_thresholds = self._thr.size
        self.curve, self.summation_method = curve, summation_method

    def result(self):
        return tf1_auc_value(*self._confusion(), curve=self.curve, summation_method=self.summation_method)


class _AtThresholds(_ConfusionMetric):
    """Precision / Recall: thresholds as given (default 0.5), a float result for a scalar threshold and a list for a list"""

    def __init__(self, thresholds, name, top_k=None, class_id=None):
        if top_k is not None or class_id is not None:
            raise NotImplementedError("%s(top_k / class_id) is not implemented" % type(self).__name__)
        self._scalar = thresholds is None or np.ndim(thresholds) == 0
        given = np.asarray([0.5] if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
        if given.size == 0 or np.any(~((given >= 0.0) & (given <= 1.0))):
            raise ValueError("thresholds must lie in [0, 1], got %r" % (thresholds,))
        self.thresholds = [float(t) for t in given]
        self._order = np.argsort(given, kind="stable")           # the kernel wants them ascending
        self._rank = np.argsort(self._order, kind="stable")      # position of each given threshold in the sorted array
        super().__init__(given[self._order].astype(np.float32), name)

    def _confusion(self):
        return tuple(v[self._rank] for v in super()._confusion())

    def _value(self, tp, fp, tn, fn):
        raise NotImplementedError

    def result(self):
        v = self._value(*self._confusion())
        return float(v[0]) if self._scalar else [float(x) for x in v]


class Precision(_AtThresholds):
    """tf.keras.metrics.Precision(thresholds=None): tp / (tp + fp), 0 where nothing was predicted positive"""

    def __init__(self, thresholds=None, top_k=None, class_id=None, name="precision"):
        super().__init__(thresholds, name, top_k, class_id)

    def _value(self, tp, fp, tn, fn):
        return _div(tp, tp + fp)


class Recall(_AtThresholds):
    """tf.keras.metrics.Recall(thresholds=None): tp / (tp + fn), 0 where there was no positive"""

    def __init__(self, thresholds=None, top_k=None, class_id=None, name="recall"):
        super().__init__(thresholds, name, top_k, class_id)

    def _value(self, tp, fp, tn, fn):
        return _div(tp, tp + fn)
