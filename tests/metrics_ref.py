"""NumPy restatement of the streaming metrics (deep_recommenders_amd/metrics.py, csrc/metrics.hip) the tests compare against.

Every confusion entry is stated the way TensorFlow computes it -- by the direct comparison `pred > threshold` in fp32, one row of
comparisons per threshold, the weights summed in fp64 -- not through a histogram.  The result formulas follow
tf.keras.metrics.AUC / Precision / Recall and tf.metrics.auc."""
import numpy as np

EPS = 1e-7


def auc_thresholds(num_thresholds=200, thresholds=None):
    if thresholds is None:
        inner = [(i + 1) * 1.0 / (num_thresholds - 1) for i in range(num_thresholds - 2)]
    else:
        inner = sorted(thresholds)
    return np.asarray([0.0 - EPS] + inner + [1.0 + EPS], dtype=np.float32)


def confusion(y_true, y_pred, thresholds, weights=None, chunk=1 << 22):
    """(tp, fp, tn, fn), fp64 [T]: tp[t] = sum of w over the examples with label != 0 and pred > thresholds[t], fn[t] = the same sum
    over those with NOT pred > thresholds[t] (a NaN prediction is never above a threshold), fp / tn likewise over label == 0.  Every
    entry is its own sum of non-negative terms (without weights the complement is the count's integer complement, which is exact)."""
    p = np.asarray(y_pred, dtype=np.float32).reshape(-1)
    pos = np.asarray(y_true).reshape(-1) != 0
    thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    w = None if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1).astype(np.float64)
    out = []
    for sel in (pos, ~pos):
        ps = p[sel]
        ws = None if w is None else w[sel][None, :]
        above, rest = np.zeros(len(thr)), np.zeros(len(thr))
        rows = max(1, chunk // max(len(ps), 1))
        for t0 in range(0, len(thr), rows):
            gt = ps[None, :] > thr[t0:t0 + rows, None]
            if w is None:
                above[t0:t0 + rows] = np.count_nonzero(gt, axis=1)
                rest[t0:t0 + rows] = len(ps) - above[t0:t0 + rows]
            else:
                above[t0:t0 + rows] = np.where(gt, ws, 0.0).sum(axis=1)
                rest[t0:t0 + rows] = np.where(gt, 0.0, ws).sum(axis=1)
        out.append((above, rest))
    (tp, fn), (fp, tn) = out
    return tp, fp, tn, fn


def hist_from_confusion(tp, fp, tn, fn):
    """the [2, T + 1] histogram whose suffix sums are these vectors (differences of neighbours; for injecting counters into a metric)"""
    def row(above, total):
        edges = np.concatenate([[total], above, [0.0]])
        return edges[:-1] - edges[1:]
    return np.stack([row(fp, fp[0] + tn[0]), row(tp, tp[0] + fn[0])])


def div(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.zeros(np.broadcast(a, b).shape)
    np.divide(a, b, out=out, where=b != 0)
    return out


def _pr_interpolation(tp, fp, fn):
    P = tp + fp
    dtp, dP = tp[:-1] - tp[1:], P[:-1] - P[1:]
    slope = div(dtp, np.maximum(dP, 0))
    icpt = tp[1:] - slope * P[1:]
    ok = (P[:-1] > 0) & (P[1:] > 0)
    ratio = np.where(ok, div(P[:-1], np.where(ok, P[1:], 1.0)), 1.0)
    return float(np.sum(div(slope * (dtp + icpt * np.log(ratio)), np.maximum(tp[1:] + fn[1:], 0))))


def _area(x, y, method):
    if method in ("interpolation", "trapezoidal", "careful_interpolation"):
        h = 0.5 * (y[:-1] + y[1:])
    elif method == "minoring":
        h = np.minimum(y[:-1], y[1:])
    elif method == "majoring":
        h = np.maximum(y[:-1], y[1:])
    else:
        raise ValueError(method)
    return float(np.sum((x[:-1] - x[1:]) * h))


def keras_auc(tp, fp, tn, fn, curve="ROC", summation_method="interpolation"):
    if curve == "PR" and summation_method == "interpolation":
        return _pr_interpolation(tp, fp, fn)
    if curve == "ROC":
        return _area(div(fp, fp + tn), div(tp, tp + fn), summation_method)
    return _area(div(tp, tp + fn), div(tp, tp + fp), summation_method)


def tf1_auc(tp, fp, tn, fn, curve="ROC", summation_method="trapezoidal"):
    eps = 1e-6
    if curve == "PR" and summation_method == "careful_interpolation":
        return _pr_interpolation(tp, fp, fn)
    rec = (tp + eps) / (tp + fn + eps)
    if curve == "ROC":
        return _area(fp / (fp + tn + eps), rec, summation_method)
    return _area(rec, (tp + eps) / (tp + fp + eps), summation_method)


def precision(tp, fp, tn, fn):
    return div(tp, tp + fp)


def recall(tp, fp, tn, fn):
    return div(tp, tp + fn)
