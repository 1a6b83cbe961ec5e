"""A numpy restatement of K12 (include/krs.h): the bucket and threshold rules in float32, every
sum in float64, and keras.metrics.AUC.result() in float64.  Not a test: the binary-metric tests import it."""

import numpy as np

EPSILON = 1e-7   # keras.backend.epsilon()


def probability(pred, from_logits=False):
    """float32: the sigmoid for logits, then the clamp to [0, 1] with NaN -> 0."""
    x = np.asarray(pred, np.float32)
    if from_logits:
        with np.errstate(over="ignore"):
            x = (np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))).astype(np.float32)
    p = np.where(x > 0, x, np.float32(0.0)).astype(np.float32)     # (NaN > 0 is false)
    return np.where(p < 1, p, np.float32(1.0)).astype(np.float32)


def default_thresholds(num_thresholds):
    """keras' list: -1e-7, 1/(T-1), .., (T-2)/(T-1), 1+1e-7 (float64)."""
    inner = [(i + 1) * 1.0 / (num_thresholds - 1) for i in range(num_thresholds - 2)]
    return np.array([0.0 - EPSILON] + inner + [1.0 + EPSILON])


def buckets(p, num_thresholds, thresholds=None):
    """b per sample (int64): the bucket route for thresholds=None, else #{i : t_i < p} - 1 on the float32 thresholds."""
    p = np.asarray(p, np.float32)
    if thresholds is None:
        assert num_thresholds >= 3
        prod = (p * np.float32(num_thresholds - 1)).astype(np.float32)
        return np.maximum(np.ceil(prod).astype(np.int64) - 1, 0)
    th = np.asarray(thresholds, np.float32)
    assert th.shape == (num_thresholds,) and np.all(th[:-1] <= th[1:])
    return np.searchsorted(th, p, side="left").astype(np.int64) - 1


def _weights(sample_weight, n):
    if sample_weight is None:
        return np.ones(n, np.float64)
    w = np.asarray(sample_weight, np.float32).astype(np.float64).reshape(-1)
    return np.broadcast_to(w, (n,)) if w.size == 1 else w


def confusion(y_true, y_pred, sample_weight=None, num_thresholds=200, thresholds=None, from_logits=False):
    """(tp, fp, tn, fn), float64 [num_thresholds] each, of one update."""
    y = np.asarray(y_true, np.float32).reshape(-1)
    x = np.asarray(y_pred, np.float32).reshape(-1)
    w = _weights(sample_weight, x.size)
    b = buckets(probability(x, from_logits), num_thresholds, thresholds)
    positive = y != 0
    pos = np.zeros(num_thresholds, np.float64)
    neg = np.zeros(num_thresholds, np.float64)
    inside = b >= 0
    np.add.at(pos, b[inside & positive], w[inside & positive])
    np.add.at(neg, b[inside & ~positive], w[inside & ~positive])
    tp = np.cumsum(pos[::-1])[::-1].copy()
    fp = np.cumsum(neg[::-1])[::-1].copy()
    return tp, fp, w[~positive].sum() - fp, w[positive].sum() - tp


def accuracy(y_true, y_pred, sample_weight=None, threshold=0.5):
    """(total, count) in float64 of one BinaryAccuracy update."""
    y = np.asarray(y_true, np.float32).reshape(-1)
    x = np.asarray(y_pred, np.float32).reshape(-1)
    w = _weights(sample_weight, x.size)
    match = (x > np.float32(threshold)).astype(np.float32) == y
    return w[match].sum(), w.sum()


def _dnn(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.where(b != 0, a / np.where(b != 0, b, 1.0), 0.0)


def auc_from_confusion(tp, fp, tn, fn, curve="ROC", summation_method="interpolation", dtype=np.float64):
    """keras.metrics.AUC.result() in `dtype` (float64; float32 gives the rounding error a plain fp32 evaluation has)."""
    tp, fp, tn, fn = (np.asarray(v, dtype) for v in (tp, fp, tn, fn))
    dnn = (lambda a, b: _dnn(a, b).astype(dtype)) if dtype == np.float64 else (
        lambda a, b: np.where(b != 0, a / np.where(b != 0, b, dtype(1)), dtype(0)).astype(dtype))
    if curve == "PR" and summation_method == "interpolation":
        dtp = tp[:-1] - tp[1:]
        p = tp + fp
        slope = dnn(dtp, np.maximum(p[:-1] - p[1:], 0))
        intercept = tp[1:] - slope * p[1:]
        ratio = np.where((p[:-1] > 0) & (p[1:] > 0), dnn(p[:-1], np.maximum(p[1:], 0)), dtype(1)).astype(dtype)
        return dnn(slope * (dtp + intercept * np.log(ratio)), np.maximum(tp[1:] + fn[1:], 0)).sum(dtype=dtype)
    recall = dnn(tp, tp + fn)
    if curve == "ROC":
        x, y = dnn(fp, fp + tn), recall
    else:
        assert curve == "PR"
        x, y = recall, dnn(tp, tp + fp)
    heights = {"interpolation": (y[:-1] + y[1:]) / dtype(2), "minoring": np.minimum(y[:-1], y[1:]),
               "majoring": np.maximum(y[:-1], y[1:])}[summation_method]
    return ((x[:-1] - x[1:]) * heights).sum(dtype=dtype)
