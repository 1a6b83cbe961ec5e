"""The metrics of the DLRM step on MI355X: `keras.metrics.BinaryAccuracy()` and `keras.metrics.AUC()` as the
reference's ml_perf example compiles them (examples/ml_perf/main.py:201-210), updated by one pass over the
predictions (krs_binary_metrics, csrc/binary_metric.hip).

Both follow keras: update_state(y_true, y_pred, sample_weight=None) adds to a device state, result() is a 0-d fp32
device tensor computed from it with torch ops, reset_state() zeroes it.  Nothing waits for the device, so an update
can be captured in a HIP graph.  y_true and y_pred may have any shapes with the same number of elements ([B],
[B, 1]); sample_weight is a scalar, [B] or y_pred's shape.  y_pred is fp32 or bf16 and is computed on in fp32.

BinaryMetricGroup updates one BinaryAccuracy and up to four AUCs from one krs_binary_metrics call; a member's state
after a group update is bit-identical to its state after updating it alone.

SparseTopKCategoricalAccuracy(k, from_sorted_ids=True) is the metric the reference's retrieval examples compile behind
BruteForceRetrieval: torch ops on the retrieved ids, no kernel of its own (FactorizedTopK, layers/retrieval.py, is the
metric that needs no retrieved ids).
"""

from __future__ import annotations

from typing import Any

import numpy as np
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import metric_ops

_EPSILON = 1e-7   # keras.backend.epsilon()
_CURVES = ("ROC", "PR")
_SUMMATION_METHODS = ("interpolation", "minoring", "majoring")


def _divide_no_nan(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    nz = b != 0
    return torch.where(nz, a / torch.where(nz, b, torch.ones_like(b)), torch.zeros_like(a))


def auc_from_confusion(tp: torch.Tensor, fp: torch.Tensor, tn: torch.Tensor, fn: torch.Tensor, curve: str = "ROC",
                       summation_method: str = "interpolation") -> torch.Tensor:
    """keras.metrics.AUC.result() from the four [T] confusion vectors (any device): the Riemann sum of the curve over
    the thresholds, or keras' interpolate_pr_auc for the PR curve with "interpolation"."""
    if curve not in _CURVES:
        raise ValueError(f'Invalid AUC curve value: "{curve}". Expected values are {list(_CURVES)}')
    if summation_method not in _SUMMATION_METHODS:
        raise ValueError(f'Invalid AUC summation method value: "{summation_method}". Expected values are '
                         f"{list(_SUMMATION_METHODS)}")
    if curve == "PR" and summation_method == "interpolation":
        dtp = tp[:-1] - tp[1:]
        p = tp + fp
        slope = _divide_no_nan(dtp, torch.clamp(p[:-1] - p[1:], min=0))
        intercept = tp[1:] - slope * p[1:]
        ratio = torch.where((p[:-1] > 0) & (p[1:] > 0), _divide_no_nan(p[:-1], torch.clamp(p[1:], min=0)),
                            torch.ones_like(p[1:]))
        return _divide_no_nan(slope * (dtp + intercept * torch.log(ratio)),
                              torch.clamp(tp[1:] + fn[1:], min=0)).sum()
    recall = _divide_no_nan(tp, tp + fn)
    if curve == "ROC":
        x, y = _divide_no_nan(fp, fp + tn), recall
    else:
        x, y = recall, _divide_no_nan(tp, tp + fp)
    if summation_method == "interpolation":
        heights = (y[:-1] + y[1:]) / 2.0
    elif summation_method == "minoring":
        heights = torch.minimum(y[:-1], y[1:])
    else:
        heights = torch.maximum(y[:-1], y[1:])
    return ((x[:-1] - x[1:]) * heights).sum()


def _check_dtype(obj, dtype) -> None:
    if dtype not in (None, "float32", torch.float32):
        raise ValueError(f"{type(obj).__name__}: the metric is computed in float32; dtype={dtype} is not supported")


def _standardize(y_true, y_pred, sample_weight):
    """(labels [n] fp32, pred [n] fp32 / bf16, weights: None, a float or [n] fp32) -- every check is made before any
    device check."""
    y_pred = y_pred if isinstance(y_pred, torch.Tensor) else torch.as_tensor(y_pred)
    dev = y_pred.device
    y_true = y_true.to(dev) if isinstance(y_true, torch.Tensor) else torch.as_tensor(y_true, device=dev)
    n = y_pred.numel()
    if y_true.numel() != n:
        raise ValueError("`y_true` and `y_pred` should have the same number of elements. Received: `y_true.shape` = "
                         f"{tuple(y_true.shape)}, `y_pred.shape` = {tuple(y_pred.shape)}.")
    weights = None
    if sample_weight is not None:
        if not isinstance(sample_weight, torch.Tensor):
            sample_weight = torch.as_tensor(sample_weight, dtype=torch.float32)
        if sample_weight.dim() == 0:
            if sample_weight.device.type == "cpu":
                weights = float(sample_weight)                  # (reaches the kernel as an argument: no upload)
            else:
                weights = sample_weight.to(device=dev, dtype=torch.float32).expand(n)
        elif sample_weight.numel() != n:
            raise ValueError(f"`sample_weight` of shape {tuple(sample_weight.shape)} cannot be broadcast to `y_pred` "
                             f"of shape {tuple(y_pred.shape)}: give a scalar, one weight per sample or `y_pred`'s "
                             "shape.")
        else:
            weights = sample_weight.to(device=dev, dtype=torch.float32).reshape(-1)
    if y_pred.dtype not in (torch.float32, torch.bfloat16):
        y_pred = y_pred.to(torch.float32)
    return y_true.to(torch.float32).reshape(-1), y_pred.reshape(-1), weights


def _update(accuracy, aucs, y_true, y_pred, sample_weight) -> None:
    """One krs_binary_metrics call for an optional BinaryAccuracy and a list of AUCs."""
    labels, pred, weights = _standardize(y_true, y_pred, sample_weight)
    L.require_device(pred, "update_state")
    dev = pred.device
    acc = None if accuracy is None else (accuracy.threshold, accuracy._device_state(dev))
    specs = []
    for m in aucs:
        state = m._device_state(dev)
        specs.append((m._device_thresholds(dev), m.num_thresholds, m.from_logits, state))
    metric_ops.binary_metrics(pred, labels, weights, accuracy=acc, aucs=specs)


class _BinaryMetric:
    _state_shape: tuple = ()
    _state = None
    name = ""

    def _device_state(self, device) -> torch.Tensor:
        if self._state is None or self._state.device != device:
            self._state = torch.zeros(self._state_shape, dtype=torch.float32, device=device)
        return self._state

    def reset_state(self) -> None:
        if self._state is not None:
            self._state.zero_()

    def __call__(self, y_true, y_pred, sample_weight=None) -> torch.Tensor:
        self.update_state(y_true, y_pred, sample_weight)
        return self.result()

    @classmethod
    def from_config(cls, config: dict):
        return cls(**config)


class BinaryAccuracy(_BinaryMetric):
    """keras.metrics.BinaryAccuracy: the weighted mean of `y_true == (y_pred > threshold)`; the state is
    keras.metrics.Mean's {total, count}.  A label that is neither 0 nor 1 matches nothing."""
    _state_shape = (2,)

    def __init__(self, name: str = "binary_accuracy", dtype: Any = None, threshold: float = 0.5):
        _check_dtype(self, dtype)
        self.name = name
        self.threshold = float(threshold)

    def update_state(self, y_true, y_pred, sample_weight=None) -> None:
        _update(self, [], y_true, y_pred, sample_weight)

    def result(self) -> torch.Tensor:
        if self._state is None:
            return torch.zeros((), dtype=torch.float32)
        return _divide_no_nan(self._state[0], self._state[1])

    @property
    def variables(self) -> list:
        state = self._device_state(torch.device("cpu") if self._state is None else self._state.device)
        return [state[0], state[1]]

    def get_config(self) -> dict:
        return {"name": self.name, "dtype": "float32", "threshold": self.threshold}


class AUC(_BinaryMetric):
    """keras.metrics.AUC for one label: the confusion counts at `num_thresholds` thresholds, accumulated on the
    device, and the area under the ROC or PR curve from them (auc_from_confusion).

    thresholds=None is keras' even set, which takes the bucket route of krs_binary_metrics exactly as keras does
    (also for a given list that is the even set within keras' tolerance); any other list, and num_thresholds=2,
    takes the comparison route.  Predictions are clamped to [0, 1] (NaN counts as 0); a sample is positive iff its
    label is non-zero."""

    def __init__(self, num_thresholds: int = 200, curve: str = "ROC", summation_method: str = "interpolation",
                 name: str | None = None, dtype: Any = None, thresholds=None, multi_label: bool = False,
                 num_labels: int | None = None, label_weights=None, from_logits: bool = False):
        if curve not in _CURVES:
            raise ValueError(f'Invalid AUC curve value: "{curve}". Expected values are {list(_CURVES)}')
        if summation_method not in _SUMMATION_METHODS:
            raise ValueError(f'Invalid AUC summation method value: "{summation_method}". Expected values are '
                             f"{list(_SUMMATION_METHODS)}")
        self._init_from_thresholds = thresholds is not None
        if thresholds is not None:
            inner = sorted(float(t) for t in thresholds)
            if any(t < 0.0 or t > 1.0 for t in inner):
                raise ValueError(f"Threshold values must be in [0, 1]. Received: {list(thresholds)}")
            num_thresholds = len(inner) + 2
        else:
            if isinstance(num_thresholds, bool) or not isinstance(num_thresholds, int) or num_thresholds <= 1:
                raise ValueError("Argument `num_thresholds` must be an integer > 1. Received: "
                                 f"num_thresholds={num_thresholds}")
            inner = [(i + 1) * 1.0 / (num_thresholds - 1) for i in range(num_thresholds - 2)]
        if num_thresholds > metric_ops.MAX_THRESHOLDS:
            raise ValueError(f"AUC: {num_thresholds} thresholds, end points included, where at most "
                             f"{metric_ops.MAX_THRESHOLDS} are supported")
        if multi_label or num_labels is not None or label_weights is not None:
            raise NotImplementedError("AUC(multi_label / num_labels / label_weights): the reference's model has one "
                                      "label (examples/ml_perf/model.py:105-163), and so has this metric")
        _check_dtype(self, dtype)
        self.num_thresholds = num_thresholds
        self.curve, self.summation_method = curve, summation_method
        self.name = name or "auc"
        self.from_logits = bool(from_logits)
        self._thresholds = np.array([0.0 - _EPSILON] + inner + [1.0 + _EPSILON])
        # keras' metrics_utils.is_evenly_distributed_thresholds
        even = np.arange(num_thresholds, dtype=np.float32) / max(num_thresholds - 1, 1)
        self._even = num_thresholds >= 3 and bool(np.allclose(self._thresholds, even, atol=_EPSILON))
        self._state_shape = (4, num_thresholds)
        self._th_dev = None

    @property
    def thresholds(self) -> list:
        return list(self._thresholds)

    def _device_thresholds(self, device):
        if self._even:
            return None
        if self._th_dev is None or self._th_dev.device != device:
            self._th_dev = torch.from_numpy(self._thresholds.astype(np.float32)).to(device)
        return self._th_dev

    @property
    def variables(self) -> list:
        """true_positives, false_positives, true_negatives, false_negatives: [num_thresholds] each."""
        state = self._device_state(torch.device("cpu") if self._state is None else self._state.device)
        return [state[0], state[1], state[2], state[3]]

    def update_state(self, y_true, y_pred, sample_weight=None) -> None:
        _update(None, [self], y_true, y_pred, sample_weight)

    def result(self) -> torch.Tensor:
        return auc_from_confusion(*self.variables, curve=self.curve, summation_method=self.summation_method)

    def get_config(self) -> dict:
        config = {"name": self.name, "dtype": "float32", "num_thresholds": self.num_thresholds, "curve": self.curve,
                  "summation_method": self.summation_method, "multi_label": False, "num_labels": None,
                  "label_weights": None, "from_logits": self.from_logits}
        if self._init_from_thresholds:
            config["thresholds"] = self.thresholds[1:-1]   # (the end points are added again)
        return config


class SparseTopKCategoricalAccuracy:
    """keras.metrics.SparseTopKCategoricalAccuracy(k, from_sorted_ids=True) as the reference's retrieval examples
    compile it behind BruteForceRetrieval(return_scores=False): y_pred [B, k'] holds each row's retrieved ids, best
    first, and a row is a hit when y_true [B] (or [B, 1]) is among its first k columns.  The state is
    keras.metrics.Mean's {total, count} as a device tensor; update_state is a handful of torch ops on y_pred's device
    and waits for nothing.  from_sorted_ids=False (y_pred = stored logits) is not implemented: FactorizedTopK gives
    the top-k accuracies of a two-tower model from the embeddings, without the logits."""
    _state = None

    def __init__(self, k: int = 5, from_sorted_ids: bool = False, name: str = "sparse_top_k_categorical_accuracy",
                 dtype: Any = None):
        _check_dtype(self, dtype)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"`k` should be an integer >= 1. Received: k={k!r}")
        if not from_sorted_ids:
            raise NotImplementedError("SparseTopKCategoricalAccuracy: only from_sorted_ids=True (y_pred = the ids "
                                      "BruteForceRetrieval returns) is implemented; for the top-k accuracy of a "
                                      "two-tower model from its embeddings use keras_rs_amd.layers.FactorizedTopK")
        self.k, self.from_sorted_ids, self.name = int(k), True, name

    def update_state(self, y_true, y_pred, sample_weight=None) -> None:
        y_pred = y_pred if isinstance(y_pred, torch.Tensor) else torch.as_tensor(np.asarray(y_pred))
        dev = y_pred.device
        y_true = y_true.to(dev) if isinstance(y_true, torch.Tensor) else torch.as_tensor(np.asarray(y_true), device=dev)
        if y_pred.dim() != 2 or y_true.numel() != y_pred.shape[0] or y_true.dim() > 2:
            raise ValueError("`y_pred` should be [batch, ids] and `y_true` one id per row. Received: `y_true.shape` = "
                             f"{tuple(y_true.shape)}, `y_pred.shape` = {tuple(y_pred.shape)}.")
        if y_pred.dtype.is_floating_point or y_true.dtype.is_floating_point:
            raise ValueError(f"`y_true` ({y_true.dtype}) and `y_pred` ({y_pred.dtype}) should be integer ids")
        b = y_pred.shape[0]
        w = None
        if sample_weight is not None:
            w = sample_weight if isinstance(sample_weight, torch.Tensor) else \
                torch.as_tensor(sample_weight, dtype=torch.float32)
            if w.dim() != 0 and w.numel() != b:
                raise ValueError(f"`sample_weight` of shape {tuple(w.shape)} cannot be broadcast to {b} rows: give a "
                                 "scalar or one weight per row.")
            w = w.to(device=dev, dtype=torch.float32).reshape(-1 if w.dim() else ())
        hit = (y_pred[:, :self.k].to(torch.int64) == y_true.reshape(b, 1).to(torch.int64)).any(dim=1)
        w = torch.ones((b,), dtype=torch.float32, device=dev) if w is None else w.expand((b,))
        if self._state is None or self._state.device != dev:
            self._state = torch.zeros((2,), dtype=torch.float32, device=dev)
        self._state.add_(torch.stack(((w * hit.to(torch.float32)).sum(), w.sum())))

    def result(self) -> torch.Tensor:
        if self._state is None:
            return torch.zeros((), dtype=torch.float32)
        return _divide_no_nan(self._state[0], self._state[1])

    def reset_state(self) -> None:
        if self._state is not None:
            self._state.zero_()

    def __call__(self, y_true, y_pred, sample_weight=None) -> torch.Tensor:
        self.update_state(y_true, y_pred, sample_weight)
        return self.result()

    def get_config(self) -> dict:
        return {"name": self.name, "dtype": "float32", "k": self.k, "from_sorted_ids": self.from_sorted_ids}

    @classmethod
    def from_config(cls, config: dict):
        return cls(**config)


class BinaryMetricGroup:
    """One optional BinaryAccuracy and one to four AUCs updated from one krs_binary_metrics call.  result() is
    {name: tensor}, so the members' names must differ."""

    def __init__(self, metrics):
        metrics = list(metrics)
        for m in metrics:
            if not isinstance(m, (BinaryAccuracy, AUC)):
                raise ValueError(f"BinaryMetricGroup takes BinaryAccuracy and AUC objects. Received: {m!r}")
        accuracies = [m for m in metrics if isinstance(m, BinaryAccuracy)]
        aucs = [m for m in metrics if isinstance(m, AUC)]
        if len(accuracies) > 1 or not 1 <= len(aucs) <= metric_ops.MAX_AUCS:
            raise ValueError(f"BinaryMetricGroup takes at most one BinaryAccuracy and 1 to {metric_ops.MAX_AUCS} "
                             f"AUCs. Received: {len(accuracies)} and {len(aucs)}.")
        if len({m.name for m in metrics}) != len(metrics):
            raise ValueError(f"The metrics of a BinaryMetricGroup need distinct names. Received: "
                             f"{[m.name for m in metrics]}.")
        self.metrics = metrics
        self._accuracy = accuracies[0] if accuracies else None
        self._aucs = aucs

    def update_state(self, y_true, y_pred, sample_weight=None) -> None:
        _update(self._accuracy, self._aucs, y_true, y_pred, sample_weight)

    def result(self) -> dict:
        return {m.name: m.result() for m in self.metrics}

    def reset_state(self) -> None:
        for m in self.metrics:
            m.reset_state()

    def __call__(self, y_true, y_pred, sample_weight=None) -> dict:
        self.update_state(y_true, y_pred, sample_weight)
        return self.result()


# ---- K24: the regression metrics -------------------------------------------------------------------------------------
class _RegressionMetric:
    """keras.metrics.Mean's {total, count} as a device fp32 tensor, fed by the batch sums of krs_regression_fwd_bwd
    (csrc/regression.hip): {sum_b w_b mean_c e^2, sum_b w_b mean_c |e|, sum_b w_b} with sample weights, the plain
    element sums and the element count without.  update_state takes the inputs of the regression losses (the same
    shape rule), waits for nothing and can be captured in a HIP graph."""
    _total = 0            # which batch sum is the total: 0 squared, 1 absolute
    _default_name = ""
    _state = None

    def __init__(self, name: str | None = None, dtype: Any = None):
        _check_dtype(self, dtype)
        self.name = name or self._default_name

    def _device_state(self, device) -> torch.Tensor:
        if self._state is None or self._state.device != device:
            self._state = torch.zeros((2,), dtype=torch.float32, device=device)
        return self._state

    def update_state(self, y_true, y_pred, sample_weight=None) -> None:
        RegressionMetricGroup([self]).update_state(y_true, y_pred, sample_weight)

    def _value(self) -> torch.Tensor:
        if self._state is None:
            return torch.zeros((), dtype=torch.float32)
        return _divide_no_nan(self._state[0], self._state[1])

    def result(self) -> torch.Tensor:
        return self._value()

    @property
    def variables(self) -> list:
        state = self._device_state(torch.device("cpu") if self._state is None else self._state.device)
        return [state[0], state[1]]

    def reset_state(self) -> None:
        if self._state is not None:
            self._state.zero_()

    def __call__(self, y_true, y_pred, sample_weight=None) -> torch.Tensor:
        self.update_state(y_true, y_pred, sample_weight)
        return self.result()

    def get_config(self) -> dict:
        return {"name": self.name, "dtype": "float32"}

    @classmethod
    def from_config(cls, config: dict):
        return cls(**config)


class MeanSquaredError(_RegressionMetric):
    """keras.metrics.MeanSquaredError: the weighted mean of mean((y_pred - y_true)^2, axis=-1)."""
    _total, _default_name = 0, "mean_squared_error"


class RootMeanSquaredError(_RegressionMetric):
    """keras.metrics.RootMeanSquaredError: sqrt(total / count) of MeanSquaredError's state."""
    _total, _default_name = 0, "root_mean_squared_error"

    def result(self) -> torch.Tensor:
        return torch.sqrt(self._value())


class MeanAbsoluteError(_RegressionMetric):
    """keras.metrics.MeanAbsoluteError: the weighted mean of mean(|y_pred - y_true|, axis=-1)."""
    _total, _default_name = 1, "mean_absolute_error"


class RegressionMetricGroup:
    """Any number of regression metrics updated from ONE krs_regression_fwd_bwd call: the call writes the three batch
    sums once and every member adds its two to its own state, so a member's state after a group update is
    bit-identical to its state after updating it alone.  The regression losses take a group (or one metric) as
    `metrics=` and then update it from the call that computes the loss and the gradient.  result() is {name: tensor},
    so the members' names must differ."""

    def __init__(self, metrics):
        metrics = list(metrics)
        for m in metrics:
            if not isinstance(m, _RegressionMetric):
                raise ValueError("RegressionMetricGroup takes RootMeanSquaredError, MeanSquaredError and "
                                 f"MeanAbsoluteError objects. Received: {m!r}")
        if not metrics:
            raise ValueError("RegressionMetricGroup needs at least one metric.")
        if len({m.name for m in metrics}) != len(metrics):
            raise ValueError(f"The metrics of a RegressionMetricGroup need distinct names. Received: "
                             f"{[m.name for m in metrics]}.")
        self.metrics = metrics
        self._sums = None

    def _batch_sums(self, device) -> torch.Tensor:
        """the [3] tensor the kernel writes (kept: a captured update replays into the same memory)"""
        if self._sums is None or self._sums.device != device:
            self._sums = torch.zeros((3,), dtype=torch.float32, device=device)
        return self._sums

    def _add(self, sums: torch.Tensor) -> None:
        for m in self.metrics:
            m._device_state(sums.device).add_(sums[m._total::2 - m._total])   # {total, count} = sums[0 or 1], sums[2]

    def update_state(self, y_true, y_pred, sample_weight=None) -> None:
        from keras_rs_amd import regression_ops
        target, pred, w, _ = regression_ops.standardize(y_true, y_pred, sample_weight, "update_state")
        L.require_device(pred, "update_state")
        sums = self._batch_sums(pred.device)
        regression_ops.regression(pred.detach(), target, w, "mse", want_loss=False, want_grad=False, sums=sums)
        self._add(sums)

    def result(self) -> dict:
        return {m.name: m.result() for m in self.metrics}

    def reset_state(self) -> None:
        for m in self.metrics:
            m.reset_state()

    def __call__(self, y_true, y_pred, sample_weight=None) -> dict:
        self.update_state(y_true, y_pred, sample_weight)
        return self.result()
