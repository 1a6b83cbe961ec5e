"""The loss of the DLRM step on MI355X: `keras.losses.BinaryCrossentropy()` as the reference's ml_perf example compiles
it (examples/ml_perf/main.py:201-210: probabilities in -- the top MLP ends in a sigmoid, model.py:105-163 --, mean over
the batch), forward and backward in ONE pass over the predictions (krs_bce_fwd_bwd, csrc/loss.hip); the softmax
crossentropies of the retrieval examples (K11); and the regression losses of the rating examples -- MeanSquaredError,
MeanAbsoluteError, Huber -- with every Keras reduction, sample weights and the regression metrics' update from one
pass over the predictions (K24, krs_regression_fwd_bwd, csrc/regression.hip)."""

from __future__ import annotations

import torch

from keras_rs_amd import losses as _reductions
from keras_rs_amd import regression_ops as _regression
from keras_rs_amd.autograd import BinaryCrossentropyFn
from keras_rs_amd.retrieval_ops import SoftmaxCrossentropyFn


class BinaryCrossentropy:
    """Callable like keras.losses.BinaryCrossentropy(from_logits=False, reduction="sum_over_batch_size"):
    loss(y_true, y_pred) -> scalar.  epsilon = keras.backend.epsilon() = 1e-7 (the clip of the probabilities)."""

    def __init__(self, from_logits: bool = False, epsilon: float = 1e-7, name: str = "binary_crossentropy"):
        if from_logits:
            raise NotImplementedError("BinaryCrossentropy(from_logits=True): the reference's model ends in a sigmoid "
                                      "(examples/ml_perf/model.py:105-163) and compiles the loss with probabilities")
        self.epsilon, self.name = float(epsilon), name

    def __call__(self, y_true: torch.Tensor, y_pred: torch.Tensor) -> torch.Tensor:
        if y_true.numel() != y_pred.numel():
            raise ValueError(f"BinaryCrossentropy: y_true {tuple(y_true.shape)} and y_pred {tuple(y_pred.shape)} differ")
        return BinaryCrossentropyFn.apply(y_pred, y_true, self.epsilon)

    def get_config(self) -> dict:
        return {"name": self.name, "from_logits": False, "epsilon": self.epsilon}


def binary_crossentropy(y_true: torch.Tensor, y_pred: torch.Tensor, epsilon: float = 1e-7) -> torch.Tensor:
    return BinaryCrossentropyFn.apply(y_pred, y_true, epsilon)


class _SoftmaxCrossentropy:
    """What CategoricalCrossentropy and SparseCategoricalCrossentropy share: the arguments this library does not
    implement, the weight and the reduction."""

    def __init__(self, from_logits, reduction, name, axis=-1, ignore_class=None):
        cls = type(self).__name__
        if not from_logits:
            raise NotImplementedError(f"{cls}(from_logits=False): the retrieval head scores with a dot product and "
                                      "hands the loss logits; probabilities in are not implemented")
        if axis != -1:
            raise NotImplementedError(f"{cls}(axis={axis}): the classes are on the last axis (axis=-1) only")
        if ignore_class is not None:
            raise NotImplementedError(f"{cls}(ignore_class={ignore_class}): not implemented; weigh the rows to leave "
                                      "out with a zero `sample_weight`")
        if reduction not in _reductions.REDUCTIONS:
            raise ValueError(f"Invalid value for argument `reduction`. Expected one of {_reductions.REDUCTIONS}. "
                             f"Received: reduction={reduction}")
        self.from_logits, self.axis, self.reduction = True, -1, reduction
        self.name = name or _reductions._snake(type(self).__name__)

    def _reduce(self, logits, labels, index, sample_weight, label_smoothing):
        """logits [..., C]; labels of the same shape or index [...]; the loss with this object's reduction."""
        shape = tuple(logits.shape[:-1])
        w = None
        if sample_weight is not None:
            if shape:
                w = _reductions._sample_weight(sample_weight, shape, logits.device)
            else:
                w = _reductions._tensor(sample_weight, logits.device).to(torch.float32)
                if w.dim() != 0:
                    raise ValueError(f"`sample_weight` of shape {tuple(w.shape)} cannot be broadcast to the scalar "
                                     "loss of a single row: give a scalar.")
            if w.dim() > 0:
                w = w.expand(shape).reshape(-1)          # one weight per row of the flattened logits
        if logits.dtype not in (torch.float32, torch.bfloat16):
            logits = logits.to(torch.float32)
        n = logits.shape[-1]
        reduction = "none" if self.reduction is None else self.reduction
        out = SoftmaxCrossentropyFn.apply(logits.reshape(-1, n), None if labels is None else labels.reshape(-1, n),
                                          None if index is None else index.reshape(-1), w, label_smoothing, reduction)
        return out.reshape(shape) if reduction == "none" else out

    @classmethod
    def from_config(cls, config: dict):
        return cls(**config)


class CategoricalCrossentropy(_SoftmaxCrossentropy):
    """Callable like keras.losses.CategoricalCrossentropy(from_logits=True): loss(y_true, y_pred, sample_weight=None).
    y_true has y_pred's shape [..., classes]; the per-row loss is -sum(y' * log_softmax(y_pred)) with
    y' = y_true * (1 - label_smoothing) + label_smoothing / classes (y_true is not renormalised)."""

    def __init__(self, from_logits: bool = True, label_smoothing: float = 0.0, axis: int = -1,
                 reduction: str | None = "sum_over_batch_size", name: str | None = None):
        super().__init__(from_logits, reduction, name, axis=axis)
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"`label_smoothing` should be in [0, 1). Received: label_smoothing={label_smoothing}")
        self.label_smoothing = float(label_smoothing)

    def __call__(self, y_true, y_pred, sample_weight=None) -> torch.Tensor:
        y_pred = _reductions._tensor(y_pred)
        y_true = _reductions._tensor(y_true, y_pred.device)
        if y_pred.dim() == 0 or tuple(y_true.shape) != tuple(y_pred.shape):
            raise ValueError("`y_true` and `y_pred` should have the same shape [..., classes]. Received: "
                             f"`y_true.shape` = {tuple(y_true.shape)}, `y_pred.shape` = {tuple(y_pred.shape)}.")
        return self._reduce(y_pred, y_true.detach(), None, sample_weight, self.label_smoothing)

    def get_config(self) -> dict:
        return {"name": self.name, "reduction": self.reduction, "from_logits": True,
                "label_smoothing": self.label_smoothing, "axis": -1}


class SparseCategoricalCrossentropy(_SoftmaxCrossentropy):
    """Callable like keras.losses.SparseCategoricalCrossentropy(from_logits=True): y_true holds one class index per
    row, of y_pred's shape without its last axis (a trailing axis of 1 is accepted).  An index outside
    [0, classes) makes that row's loss and gradient NaN."""

    def __init__(self, from_logits: bool = True, ignore_class=None, reduction: str | None = "sum_over_batch_size",
                 axis: int = -1, name: str | None = None):
        super().__init__(from_logits, reduction, name, axis=axis, ignore_class=ignore_class)

    def __call__(self, y_true, y_pred, sample_weight=None) -> torch.Tensor:
        y_pred = _reductions._tensor(y_pred)
        y_true = _reductions._tensor(y_true, y_pred.device)
        rows = tuple(y_pred.shape[:-1])
        if y_pred.dim() == 0 or tuple(y_true.shape) not in (rows, rows + (1,)):
            raise ValueError("`y_true` should have the shape of `y_pred` without its last axis. Received: "
                             f"`y_true.shape` = {tuple(y_true.shape)}, `y_pred.shape` = {tuple(y_pred.shape)}.")
        if y_true.dtype.is_floating_point or y_true.dtype == torch.bool:
            y_true = y_true.to(torch.int64)
        return self._reduce(y_pred, None, y_true.detach().reshape(rows), sample_weight, 0.0)

    def get_config(self) -> dict:
        return {"name": self.name, "reduction": self.reduction, "from_logits": True, "ignore_class": None}


# ---- K24: the regression losses --------------------------------------------------------------------------------------
class _RegressionLoss:
    """What MeanSquaredError, MeanAbsoluteError and Huber share: loss(y_true, y_pred, sample_weight=None), one
    krs_regression_fwd_bwd call (csrc/regression.hip) that reads y_pred once and leaves the reduced loss, the gradient
    and -- with `metrics` -- the batch sums the regression metrics add to their states.

    Shapes: y_pred [..., C] is fp32 or bf16 (computed on in fp32), the per-row value is the mean over the last axis
    and the rows are weighted by sample_weight (a scalar, the leading shape, or one weight per batch row).  The ranks
    of y_true and y_pred may differ by one when the longer shape ends in 1 (y_true [B] with y_pred [B, 1]); after
    that the shapes must be equal, else ValueError.  This DIVERGES from the raw Keras ops, which broadcast [B]
    against [B, 1] into [B, B]: that is never what a rating model means, and it is refused here.  Rank-1 inputs are
    one row, whose sample_weight must be a scalar.  y_true gets no gradient.

    metrics: a RegressionMetricGroup or one regression metric (here, or per call): its update_state runs from the
    same kernel call as the loss and the gradient."""
    _kind = ""
    _delta = 1.0

    def __init__(self, reduction: str | None = "sum_over_batch_size", name: str | None = None, dtype=None,
                 metrics=None):
        if reduction not in _reductions.REDUCTIONS:
            raise ValueError(f"Invalid value for argument `reduction`. Expected one of {_reductions.REDUCTIONS}. "
                             f"Received: reduction={reduction}")
        if dtype not in (None, "float32", torch.float32):
            raise ValueError(f"{type(self).__name__}: the loss is computed in float32; dtype={dtype} is not supported")
        self.reduction = reduction
        self.name = name or _reductions._snake(type(self).__name__)
        self.metrics = _as_metric_group(metrics)

    def __call__(self, y_true, y_pred, sample_weight=None, metrics=None) -> torch.Tensor:
        group = self.metrics if metrics is None else _as_metric_group(metrics)
        target, pred, w, shape = _regression.standardize(y_true, y_pred, sample_weight, type(self).__name__)
        sums = None if group is None else group._batch_sums(pred.device)
        reduction = "none" if self.reduction is None else self.reduction
        out = _regression.RegressionLossFn.apply(pred, target, w, self._kind, self._delta, reduction, sums)
        if group is not None:
            group._add(sums)
        return out.reshape(shape) if reduction == "none" else out

    def get_config(self) -> dict:
        return {"name": self.name, "reduction": self.reduction, "dtype": "float32"}

    @classmethod
    def from_config(cls, config: dict):
        return cls(**config)


def _as_metric_group(metrics):
    if metrics is None:
        return None
    from keras_rs_amd.layers.metrics import RegressionMetricGroup, _RegressionMetric
    if isinstance(metrics, RegressionMetricGroup):
        return metrics
    if isinstance(metrics, _RegressionMetric):
        return RegressionMetricGroup([metrics])
    raise ValueError("`metrics` should be a RegressionMetricGroup or one of RootMeanSquaredError, MeanSquaredError "
                     f"and MeanAbsoluteError from keras_rs_amd.layers. Received: {metrics!r}")


class MeanSquaredError(_RegressionLoss):
    """Callable like keras.losses.MeanSquaredError: per row mean((y_pred - y_true)^2) over the last axis."""
    _kind = "mse"


class MeanAbsoluteError(_RegressionLoss):
    """Callable like keras.losses.MeanAbsoluteError: per row mean(|y_pred - y_true|) over the last axis.  The gradient
    at y_pred == y_true is 0 (sign(0) = 0, as autodiff of abs gives in every Keras backend)."""
    _kind = "mae"


class Huber(_RegressionLoss):
    """Callable like keras.losses.Huber(delta): with e = y_pred - y_true, per element 0.5 e^2 where |e| <= delta and
    delta |e| - 0.5 delta^2 beyond, then the mean over the last axis.  The two gradients agree at |e| == delta."""
    _kind = "huber"

    def __init__(self, delta: float = 1.0, reduction: str | None = "sum_over_batch_size", name: str | None = None,
                 dtype=None, metrics=None):
        if not float(delta) > 0.0:
            raise ValueError(f"`delta` should be a positive float. Received: delta={delta}")
        super().__init__(reduction=reduction, name=name or "huber_loss", dtype=dtype, metrics=metrics)
        self._delta = self.delta = float(delta)

    def get_config(self) -> dict:
        return {**super().get_config(), "delta": self.delta}
