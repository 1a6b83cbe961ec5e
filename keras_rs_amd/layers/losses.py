"""The loss of the DLRM step on MI355X: `keras.losses.BinaryCrossentropy()` as the reference's ml_perf example compiles
it (examples/ml_perf/main.py:201-210: probabilities in -- the top MLP ends in a sigmoid, model.py:105-163 --, mean over
the batch), forward and backward in ONE pass over the predictions (krs_bce_fwd_bwd, csrc/loss.hip)."""

from __future__ import annotations

import torch

from keras_rs_amd import losses as _reductions
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
