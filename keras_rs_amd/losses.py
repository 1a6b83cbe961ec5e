"""keras_rs.losses on MI355X: the pairwise ranking losses and ListMLE (keras_rs/src/losses/), unreduced loss and
logit gradient from one pass over each list (K9, csrc/ranking_loss.hip).

The classes are plain callables like layers.BinaryCrossentropy: loss(y_true, y_pred, sample_weight=None).

Inputs, as in the reference (pairwise_loss.py:call, metrics/utils.py:standardize_call_inputs_ranks):
  * y_true is a tensor of labels, or a dict {"labels": ..., "mask": ...}.  An item is valid when its label is >= 0
    and its mask entry is set; invalid items form no pairs and take no part in ListMLE.
  * y_true, y_pred and mask have one shape, [list] (one list, treated as [1, list]) or [batch, list];
    1 <= list <= 4096 (a longer list raises KrsError).
  * y_pred is fp32 or bf16 and is computed on in fp32; the loss is fp32 and the gradient has y_pred's dtype.  Labels
    of any real dtype are cast to fp32 and get no gradient.

Reductions follow keras.losses.Loss (Keras 3).  With v the unreduced losses ([batch, list] for the pairwise losses,
[batch] for ListMLE) and w the sample weight broadcast to v (a scalar, v's shape, or one weight per list as [batch]
or [batch, 1]):
  "none" / None                      v * w
  "sum"                              sum(v * w)
  "sum_over_batch_size", "mean"      sum(v * w) / v.numel()
  "mean_with_sample_weight"          sum(v * w) / sum(w), 0 when sum(w) == 0 (v.numel() without a weight)

The gradient is the one autodiff takes of the reference's expression in every Keras backend, including its
non-smooth points: PairwiseLogisticLoss has gradient 0 at a score tie (relu'(0) = abs'(0) = 0), PairwiseHingeLoss
gradient 0 at x == 1, and ListMLE's includes the 1e-10 of its normalisers and the path through the max shift.
"""

from __future__ import annotations

import abc
import re
from typing import Any

import torch

from keras_rs_amd.ranking_ops import RankingLossFn

REDUCTIONS = ("sum", "sum_over_batch_size", "mean", "mean_with_sample_weight", "none", None)


def _snake(name: str) -> str:
    """keras' default loss name: ListMLELoss -> list_mle_loss."""
    name = re.sub(r"(.)([A-Z][a-z]+)", r"\1_\2", name)
    return re.sub(r"([a-z])([A-Z])", r"\1_\2", name).lower()


def _tensor(x, device=None) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x if device is None else x.to(device)
    return torch.as_tensor(x, device=device)


def _standardize(y_true, y_pred):
    """(labels, y_pred, mask) as [batch, list] tensors, after the reference's checks (all before any device check)."""
    mask = None
    if isinstance(y_true, dict):
        if "labels" not in y_true:
            raise ValueError(f'`"labels"` should be present in `y_true`. Received: `y_true` = {y_true}')
        mask = y_true.get("mask", None)
        y_true = y_true["labels"]
    y_pred = _tensor(y_pred)
    y_true = _tensor(y_true, y_pred.device)
    if mask is not None:
        mask = _tensor(mask, y_pred.device)
    for t, name in ((y_true, "y_true"), (y_pred, "y_pred"), (mask, "mask")):
        if t is not None and t.dim() not in (1, 2):
            raise ValueError(f"`{name}` should have a rank from `(1, 2)`. Received: rank {t.dim()}, shape "
                             f"{tuple(t.shape)}.")
    if tuple(y_true.shape) != tuple(y_pred.shape):
        raise ValueError("`y_true` and `y_pred` should have the same shape. Received: "
                         f"`y_true.shape` = {tuple(y_true.shape)}, `y_pred.shape` = {tuple(y_pred.shape)}.")
    if mask is not None and tuple(mask.shape) != tuple(y_true.shape):
        raise ValueError("`y_true['labels']` and `y_true['mask']` should have the same shape. Received: "
                         f"`y_true['labels'].shape` = {tuple(y_true.shape)}, `y_true['mask'].shape` = "
                         f"{tuple(mask.shape)}.")
    if y_true.dim() == 1:
        y_true, y_pred = y_true.unsqueeze(0), y_pred.unsqueeze(0)
        mask = None if mask is None else mask.unsqueeze(0)
    if y_pred.dtype not in (torch.float32, torch.bfloat16):
        y_pred = y_pred.to(torch.float32)
    return y_true, y_pred, mask


def _sample_weight(sample_weight, shape, device) -> torch.Tensor | None:
    """The weight as a tensor broadcastable to v's `shape` ([batch, list] or [batch]), or ValueError."""
    if sample_weight is None:
        return None
    w = _tensor(sample_weight, device).to(torch.float32)
    batch = shape[0]
    if w.dim() == 0 or tuple(w.shape) == tuple(shape):
        return w
    if len(shape) == 2 and tuple(w.shape) in ((batch,), (batch, 1)):
        return w.reshape(batch, 1)
    if len(shape) == 1 and tuple(w.shape) == (batch, 1):
        return w.reshape(batch)
    raise ValueError(f"`sample_weight` of shape {tuple(w.shape)} cannot be broadcast to the unreduced loss of shape "
                     f"{tuple(shape)}: give a scalar, the loss's shape, or one weight per list ({batch},) / "
                     f"({batch}, 1).")


class _RankingLoss(abc.ABC):
    _kind = ""

    def __init__(self, temperature: float = 1.0, reduction: str | None = "sum_over_batch_size",
                 name: str | None = None, dtype: Any = None):
        if temperature <= 0.0:
            raise ValueError(f"`temperature` should be a positive float. Received: `temperature` = {temperature}.")
        if reduction not in REDUCTIONS:
            raise ValueError(f"Invalid value for argument `reduction`. Expected one of {REDUCTIONS}. Received: "
                             f"reduction={reduction}")
        if dtype not in (None, "float32", torch.float32):
            raise ValueError(f"{type(self).__name__}: the loss is computed in float32; dtype={dtype} is not supported")
        self.temperature = float(temperature)
        self.reduction = reduction
        self.name = name or _snake(type(self).__name__)

    def _unreduced_shape(self, b: int, n: int):
        return (b,) if self._kind == "listmle" else (b, n)

    def __call__(self, y_true, y_pred, sample_weight=None) -> torch.Tensor:
        labels, logits, mask = _standardize(y_true, y_pred)
        w = _sample_weight(sample_weight, self._unreduced_shape(*logits.shape), logits.device)
        reduction = "none" if self.reduction is None else self.reduction
        inv_t = 1.0 if self._kind == "mse" else 1.0 / self.temperature
        return RankingLossFn.apply(logits, labels, mask, w, self._kind, inv_t, reduction)

    def get_config(self) -> dict:
        return {"name": self.name, "reduction": self.reduction, "dtype": "float32", "temperature": self.temperature}

    @classmethod
    def from_config(cls, config: dict):
        return cls(**config)


class PairwiseLoss(_RankingLoss):
    """Base of the pairwise ranking losses (pairwise_loss.py): per item i, sum_j I(y_i > y_j) valid_i valid_j
    loss(x_ij), x_ij = (s_i - s_j) / temperature; unreduced shape [batch, list]."""

    @abc.abstractmethod
    def _pair_formula(self) -> str:
        """The per-pair term (documentation only: the arithmetic is K9's)."""


class PairwiseHingeLoss(PairwiseLoss):
    """keras_rs.losses.PairwiseHingeLoss: per pair relu(1 - x).  Gradient 0 at x == 1."""
    _kind = "hinge"

    def _pair_formula(self) -> str:
        return "relu(1 - x)"


class PairwiseLogisticLoss(PairwiseLoss):
    """keras_rs.losses.PairwiseLogisticLoss: per pair relu(-x) + log(1 + exp(-|x|)).  Gradient 0 at a score tie."""
    _kind = "logistic"

    def _pair_formula(self) -> str:
        return "relu(-x) + log(1 + exp(-|x|))"


class PairwiseSoftZeroOneLoss(PairwiseLoss):
    """keras_rs.losses.PairwiseSoftZeroOneLoss: per pair where(x > 0, 1 - sigmoid(x), sigmoid(-x))."""
    _kind = "soft_zero_one"

    def _pair_formula(self) -> str:
        return "where(x > 0, 1 - sigmoid(x), sigmoid(-x))"


class PairwiseMeanSquaredError(PairwiseLoss):
    """keras_rs.losses.PairwiseMeanSquaredError: per item i, sum over the valid j != i of
    ((y_i - y_j) - (s_i - s_j))^2.  The temperature is accepted and validated but, as in the reference, not used."""
    _kind = "mse"

    def _pair_formula(self) -> str:
        return "((y_i - y_j) - (s_i - s_j))^2"


class ListMLELoss(_RankingLoss):
    """keras_rs.losses.ListMLELoss: per list -sum_r log(exp(z_r) / (sum_{q >= r} exp(z_q) + 1e-10)) over the valid
    items in label order, z = s / temperature shifted by its largest valid value; 0 for a list without a valid item.
    Unreduced shape [batch].

    The order is label descending, then index ascending, exactly (the order of top_k in JAX and TensorFlow; the
    reference's torch backend approximates it with a 1e-6 * index offset)."""
    _kind = "listmle"


__all__ = ["ListMLELoss", "PairwiseHingeLoss", "PairwiseLogisticLoss", "PairwiseLoss", "PairwiseMeanSquaredError",
           "PairwiseSoftZeroOneLoss"]
