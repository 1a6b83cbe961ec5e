"""keras_rs.metrics on MI355X: DCG, NDCG, MeanAveragePrecision, MeanReciprocalRank, PrecisionAtK and RecallAtK
(keras_rs/src/metrics/), every requested metric of an evaluation batch from one sort of each list (K10,
csrc/ranking_metric.hip).

The classes follow keras.metrics.Mean: update_state(y_true, y_pred, sample_weight=None) adds
sum(per-list value * per-list weight) and sum(per-list weight) to a two-float device state, result() is their
quotient (0 when the count is 0) as a 0-d fp32 device tensor, reset_state() zeroes the state.  Nothing waits for the
device, so an update can be captured in a HIP graph.

Inputs, as in the reference (ranking_metric.py:97-181):
  * y_true is a tensor of labels, or a dict {"labels": ..., "mask": ...}; y_true, y_pred and mask have one shape,
    [list] (one list) or [batch, list]; 1 <= list <= 4096 (a longer list raises KrsError).
  * sample_weight is a scalar, [batch] (one weight per list), [batch, list], or [list] for an unbatched list.
  * an item is valid when its label is >= 0, its mask entry is set and its weight is > 0.  An invalid item counts
    with label 0 and weight 0 and ranks after every valid item.
  * y_pred is fp32 or bf16 and is computed on in fp32.

Order within a list: valid items first, score descending, then ties.  shuffle_ties=False keeps ties in index order
(exactly: no offset is added to the scores).  shuffle_ties=True orders a tie group by a hash of (seed, draw, list,
index) computed in the kernel; `draw` is a device counter that every update advances, a replayed HIP graph included,
so every update breaks ties afresh and every order of a tie group is equally likely.  keras' random stream is not
reproduced.  Unlike the reference, shuffle_ties=False never shuffles (the reference shuffles whenever a mask is
passed, which in its metrics is always).

RankingMetricGroup updates several metrics from one launch and one sort.
"""

from __future__ import annotations

from typing import Any, Callable

import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import metric_ops
from keras_rs_amd.losses import _snake, _tensor


def default_gain_fn(label: torch.Tensor) -> torch.Tensor:
    """2^label - 1 (computed in the kernel unless a custom function replaces it)."""
    return torch.pow(2.0, label) - 1.0


def default_rank_discount_fn(rank: torch.Tensor) -> torch.Tensor:
    """1 / log2(1 + rank) (computed in the kernel unless a custom function replaces it)."""
    return 1.0 / torch.log2(1.0 + rank)


_NAMED_FNS = {"default_gain_fn": default_gain_fn, "default_rank_discount_fn": default_rank_discount_fn}


def _check_rank(rank: int, allowed, name: str) -> None:
    if rank not in allowed:
        raise ValueError(f"`{name}` should have a rank from `{tuple(allowed)}`.Received: `{rank}`.")


def _standardize(y_true, y_pred, sample_weight):
    """(labels, scores, mask or None, weights) after the reference's checks -- all of them before any device check.
    labels, scores and mask are [batch, list] tensors on y_pred's device; weights is None, a float (a scalar
    sample_weight), a [batch] tensor (one weight per list) or a [batch, list] tensor: K10 takes each form as it is,
    so no weight is written out per item."""
    mask = None
    if isinstance(y_true, dict):
        if "labels" not in y_true:
            raise ValueError(f'`"labels"` should be present in `y_true`. Received: `y_true` = {y_true}')
        mask = y_true.get("mask", None)
        y_true = y_true["labels"]
    y_pred = _tensor(y_pred)
    dev = y_pred.device
    y_true = _tensor(y_true, dev)
    if mask is not None:
        mask = _tensor(mask, dev)
    scalar_weight = None
    if sample_weight is not None and not isinstance(sample_weight, torch.Tensor):
        sample_weight = torch.as_tensor(sample_weight, dtype=torch.float32)
    if sample_weight is not None and sample_weight.dim() == 0 and sample_weight.device.type == "cpu":
        scalar_weight, sample_weight = float(sample_weight), None     # (filled on the device: no upload)
    _check_rank(y_true.dim(), (1, 2), "y_true")
    if sample_weight is not None:
        _check_rank(sample_weight.dim(), tuple(range(y_true.dim() + 1)), "sample_weight")
    _check_rank(y_pred.dim(), (1, 2), "y_pred")
    if mask is not None:
        _check_rank(mask.dim(), (1, 2), "mask")
    if tuple(y_true.shape) != tuple(y_pred.shape):
        raise ValueError("`y_true` and `y_pred` should have the same shape. Received: "
                         f"`y_true.shape` = {tuple(y_true.shape)}, `y_pred.shape` = {tuple(y_pred.shape)}.")
    if mask is not None and tuple(mask.shape) != tuple(y_true.shape):
        raise ValueError("`y_true['labels']` and `y_true['mask']` should have the same shape. Received: "
                         f"`y_true['labels'].shape` = {tuple(y_true.shape)}, `y_true['mask'].shape` = "
                         f"{tuple(mask.shape)}.")
    shape = tuple(y_true.shape)
    if sample_weight is not None and sample_weight.dim() > 0:
        ok = (shape,) if len(shape) == 1 else (shape, shape[:1])
        if tuple(sample_weight.shape) not in ok:
            raise ValueError(f"`sample_weight` of shape {tuple(sample_weight.shape)} cannot be broadcast to `y_true` "
                             f"of shape {shape}: give a scalar, `y_true`'s shape"
                             + (f", or one weight per list ({shape[0]},)." if len(shape) == 2 else "."))
    if len(shape) == 1:
        y_true, y_pred = y_true.unsqueeze(0), y_pred.unsqueeze(0)
        mask = None if mask is None else mask.unsqueeze(0)
    if y_pred.dtype not in (torch.float32, torch.bfloat16):
        y_pred = y_pred.to(torch.float32)
    weights = scalar_weight
    if sample_weight is not None:
        weights = sample_weight.to(device=dev, dtype=torch.float32)
        if weights.dim() == 0:                      # (a scalar already on a device: one weight per list)
            weights = weights.expand(y_pred.shape[0])
        elif len(shape) == 1:
            weights = weights.unsqueeze(0)
    return y_true.to(torch.float32), y_pred, None if mask is None else mask.to(torch.bool), weights


def _update(members, shuffle_ties: bool, seed: int, draw_owner, y_true, y_pred, sample_weight) -> None:
    """One stage A launch and one stage B call for all `members` (RankingMetric objects that agree on their custom
    functions)."""
    labels, scores, mask, weights = _standardize(y_true, y_pred, sample_weight)
    L.require_device(scores, "RankingMetric.update_state")
    dev, n = scores.device, scores.shape[1]
    graded = [m for m in members if m._kind in ("dcg", "ndcg")]
    gain = discount = None
    if graded and graded[0].gain_fn is not default_gain_fn:
        valid = labels >= 0
        if mask is not None:
            valid = valid & mask
        if isinstance(weights, float):
            valid = valid if weights > 0 else torch.zeros_like(valid)
        elif weights is not None:
            valid = valid & ((weights if weights.dim() == 2 else weights[:, None]) > 0)
        gain = graded[0].gain_fn(torch.where(valid, labels, torch.zeros_like(labels)))
    if graded and graded[0].rank_discount_fn is not default_rank_discount_fn:
        k_max = max(min(m.k or n, n) for m in graded)
        discount = graded[0].rank_discount_fn(torch.arange(1, k_max + 1, dtype=torch.float32, device=dev))
    draw = draw_owner._device_draw(dev)
    states = [m._device_state(dev) for m in members]
    kinds = [m._kind for m in members]
    values, sums, _ = metric_ops.ranking_metrics([(m._kind, m.k) for m in members], scores, labels, mask, weights,
                                                 gain=gain, discount=discount, shuffle_ties=shuffle_ties, seed=seed,
                                                 draw=draw)
    metric_ops.ranking_metrics_accumulate(kinds, values, sums, states, draw=draw)


class _DrawCounter:
    """The device int64 that numbers the updates of a metric (or group): part of the tie hash, advanced on the
    device by every update."""
    _draw = None

    def _device_draw(self, device) -> torch.Tensor:
        if self._draw is None or self._draw.device != device:
            self._draw = torch.zeros(1, dtype=torch.int64, device=device)
        return self._draw


class RankingMetric(_DrawCounter):
    """Base of the ranking metrics (ranking_metric.py): a weighted mean over lists of a per-list value computed from
    the list sorted by score.  Subclasses name the kernel's metric kind."""
    _kind = ""

    def __init__(self, k: int | None = None, shuffle_ties: bool = True, seed: int | None = None,
                 name: str | None = None, dtype: Any = None):
        if not self._kind:
            raise TypeError(f"{type(self).__name__} names no metric kind: construct DCG, NDCG, MeanAveragePrecision, "
                            "MeanReciprocalRank, PrecisionAtK or RecallAtK")
        if k is not None and (not isinstance(k, int) or k < 1):
            raise ValueError(f"`k` should be a positive integer. Received: `k` = {k}.")
        if dtype not in (None, "float32", torch.float32):
            raise ValueError(f"{type(self).__name__}: the metric is computed in float32; dtype={dtype} is not "
                             "supported")
        self.k = k
        self.shuffle_ties = bool(shuffle_ties)
        self.seed = seed
        # seed=None: drawn from torch's default CPU generator, so torch.manual_seed reproduces a run
        self._seed_value = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
        self.name = name or _snake(type(self).__name__)
        self._state = None

    def _device_state(self, device) -> torch.Tensor:
        if self._state is None or self._state.device != device:
            self._state = torch.zeros(2, dtype=torch.float32, device=device)
        return self._state

    def update_state(self, y_true, y_pred, sample_weight=None) -> None:
        _update([self], self.shuffle_ties, self._seed_value, self, y_true, y_pred, sample_weight)

    def result(self) -> torch.Tensor:
        if self._state is None:
            return torch.zeros((), dtype=torch.float32)
        total, count = self._state[0], self._state[1]
        return torch.where(count != 0, total / torch.where(count != 0, count, torch.ones_like(count)),
                           torch.zeros_like(total))

    def reset_state(self) -> None:
        if self._state is not None:
            self._state.zero_()

    def __call__(self, y_true, y_pred, sample_weight=None) -> torch.Tensor:
        self.update_state(y_true, y_pred, sample_weight)
        return self.result()

    def get_config(self) -> dict:
        return {"name": self.name, "dtype": "float32", "k": self.k, "shuffle_ties": self.shuffle_ties,
                "seed": self.seed}

    @classmethod
    def from_config(cls, config: dict):
        return cls(**config)


def _fn_config(fn: Callable):
    """The default functions serialise by name; a custom callable is kept as the object (there is no registry)."""
    for name, named in _NAMED_FNS.items():
        if fn is named:
            return name
    return fn


class _GradedMetric(RankingMetric):
    def __init__(self, k: int | None = None, gain_fn: Callable = default_gain_fn,
                 rank_discount_fn: Callable = default_rank_discount_fn, **kwargs):
        super().__init__(k=k, **kwargs)
        self.gain_fn = _NAMED_FNS.get(gain_fn, gain_fn) if isinstance(gain_fn, str) else gain_fn
        self.rank_discount_fn = (_NAMED_FNS.get(rank_discount_fn, rank_discount_fn)
                                 if isinstance(rank_discount_fn, str) else rank_discount_fn)
        for fn, arg in ((self.gain_fn, "gain_fn"), (self.rank_discount_fn, "rank_discount_fn")):
            if not callable(fn):
                raise ValueError(f"`{arg}` should be a callable or the name of a default function. Received: {fn!r}")

    def get_config(self) -> dict:
        config = super().get_config()
        config.update({"gain_fn": _fn_config(self.gain_fn), "rank_discount_fn": _fn_config(self.rank_discount_fn)})
        return config


class DCG(_GradedMetric):
    """keras_rs.metrics.DCG: per list sum_{r <= k} w_r gain(y_r) discount(r) over the list weight, averaged with
    the list weights of get_list_weights on the gains."""
    _kind = "dcg"


class NDCG(_GradedMetric):
    """keras_rs.metrics.NDCG: DCG over the DCG of the order w * gain(y) descending, 0 when that is 0."""
    _kind = "ndcg"


class MeanAveragePrecision(RankingMetric):
    """keras_rs.metrics.MeanAveragePrecision: per list sum_{r <= k} P@r w_r rel_r / sum w rel, rel = (y >= 1)."""
    _kind = "map"


class MeanReciprocalRank(RankingMetric):
    """keras_rs.metrics.MeanReciprocalRank: per list 1 / rank of the first relevant item within the top k, else 0."""
    _kind = "mrr"


class PrecisionAtK(RankingMetric):
    """keras_rs.metrics.PrecisionAtK: relevant items within the top k over min(k, number of valid items)."""
    _kind = "precision"


class RecallAtK(RankingMetric):
    """keras_rs.metrics.RecallAtK: relevant items within the top k over all relevant items of the list."""
    _kind = "recall"


class RankingMetricGroup(_DrawCounter):
    """Several ranking metrics updated from one launch and one sort of each list.

    Members must agree on `shuffle_ties` and `seed` (and, among DCG / NDCG members, on `gain_fn` and
    `rank_discount_fn`), otherwise ValueError; with seed=None the group breaks ties with its first member's drawn
    seed.  The group numbers its updates with a counter of its own; a member's state after a group update is
    bit-identical to its state after updating it alone at the same draw number."""

    def __init__(self, metrics):
        metrics = list(metrics)
        if not 1 <= len(metrics) <= metric_ops.MAX_SPECS:
            raise ValueError(f"RankingMetricGroup takes 1 to {metric_ops.MAX_SPECS} metrics. Received: {len(metrics)}.")
        for m in metrics:
            if not isinstance(m, RankingMetric):
                raise ValueError(f"RankingMetricGroup takes RankingMetric objects. Received: {m!r}")
        first = metrics[0]
        for m in metrics[1:]:
            if m.shuffle_ties != first.shuffle_ties or m.seed != first.seed:
                raise ValueError("The metrics of a RankingMetricGroup share one sort and should agree on "
                                 f"`shuffle_ties` and `seed`. Received: {first.name} with ({first.shuffle_ties}, "
                                 f"{first.seed}) and {m.name} with ({m.shuffle_ties}, {m.seed}).")
        graded = [m for m in metrics if isinstance(m, _GradedMetric)]
        for m in graded[1:]:
            if m.gain_fn is not graded[0].gain_fn or m.rank_discount_fn is not graded[0].rank_discount_fn:
                raise ValueError("The DCG / NDCG metrics of a RankingMetricGroup should agree on `gain_fn` and "
                                 "`rank_discount_fn`.")
        self.metrics = metrics

    def update_state(self, y_true, y_pred, sample_weight=None) -> None:
        first = self.metrics[0]
        _update(self.metrics, first.shuffle_ties, first._seed_value, self, y_true, y_pred, sample_weight)

    def result(self) -> dict:
        return {m.name: m.result() for m in self.metrics}

    def reset_state(self) -> None:
        for m in self.metrics:
            m.reset_state()

    def __call__(self, y_true, y_pred, sample_weight=None) -> dict:
        self.update_state(y_true, y_pred, sample_weight)
        return self.result()


__all__ = ["DCG", "MeanAveragePrecision", "MeanReciprocalRank", "NDCG", "PrecisionAtK", "RankingMetric",
           "RankingMetricGroup", "RecallAtK", "default_gain_fn", "default_rank_discount_fn"]
