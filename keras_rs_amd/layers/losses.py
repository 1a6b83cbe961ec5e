"""The loss of the DLRM step on MI355X: `keras.losses.BinaryCrossentropy()` as the reference's ml_perf example compiles
it (examples/ml_perf/main.py:201-210: probabilities in -- the top MLP ends in a sigmoid, model.py:105-163 --, mean over
the batch), forward and backward in ONE pass over the predictions (krs_bce_fwd_bwd, csrc/loss.hip); the softmax
crossentropies of the retrieval examples (K11); and the regression losses of the rating examples -- MeanSquaredError,
MeanAbsoluteError, Huber -- with every Keras reduction, sample weights and the regression metrics' update from one
pass over the predictions (K24, krs_regression_fwd_bwd, csrc/regression.hip); and the two sampled-item losses of the
sequence models: the binary cross-entropy over per-token negatives (K29, krs_sampled_bce_fwd_bwd, csrc/sampled_bce.hip)
and the softmax over shared negatives (K30, krs_sampled_softmax_fwd_bwd, csrc/sampled_softmax.hip)."""

from __future__ import annotations

import os

import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import losses as _reductions
from keras_rs_amd import regression_ops as _regression
from keras_rs_amd.autograd import BinaryCrossentropyFn, _switch
from keras_rs_amd.layers.embed_reduce import as_index_tensor
from keras_rs_amd.retrieval_ops import SoftmaxCrossentropyFn
from keras_rs_amd.sampled_ops import SampledItemBceFn, SampledSoftmaxFn


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


# ---- K29: the sampled-item binary cross-entropy of a sequence model ----------------------------------------------------
# 1: the fused kernel; 0: the stored torch composition (A/B).  The environment is read once, at import; the module
# global is what every call looks at, as with sequence.FUSE_NORM
FUSE_SAMPLED_BCE = _switch(os.environ.get("KRS_FUSE_SAMPLED_BCE", "1"))


def sampled_item_crossentropy_stored(embedding_layer, sequence_embedding, positive, negative, sample_weight=None):
    """The torch composition the fused loss replaces: two embedding lookups that store [B, L, d] and [B, L, N, d],
    fp32 copies of the three blocks, the [B, (1 + N) L] logits and the element-wise BCE with logits, weighted and
    divided by the sum of the weights (0 when that sum is 0)."""
    emb = sequence_embedding.float()
    b, length = positive.shape
    neg_ids = negative.reshape(b, length, -1)
    n = neg_ids.shape[2]
    pos = embedding_layer(positive).float()
    neg = embedding_layer(neg_ids.reshape(b, length * n)).float().reshape(b, length, n, -1)
    logits = torch.cat([(pos * emb).sum(-1), (neg * emb.unsqueeze(2)).sum(-1).reshape(b, length * n)], dim=1)
    labels = torch.cat([torch.ones_like(logits[:, :length]), torch.zeros_like(logits[:, length:])], dim=1)
    w = torch.ones((b, length), device=emb.device) if sample_weight is None else sample_weight.float()
    weight = torch.cat([w, w.repeat_interleave(n, dim=1)], dim=1)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels, reduction="none") * weight
    total = weight.sum()
    return torch.where(total > 0, loss.sum() / total.clamp_min(1e-30), torch.zeros_like(total))


class SampledItemCrossentropy:
    """The training loss of SASRec and its family: loss(embedding_layer, sequence_embedding [B, L, d], positive [B, L],
    negative [B, L] or [B, L, N], sample_weight=None | [B, L] float or bool) -> scalar.  Every token scores its positive
    item and its N sampled negatives by a dot product of its sequence embedding with the items' rows of
    `embedding_layer` (a layers.Embedding); the loss is keras' binary cross-entropy from logits (label 1 for the
    positive, 0 for a negative) weighted per token and divided by (1 + N) * sum(sample_weight), 0 when that is 0.

    One kernel call (K29, csrc/sampled_bce.hip) gathers every row once and leaves the loss, the logit gradients and the
    gradient to the sequence embedding; the table's gradient is one K2 call over the (1 + N) B L lookups.  An id outside
    the table raises IndexError (one host read of the kernel's error word per call).  A quantized embedding layer,
    d > 512 and KRS_FUSE_SAMPLED_BCE=0 take sampled_item_crossentropy_stored; N > 64 raises ValueError.

    Three things to know.  The fused loss reads the layer's STORED rows (fp32 under "mixed_bfloat16"), where the stored
    composition's lookups round every gathered row to the compute dtype first: under a mixed policy the two differ by
    that rounding of the rows (2^-8 relative per element), the fused loss being the closer to exact arithmetic.  Its
    gradient buffers are scaled in place by the upstream scalar, so it can be differentiated once: a second backward
    (retain_graph=True) raises RuntimeError.  And it refuses a capturing stream (KrsError): a step that contains it
    runs eagerly."""

    def __init__(self, name: str | None = None):
        self.name = name or "sampled_item_crossentropy"

    def __call__(self, embedding_layer, sequence_embedding, positive, negative, sample_weight=None) -> torch.Tensor:
        emb = sequence_embedding
        if emb.dim() != 3 or tuple(positive.shape) != tuple(emb.shape[:2]):
            raise ValueError("`sequence_embedding` should be [B, L, d] and `positive` [B, L]. Received: "
                             f"{tuple(emb.shape)} and {tuple(positive.shape)}.")
        b, length, d = emb.shape
        if negative.dim() not in (2, 3) or tuple(negative.shape[:2]) != (b, length):
            raise ValueError(f"`negative` should be [B, L] or [B, L, N]. Received: {tuple(negative.shape)}.")
        if sample_weight is not None and tuple(sample_weight.shape) != (b, length):
            raise ValueError(f"`sample_weight` should be [B, L]. Received: {tuple(sample_weight.shape)}.")
        if not embedding_layer.built:
            embedding_layer.build()
        n = 1 if negative.dim() == 2 else negative.shape[2]
        if n > L.SBCE_MAX_NEGATIVES:
            raise ValueError(f"`negative` holds {n} items per position; at most {L.SBCE_MAX_NEGATIVES} are supported.")
        if not FUSE_SAMPLED_BCE or embedding_layer.quantization_mode or d > L.SBCE_MAX_DIM:
            return sampled_item_crossentropy_stored(embedding_layer, emb, positive, negative, sample_weight)
        table = embedding_layer.embeddings
        if table.shape[1] != d:
            raise ValueError(f"`sequence_embedding` is {d} wide, the embedding layer's rows {table.shape[1]}.")
        if emb.dtype not in (torch.float32, torch.bfloat16):
            emb = emb.to(torch.float32)
        tokens = b * length
        pos = as_index_tensor(positive, table.device).reshape(tokens)
        neg = as_index_tensor(negative, table.device).to(pos.dtype).reshape(tokens, n) if n else None
        w = None if sample_weight is None else sample_weight.detach().to(torch.float32).reshape(tokens)
        err = torch.zeros(1, dtype=torch.int32, device=table.device)
        loss = SampledItemBceFn.apply(embedding_layer._fused("sum"), emb.reshape(tokens, d), pos, neg, w, err, table)
        if int(err.item()) & L.FLAG_ID_OUT_OF_RANGE:
            raise IndexError("embedding id out of range for its table (ids are never clamped)")
        return loss

    def get_config(self) -> dict:
        return {"name": self.name}

    @classmethod
    def from_config(cls, config: dict):
        return cls(**config)


# ---- K30: the sampled softmax over negatives a sequence, or the batch, shares -------------------------------------------
FUSE_SAMPLED_SOFTMAX = _switch(os.environ.get("KRS_FUSE_SAMPLED_SOFTMAX", "1"))


def sampled_softmax_crossentropy_stored(embedding_layer, sequence_embedding, positive, negative, sample_weight=None,
                                        positive_log_q=None, negative_log_q=None, remove_accidental_hits=True):
    """The torch composition the fused loss replaces, and its A/B baseline: two embedding lookups, the [B, L, 1 + N]
    fp32 logits (a batched product with the shared rows), the log-q correction, the accidental hits masked to -inf, and
    a log-softmax at the positive, weighted and divided by the sum of the weights (0 when that sum is 0).  Autograd
    keeps the logits and their softmax."""
    emb = sequence_embedding.float()
    b, length, _ = emb.shape
    neg_ids = negative.reshape(1, -1) if negative.dim() == 1 else negative
    pos = embedding_layer(positive).float()
    neg = embedding_layer(neg_ids).float()                                   # [B, N, d] or [1, N, d]
    x0 = (pos * emb).sum(-1, keepdim=True)
    xn = torch.matmul(emb, neg.transpose(1, 2))                              # [B, L, N]
    if positive_log_q is not None:
        x0 = x0 - positive_log_q.float().unsqueeze(-1)
        xn = xn - negative_log_q.float().reshape(neg_ids.shape[0], 1, -1)
    if remove_accidental_hits:
        xn = xn.masked_fill(neg_ids.unsqueeze(1) == positive.unsqueeze(-1), float("-inf"))
    per_token = torch.logsumexp(torch.cat([x0, xn], dim=-1), dim=-1) - x0.squeeze(-1)
    w = torch.ones((b, length), device=emb.device) if sample_weight is None else sample_weight.float()
    total = w.sum()
    return torch.where(total > 0, (per_token * w).sum() / total.clamp_min(1e-30), torch.zeros_like(total))


class SampledSoftmaxCrossentropy:
    """The sampled softmax sequence models are mostly trained with: loss(embedding_layer, sequence_embedding [B, L, d],
    positive [B, L], negative [B, N] (per sequence) or [N] (one set for the batch), sample_weight=None | [B, L],
    positive_log_q=None | [B, L], negative_log_q=None | negative's shape) -> scalar.  Every token takes the softmax
    cross-entropy of its positive item among it and the N shared negatives, scored by dot products with the rows of
    `embedding_layer`; the log q (log of the sampling probability) are subtracted from the logits when given, both or
    neither.  With remove_accidental_hits a negative that equals a token's positive is left out of that token's softmax.
    Tokens are weighted and the sum divided by sum(sample_weight), 0 when that is 0.

    K30 (csrc/sampled_softmax.hip): the scores are an MFMA product per group whose streamed side is gathered from the
    table, never stored; one call leaves the loss, the gradient to the sequence embedding and to the N shared rows, and
    the table's gradient is two K2 calls.  bf16 sequence embeddings up to d = 128 take the MFMA route -- the table may
    be fp32, as under "mixed_bfloat16", its rows are rounded to bf16 on the way in --; fp32, or d up to 512, the fp32
    route.  A quantized layer, d > 512 and KRS_FUSE_SAMPLED_SOFTMAX=0 take sampled_softmax_crossentropy_stored.
    N > 4096 raises ValueError, an id outside the table IndexError.  As SampledItemCrossentropy, the loss can be
    differentiated once and refuses a capturing stream (KrsError)."""

    def __init__(self, remove_accidental_hits: bool = True, name: str | None = None):
        self.remove_accidental_hits = bool(remove_accidental_hits)
        self.name = name or "sampled_softmax_crossentropy"

    def __call__(self, embedding_layer, sequence_embedding, positive, negative, sample_weight=None,
                 positive_log_q=None, negative_log_q=None) -> torch.Tensor:
        emb = sequence_embedding
        if emb.dim() != 3 or tuple(positive.shape) != tuple(emb.shape[:2]):
            raise ValueError("`sequence_embedding` should be [B, L, d] and `positive` [B, L]. Received: "
                             f"{tuple(emb.shape)} and {tuple(positive.shape)}.")
        b, length, d = emb.shape
        if negative.dim() not in (1, 2) or (negative.dim() == 2 and negative.shape[0] != b) or negative.shape[-1] < 1:
            raise ValueError(f"`negative` should be [B, N] or [N] with N >= 1. Received: {tuple(negative.shape)}.")
        n = negative.shape[-1]
        if n > L.SSM_MAX_NEGATIVES:
            raise ValueError(f"`negative` holds {n} items; at most {L.SSM_MAX_NEGATIVES} are supported.")
        if (positive_log_q is None) != (negative_log_q is None):
            raise ValueError("`positive_log_q` and `negative_log_q` are given both or neither.")
        for name, x, shape in (("sample_weight", sample_weight, (b, length)), ("positive_log_q", positive_log_q, (b, length)),
                               ("negative_log_q", negative_log_q, tuple(negative.shape))):
            if x is not None and tuple(x.shape) != shape:
                raise ValueError(f"`{name}` should be {shape}. Received: {tuple(x.shape)}.")
        if not embedding_layer.built:
            embedding_layer.build()
        if not FUSE_SAMPLED_SOFTMAX or embedding_layer.quantization_mode or d > L.SSM_MAX_DIM:
            return sampled_softmax_crossentropy_stored(embedding_layer, emb, positive, negative, sample_weight,
                                                       positive_log_q, negative_log_q, self.remove_accidental_hits)
        table = embedding_layer.embeddings
        if table.shape[1] != d:
            raise ValueError(f"`sequence_embedding` is {d} wide, the embedding layer's rows {table.shape[1]}.")
        if emb.dtype not in (torch.float32, torch.bfloat16):
            emb = emb.to(torch.float32)
        tokens = b * length
        pos = as_index_tensor(positive, table.device).reshape(tokens)
        neg = as_index_tensor(negative, table.device).to(pos.dtype).reshape(-1, n)
        flat = lambda x, shape: None if x is None else x.detach().to(torch.float32).reshape(shape)      # noqa: E731
        err = torch.zeros(1, dtype=torch.int32, device=table.device)
        loss = SampledSoftmaxFn.apply(embedding_layer._fused("sum"), emb.reshape(tokens, d), pos, neg,
                                      flat(sample_weight, (tokens,)), flat(positive_log_q, (tokens,)),
                                      flat(negative_log_q, tuple(neg.shape)), self.remove_accidental_hits, err, table)
        if int(err.item()) & L.FLAG_ID_OUT_OF_RANGE:
            raise IndexError("embedding id out of range for its table (ids are never clamped)")
        return loss

    def get_config(self) -> dict:
        return {"name": self.name, "remove_accidental_hits": self.remove_accidental_hits}

    @classmethod
    def from_config(cls, config: dict):
        return cls(**config)
