"""K24 on the host: krs_regression_fwd_bwd (csrc/regression.hip) behind a function, its autograd Function and the
input rules the regression losses and metrics share (layers/losses.py, layers/metrics.py).

One call reads the predictions once and leaves any of: the loss with its Keras reduction, the gradient to the
predictions, and the batch sums {sum w mse, sum w mae, sum w} the metric states add.  There is no CPU fallback."""

from __future__ import annotations

import ctypes as C

import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import losses as _reductions

KINDS = {"mse": L.REG_MSE, "mae": L.REG_MAE, "huber": L.REG_HUBER}
REDUCTION_CODES = {"none": L.REG_NONE, None: L.REG_NONE, "sum": L.REG_SUM,
                   "sum_over_batch_size": L.REG_SUM_OVER_BATCH_SIZE, "mean": L.REG_SUM_OVER_BATCH_SIZE,
                   "mean_with_sample_weight": L.REG_MEAN_WITH_SAMPLE_WEIGHT}


def workspace_bytes(b: int, c: int) -> int:
    return int(L.lib().krs_regression_workspace_bytes(b, c))


def last_route() -> L.RegressionRoute:
    route = L.RegressionRoute()
    L.lib().krs_regression_last_route(C.byref(route))
    return route


def standardize(y_true, y_pred, sample_weight, what: str):
    """(target [B, C], pred [B, C], weight [B] fp32 or None, the shape of the unreduced loss) after the shape rule:
    the ranks may differ by one when the longer shape ends in 1 (y_true [B] with y_pred [B, 1]); after that the shapes
    must be equal.  Rank-1 (and rank-0) inputs are one row, whose weight must be a scalar.  Every check is made before
    any device check."""
    y_pred = _reductions._tensor(y_pred)
    y_true = _reductions._tensor(y_true, y_pred.device)
    if y_true.dim() == y_pred.dim() + 1 and y_true.shape[-1] == 1:
        y_pred = y_pred.unsqueeze(-1)
    elif y_pred.dim() == y_true.dim() + 1 and y_pred.shape[-1] == 1:
        y_true = y_true.unsqueeze(-1)
    if tuple(y_true.shape) != tuple(y_pred.shape):
        raise ValueError(f"{what}: `y_true` and `y_pred` should have the same shape, up to one trailing axis of 1. "
                         f"Received: `y_true.shape` = {tuple(y_true.shape)}, `y_pred.shape` = {tuple(y_pred.shape)}.")
    if y_pred.dim() == 0:
        y_true, y_pred = y_true.reshape(1), y_pred.reshape(1)
    shape = tuple(y_pred.shape[:-1])
    c = y_pred.shape[-1]
    if c < 1:
        raise ValueError(f"{what}: the last axis of `y_pred` {tuple(y_pred.shape)} is empty")
    w = None
    if sample_weight is not None:
        if shape:
            w = _reductions._sample_weight(sample_weight, shape, y_pred.device)
        else:
            w = _reductions._tensor(sample_weight, y_pred.device).to(torch.float32)
            if w.dim() != 0:
                raise ValueError(f"`sample_weight` of shape {tuple(w.shape)} cannot be broadcast to the scalar "
                                 "loss of a single row: give a scalar.")
        w = w.detach().expand(shape).reshape(-1)
    if y_pred.dtype not in (torch.float32, torch.bfloat16):
        y_pred = y_pred.to(torch.float32)
    return y_true.detach().to(torch.float32).reshape(-1, c), y_pred.reshape(-1, c), w, shape


def regression(pred: torch.Tensor, target: torch.Tensor, weight: torch.Tensor | None, kind: str, delta: float = 1.0,
               reduction: str | None = "sum_over_batch_size", g: torch.Tensor | None = None, g_scale: float = 1.0,
               want_loss: bool = True, want_grad: bool = True, sums: torch.Tensor | None = None):
    """(loss | None, dpred | None) of pred [B, C] fp32 / bf16 against target [B, C] fp32 with weight [B] fp32 or None.
    loss is [B] under reduction "none" and a 0-d tensor otherwise; dpred has pred's dtype; `sums` ([3] fp32 on pred's
    device) is overwritten with the batch sums.  g [B] fp32 is the upstream gradient of reduction "none"."""
    if kind not in KINDS:
        raise ValueError(f"regression: kind {kind!r} is not one of {sorted(KINDS)}")
    if reduction not in REDUCTION_CODES:
        raise ValueError(f"Invalid value for argument `reduction`. Expected one of {_reductions.REDUCTIONS}. "
                         f"Received: reduction={reduction}")
    p = L.rowmajor(pred, "regression y_pred")
    y = L.rowmajor(target, "regression y_true")
    if y.dtype != torch.float32 or tuple(y.shape) != tuple(p.shape):
        raise L.KrsError(f"regression: y_true {tuple(y.shape)} {y.dtype} must be float32 of y_pred's shape "
                         f"{tuple(p.shape)}")
    b, c = p.shape
    dev = p.device
    for t, name, n in ((weight, "sample_weight", b), (g, "g", b), (sums, "sums", 3)):
        if t is not None:
            L.require_device(t, f"regression {name}")
            if t.dtype != torch.float32 or tuple(t.shape) != (n,):
                raise L.KrsError(f"regression: {name} must be {n} float32 values, got {tuple(t.shape)} {t.dtype}")
    w = None if weight is None else weight.contiguous()
    g = None if g is None else g.contiguous()
    if sums is not None and not sums.is_contiguous():
        raise L.KrsError("regression: sums must be contiguous")
    code = REDUCTION_CODES[reduction]
    loss = dp = None
    if want_loss:      # (no rows: the kernel writes nothing, and the loss of no rows is 0)
        loss = torch.zeros((b,) if code == L.REG_NONE else (), dtype=torch.float32, device=dev) if b == 0 else \
            torch.empty((b,) if code == L.REG_NONE else (), dtype=torch.float32, device=dev)
    if want_grad:
        dp = torch.empty((b, c), dtype=p.dtype, device=dev)
    if b == 0 and sums is not None:
        sums.zero_()
    size = workspace_bytes(b, c)
    ws = torch.empty(max(1, size), dtype=torch.uint8, device=dev)
    ldp = p.stride(0) if b > 1 else c
    ldy = y.stride(0) if b > 1 else c
    rc = L.lib().krs_regression_fwd_bwd(KINDS[kind], float(delta), code, L.ptr(p), ldp, L.fdtype(p), L.ptr(y), ldy,
                                        L.ptr(w), b, c, L.ptr(g), float(g_scale), L.ptr(loss), L.ptr(dp), c,
                                        L.ptr(sums), L.ptr(ws), size, L.stream_ptr())
    L.check(rc, "krs_regression_fwd_bwd")
    return loss, dp


class RegressionLossFn(torch.autograd.Function):
    """The regression loss of pred [B, C] with its Keras reduction, in SoftmaxCrossentropyFn's scheme: a scalar
    reduction takes loss and gradient (at unit upstream) from ONE call and the backward only scales that gradient by
    the incoming scalar; reduction "none" computes the losses alone and its backward is a gradient-only call with the
    incoming [B].  `sums` ([3] or None) receives the batch sums of the forward call.  target gets no gradient."""

    @staticmethod
    def forward(ctx, pred, target, weight, kind, delta, reduction, sums):
        reduction = "none" if reduction is None else reduction
        ctx.meta = (kind, delta, reduction)
        need = ctx.needs_input_grad[0]
        if reduction == "none":
            loss, _ = regression(pred, target, weight, kind, delta, reduction, want_grad=False, sums=sums)
            ctx.save_for_backward(pred, target, weight)
            return loss
        loss, dp = regression(pred, target, weight, kind, delta, reduction, want_grad=need, sums=sums)
        ctx.save_for_backward(dp)
        return loss

    @staticmethod
    def backward(ctx, up):
        kind, delta, reduction = ctx.meta
        if reduction != "none":
            (dp,) = ctx.saved_tensors
            return (dp.float() * up).to(dp.dtype), None, None, None, None, None, None
        pred, target, weight = ctx.saved_tensors
        _, dp = regression(pred, target, weight, kind, delta, reduction, g=up.to(torch.float32).reshape(-1),
                           want_loss=False)
        return dp, None, None, None, None, None, None
