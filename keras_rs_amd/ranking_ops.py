"""Host side of K9: thin torch wrappers over krs_pairwise_loss and krs_listmle_loss (include/krs.h).

Both run on the current stream and never wait for the device, so forward and backward can be captured in a HIP
graph.  Each returns (unreduced loss or None, dL/dlogits or None).
"""

from __future__ import annotations

import torch

from keras_rs_amd import _lib as L

MAX_LIST = L.MAX_LIST
PAIRWISE_KINDS = {"hinge": 0, "logistic": 1, "soft_zero_one": 2, "mse": 3}   # krs_rank_loss


def _operands(logits: torch.Tensor, labels: torch.Tensor, mask: torch.Tensor | None, what: str):
    logits = L.rowmajor(logits, what, "[batch, list] logits")
    b, n = logits.shape
    ld = logits.stride(0) if b > 1 else n
    y = labels.to(device=logits.device, dtype=torch.float32).contiguous()
    m = None if mask is None else mask.to(device=logits.device, dtype=torch.bool).contiguous().view(torch.uint8)
    for t, name in ((y, "labels"), (m, "mask")):
        if t is not None and tuple(t.shape) != (b, n):
            raise L.KrsError(f"{what}: {name} shape {tuple(t.shape)} differs from logits {(b, n)}")
    return logits, ld, y, m


def _weights(g: torch.Tensor | None, shape, device) -> torch.Tensor | None:
    if g is None:
        return None
    return g.to(device=device, dtype=torch.float32).expand(shape).contiguous()


def pairwise_loss(kind: str, logits: torch.Tensor, labels: torch.Tensor, mask: torch.Tensor | None = None, *,
                  inv_temperature: float = 1.0, g: torch.Tensor | None = None, g_scale: float = 1.0,
                  want_loss: bool = True, want_grad: bool = True):
    """Per-item pairwise loss [B, L] fp32 and d(sum g * loss)/dlogits [B, L] in logits' dtype (g = g_scale * g,
    g broadcast to [B, L]).  kind: one of PAIRWISE_KINDS."""
    x, ld, y, m = _operands(logits, labels, mask, "pairwise_loss")
    b, n = x.shape
    gw = _weights(g, (b, n), x.device)
    loss = torch.empty((b, n), dtype=torch.float32, device=x.device) if want_loss else None
    dx = torch.empty((b, n), dtype=x.dtype, device=x.device) if want_grad else None
    rc = L.lib().krs_pairwise_loss(PAIRWISE_KINDS[kind], L.ptr(x), ld, L.fdtype(x), L.ptr(y), L.ptr(m), L.ptr(gw),
                                   g_scale, inv_temperature, b, n, L.ptr(loss), L.ptr(dx), L.stream_ptr())
    L.check(rc, "krs_pairwise_loss")
    return loss, dx


def listmle_loss(logits: torch.Tensor, labels: torch.Tensor, mask: torch.Tensor | None = None, *,
                 inv_temperature: float = 1.0, g: torch.Tensor | None = None, g_scale: float = 1.0,
                 want_loss: bool = True, want_grad: bool = True):
    """Per-list ListMLE loss [B] fp32 and d(sum g * loss)/dlogits [B, L] in logits' dtype (g = g_scale * g, g
    broadcast to [B])."""
    x, ld, y, m = _operands(logits, labels, mask, "listmle_loss")
    b, n = x.shape
    gw = _weights(g, (b,), x.device)
    loss = torch.empty((b,), dtype=torch.float32, device=x.device) if want_loss else None
    dx = torch.empty((b, n), dtype=x.dtype, device=x.device) if want_grad else None
    rc = L.lib().krs_listmle_loss(L.ptr(x), ld, L.fdtype(x), L.ptr(y), L.ptr(m), L.ptr(gw),
                                  g_scale, inv_temperature, b, n,
                                  L.ptr(loss), L.ptr(dx), L.stream_ptr())
    L.check(rc, "krs_listmle_loss")
    return loss, dx


def ranking_loss(kind: str, logits, labels, mask=None, **kw):
    """pairwise_loss for a PAIRWISE_KINDS key, listmle_loss for "listmle"."""
    if kind == "listmle":
        return listmle_loss(logits, labels, mask, **kw)
    return pairwise_loss(kind, logits, labels, mask, **kw)


class RankingLossFn(torch.autograd.Function):
    """A keras_rs.losses ranking loss with its Keras reduction (keras_rs_amd/losses.py).

    Scalar reductions: the forward knows every item's share g = weight / divisor of the result and takes loss and
    gradient from ONE launch; the backward only scales that gradient by the incoming scalar.  reduction "none": the
    forward computes the losses alone and the backward runs a second launch with g = upstream * weight."""

    @staticmethod
    def forward(ctx, y_pred, labels, mask, weight, kind, inv_t, reduction):
        ctx.meta = (kind, inv_t, reduction)
        want_grad = ctx.needs_input_grad[0]
        if reduction == "none":
            v, _ = ranking_loss(kind, y_pred, labels, mask, inv_temperature=inv_t, want_grad=False)
            ctx.save_for_backward(y_pred, labels, mask, weight)
            return v if weight is None else v * weight
        shape = (y_pred.shape[0],) if kind == "listmle" else tuple(y_pred.shape)
        numel = shape[0] * (shape[1] if len(shape) > 1 else 1)
        g, scale = weight, 1.0
        if reduction == "mean_with_sample_weight" and weight is not None:
            div = weight.expand(shape).sum()
            g = torch.where(div != 0, weight / div, torch.zeros_like(weight))   # divide_no_nan
        elif reduction != "sum":
            scale = 1.0 / numel if numel else 0.0
        v, dx = ranking_loss(kind, y_pred, labels, mask, inv_temperature=inv_t, g=g, g_scale=scale,
                             want_grad=want_grad)
        ctx.save_for_backward(dx)
        return (v.sum() if g is None else (v * g).sum()) * scale

    @staticmethod
    def backward(ctx, up):
        kind, inv_t, reduction = ctx.meta
        if reduction != "none":
            (dx,) = ctx.saved_tensors
            return dx * up.to(dx.dtype), None, None, None, None, None, None
        y_pred, labels, mask, weight = ctx.saved_tensors
        g = up.to(torch.float32)
        if weight is not None:
            g = g * weight
        _, dx = ranking_loss(kind, y_pred, labels, mask, inv_temperature=inv_t, g=g, want_loss=False)
        return dx, None, None, None, None, None, None
