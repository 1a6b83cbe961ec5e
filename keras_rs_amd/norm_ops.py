"""K22: fused residual add + dropout + layer norm over the last axis (csrc/layer_norm.hip; the arithmetic is fixed in
include/krs.h).  No dropout mask is stored: the backward recomputes it from (seed, draw, position)."""

import ctypes as C

import torch

from . import _lib as L

VEC, ELEM = 1, 2              # krs_ln_last_route's kernels (KRS_LN_*)
MAX_D = 4096                  # the row lives in a wave's registers


def ln_workspace_bytes(n: int, d: int) -> int:
    return int(L.lib().krs_ln_workspace_bytes(n, d))


def last_route() -> tuple:
    """(kernel, lanes_per_row, vec) of the last forward or backward call."""
    kernel, lanes, vec = C.c_int(0), C.c_int(0), C.c_int(0)
    L.lib().krs_ln_last_route(C.addressof(kernel), C.addressof(lanes), C.addressof(vec))
    return kernel.value, lanes.value, vec.value


def supported(x: torch.Tensor) -> bool:
    """Whether K22 takes x: a device tensor of float32 or bfloat16 with a last axis of at most 4096."""
    return x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and x.dim() >= 1 and 1 <= x.shape[-1] <= MAX_D


def _rows(t: torch.Tensor, d: int, what: str) -> torch.Tensor:
    return L.rowmajor(t.reshape(-1, d), what, "rows of the last axis")


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


class _ResidualLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, gamma, beta, epsilon, dropout_p, seed, draw, norm, return_sum, train):
        shape, d = x.shape, x.shape[-1]
        x2 = _rows(x, d, "residual_layer_norm: x")
        r2 = None if residual is None else _rows(residual, d, "residual_layer_norm: residual")
        n = x2.shape[0]
        gamma = None if gamma is None else gamma.contiguous()
        beta = None if beta is None else beta.contiguous()
        plain = r2 is None and dropout_p == 0.0            # s is x itself
        used = None
        if dropout_p > 0.0:
            # the draw number this call uses, kept for the backward; the caller's counter moves on, on the device
            used = draw.clone() if draw is not None else torch.zeros(1, dtype=torch.int64, device=x.device)
        y = torch.empty((n, d), dtype=x.dtype, device=x.device) if norm else None
        s = None
        if not norm or return_sum or (train and not plain):
            s = torch.empty((n, d), dtype=x.dtype, device=x.device)
        mean = rstd = None
        if norm and train:
            mean = torch.empty(n, dtype=torch.float32, device=x.device)
            rstd = torch.empty(n, dtype=torch.float32, device=x.device)
        rc = L.lib().krs_ln_fwd(L.ptr(x2), _ld(x2), L.ptr(r2), 0 if r2 is None else _ld(r2), L.ptr(gamma), L.ptr(beta),
                                L.fdtype(x), n, d, float(epsilon), float(dropout_p), int(seed) & (2 ** 64 - 1),
                                L.ptr(used), L.ptr(y), d, L.ptr(s), d, L.ptr(mean), L.ptr(rstd), L.stream_ptr())
        L.check(rc, "krs_ln_fwd")
        if dropout_p > 0.0 and draw is not None:
            draw.add_(1)
        ctx.save_for_backward((x2 if plain else s) if (norm and train) else None, gamma, mean, rstd, used)
        ctx.conf = (shape, n, d, x.dtype, x.device, dropout_p, seed, residual is not None)
        ctx.set_materialize_grads(False)
        y_out = None if y is None else y.view(shape)
        s_out = s.view(shape) if (s is not None and (return_sum or not norm)) else None
        return y_out, s_out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, dsum):
        s, gamma, mean, rstd, used = ctx.saved_tensors
        shape, n, d, dtype, dev, dropout_p, seed, has_res = ctx.conf
        want_x, want_res, want_gamma, want_beta = ctx.needs_input_grad[:4]
        want_res = want_res and has_res
        none7 = (None,) * 7
        wzeros = lambda want: torch.zeros(d, dtype=torch.float32, device=dev) if want else None

        def run(dy2, ds2, dx, dres, dgamma, dbeta):
            wg = dgamma is not None or dbeta is not None
            size = ln_workspace_bytes(n, d) if wg else 0
            ws = torch.empty(max(1, size), dtype=torch.uint8, device=dev) if wg else None
            rc = L.lib().krs_ln_bwd(None if dy2 is None else L.ptr(s), d if (s is None or dy2 is None) else _ld(s),
                                    L.ptr(dy2), 0 if dy2 is None else _ld(dy2), L.ptr(ds2), 0 if ds2 is None else _ld(ds2),
                                    L.ptr(gamma), L.ptr(mean), L.ptr(rstd), L.F32 if dtype == torch.float32 else L.BF16,
                                    n, d, float(dropout_p), int(seed) & (2 ** 64 - 1), L.ptr(used), L.ptr(dx), d,
                                    L.ptr(dres), d, L.ptr(dgamma), L.ptr(dbeta), L.ptr(ws), size, L.stream_ptr())
            L.check(rc, "krs_ln_bwd")

        ds2 = None if dsum is None else _rows(dsum.to(dtype), d, "residual_layer_norm: dsum")
        if dy is None:
            # only the sum reached the loss (always so in the add form): gamma and beta took no part, the residual takes
            # dsum as it is, and so does x unless the dropout mask has to be applied
            if dsum is None:
                zx = torch.zeros(shape, dtype=dtype, device=dev)
                return (zx if want_x else None, zx if want_res else None, wzeros(want_gamma), wzeros(want_beta), *none7)
            gx = None
            if want_x and dropout_p == 0.0:
                gx = dsum
            elif want_x:
                gx = torch.empty((n, d), dtype=dtype, device=dev)
                if n > 0:
                    run(None, ds2, gx, None, None, None)
                gx = gx.view(shape)
            return (gx, dsum if want_res else None, wzeros(want_gamma), wzeros(want_beta), *none7)
        dy2 = _rows(dy.to(dtype), d, "residual_layer_norm: dy")
        one = dropout_p == 0.0                   # dx and dres are one tensor, written once
        dx = torch.empty((n, d), dtype=dtype, device=dev) if (want_x or (one and want_res)) else None
        dres = torch.empty((n, d), dtype=dtype, device=dev) if (want_res and not one) else None
        dgamma = torch.empty(d, dtype=torch.float32, device=dev) if want_gamma else None
        dbeta = torch.empty(d, dtype=torch.float32, device=dev) if want_beta else None
        if n == 0:
            dgamma, dbeta = wzeros(want_gamma), wzeros(want_beta)
        elif not all(g is None for g in (dx, dres, dgamma, dbeta)):
            run(dy2, ds2, dx, dres, dgamma, dbeta)
        gx = dx.view(shape) if want_x else None
        gres = (dx if one else dres).view(shape) if want_res else None
        return (gx, gres, dgamma, dbeta, *none7)


def residual_layer_norm(x: torch.Tensor, residual: torch.Tensor | None = None, gamma: torch.Tensor | None = None,
                        beta: torch.Tensor | None = None, *, epsilon: float, dropout_p: float = 0.0, seed: int = 0,
                        draw: torch.Tensor | None = None, norm: bool = True, return_sum: bool = False):
    """s = residual + dropout(x); y = layer_norm(s) * gamma + beta over the last axis, in one kernel (include/krs.h, K22).
    x, residual: [..., d], float32 or bfloat16, one dtype and shape; gamma, beta: float32 [d] or None (1 and 0).
    Returns y; (y, s) with return_sum (s is the next residual of a pre-norm block); with norm=False only s = residual +
    dropout(x) and no statistics are taken (gamma and beta must be None).  Dropout keeps element (row, j) by a hash of
    (seed, draw, row, j): `draw` is a device int64 of one element that this call reads and then advances by one on the
    device (None: draw number 0 every call).  No host synchronisation; differentiable in x, residual, gamma and beta, any
    subset, and a gradient that is not needed is not computed."""
    what = "residual_layer_norm"
    L.require_device(x, f"{what}: x")
    if x.dim() < 1 or x.shape[-1] < 1:
        raise L.KrsError(f"{what}: x needs a last axis of at least 1, got shape {tuple(x.shape)}")
    L.fdtype(x)
    d = x.shape[-1]
    if d > MAX_D:
        raise L.KrsError(f"{what}: last axis {d} > {MAX_D} (the row lives in a wave's registers)")
    if residual is not None and (residual.shape != x.shape or residual.dtype != x.dtype or residual.device != x.device):
        raise L.KrsError(f"{what}: residual must match x ({tuple(x.shape)}, {x.dtype}, {x.device}), got "
                         f"{tuple(residual.shape)}, {residual.dtype}, {residual.device}")
    for name, w in (("gamma", gamma), ("beta", beta)):
        if w is None:
            continue
        if not norm:
            raise L.KrsError(f"{what}: norm=False takes no {name}")
        if w.shape != (d,) or w.dtype != torch.float32 or w.device != x.device:
            raise L.KrsError(f"{what}: {name} must be float32 [{d}] on {x.device}, got {w.dtype} {tuple(w.shape)} on "
                             f"{w.device}")
    if not 0.0 <= dropout_p < 1.0:
        raise L.KrsError(f"{what}: dropout_p {dropout_p} outside [0, 1)")
    if not epsilon >= 0.0:
        raise L.KrsError(f"{what}: epsilon {epsilon} is negative")
    if draw is not None and (draw.dtype != torch.int64 or draw.device != x.device or draw.numel() != 1):
        raise L.KrsError(f"{what}: draw must be one int64 on {x.device}")
    if not norm and return_sum:
        raise L.KrsError(f"{what}: norm=False already returns the sum")
    train = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, residual, gamma, beta))
    y, s = _ResidualLayerNorm.apply(x, residual, gamma, beta, float(epsilon), float(dropout_p), int(seed), draw, bool(norm),
                                    bool(return_sum), train)
    if not norm:
        return s
    return (y, s) if return_sum else y
