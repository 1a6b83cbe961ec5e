"""K19: fused multi-head self-attention over token sequences (csrc/seq_attention.hip; the arithmetic is fixed in
include/krs.h).  The score matrix, the probabilities and the dropout mask are never stored: the backward recomputes
them from q, k, v, the saved output and one log-sum-exp per (b, h, row)."""

import math

import torch

from . import _lib as L

FAST, GENERIC = 1, 2          # krs_seq_attn_last_route's kernels (KRS_SEQ_ATTN_*)


def seq_attn_workspace_bytes(b: int, h: int, l: int, dh: int, dtype: torch.dtype = torch.bfloat16) -> int:
    dt = L.BF16 if dtype == torch.bfloat16 else L.F32
    return int(L.lib().krs_seq_attn_workspace_bytes(b, h, l, dh, dt))


def last_route() -> tuple:
    """(kernel, dpad) of the last forward or backward call."""
    import ctypes as C

    kernel, dpad = C.c_int(0), C.c_int(0)
    L.lib().krs_seq_attn_last_route(C.addressof(kernel), C.addressof(dpad))
    return kernel.value, dpad.value


def _tokens(t: torch.Tensor) -> torch.Tensor:
    """t [B, L, H, Dh] itself when the kernels can walk it (token (b, i) at row b * L + i of one stride, head h at column
    h * Dh: a column slice of a packed projection output qualifies), else a contiguous copy."""
    b, l, h, dh = t.shape
    if t.numel() == 0:
        return t.contiguous()
    ok = (dh == 1 or t.stride(3) == 1) and (h == 1 or t.stride(2) == dh) and t.stride(1) >= h * dh \
        and (b == 1 or t.stride(0) == l * t.stride(1))
    if l == 1 and b > 1:
        ok = ok and t.stride(0) >= h * dh
    return t if ok else t.contiguous()


def _ld(t: torch.Tensor) -> int:
    b, l, h, dh = t.shape
    if l > 1:
        return t.stride(1)
    return t.stride(0) if b > 1 else h * dh


def _check(q, k, v, key_valid, dropout_p, draw, what):
    for name, t in (("q", q), ("k", k), ("v", v)):
        L.require_device(t, f"{what}: {name}")
        if t.dim() != 4:
            raise L.KrsError(f"{what}: {name} must be [B, L, H, Dh], got shape {tuple(t.shape)}")
    if not (q.shape == k.shape == v.shape):
        raise L.KrsError(f"{what}: q {tuple(q.shape)}, k {tuple(k.shape)} and v {tuple(v.shape)} must have one shape "
                         "(self-attention: equal lengths and head widths)")
    if not (q.dtype == k.dtype == v.dtype):
        raise L.KrsError(f"{what}: q, k, v must share a dtype, got {q.dtype}, {k.dtype}, {v.dtype}")
    L.fdtype(q)
    if key_valid is not None:
        if key_valid.shape != q.shape[:2] or key_valid.device != q.device:
            raise L.KrsError(f"{what}: key_valid must be [B, L] = {tuple(q.shape[:2])} on {q.device}, got "
                             f"{tuple(key_valid.shape)} on {key_valid.device}")
    if not 0.0 <= dropout_p < 1.0:
        raise L.KrsError(f"{what}: dropout_p {dropout_p} outside [0, 1)")
    if draw is not None and (draw.dtype != torch.int64 or draw.device != q.device or draw.numel() != 1):
        raise L.KrsError(f"{what}: draw must be one int64 on {q.device}")


def _args(q, k, v, key_valid, causal, scale, dropout_p, seed, used):
    b, l, h, dh = q.shape
    return (L.ptr(q), _ld(q), L.ptr(k), _ld(k), L.ptr(v), _ld(v), L.fdtype(q), b, h, l, dh, L.ptr(key_valid),
            int(bool(causal)), float(scale), float(dropout_p), int(seed) & (2 ** 64 - 1), L.ptr(used))


class _SeqAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, key_valid, causal, scale, dropout_p, seed, draw):
        q, k, v = _tokens(q), _tokens(k), _tokens(v)
        b, l, h, dh = q.shape
        used = None
        if dropout_p > 0.0:
            # the draw number this call uses, kept for the backward; the caller's counter moves on, on the device
            used = draw.clone() if draw is not None else torch.zeros(1, dtype=torch.int64, device=q.device)
        out = torch.empty((b, l, h, dh), dtype=q.dtype, device=q.device)
        lse = torch.empty((b, h, l), dtype=torch.float32, device=q.device)
        rc = L.lib().krs_seq_attn_fwd(*_args(q, k, v, key_valid, causal, scale, dropout_p, seed, used), L.ptr(out), h * dh,
                                      L.ptr(lse), None, 0, L.stream_ptr())
        L.check(rc, "krs_seq_attn_fwd")
        if dropout_p > 0.0 and draw is not None:
            draw.add_(1)
        ctx.save_for_backward(q, k, v, out, lse, key_valid, used)
        ctx.conf = (causal, scale, dropout_p, seed)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout, _dlse):
        q, k, v, out, lse, key_valid, used = ctx.saved_tensors
        causal, scale, dropout_p, seed = ctx.conf
        b, l, h, dh = q.shape
        want = ctx.needs_input_grad[:3]
        grads = [torch.empty((b, l, h, dh), dtype=q.dtype, device=q.device) if w else None for w in want]
        if q.numel() == 0 or not any(want):
            return (*grads, None, None, None, None, None, None)
        dout = _tokens(dout)
        size = seq_attn_workspace_bytes(b, h, l, dh, q.dtype)
        ws = torch.empty(max(1, size), dtype=torch.uint8, device=q.device)
        rc = L.lib().krs_seq_attn_bwd(*_args(q, k, v, key_valid, causal, scale, dropout_p, seed, used), L.ptr(out), h * dh,
                                      L.ptr(dout), _ld(dout), L.ptr(lse), L.ptr(grads[0]), h * dh, L.ptr(grads[1]),
                                      h * dh, L.ptr(grads[2]), h * dh, L.ptr(ws), size, L.stream_ptr())
        L.check(rc, "krs_seq_attn_bwd")
        return (*grads, None, None, None, None, None, None)


def seq_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, key_valid: torch.Tensor | None = None,
                  causal: bool = False, scale: float | None = None, dropout_p: float = 0.0, seed: int = 0,
                  draw: torch.Tensor | None = None, return_lse: bool = False):
    """Masked multi-head self-attention.  q, k, v: [B, L, H, Dh], float32 or bfloat16 (views into one packed projection
    output are read in place); key_valid: [B, L], truthy = a real token; scale defaults to 1 / sqrt(Dh).  Returns out
    [B, L, H, Dh] (and lse [B, H, L] fp32 with return_lse).  A query with no allowed key gives a zero row and takes no
    part in any gradient.  Dropout keeps element (b, h, i, j) by a hash of (seed, draw, b, h, i, j): `draw` is a device
    int64 of one element that this call reads and then advances by one on the device (None: draw number 0 every call).
    No host synchronisation; differentiable in q, k and v, any subset."""
    what = "seq_attention"
    _check(q, k, v, key_valid, dropout_p, draw, what)
    if key_valid is not None:
        key_valid = (key_valid != 0).to(torch.uint8).contiguous()
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[3])
    out, lse = _SeqAttention.apply(q, k, v, key_valid, bool(causal), float(scale), float(dropout_p), int(seed), draw)
    return (out, lse) if return_lse else out
