"""K20: the recurrence of a GRU layer, all steps in one launch per sweep (csrc/gru.hip; the arithmetic is fixed in
include/krs.h).  The input projection xz = x . kernel + bias[0] is the caller's (layers.GRU runs it as a Dense
product); the weight gradients of the recurrent kernel and bias are one krs_gemm and one krs_colsum on what the
backward sweep wrote."""

import ctypes as C

import torch

from . import _lib as L

FAST, GENERIC = 1, 2          # krs_gru_last_route's kernels (KRS_GRU_*)


def gru_reserve_bytes(b: int, l: int, u: int, dtype: torch.dtype = torch.bfloat16) -> int:
    dt = L.BF16 if dtype == torch.bfloat16 else L.F32
    return int(L.lib().krs_gru_reserve_bytes(b, l, u, dt))


def last_route() -> tuple:
    """(kernel, upad) of the last forward or backward call."""
    kernel, upad = C.c_int(0), C.c_int(0)
    L.lib().krs_gru_last_route(C.addressof(kernel), C.addressof(upad))
    return kernel.value, upad.value


def _ld(t: torch.Tensor) -> int | None:
    """The one row stride that walks t [B, L, W] as tokens (token (b, i) at row b * L + i), or None when there is none."""
    b, l, w = t.shape
    if t.stride(2) != 1:
        return None
    ld = t.stride(1) if l > 1 else (t.stride(0) if b > 1 else w)
    if ld < w or (l > 1 and b > 1 and t.stride(0) != l * ld):
        return None
    return ld


def _tokens(t: torch.Tensor) -> torch.Tensor:
    """t itself when the kernels can walk it in place (a column slice of a wider buffer qualifies), else a contiguous
    copy."""
    return t if t.numel() and _ld(t) is not None else t.contiguous()


class _GRU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xz, rk, rb, valid, h0, want_seq):
        xz = _tokens(xz)
        b, l, u3 = xz.shape
        u = u3 // 3
        dt = xz.dtype
        rkc = rk.to(dt).contiguous()
        rbc = None if rb is None else rb.detach().float().contiguous()
        h0c = None if h0 is None else h0.to(dt).contiguous()
        train = any(ctx.needs_input_grad)
        hs = torch.empty((b, l, u), dtype=dt, device=xz.device) if (want_seq or train) else None
        h_last = torch.empty((b, u), dtype=dt, device=xz.device)
        reserve = torch.empty((b, l, 4 * u), dtype=dt, device=xz.device) if train else None
        if b == 0 or l == 0:       # (nothing to walk: the state is the initial state)
            h_last = torch.zeros((b, u), dtype=dt, device=xz.device) if h0c is None else h0c.clone()
        else:
            rc = L.lib().krs_gru_fwd(L.ptr(xz), _ld(xz), L.ptr(rkc), L.ptr(rbc), L.ptr(valid), L.ptr(h0c), L.fdtype(xz),
                                     b, l, u, L.ptr(hs), L.ptr(h_last), L.ptr(reserve), L.stream_ptr())
            L.check(rc, "krs_gru_fwd")
        ctx.save_for_backward(rkc, valid, h0c, hs, reserve)
        ctx.dims = (b, l, u)
        ctx.dtypes = (rk.dtype, None if rb is None else rb.dtype, None if h0 is None else h0.dtype)
        ctx.set_materialize_grads(False)
        if hs is None:
            hs = torch.empty((b, 0, u), dtype=dt, device=xz.device)
            ctx.mark_non_differentiable(hs)
        return hs, h_last

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dhs, dh_last):
        from . import dense_ops as D

        rkc, valid, h0c, hs, reserve = ctx.saved_tensors
        b, l, u = ctx.dims
        rk_dt, rb_dt, h0_dt = ctx.dtypes
        want_xz, want_rk, want_rb, _, want_h0 = ctx.needs_input_grad[:5]
        dt, dev = rkc.dtype, rkc.device
        if b == 0 or l == 0:
            z = lambda shape, d: torch.zeros(shape, dtype=d, device=dev)  # noqa: E731
            dh0 = None
            if want_h0:
                dh0 = z((b, u), h0_dt) if dh_last is None else dh_last.to(h0_dt)
            return (z((b, l, 3 * u), dt) if want_xz else None, z((u, 3 * u), rk_dt) if want_rk else None,
                    z((3 * u,), rb_dt) if want_rb else None, None, dh0, None)
        dhs = None if dhs is None else dhs.to(dt).contiguous()
        dh_last = None if dh_last is None else dh_last.to(dt).contiguous()
        dxz = torch.empty((b, l, 3 * u), dtype=dt, device=dev)
        da = torch.empty((b, l, 3 * u), dtype=dt, device=dev)
        hprev = torch.empty((b, l, u), dtype=dt, device=dev) if want_rk else None
        dh0 = torch.empty((b, u), dtype=dt, device=dev) if want_h0 else None
        rc = L.lib().krs_gru_bwd(L.ptr(rkc), L.ptr(valid), L.ptr(h0c), L.ptr(hs), L.ptr(reserve), L.ptr(dhs),
                                 L.ptr(dh_last), L.fdtype(rkc), b, l, u, L.ptr(dxz), L.ptr(da), L.ptr(hprev), L.ptr(dh0),
                                 L.stream_ptr())
        L.check(rc, "krs_gru_bwd")
        drk = drb = None
        if want_rk:      # sum_t h_{t-1}^T da_t as ONE weight-gradient product over all b * l tokens
            drk, _ = D.gemm(hprev.view(b * l, u), da.view(b * l, 3 * u), a_is_km=True, out_dtype=torch.float32)
            drk = drk.to(rk_dt)
        if want_rb:
            drb = D.colsum(da.view(b * l, 3 * u)).to(rb_dt)
        return (dxz if want_xz else None, drk, drb, None, None if dh0 is None else dh0.to(h0_dt), None)


def gru(xz: torch.Tensor, recurrent_kernel: torch.Tensor, recurrent_bias: torch.Tensor | None, *,
        mask: torch.Tensor | None = None, initial_state: torch.Tensor | None = None, return_sequences: bool = False):
    """The recurrence of keras.layers.GRU (reset_after=True, tanh, sigmoid) over projected inputs.  xz: [B, L, 3U] =
    x . kernel + bias[0], float32 or bfloat16, gates in Keras' order z, r, h (a view with a row stride is read in place);
    recurrent_kernel [U, 3U]; recurrent_bias [3U] or None; mask [B, L], truthy = a real step; initial_state [B, U] or
    None (zeros).  Returns (outputs, state): outputs is the sequence output [B, L, U] with return_sequences, else the
    last step's output [B, U]; state is the final state [B, U].  A masked step carries the state and repeats the previous
    output, which is zeros before the first valid step.  No host synchronisation; differentiable in xz,
    recurrent_kernel, recurrent_bias and initial_state, any subset."""
    what = "gru"
    L.require_device(xz, f"{what}: xz")
    if xz.dim() != 3 or xz.shape[2] % 3:
        raise L.KrsError(f"{what}: xz must be [B, L, 3U], got shape {tuple(xz.shape)}")
    L.fdtype(xz)
    b, l, u3 = xz.shape
    u = u3 // 3
    if tuple(recurrent_kernel.shape) != (u, u3) or recurrent_kernel.device != xz.device:
        raise L.KrsError(f"{what}: recurrent_kernel must be [U, 3U] = {(u, u3)} on {xz.device}, got "
                         f"{tuple(recurrent_kernel.shape)} on {recurrent_kernel.device}")
    if recurrent_bias is not None and (tuple(recurrent_bias.shape) != (u3,) or recurrent_bias.device != xz.device):
        raise L.KrsError(f"{what}: recurrent_bias must be [3U] = {(u3,)} on {xz.device}, got "
                         f"{tuple(recurrent_bias.shape)} on {recurrent_bias.device}")
    if mask is not None:
        if tuple(mask.shape) != (b, l) or mask.device != xz.device:
            raise L.KrsError(f"{what}: mask must be [B, L] = {(b, l)} on {xz.device}, got {tuple(mask.shape)} on "
                             f"{mask.device}")
        mask = (mask != 0).to(torch.uint8).contiguous()
    if initial_state is not None and (tuple(initial_state.shape) != (b, u) or initial_state.device != xz.device):
        raise L.KrsError(f"{what}: initial_state must be [B, U] = {(b, u)} on {xz.device}, got "
                         f"{tuple(initial_state.shape)} on {initial_state.device}")
    hs, state = _GRU.apply(xz, recurrent_kernel, recurrent_bias, mask, initial_state, bool(return_sequences))
    if return_sequences:
        return hs, state
    if mask is None:
        return state, state
    # the last step's OUTPUT: the state, except for a sequence with no valid step at all (zeros)
    return state * mask.any(dim=1, keepdim=True).to(state.dtype), state
