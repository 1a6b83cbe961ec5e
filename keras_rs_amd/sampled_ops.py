"""K29 on the host: krs_sampled_bce_fwd_bwd (csrc/sampled_bce.hip) behind a function and its autograd Function.

One call gathers the positive and the N sampled negative rows of every token once and leaves the sample-weighted BCE
with logits, the logit gradients glog [T, 1 + N] and the gradient to the sequence embedding.  The table gradient is K2
(FusedBags.plan_backward + backward_dense) over one bag (pos, neg ..) per token, with glog as the per-lookup weights
and the sequence embedding as the bag gradient.  There is no CPU fallback."""

from __future__ import annotations

import ctypes as C

import torch

from keras_rs_amd import _lib as L


def workspace_bytes(t: int) -> int:
    return int(L.lib().krs_sampled_bce_workspace_bytes(t))


def last_route() -> L.SampledBceRoute:
    route = L.SampledBceRoute()
    L.lib().krs_sampled_bce_last_route(C.byref(route))
    return route


def plan_route(emb: torch.Tensor, table: torch.Tensor, n: int, weighted: bool, want_demb: bool = True) -> L.SampledBceRoute:
    """What krs_sampled_bce_plan_route answers for sampled_bce(emb, table, ..) with n negatives (the planner reads the
    operands' addresses and strides only; the outputs sampled_bce allocates start on 16 bytes)."""
    route = L.SampledBceRoute()
    t, d = emb.shape
    rc = L.lib().krs_sampled_bce_plan_route(L.ptr(emb), emb.stride(0) if t > 1 else d, L.fdtype(emb), L.ptr(table),
                                            table.stride(0) if table.shape[0] > 1 else d, L.fdtype(table), table.shape[0],
                                            16, 16 if n else None, L.I32, 16 if weighted else None, t, d, n, 16,
                                            16 if want_demb else None, d, C.byref(route))
    L.check(rc, "krs_sampled_bce_plan_route")
    return route


def sampled_bce(emb: torch.Tensor, table: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor | None,
                weight: torch.Tensor | None = None, want_demb: bool = True, err_flag: torch.Tensor | None = None):
    """(loss 0-d fp32, glog [T, 1 + N] fp32, demb [T, d] in emb's dtype | None) of emb [T, d] against table [V, d] (each
    fp32 or bf16, rows a stride apart), pos [T] and neg [T, N] (None: N = 0) of one integer type, weight [T] fp32 or
    None.  The gradients are those of the loss at unit upstream.  err_flag: device int32[1] the kernel ORs
    FLAG_ID_OUT_OF_RANGE into."""
    e = L.rowmajor(emb, "sampled_bce emb")
    tab = L.rowmajor(table, "sampled_bce table")
    t, d = e.shape
    dev = e.device
    if tab.shape[1] != d:
        raise L.KrsError(f"sampled_bce: table width {tab.shape[1]} differs from the embedding's {d}")
    L.require_device(pos, "sampled_bce positive")
    pos = pos.contiguous().reshape(-1)
    n = 0
    if neg is not None:
        L.require_device(neg, "sampled_bce negative")
        neg = neg.contiguous().reshape(t, -1)
        n = neg.shape[1]
        if neg.dtype != pos.dtype:
            raise L.KrsError(f"sampled_bce: positive ids are {pos.dtype}, negative ids {neg.dtype}")
    if pos.numel() != t:
        raise L.KrsError(f"sampled_bce: {pos.numel()} positive ids for {t} tokens")
    if weight is not None:
        L.require_device(weight, "sampled_bce weight")
        if weight.dtype != torch.float32 or tuple(weight.shape) != (t,):
            raise L.KrsError(f"sampled_bce: weight must be {t} float32 values, got {tuple(weight.shape)} {weight.dtype}")
        weight = weight.contiguous()
    make = torch.zeros if t == 0 else torch.empty       # (no token: the kernel writes nothing, the loss is 0)
    loss = make((), dtype=torch.float32, device=dev)
    glog = make((t, 1 + n), dtype=torch.float32, device=dev)
    demb = make((t, d), dtype=e.dtype, device=dev) if want_demb else None
    size = workspace_bytes(t)
    ws = torch.empty(max(1, size), dtype=torch.uint8, device=dev)
    rc = L.lib().krs_sampled_bce_fwd_bwd(L.ptr(e), e.stride(0) if t > 1 else d, L.fdtype(e), L.ptr(tab),
                                         tab.stride(0) if tab.shape[0] > 1 else d, L.fdtype(tab), tab.shape[0], L.ptr(pos),
                                         L.ptr(neg) if n else None, L.itype(pos), L.ptr(weight), t, d, n, L.ptr(loss),
                                         L.ptr(glog), L.ptr(demb), d, L.ptr(err_flag), L.ptr(ws), size, L.stream_ptr())
    L.check(rc, "krs_sampled_bce_fwd_bwd")
    return loss, glog, demb


class SampledItemBceFn(torch.autograd.Function):
    """loss = SampledItemBceFn.apply(bags, emb [T, d], pos [T], neg [T, N] | None, weight [T] | None, err_flag, table).

    The forward is ONE kernel call that leaves loss, glog and demb.  The backward scales demb and glog by the incoming
    scalar with in-place torch multiplies (no host read) and, for the table, runs one K2 plan and one dense apply over
    the (1 + N) T lookups with hots = (1 + N,), weights = glog and grad = emb.  `bags` is the embedding layer's
    FusedBags over `table` (passed as well so that autograd tracks it, as EmbedBagFn does).

    Two limits.  The gradient buffers are scaled in place, so the loss can be differentiated ONCE: a second backward
    (retain_graph=True) raises RuntimeError.  And the loss refuses a stream that is capturing: a captured loss + backward
    faulted when it was replayed and the cause was not found, so a graph is not offered."""

    @staticmethod
    def forward(ctx, bags, emb, pos, neg, weight, err_flag, table):
        if torch.cuda.is_current_stream_capturing():
            raise L.KrsError("SampledItemBceFn cannot be captured into a HIP graph: run the loss and its backward eagerly "
                             "(a replayed capture of them faulted; see DESIGN.md, K29)")
        need_emb, need_table = ctx.needs_input_grad[1], ctx.needs_input_grad[6]
        loss, glog, demb = sampled_bce(emb, table, pos, neg, weight, want_demb=need_emb, err_flag=err_flag)
        ctx.bags, ctx.glog, ctx.demb, ctx.spent = bags, glog, demb, False
        ctx.emb_shape, ctx.table_dtype = emb.shape, table.dtype
        ids = None
        if need_table:          # one bag per token: (pos, neg ..), the layout glog has
            ids = pos.reshape(-1, 1) if neg is None else torch.cat([pos.reshape(-1, 1), neg.reshape(pos.numel(), -1)], 1)
        ctx.save_for_backward(emb if need_table else None, ids)
        return loss

    @staticmethod
    def backward(ctx, up):
        if ctx.spent:
            raise RuntimeError("SampledItemBceFn: a second backward through the same loss; its gradient buffers were "
                               "scaled in place by the first")
        ctx.spent = True
        emb, ids = ctx.saved_tensors
        up = up.to(torch.float32)
        d_emb = d_table = None
        if ctx.demb is not None:
            d_emb = ctx.demb.mul_(up).reshape(ctx.emb_shape)
        if ids is not None:
            t, hot = ids.shape
            if t == 0:
                d_table = torch.zeros(ctx.bags.tables[0].shape, dtype=ctx.table_dtype, device=ids.device)
            else:
                weights = ctx.glog.mul_(up).reshape(-1)
                ws = ctx.bags.plan_backward(ids.reshape(-1), t, hots=(hot,), global_order=False)
                d_table = ctx.bags.backward_dense(ws, L.rowmajor(emb, "sampled_bce emb"), t, ids.numel(), hots=(hot,),
                                                  weights=weights)[0].to(ctx.table_dtype)
        return None, d_emb, None, None, None, None, d_table
