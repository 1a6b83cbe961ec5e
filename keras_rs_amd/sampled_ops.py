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


# ---- K30: the shared-negative sampled softmax (csrc/sampled_softmax.hip) -------------------------------------------------
def softmax_workspace_bytes(t: int, g: int, n: int, d: int, emb_dtype: torch.dtype) -> int:
    code = L.BF16 if emb_dtype == torch.bfloat16 else L.F32
    return int(L.lib().krs_sampled_softmax_workspace_bytes(t, g, n, d, code))


def softmax_last_route() -> L.SampledSoftmaxRoute:
    route = L.SampledSoftmaxRoute()
    L.lib().krs_sampled_softmax_last_route(C.byref(route))
    return route


def sampled_softmax(emb: torch.Tensor, table: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor,
                    weight: torch.Tensor | None = None, pos_logq: torch.Tensor | None = None,
                    neg_logq: torch.Tensor | None = None, remove_hits: bool = True,
                    err_flag: torch.Tensor | None = None, out=None, workspace: torch.Tensor | None = None):
    """(loss 0-d, lse [T], gpos [T], demb [T, d] in emb's dtype, dneg [G, N, d]) -- fp32 unless said -- of emb [T, d]
    against table [V, d] (each fp32 or bf16, rows a stride apart), pos [T] and the shared negatives neg [G, N] of one
    integer type (T = G Lg, token t in group t // Lg), weight [T] fp32 or None, pos_logq [T] and neg_logq [G, N] fp32
    (both or neither).  The gradients are those of the loss at unit upstream (include/krs.h, K30).  err_flag: device
    int32[1] the kernels OR FLAG_ID_OUT_OF_RANGE into.  out / workspace: the five outputs and the workspace to write
    into instead of fresh ones (the tests hand in poisoned buffers)."""
    e = L.rowmajor(emb, "sampled_softmax emb")
    tab = L.rowmajor(table, "sampled_softmax table")
    t, d = e.shape
    dev = e.device
    if tab.shape[1] != d:
        raise L.KrsError(f"sampled_softmax: table width {tab.shape[1]} differs from the embedding's {d}")
    L.require_device(pos, "sampled_softmax positive")
    L.require_device(neg, "sampled_softmax negative")
    if neg.dim() != 2 or neg.dtype != pos.dtype or pos.numel() != t:
        raise L.KrsError(f"sampled_softmax: {t} tokens, positive {tuple(pos.shape)} {pos.dtype}, negative "
                         f"{tuple(neg.shape)} {neg.dtype}: wants [T] and [G, N] of one integer type")
    pos, neg = pos.contiguous().reshape(-1), neg.contiguous()
    g, n = neg.shape

    def f32(x, shape, what):
        if x is None:
            return None
        L.require_device(x, what)
        if x.dtype != torch.float32 or tuple(x.shape) != shape:
            raise L.KrsError(f"{what} must be float32 {shape}, got {tuple(x.shape)} {x.dtype}")
        return x.contiguous()

    weight = f32(weight, (t,), "sampled_softmax weight")
    pos_logq, neg_logq = f32(pos_logq, (t,), "sampled_softmax pos_logq"), f32(neg_logq, (g, n), "sampled_softmax neg_logq")
    if out is None:
        make = torch.zeros if t == 0 else torch.empty       # (no token: the kernels write nothing)
        out = (make((), dtype=torch.float32, device=dev), make((t,), dtype=torch.float32, device=dev),
               make((t,), dtype=torch.float32, device=dev), make((t, d), dtype=e.dtype, device=dev),
               make((g, n, d), dtype=torch.float32, device=dev))
    loss, lse, gpos, demb, dneg = out
    size = softmax_workspace_bytes(t, g, n, d, e.dtype)
    ws = torch.empty(max(1, size), dtype=torch.uint8, device=dev) if workspace is None else workspace
    rc = L.lib().krs_sampled_softmax_fwd_bwd(
        L.ptr(e), e.stride(0) if t > 1 else d, L.fdtype(e), L.ptr(tab), tab.stride(0) if tab.shape[0] > 1 else d,
        L.fdtype(tab), tab.shape[0], L.ptr(pos), L.ptr(neg), L.itype(pos), L.ptr(weight), L.ptr(pos_logq), L.ptr(neg_logq),
        t, g, n, d, int(bool(remove_hits)), L.ptr(loss), L.ptr(lse), L.ptr(gpos), L.ptr(demb), d, L.ptr(dneg),
        L.ptr(err_flag), L.ptr(ws), ws.numel(), L.stream_ptr())
    L.check(rc, "krs_sampled_softmax_fwd_bwd")
    return loss, lse, gpos, demb, dneg


class SampledSoftmaxFn(torch.autograd.Function):
    """loss = SampledSoftmaxFn.apply(bags, emb [T, d], pos [T], neg [G, N], weight, pos_logq, neg_logq, remove_hits,
    err_flag, table).

    The forward is ONE call of krs_sampled_softmax_fwd_bwd that leaves loss, gpos, demb and dneg.  The backward scales
    them by the incoming scalar in place and, for the table, runs K2 twice into one sum: the T positive lookups with
    weights gpos and bag gradient emb, the G N negative lookups with bag gradient dneg; ids shared within `neg`,
    across groups or between the two are summed there.  The limits are SampledItemBceFn's: one backward (a second
    raises RuntimeError), and no capturing stream -- K29's captured replay faulted, its cause was not found, and this
    backward takes the same K2 plan path, so a capture is refused, not tried."""

    @staticmethod
    def forward(ctx, bags, emb, pos, neg, weight, pos_logq, neg_logq, remove_hits, err_flag, table):
        if torch.cuda.is_current_stream_capturing():
            raise L.KrsError("SampledSoftmaxFn cannot be captured into a HIP graph: run the loss and its backward eagerly "
                             "(a replayed capture of K29's, which shares this backward's plan path, faulted; see DESIGN.md, K30)")
        loss, _, gpos, demb, dneg = sampled_softmax(emb, table, pos, neg, weight, pos_logq, neg_logq, remove_hits, err_flag)
        need_table = ctx.needs_input_grad[9]
        ctx.bags, ctx.gpos, ctx.demb, ctx.dneg, ctx.spent = bags, gpos, demb, dneg, False
        ctx.emb_shape, ctx.table_dtype = emb.shape, table.dtype
        ctx.save_for_backward(*((emb, pos.reshape(-1), neg.reshape(-1)) if need_table else (None, None, None)))
        return loss

    @staticmethod
    def backward(ctx, up):
        if ctx.spent:
            raise RuntimeError("SampledSoftmaxFn: a second backward through the same loss; its gradient buffers were "
                               "scaled in place by the first")
        ctx.spent = True
        emb, pos, neg = ctx.saved_tensors
        up = up.to(torch.float32)
        d_emb = ctx.demb.mul_(up).reshape(ctx.emb_shape) if ctx.needs_input_grad[1] else None
        d_table = None
        if pos is not None:
            t, gn = pos.numel(), neg.numel()
            d_table = torch.zeros(ctx.bags.tables[0].shape, dtype=torch.float32, device=pos.device)
            if t:
                ws = ctx.bags.plan_backward(pos, t, hots=(1,), global_order=False)
                ctx.bags.backward_dense(ws, L.rowmajor(emb, "sampled_softmax emb"), t, t, hots=(1,), weights=ctx.gpos.mul_(up),
                                        out=[d_table])
                part = torch.zeros_like(d_table)
                ws = ctx.bags.plan_backward(neg, gn, hots=(1,), global_order=False, ws=ws)
                ctx.bags.backward_dense(ws, ctx.dneg.reshape(gn, -1).mul_(up), gn, gn, hots=(1,), out=[part])
                d_table += part
            d_table = d_table.to(ctx.table_dtype)
        return None, d_emb, None, None, None, None, None, None, None, d_table
