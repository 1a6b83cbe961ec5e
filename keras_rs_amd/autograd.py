"""torch.autograd.Function wrappers: one per op of the hot path, each calling the
HIP kernels through the C ABI (embedding_ops / dense_ops).  Gradients follow
SURVEY.md section 8 rows a4 (embedding), a9 (FeatureCross) and a11 (DotInteraction).
The relays and records the dense backward's hand-offs pass around are in relays.py, the opt-in second stream for the
cross layers' weight gradients in wgrad_side.py; the switches of both stay here and are read here, at call time.
"""

from __future__ import annotations

import os
import weakref
from typing import NamedTuple

import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import dense_ops as D
from keras_rs_amd import wgrad_side
from keras_rs_amd.relays import (CrossLower, DenseActRelay, DenseLower, Dx0Relay, Handoff, SlabGradRelay,  # noqa: F401
                                 graph_task)
from keras_rs_amd.wgrad_side import wgrad_stream_sync  # noqa: F401  (dp.GradAllReduce and callers know it under this name)


_SIDE_STREAMS: dict = {}


def _side_stream(device) -> "torch.cuda.Stream":
    key = str(device)
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return st


def _switch(value: str) -> bool:
    """An on / off switch from its environment string, "0" or "1"."""
    return bool(int(value))


# The cross layers' weight-gradient GEMMs on a second stream: opt-in, see wgrad_side.py (`set_wgrad_side_stream(True)` or
# KRS_WGRAD_SIDE=1); taken from WGRAD_SIDE_MIN_ROWS rows on.
WGRAD_SIDE_STREAM = _switch(os.environ.get("KRS_WGRAD_SIDE", "0"))
WGRAD_SIDE_MIN_ROWS = 32768
# Round 4: dx = dh U^T + g of a layer IS dL/dy of the layer below it in the stack, whose elementwise backward starts
# by re-reading it.  krs_gemm_cross_bwd does that pass in the product's epilogue (one 453 MB stream less per layer at C3,
# and the other streams at the epilogue's rate): environment KRS_FUSE_CROSS_BWD=0 switches it off (A/B).
FUSE_CROSS_BWD = _switch(os.environ.get("KRS_FUSE_CROSS_BWD", "1"))
# ... and the TOP layer's own term of dL/dx0 is computed in that epilogue too (it writes dz only): KRS_FUSE_TOP_DX0=0 for A/B
FUSE_TOP_DX0 = _switch(os.environ.get("KRS_FUSE_TOP_DX0", "1"))
# development switch: 0 = every Dense layer runs its own activation backward (krs_dense_act_bwd), as before round 6
FUSE_DENSE_BWD = _switch(os.environ.get("KRS_FUSE_DENSE_BWD", "1"))


def set_wgrad_side_stream(on: bool) -> bool:
    """Switch the second stream for the cross layers' weight gradients on or off (wgrad_side.py); returns the old value."""
    global WGRAD_SIDE_STREAM
    old, WGRAD_SIDE_STREAM = WGRAD_SIDE_STREAM, bool(on)
    return old


def _release_plan_ws(bags_ref, owns) -> None:
    """The plan workspace kept on a FusedBags is free again (EmbedBagFusedFn: after its backward, or when the graph
    that borrowed it is dropped without one -- otherwise every later step would allocate a fresh workspace)."""
    if not owns[0]:
        return
    owns[0] = False
    bags = bags_ref()
    if bags is not None:
        bags._plan_ws_busy = False


def _split_columns(out: torch.Tensor, n: int, dim: int, lead: int = 0):
    """Per-feature [B, dim] column views of the fused [B, lead + n*dim] lookup output."""
    return tuple(out[:, lead + i * dim:lead + (i + 1) * dim] for i in range(n))


def _sum_slab_and_feature_grads(g_slab, gs, lead, batch, n, dim, dtype, device):
    """Gradient of the fused lookup output [B, n*dim] from the gradient of the slab (its columns
    lead..) and of the per-feature views; either side may be absent."""
    gv = _gather_feature_grads(gs, batch, dim, dtype, device) if any(g is not None for g in gs) else None
    if g_slab is None:
        return gv if gv is not None else torch.zeros((batch, n * dim), dtype=dtype, device=device)
    g_s = g_slab[:, lead:lead + n * dim]
    return g_s if gv is None else g_s + gv


def _gather_feature_grads(grads, batch: int, dim: int, dtype, device):
    """The per-feature output gradients as ONE [B, n*dim] matrix for K2.  When autograd hands
    back consecutive column slices of a single buffer (the gradient of a concat), that buffer is
    used in place (zero copies); otherwise the pieces are concatenated once."""
    n = len(grads)
    if all(g is not None for g in grads):
        g0 = grads[0]
        es = g0.element_size()
        ok = g0.dim() == 2 and g0.stride(1) == 1
        for i, g in enumerate(grads):
            ok = ok and g.dtype == g0.dtype and g.stride() == g0.stride() and \
                g.untyped_storage().data_ptr() == g0.untyped_storage().data_ptr() and \
                g.data_ptr() - g0.data_ptr() == i * dim * es
        if ok and g0.stride(0) >= n * dim:
            return torch.as_strided(g0, (batch, n * dim), (g0.stride(0), 1), g0.storage_offset())
    parts = [g if g is not None else torch.zeros((batch, dim), dtype=dtype, device=device) for g in grads]
    return torch.cat(parts, dim=1)


def _fusable_below(up, a, x_dtype, task) -> bool:
    """May the product `a @ Bt^T` run the elementwise backward of the cross layer behind relay `up` in its epilogue?"""
    low = up.lower if up is not None else None
    return not (low is None or task == -1 or not FUSE_CROSS_BWD or low.diag_scale != 0.0 or a.dtype != torch.bfloat16
                or x_dtype != a.dtype       # (the product is handed to autograd as it is: a cast would be a different tensor)
                or low.x0c.dtype != a.dtype or (up.buf is not None and up.task == task))


def _dense_fusable_below(rel, dz, x_dtype, task) -> bool:
    """May the product `dz @ K^T` run the activation backward of the Dense layer behind relay `rel` in its epilogue?"""
    if rel is None or rel.lower is None or not FUSE_DENSE_BWD or task == -1 or x_dtype != dz.dtype:
        return False
    if rel.lower.act == L.ACT_NONE and not rel.lower.has_bias:
        return False            # (nothing to do below: a plain product)
    if rel.fused is not None and rel.fused.task == task:
        return False            # (another consumer of that output already did it in this pass)
    out = rel.out_ref() if rel.out_ref is not None else None
    # (the output keeps its .grad: the launches of the unfused pass, so that every gradient of the step matches that pass
    #  bit for bit, bias gradients included -- .grad itself would be the same dL/dy either way)
    return out is None or not out.retains_grad


class _CrossMeta(NamedTuple):
    diag_scale: float
    act: int
    x_is_x0: bool
    low_rank: bool
    has_bias: bool
    x0_dtype: torch.dtype
    x_dtype: torch.dtype
    down_dtype: torch.dtype | None
    kernel_dtype: torch.dtype


def _take_handed_down(rin, x0c, task):
    """Empties the relay a consumer of y may have filled and returns what it left during THIS backward pass:
    (incoming, extra, handoff) -- dL/dx0 of the layers above as a buffer this layer can accumulate into, or (`extra`) as
    one it can only add; the Handoff of a consumer that ran this layer's elementwise backward (not yet checked)."""
    if rin is None:
        return None, None, None
    handoff, rin.fused = rin.fused, None
    incoming, extra = None, None
    if rin.buf is not None:
        if rin.task == task and task != -1:
            if rin.buf.dtype == x0c.dtype and rin.buf.shape == x0c.shape and rin.buf.is_contiguous():
                incoming = rin.buf
            else:
                extra = rin.buf
        rin.buf = None
    return incoming, extra, handoff


def _cross_elementwise(ctx, saved, g, task, incoming, extra, handoff):
    """The elementwise part of a cross layer's backward in one of four forms.  Returns (dz, dx0, dxd, dbias, defer_dx0);
    defer_dx0: no dL/dx0 exists yet, this layer's term g * u joins it inside its data-gradient product (u_upper)."""
    x0c, xc, _, u, _, _ = saved
    m = ctx.meta
    same, diag, act = m.x_is_x0, m.diag_scale, m.act
    # (in both uses of is_gradient below g has been through .to(x0c.dtype).contiguous() and G is a fresh contiguous
    #  matrix of that dtype: the stride and dtype it compares add nothing to pointer, shape and version here)
    if handoff is not None and handoff.deferred:
        # deferred: the consumer (a Dense layer) ran this layer's elementwise backward but left its term of dL/dx0 to
        # THIS layer's data-gradient product (u_upper).  Anything that is not the plain case -- another consumer's
        # buffer, a summed gradient, the layer below no longer fusable -- redoes this layer from g in the forms below.
        if not (incoming is None and extra is None and handoff.is_gradient(g, task)
                and _fusable_below(ctx.relay_up, g, m.x_dtype, task)):
            handoff = None
    elif handoff is not None and (incoming is None or handoff.task != task):
        handoff = None
    if handoff is not None and handoff.deferred:
        return handoff.dz, None, None, handoff.dbias, True
    if handoff is not None:
        # The consumer of y ran this layer's elementwise backward inside its data-gradient product
        # (krs_gemm_cross_bwd): `incoming` already holds this layer's term, dz and dbias are done.  That is only
        # right when its G is ALL of dL/dy -- the very tensor autograd hands over, untouched.  If y had another
        # consumer the engine summed their gradients (a new tensor, or in place: the version moves): the difference
        # goes through the elementwise kernel (linear in g), dz and dbias are redone.
        if handoff.is_gradient(g, task):
            return handoff.dz, incoming, (incoming if same else None), handoff.dbias, False
        delta = (g.float() - handoff.g.float()).to(g.dtype)
        _, dx0, _, _ = D.cross_epilogue_bwd(delta, u, x0c, xc, diag, act=act, want_du=False, want_dxd=False,
                                            want_dbias=False, fold_direct=same, dx0_into=incoming)
        dz, _, _, dbias = D.cross_epilogue_bwd(g, u, x0c, xc, diag, act=act, want_dxd=False,
                                               want_dbias=m.has_bias, want_dx0=False)
        return dz, dx0, (dx0 if same else None), dbias, False
    if (incoming is None and extra is None and not same and m.low_rank and not diag and FUSE_TOP_DX0
            and _fusable_below(ctx.relay_up, g, m.x_dtype, task)):
        # The TOP layer of a stack (nothing above it left a dL/dx0) whose data-gradient product is going to run the
        # layer below's elementwise backward: its own term g * u is computed THERE (g is that product's residual, already
        # in registers), so this pass writes dz only -- three [B, d] streams instead of five, and no matrix for dL/dx0 is
        # written here and read back there.
        dz, _, dxd, dbias = D.cross_epilogue_bwd(g, u if act != L.ACT_NONE else None, x0c, xc, diag, act=act,
                                                 want_dxd=False, want_dbias=m.has_bias, want_dx0=False)
        return dz, None, dxd, dbias, True
    # x is x0 (the first layer of a stack): both halves of dL/dx0 go through one buffer, which
    # the data-gradient GEMM then takes as its residual -- no separate add.
    dz, dx0, dxd, dbias = D.cross_epilogue_bwd(g, u, x0c, xc, diag, act=act, want_dxd=bool(diag) and not same,
                                               want_dbias=m.has_bias, fold_direct=same, dx0_into=incoming)
    return dz, dx0, dxd, dbias, False


def _dx_product(ctx, dh, dc, direct, dx0, x0c, task, u_own=None):
    """dx = dh U^T + direct.  When x was produced by a cross layer on the same x0 (ctx.relay_up) whose elementwise
    backward can ride in this product's epilogue, it does: that layer's dz / dbias and its term of dL/dx0 (added into
    this layer's dx0 buffer) are left on its relay.  Returns (dx, dx0).
    dx0 None + u_own (the TOP layer of a stack, see _cross_elementwise): this layer wrote no dL/dx0 of its own -- it chose
    that because the layer below is fusable -- and its term direct * u_own starts the matrix inside the fused epilogue."""
    up = ctx.relay_up
    if dx0 is not None and (not _fusable_below(up, dh, ctx.meta.x_dtype, task) or not dx0.is_contiguous()
                            or dx0.dtype != dh.dtype):
        dx, _ = D.gemm(dh, dc, b_is_nk=True, r=direct, beta=1.0)
        return dx, dx0
    low = up.lower
    dx, dz_low, dx0, db_low = D.gemm_cross_bwd(dh, dc, direct, x0c, low.u, act=low.act, dx0_into=dx0,
                                               want_dbias=low.has_bias, fold_direct=low.x_is_x0, u_upper=u_own)
    up.fused = Handoff(dx, dx._version, dz_low, db_low, task)
    return dx, dx0


def _cross_products(ctx, saved, dz, direct, dx0, u_own, task):
    """The data- and weight-gradient products of a cross layer.  Returns (dx, dx0, dK, dU | None)."""
    x0c, xc, h, _, dc, kc = saved
    m = ctx.meta
    side = wgrad_side.may_use(ctx.uses, task, dz, enabled=m.low_rank and WGRAD_SIDE_STREAM, min_rows=WGRAD_SIDE_MIN_ROWS)
    if not m.low_rank:
        dk, _ = D.gemm(xc, dz, a_is_km=True, out_dtype=torch.float32)      # dK = x^T dz     [d, d]
        dx, _ = D.gemm(dz, kc, b_is_nk=True, r=direct, beta=1.0)           # dx = dz K^T + direct
        return dx, dx0, dk, None
    if side:
        # Data-gradient path first; the two weight gradients (off the critical path: only the optimizer reads them)
        # go to the second stream, which starts when dx is done
        dh, _ = D.gemm(dz, kc, b_is_nk=True)                               # dh = dz K^T     [B, p]
        dx, dx0 = _dx_product(ctx, dh, dc, direct, dx0, x0c, task, u_own)  # dx = dh U^T + direct
        dk, dd = wgrad_side.weight_grads(h, dz, xc, dh, m.kernel_dtype, m.down_dtype, task)
        return dx, dx0, dk, dd
    dk, _ = D.gemm(h, dz, a_is_km=True, out_dtype=torch.float32)           # dK = h^T dz     [p, d]
    dh, _ = D.gemm(dz, kc, b_is_nk=True)                                   # dh = dz K^T     [B, p]
    dd, _ = D.gemm(xc, dh, a_is_km=True, out_dtype=torch.float32)          # dU = x^T dh     [d, p]
    dx, dx0 = _dx_product(ctx, dh, dc, direct, dx0, x0c, task, u_own)      # dx = dh U^T + direct
    return dx, dx0, dk, dd


class CrossLayerFn(torch.autograd.Function):
    """y = x0 * (act(h @ K + b) + diag * x) + x,  h = x (full rank) or x @ U (low rank).

    Reference: FeatureCross.call, feature_cross.py:182-194.  Forward = one MFMA GEMM
    per Dense with the cross epilogue fused; backward = one elementwise pass
    (dz, dx0, bias gradient) + the data/weight-gradient GEMMs.
    Weight layouts are the keras ones: U [d, p], K [p or d, d], b [d].
    relay_in: the Dx0Relay a consumer of y may fill; relay_up: the relay of the layer that produced x
    (None when x does not come from a cross layer on the same x0)."""

    @staticmethod
    def forward(ctx, x0, x, down, kernel, bias, diag_scale, act, compute_dtype, relay_in=None, relay_up=None):
        same = x is x0 or (x.data_ptr() == x0.data_ptr() and x.shape == x0.shape and x.stride() == x0.stride())
        cd = compute_dtype
        x0c = x0.to(cd).contiguous()
        xc = x0c if same else x.to(cd).contiguous()
        # The forward contracts over the kernels' leading axis: hand the (small) weights to the MFMA
        # kernel K-contiguous (one transposed copy per step, a few microseconds) so that both GEMM
        # operands stream into LDS with row-wise 16-byte stores.
        # (cast + transposed copy of a weight = one launch, krs_cast_transpose)
        kc, kct = D.cast_transpose(kernel, cd)
        h = xc
        dc = None
        if down is not None:
            dc, dct = D.cast_transpose(down, cd)
            h, _ = D.gemm(xc, dct, b_is_nk=True)
        y, u = D.gemm(h, kct, b_is_nk=True, bias=bias, act=act, diag_scale=diag_scale,
                      x0=x0c, x=xc, want_u=True)
        ctx.save_for_backward(x0c, xc, h if down is not None else None, u, dc, kc)
        ctx.meta = _CrossMeta(diag_scale, act, same, down is not None, bias is not None,
                              x0.dtype, x.dtype, None if down is None else down.dtype, kernel.dtype)
        ctx.relay_in = relay_in
        both = ctx.needs_input_grad[0] and ctx.needs_input_grad[1]
        ctx.relay_up = relay_up if (relay_up is not None and not same and both and relay_up.matches(x0)) else None
        if relay_in is not None and FUSE_CROSS_BWD and down is not None:
            relay_in.lower = CrossLower(u, act, float(diag_scale or 0.0), bias is not None, same, x0c, ctx.relay_up, x.dtype)
        ctx.uses = wgrad_side.PendingUses(ctx, (down, kernel), any(ctx.needs_input_grad[i] for i in (2, 3)))
        return y

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        x0c, _, _, u, _, _ = saved
        m = ctx.meta
        same = m.x_is_x0
        g = g.to(x0c.dtype).contiguous()
        task = graph_task()
        # dL/dx0 of the layers above, left by the consumer of y during this backward pass
        incoming, extra, handoff = _take_handed_down(ctx.relay_in, x0c, task)
        dz, dx0, dxd, dbias, defer_dx0 = _cross_elementwise(ctx, saved, g, task, incoming, extra, handoff)
        if extra is not None:
            dx0 = dx0 + extra.to(dx0.dtype)
        direct = dx0 if same else (dxd if m.diag_scale else g)  # dL/dx through "+ x" and "diag * x"
        dx, dx0, dk, dd = _cross_products(ctx, saved, dz, direct, dx0, u if defer_dx0 else None, task)
        if same:
            gx0, gx = dx.to(m.x0_dtype), None
        else:
            gx, up = dx.to(m.x_dtype), ctx.relay_up
            if up is not None and task != -1:
                # the producer of x takes it from here (its backward runs later in this pass: it is owed dL/dx)
                if up.buf is not None and up.task == task:
                    dx0 = dx0 + up.buf      # x has a second cross-layer consumer that already left its term
                up.buf, up.task = dx0, task
                gx0 = None
            else:
                gx0 = dx0.to(m.x0_dtype)
        return (gx0, gx, None if dd is None else dd.to(m.down_dtype), dk.to(m.kernel_dtype),
                dbias if m.has_bias else None, None, None, None, None, None)


def cross_layer(x0, x, down, kernel, bias, diag_scale, act, compute_dtype):
    """CrossLayerFn on inputs of any rank, wired into the hand-offs as every layer class wires it: dL/dx0 travels down a
    stack of layers on the same x0 through relays instead of autograd adds -- this call's relay goes on its output, where
    the next layer (or a Dense layer, DenseFn) finds it; the relay of the layer that produced `x` is read off `x`."""
    lead, d = x0.shape[:-1], x0.shape[-1]
    same = x is x0
    x02 = x0.reshape(-1, d)
    x2 = x02 if same else x.reshape(-1, d)
    relay = Dx0Relay(x02)
    y = CrossLayerFn.apply(x02, x2, down, kernel, bias, diag_scale, act, compute_dtype, relay,
                           None if same else getattr(x, "_krs_dx0_relay", None))
    out = y.reshape(*lead, d)
    out._krs_dx0_relay = relay
    return out


class _DenseMeta(NamedTuple):
    act: int
    has_bias: bool
    x_dtype: torch.dtype
    kernel_dtype: torch.dtype


def _dense_dx_product(ctx, xc, kc, dz, task):
    """dx = dz K^T of a Dense layer, with the first backward step of the layer that produced x in its epilogue when
    that is a cross layer (ctx.relay_up) or a Dense layer (ctx.dense_up) and the hand-off is legal."""
    x_dt, up = ctx.meta.x_dtype, ctx.relay_up
    if _fusable_below(up, dz, x_dt, task):
        # x is the output of a cross layer: dx = dz K^T is its dL/dy, and its elementwise backward (dz, its
        # term of dL/dx0, bias gradient) rides in the epilogue of this product
        low = up.lower
        # (that layer's own term of dL/dx0 waits for ITS data-gradient product when that one is going to be a fused
        #  launch as well: u_upper there, one [B, d] matrix less written here and read there)
        defer = FUSE_TOP_DX0 and not low.x_is_x0 and _fusable_below(low.below, dz, low.x_dtype, task)
        dx, dz_low, dx0, db_low = D.gemm_cross_bwd(dz, kc, None, low.x0c, low.u, act=low.act, want_dbias=low.has_bias,
                                                   fold_direct=low.x_is_x0, want_dx0=not defer)
        if not defer:
            up.buf, up.task = dx0, task
        up.fused = Handoff(dx, dx._version, dz_low, db_low, task, defer)
        return dx
    if _dense_fusable_below(ctx.dense_up, dz, x_dt, task):
        # x is the output of a Dense layer: its activation backward and bias gradient ride in this product's epilogue;
        # what goes back to autograd is dx itself, the true dL/dy of that output (its backward recognises it)
        below = ctx.dense_up
        # (xc IS the lower layer's output y)
        dz_low, db_low, dx = D.gemm_dense_bwd(dz, kc, xc, below.lower.act, want_dbias=below.lower.has_bias, want_g=True)
        below.fused = Handoff(dx, dx._version, dz_low, db_low, task)
        return dx
    dx, _ = D.gemm(dz, kc, b_is_nk=True)                               # [B, in]
    return dx.to(x_dt)


class DenseFn(torch.autograd.Function):
    """y = act(x @ K + b): the Dense layers of the DLRM bottom / top MLPs
    (examples/ml_perf/model.py:214-262) on krs_gemm with the bias + activation epilogue fused.
    Backward: dz = g * act'(y) written through the output, dK = x^T dz (transposing-read GEMM),
    db = column sum, dx = dz K^T."""

    @staticmethod
    def forward(ctx, x, kernel, bias, act, compute_dtype, relay_up=None, dense_up=None, relay_out=None):
        # relay_up: the Dx0Relay of the cross layer that produced x (dense_layer reads it off its input): this layer's
        # data-gradient product then runs that layer's elementwise backward in its epilogue (krs_gemm_cross_bwd)
        # dense_up / relay_out: the DenseActRelay of the Dense layer that produced x / of this layer's own output
        xc = x.to(compute_dtype).contiguous()
        kc, kct = D.cast_transpose(kernel, compute_dtype)
        y, _ = D.gemm(xc, kct, b_is_nk=True, bias=bias, act=act)
        ctx.save_for_backward(xc, kc, y if act != L.ACT_NONE else None)
        ctx.meta = _DenseMeta(act, bias is not None, x.dtype, kernel.dtype)
        ctx.relay_up = relay_up if ctx.needs_input_grad[0] else None
        # (the lower layer's saved output is this layer's saved input when no cast / copy came between)
        ctx.dense_up = dense_up if (ctx.needs_input_grad[0] and xc.data_ptr() == x.data_ptr() and xc.dtype == x.dtype) else None
        ctx.relay_out = relay_out
        if relay_out is not None:
            relay_out.lower = DenseLower(act, bias is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        xc, kc, y = ctx.saved_tensors
        m = ctx.meta
        task = graph_task()
        rel, handoff = ctx.relay_out, None
        if rel is not None:
            handoff, rel.fused = rel.fused, None
        # the consumer of y ran this layer's activation backward inside its data-gradient product: right only when
        # what arrives is that product's G, untouched (no second consumer summed in, no hook replaced or changed it)
        if handoff is not None and handoff.is_gradient(g, task):
            dz, db = handoff.dz, handoff.dbias
        else:
            g = g.to(xc.dtype)
            # dz = g * act'(y) and the bias gradient in one pass (krs_dense_act_bwd)
            dz, db = D.dense_act_bwd(g, y, m.act, want_dbias=m.has_bias)
        dz = dz.contiguous()
        dk, _ = D.gemm(xc, dz, a_is_km=True, out_dtype=torch.float32)            # [in, units]
        dx = _dense_dx_product(ctx, xc, kc, dz, task) if ctx.needs_input_grad[0] else None
        return dx, dk.to(m.kernel_dtype), db, None, None, None, None, None


def dense_layer(x, kernel, bias, act, compute_dtype, host_activation=None):
    """DenseFn on an input of any rank, wired into the hand-offs as layers.Dense wires it.  A 2-D input that is the output
    of a FeatureCross stack carries that layer's relay: the data gradient of this layer then runs the cross layer's
    elementwise backward in its epilogue.  Likewise one that is the output of another Dense layer carries a DenseActRelay:
    that layer's activation backward and bias gradient then ride in this layer's data-gradient product; this layer's own
    output gets one -- unless `host_activation` (a callable applied to the product's output: `act` is ACT_NONE then)
    stands between the product and the output."""
    lead, d = x.shape[:-1], x.shape[-1]
    two_d = x.dim() == 2
    relay_out = DenseActRelay() if (two_d and host_activation is None) else None
    y = DenseFn.apply(x.reshape(-1, d), kernel, bias, act, compute_dtype,
                      getattr(x, "_krs_dx0_relay", None) if two_d else None,
                      getattr(x, "_krs_dense_relay", None) if two_d else None, relay_out)
    if host_activation is not None:
        y = host_activation(y)
    y = y.reshape(*lead, kernel.shape[1])
    if relay_out is not None:
        relay_out.out_ref = weakref.ref(y)
        y._krs_dense_relay = relay_out
    return y


class BinaryCrossentropyFn(torch.autograd.Function):
    """loss = mean(-(y log p + (1 - y) log(1 - p))), p = clip(pred, eps, 1 - eps): keras.losses.BinaryCrossentropy()
    as examples/ml_perf/main.py:201-210 compiles it.  The gradient is produced by the forward's single pass over the
    predictions (krs_bce_fwd_bwd) and scaled by the incoming scalar in the backward."""

    @staticmethod
    def forward(ctx, pred, labels, epsilon):
        loss, dp = D.bce_fwd_bwd(pred, labels, epsilon, want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(dp)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return (dp if dp is None else dp * g.to(dp.dtype)), None, None


class CrossEpilogueFn(torch.autograd.Function):
    """y = x0 * (u + diag*x) + x for a host-composed u (arbitrary pre_activation callables)."""

    @staticmethod
    def forward(ctx, u, x0, x, diag_scale):
        u, x0, x = u.contiguous(), x0.contiguous(), x.contiguous()
        ctx.save_for_backward(u, x0, x)
        ctx.diag = diag_scale
        return D.cross_epilogue_fwd(u, x0, x, diag_scale)

    @staticmethod
    def backward(ctx, g):
        u, x0, x = ctx.saved_tensors
        du, dx0, dxd, _ = D.cross_epilogue_bwd(g.contiguous(), u, x0, x, ctx.diag, want_dbias=False)
        return du, dx0, dxd, None


class DotInteractionFn(torch.autograd.Function):
    """DotInteraction.call (dot_interaction.py:170-203) and its gradient.
    relay / n_heads: see SlabGradRelay -- feats[n_heads:] are the feature views of the relay's slab, in order."""

    @staticmethod
    def forward(ctx, self_interaction, skip_gather, relay, n_heads, *feats):
        ctx.save_for_backward(*feats)
        ctx.flags = (self_interaction, skip_gather)
        ctx.relay, ctx.n_heads = relay, n_heads
        # the joined path hands the slab views no gradient of their own: not when somebody watches one of them
        ctx.view_refs = [weakref.ref(t) for t in feats[n_heads:]] if relay is not None else []
        return D.dot_interaction_fwd(feats, self_interaction, skip_gather)

    @staticmethod
    def backward(ctx, g):
        feats = ctx.saved_tensors
        si, sg = ctx.flags
        relay = ctx.relay
        watched = any((t := r()) is not None and (t.retains_grad or t._backward_hooks) for r in ctx.view_refs)
        if relay is not None and relay.buf is not None and not watched:
            buf, task = relay.buf, graph_task()
            n, (batch, dim) = len(feats), feats[0].shape
            if (relay.task == task and task != -1 and tuple(buf.shape) == (batch, n * dim) and buf.is_contiguous()
                    and buf.dtype == feats[0].dtype and g.dtype == buf.dtype):
                relay.buf = None
                SlabGradRelay.joined += 1
                mask = ((1 << n) - 1) & ~((1 << ctx.n_heads) - 1)
                grads = D.dot_interaction_bwd(feats, g, si, sg, into=buf, accumulate_mask=mask)
                return (None, None, None, None, *grads)
        grads = D.dot_interaction_bwd(feats, g, si, sg)
        return (None, None, None, None, *grads)


class EmbedBagFn(torch.autograd.Function):
    """Fused gather+pool over a FusedBags group with the reference's autodiff semantics:
    dense [V, D] table gradients, computed by the sort-based K2.
    Returns one [B, D] tensor per feature (column views of one fused buffer)."""

    @staticmethod
    def forward(ctx, bags, ids, batch, hots, offsets, weights, out_dtype, check_ids, *tables):
        # `tables` are passed explicitly so autograd tracks them; `bags.tables` hold the same storage.
        # check_ids: True = read the kernel's error word now (one host sync; EmbedReduce does that);
        # a device int32[1] tensor = let the kernel OR its bits into it and return (the caller reads it
        # later: DistributedEmbedding.check_ids); False / None = no report.
        lazy = isinstance(check_ids, torch.Tensor)
        err = check_ids if lazy else (torch.zeros(1, dtype=torch.int32, device=ids.device) if check_ids else None)
        out, scale = bags.forward(ids, batch, hots=hots, offsets=offsets, weights=weights, out_dtype=out_dtype,
                                  want_scale=any(comb != L.SUM for _, comb, _ in bags.features), err_flag=err)
        if check_ids is True and int(err.item()) & L.FLAG_ID_OUT_OF_RANGE:
            raise IndexError("embedding id out of range for its table (ids are never clamped)")
        ctx.bags, ctx.batch, ctx.hots = bags, batch, hots
        ctx.save_for_backward(ids, offsets, weights, scale)
        ctx.table_dtypes = [t.dtype for t in tables]
        ctx.out_meta = (out.dtype, out.device)
        return _split_columns(out, len(bags.features), bags.dim)

    @staticmethod
    def backward(ctx, *gs):
        ids, offsets, weights, scale = ctx.saved_tensors
        bags = ctx.bags
        g = _gather_feature_grads(gs, ctx.batch, bags.dim, *ctx.out_meta)
        ws = bags.plan_backward(ids, ctx.batch, hots=ctx.hots, offsets=offsets, global_order=False)
        grads = bags.backward_dense(ws, g, ctx.batch, ids.numel(), hots=ctx.hots, weights=weights,
                                    bag_scale=scale)
        grads = [gr.to(dt) for gr, dt in zip(grads, ctx.table_dtypes)]
        return (None, None, None, None, None, None, None, None, *grads)


# development switch (A/B of the two orders, see EmbedBagFusedFn.forward)
_PLAN_AFTER_GATHER = _switch(os.environ.get("KRS_PLAN_AFTER_GATHER", "0"))


class EmbedBagFusedFn(torch.autograd.Function):
    """Fused gather+pool whose backward applies the per-table optimizer to the touched rows
    in place (the SparseCore-style path: jax/embedding_lookup.py:174-273 returns updated
    tables instead of gradients).  `anchor` is a dummy scalar that requires grad so that the
    backward runs; it receives a zero gradient."""

    @staticmethod
    def forward(ctx, bags, ids, batch, hots, offsets, weights, out_dtype, optimizer, anchor, lead=0, err_flag=None):
        # outputs: the whole slab [B, lead + n*dim] (columns 0..lead are left for the caller, see
        # layers.concat_features) followed by the per-feature column views
        ctx.set_materialize_grads(False)  # unused outputs (slab or views) arrive as None, not as zero tensors
        n = len(bags.features)
        slab = torch.empty((batch, lead + n * bags.dim), dtype=out_dtype or bags.dtype, device=ids.device)
        # The backward's plan (sort of the lookups by row) depends only on the ids: start it now on a side
        # stream, BEFORE the gather is enqueued, so that the two run side by side -- the gather is bound by
        # HBM, the sort's scatter passes by LDS ranking work -- and the plan is done when the dense part starts
        # (queued behind the gather it ran under the first FeatureCross GEMMs and slowed them by 0.4 ms).
        ctx.plan = None
        ctx.owns_plan_ws = False
        plan_first = not _PLAN_AFTER_GATHER
        # the per-bag combiner scale (1 / sum w, 1 / sqrt(sum w^2)) is what the backward multiplies by: all ones for
        # "sum" bags, which then neither write it here nor gather it per lookup there
        want_scale = any(comb != L.SUM for _, comb, _ in bags.features)
        if not plan_first:
            out, scale = bags.forward(ids, batch, hots=hots, offsets=offsets, weights=weights,
                                      out=slab[:, lead:], want_scale=want_scale, err_flag=err_flag)
        if ctx.needs_input_grad[8]:  # a backward will follow (not under torch.no_grad())
            main = torch.cuda.current_stream()
            side = _side_stream(ids.device)
            # The descriptor blocks are uploaded (and cached) by whoever asks first: do that HERE, on the main
            # stream, so that the copy is ordered before both users -- the plan (side waits for main below) and
            # the gather (main).  Uploaded on the side stream by a cold cache, the gather on main would have read
            # them with nothing ordering it behind the copy (first step, first-seen batch size, after .to()).
            bags.table_desc()
            bags.feature_desc(batch, hots, ids.device)
            side.wait_stream(main)
            # The plan's workspace (0.36 GB at C3) lives on the bags across steps.  Allocated per step inside the side
            # stream's context it could only be re-used once the DEVICE had passed the step that used it (record_stream
            # below), and a host that enqueues a step in 2 ms against 10 ms of device time gets ever further ahead: a
            # fresh hipMalloc every other step (1 - 11 ms of host time each, box-dependent: one bench leg in three ran
            # host-bound at 21 ms per step).  Safe: the side stream has just waited for everything the main stream holds,
            # including the previous step's apply; a second forward before that step's backward gets its own tensor.
            keep = None if getattr(bags, "_plan_ws_busy", False) else getattr(bags, "_plan_ws", None)
            with torch.cuda.stream(side):
                ws = bags.plan_backward(ids, batch, hots=hots, offsets=offsets, global_order=False, ws=keep)
                done = torch.cuda.Event()
                done.record(side)
            if not getattr(bags, "_plan_ws_busy", False):
                bags._plan_ws, bags._plan_ws_busy = ws, True
                ctx.owns_plan_ws = [True]
                weakref.finalize(ctx, _release_plan_ws, weakref.ref(bags), ctx.owns_plan_ws)
            for t in (ws, ids, offsets):
                if t is not None:
                    t.record_stream(side)
            ctx.plan = (ws, done)
        # err_flag: device int32[1] the kernel ORs KRS_FLAG_* into (out-of-range ids contribute nothing and are
        # never clamped); read later by the layer, so the step keeps running without a host sync
        if plan_first:
            out, scale = bags.forward(ids, batch, hots=hots, offsets=offsets, weights=weights,
                                      out=slab[:, lead:], want_scale=want_scale, err_flag=err_flag)
        ctx.bags, ctx.batch, ctx.hots, ctx.optimizer, ctx.lead = bags, batch, hots, optimizer, lead
        ctx.save_for_backward(ids, offsets, weights, scale)
        ctx.out_meta = (out.dtype, out.device)
        return (slab,) + _split_columns(slab, n, bags.dim, lead)

    @staticmethod
    def backward(ctx, g_slab, *gs):
        ids, offsets, weights, scale = ctx.saved_tensors
        bags = ctx.bags
        g = _sum_slab_and_feature_grads(g_slab, gs, ctx.lead, ctx.batch, len(bags.features), bags.dim,
                                        *ctx.out_meta)
        if ctx.plan is not None:
            ws, done = ctx.plan
            torch.cuda.current_stream().wait_event(done)
            ws.record_stream(torch.cuda.current_stream())
        else:
            ws = bags.plan_backward(ids, ctx.batch, hots=ctx.hots, offsets=offsets, global_order=False)
        opt = ctx.optimizer  # a kind string, or an object with .fused_kind / .next_hyper() (the layer's group)
        kind = opt if isinstance(opt, str) else opt.fused_kind
        hyper = None if isinstance(opt, str) else opt.next_hyper()   # also refreshes scheduled learning rates
        bags.backward_fused(kind, ws, g, ctx.batch, ids.numel(), hots=ctx.hots, weights=weights,
                            bag_scale=scale, hyper=hyper)
        if ctx.owns_plan_ws:
            # (the next forward's plan is ordered behind this apply: it may take the buffer)
            _release_plan_ws(weakref.ref(bags), ctx.owns_plan_ws)
        # (no gradient for the anchor -- it exists only to make autograd call this function; a zero tensor here cost a fill and an
        #  accumulate launch per step)
        return (None,) * 11


class SlabFillFn(torch.autograd.Function):
    """concat([*heads, slab[:, lead:]]) without the copy of the slab: the heads (lead columns in
    total) are written into the slab's reserved leading columns and the slab itself is the result.
    The write goes through `.data`, so tensors that saved views of the slab keep their version."""

    @staticmethod
    def forward(ctx, slab, relay, *heads):
        col = 0
        ctx.cols = []
        ctx.relay = relay
        with torch.no_grad():
            for h in heads:
                w = h.shape[1]
                slab.data[:, col:col + w].copy_(h)
                ctx.cols.append((col, col + w))
                col += w
        return slab.data.as_strided(slab.shape, slab.stride(), slab.storage_offset())

    @staticmethod
    def backward(ctx, g):
        relay = ctx.relay
        if relay is not None:
            # (a concat result nobody holds any more cannot show its .grad to anyone)
            out = relay.out_ref() if relay.out_ref is not None else None
            plain = (out is None or (not out.retains_grad and not out._backward_hooks)) and not relay.disabled
            task = graph_task()
            relay.buf, relay.task = (g, task) if (plain and task != -1 and g.is_contiguous()) else (None, -1)
        return (g, None) + tuple(g[:, a:b] for a, b in ctx.cols)
