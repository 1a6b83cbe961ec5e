"""The opt-in second stream for the weight gradients of the cross layers (autograd.CrossLayerFn.backward).

Weight-gradient GEMMs of the cross layers on a second stream: they are off the critical path, and started behind a layer's
dx product they run beside the HBM-bound dz / dx0 pass of the layer below (or the DotInteraction gradient and the table
update behind the bottom layer) -- an elementwise pass and a ring GEMM do overlap a little on this part
(scripts/exp/overlap_probe2.py: 563 + 271 us apart, 707 together), two GEMMs or a GEMM and the table update do not.
Measured in the step: 10.31-10.48 -> 10.20-10.29 ms.  Deferring all six to the table update was slower (10.49).
OPT-IN since round 4 (`autograd.set_wgrad_side_stream(True)` or KRS_WGRAD_SIDE=1), and no longer used by bench.py / the
example: with the elementwise backward inside the data-gradient products (krs_gemm_cross_bwd) the pass these GEMMs
overlapped with is gone -- beside the next layer's ring GEMMs they measured 10.26 against 10.13-10.18 ms
(profiles/archive/r4k_wgrad_side_ab.txt).  Also: a gradient produced on a private stream is only safe when NOTHING but the
end-of-backward rejoin reads it, and a backward function cannot see every reader -- a second gradient contribution to the
same weight (a manual L2 term, a weight shared by two layers) is summed by autograd's input buffer on the main stream with
nothing ordering it behind this stream.  The owner of the training step can promise that; a library default cannot.  What
the function can see it still checks (`_wgrad_side_ok`): an accumulated .grad, tensor hooks, foreign post-accumulate
hooks, a regulariser on the weight (layers.base marks it: its penalty is a second contribution), the weight used by
more than one pending CrossLayerFn.

Whether the stream is enabled is the caller's switch (autograd.WGRAD_SIDE_STREAM): `may_use` is told, it keeps no copy.
"""

from __future__ import annotations

import weakref

import torch

from keras_rs_amd import dense_ops as D

_WGRAD_STREAMS: dict = {}
_WGRAD_SYNC_QUEUED: set = set()


def _wgrad_stream(device) -> "torch.cuda.Stream":
    key = str(device)
    st = _WGRAD_STREAMS.get(key)
    if st is None:
        st = _WGRAD_STREAMS[key] = torch.cuda.Stream(device=device)
    return st


class PendingUses:
    """The pending uses of the weights of ONE CrossLayerFn call (a weight shared by two layer calls gets two gradient
    contributions).  The count is given back by the backward -- or, when no backward ever runs on this graph (a
    grad-enabled validation pass, an exception, a discarded output), by the finalizer of the graph node `owner`: a count
    left above one would keep the weight off the second stream for good, silently."""

    __slots__ = ("w_refs", "counted")

    def __init__(self, owner, weights, counted: bool):
        self.w_refs = tuple(weakref.ref(w) for w in weights if w is not None)
        self.counted = counted
        if counted:
            for w in weights:
                if w is not None:
                    w._krs_pending_cross = getattr(w, "_krs_pending_cross", 0) + 1
            weakref.finalize(owner, self.release)

    def release(self) -> None:
        """Gives back one pending use of each weight, once."""
        if not self.counted:
            return
        self.counted = False
        for r in self.w_refs:
            w = r()
            if w is not None:
                w._krs_pending_cross = max(0, getattr(w, "_krs_pending_cross", 1) - 1)


def _wgrad_side_ok(w) -> bool:
    """May this weight's gradient come off the second stream?  Only when nothing reads it before the end of the backward
    pass: no gradient to accumulate into yet (the first accumulation is an assignment, a later one is an add kernel on
    the main stream), no tensor hooks, no post-accumulate hooks other than ones that rejoin the stream themselves
    (dp.GradAllReduce marks its parameters), no second consumer this function knows of (a regulariser attached by
    `Layer.add_weight`, a second CrossLayerFn whose backward is still pending)."""
    if w is None:
        return True
    if w.grad is not None or w._backward_hooks:
        return False
    if getattr(w, "_krs_has_regularizer", False) or getattr(w, "_krs_pending_cross", 1) != 1:
        return False
    hooks = getattr(w, "_post_accumulate_grad_hooks", None)
    return not hooks or bool(getattr(w, "_krs_hooks_rejoin_wgrad_stream", False))


def may_use(uses: PendingUses, task: int, dz: torch.Tensor, enabled: bool, min_rows: int) -> bool:
    """May the backward that owns `uses` put its weight gradients on the second stream in pass `task`?  Gives the
    pending uses back, whatever the answer.
    (Worth it when the kernels are long against a launch: at a per-rank batch of 8192 the step is bound by the host's
    enqueue rate and the extra events cost more than the overlap returns: 2.42 -> 2.54 ms; hence `min_rows`.)"""
    # a weight with several pending uses gets several contributions in THIS pass (summed by autograd's input buffer
    # on the main stream): the first backward that runs sees the full count and marks the pass, the later ones --
    # which see a count of one again -- read the mark
    shared = False
    for r in uses.w_refs:
        w = r()
        if w is None:
            continue
        if getattr(w, "_krs_pending_cross", 1) != 1:
            w._krs_shared_in_task = task
        shared = shared or (task != -1 and getattr(w, "_krs_shared_in_task", None) == task)
    ok = enabled and dz.is_cuda and dz.shape[0] >= min_rows and not shared and all(_wgrad_side_ok(r()) for r in uses.w_refs)
    uses.release()
    return ok


def weight_grads(h, dz, xc, dh, k_dt, down_dt, task: int):
    """(dK = h^T dz, dU = x^T dh) in the weights' dtypes, on the second stream, which starts when everything the main
    stream holds so far -- the data-gradient path -- is done, i.e. beside the HBM-bound kernel that follows there (the
    dz / dx0 pass of the layer below, or the DotInteraction gradient and the table update behind the bottom layer).  The
    main stream rejoins at the end of the backward pass (wgrad_stream_sync)."""
    main = torch.cuda.current_stream()
    side = _wgrad_stream(dz.device)
    ev = torch.cuda.Event()
    ev.record(main)
    dk = torch.empty((h.shape[1], dz.shape[1]), dtype=torch.float32, device=dz.device)
    dd = torch.empty((xc.shape[1], dh.shape[1]), dtype=torch.float32, device=dz.device)

    side.wait_event(ev)
    with torch.cuda.stream(side):
        D.gemm(h, dz, a_is_km=True, out_dtype=torch.float32, out=dk)   # dK = h^T dz     [p, d]
        D.gemm(xc, dh, a_is_km=True, out_dtype=torch.float32, out=dd)  # dU = x^T dh     [d, p]
        # the casts to the weights' dtype (bf16 variables) belong to this stream too: on the main stream they
        # would read dk / dd with nothing ordering them behind the two products
        dk_out, dd_out = dk.to(k_dt), dd.to(down_dt)
    for t in (h, dz, xc, dh, dk, dd, dk_out, dd_out):
        t.record_stream(side)
    _queue_wgrad_sync(task)
    return dk_out, dd_out


def wgrad_stream_sync() -> None:
    """The current stream waits for the weight-gradient stream(s): before anything reads those gradients (the end of
    the backward pass does it by itself; dp.GradAllReduce calls it before it reduces a gradient)."""
    for st in _WGRAD_STREAMS.values():
        torch.cuda.current_stream(st.device).wait_stream(st)


def _queue_wgrad_sync(task: int) -> None:
    """Once per backward pass: rejoin the main stream when the graph task ends."""
    if task in _WGRAD_SYNC_QUEUED:
        return
    if task == -1:          # not inside a backward pass (a direct call): rejoin at once
        wgrad_stream_sync()
        return
    _WGRAD_SYNC_QUEUED.add(task)

    def done():
        _WGRAD_SYNC_QUEUED.discard(task)
        wgrad_stream_sync()

    torch.autograd.Variable._execution_engine.queue_callback(done)
