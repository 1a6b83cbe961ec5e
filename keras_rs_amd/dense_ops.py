"""Host side of K3/K4/K5: thin torch wrappers over krs_gemm, the cross epilogue
kernels, krs_dot_interaction_{fwd,bwd} and krs_mod_bucketize.

Everything here marshals raw device pointers into the C ABI (include/krs.h);
torch only provides memory and the current stream.
"""

from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import probe

ACTS = {None: L.ACT_NONE, "linear": L.ACT_NONE, "relu": L.ACT_RELU, "sigmoid": L.ACT_SIGMOID,
        "tanh": L.ACT_TANH}


def gemm(a: torch.Tensor, b: torch.Tensor, *, a_is_km: bool = False, b_is_nk: bool = False,
         out_dtype: torch.dtype | None = None, bias: torch.Tensor | None = None, act: int = L.ACT_NONE,
         diag_scale: float = 0.0, x0: torch.Tensor | None = None, x: torch.Tensor | None = None,
         want_u: bool = False, r: torch.Tensor | None = None, beta: float = 1.0,
         out: torch.Tensor | None = None):
    """C = epilogue(A @ B) (include/krs.h: krs_gemm).  Returns (C, u_or_None).

    a: [M,K] (or [K,M] when a_is_km);  b: [K,N] (or [N,K] when b_is_nk)."""
    a = L.rowmajor(a, "gemm A")
    b = L.rowmajor(b, "gemm B")
    if a.dtype != b.dtype:
        raise L.KrsError("gemm: A and B must share a dtype")
    m, k = (a.shape[1], a.shape[0]) if a_is_km else (a.shape[0], a.shape[1])
    kb, n = (b.shape[1], b.shape[0]) if b_is_nk else (b.shape[0], b.shape[1])
    if k != kb:
        raise L.KrsError(f"gemm: inner dimensions differ ({k} vs {kb})")
    odt = out_dtype or a.dtype
    c = out if out is not None else torch.empty((m, n), dtype=odt, device=a.device)
    ep = L.GemmEpilogue()
    keep = []
    if bias is not None:
        bias = bias.float().contiguous()
        keep.append(bias)
        ep.bias = bias.data_ptr()
    ep.act = act
    ep.diag_scale = float(diag_scale or 0.0)
    if x0 is not None:
        x0 = L.rowmajor(x0, "gemm x0")
        x = L.rowmajor(x, "gemm x")
        if x0.stride(0) != x.stride(0):
            x0, x = x0.contiguous(), x.contiguous()
        if x0.dtype != odt or x.dtype != odt:
            raise L.KrsError("gemm: x0/x must have the output dtype")
        keep += [x0, x]
        ep.x0, ep.x, ep.ldx = x0.data_ptr(), x.data_ptr(), x.stride(0)
    u = None
    if want_u:
        u = torch.empty((m, n), dtype=odt, device=a.device)
        ep.u_out, ep.ldu = u.data_ptr(), u.stride(0)
    if r is not None:
        r = L.rowmajor(r, "gemm R")
        if r.dtype != odt:
            raise L.KrsError("gemm: R must have the output dtype")
        keep.append(r)
        ep.r, ep.ldr, ep.beta = r.data_ptr(), r.stride(0), float(beta)
    wsb = L.lib().krs_gemm_workspace_bytes(m, n, k, int(a_is_km))
    ws = torch.empty(int(wsb), dtype=torch.uint8, device=a.device) if wsb else None
    # (bench.py's per-product roofline: one span name per product FAMILY -- operand layout, epilogue form, dtype, shape)
    name = "gemm"
    if probe.ACTIVE is not None:
        name = "gemm[%s%s %s] %dx%dx%d" % ("tn" if a_is_km else ("nt" if b_is_nk else "nn"),
                                           ":cross" if x0 is not None else (":res" if r is not None else ""),
                                           "bf16" if a.dtype == torch.bfloat16 else "f32", m, n, k)
    with probe.span(name, 2.0 * m * n * k):
        rc = L.lib().krs_gemm(
            L.ptr(a), a.stride(0), int(a_is_km),
            L.ptr(b), b.stride(0), int(b_is_nk),
            L.ptr(c), c.stride(0), m, n, k,
            L.fdtype(a), L.fdtype(c), C.byref(ep),
            L.ptr(ws), int(wsb), L.stream_ptr())
    L.check(rc, "krs_gemm")
    return c, u


def cross_epilogue_fwd(u, x0, x, diag_scale=0.0):
    u, x0, x = (L.rowmajor(t, "cross_epilogue_fwd").contiguous() for t in (u, x0, x))
    y = torch.empty_like(x)
    m, n = x.shape
    rc = L.lib().krs_cross_epilogue_fwd(L.ptr(u), L.ptr(x0), L.ptr(x), L.ptr(y), m, n,
                                        n, diag_scale or 0.0, L.fdtype(x),
                                        L.stream_ptr())
    L.check(rc, "krs_cross_epilogue_fwd")
    return y


def _colsum_ws(m: int, n: int, device):
    """(pointer, byte count) arguments of the two-stage column sums (run-to-run identical bias gradients) + the
    tensor that keeps the workspace alive until the call has been enqueued."""
    nbytes = int(L.lib().krs_colsum_workspace_bytes(m, n))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
    return ws, L.ptr(ws), nbytes


def cross_epilogue_bwd(g, u, x0, x, diag_scale=0.0, *, act: int = L.ACT_NONE,
                       dx0_into: torch.Tensor | None = None,
                       want_du=True, want_dxd=True, want_dbias=True, fold_direct=False, want_dx0=True):
    """Returns (du, dx0, dxd, dbias); dx0 accumulates into `dx0_into` when given.
    fold_direct (the case x is x0): the direct term g + diag*g*x0 is added into dx0 instead of
    being written to its own buffer (the C ABI's `dxd == dx0` aliasing rule); dxd is then dx0."""
    g, x0, x = (L.rowmajor(t, "cross_epilogue_bwd").contiguous() for t in (g, x0, x))
    # (u None: allowed when neither dL/dx0 nor an activation derivative is wanted -- dz = g * x0 needs no third stream)
    u = None if u is None else L.rowmajor(u, "cross_epilogue_bwd").contiguous()
    if u is None and (want_dx0 or act != L.ACT_NONE):
        raise L.KrsError("cross_epilogue_bwd: u is needed for dL/dx0 and for an activation's derivative")
    m, n = x.shape
    du = torch.empty_like(x) if want_du else None
    dx0 = None
    if want_dx0:
        dx0 = dx0_into if dx0_into is not None else torch.empty_like(x)
        if not dx0.is_contiguous():
            raise L.KrsError("cross_epilogue_bwd: dx0 buffer must be contiguous")
    dxd = dx0 if fold_direct else (torch.empty_like(x) if want_dxd else None)
    dbias = torch.empty(n, dtype=torch.float32, device=x.device) if want_dbias else None
    ws, ws_ptr, ws_bytes = _colsum_ws(m, n, x.device) if want_dbias else (None, None, 0)
    rc = L.lib().krs_cross_epilogue_bwd(
        L.ptr(g), L.ptr(u), L.ptr(x0), L.ptr(x), L.ptr(du), L.ptr(dx0), int(dx0_into is not None),
        L.ptr(dxd), L.ptr(dbias), m, n, n, diag_scale or 0.0,
        act, L.fdtype(x), ws_ptr, ws_bytes, L.stream_ptr())
    L.check(rc, "krs_cross_epilogue_bwd")
    return du, dx0, dxd, dbias


def gemm_cross_bwd(a: torch.Tensor, bt: torch.Tensor, r: torch.Tensor, x0: torch.Tensor, u: torch.Tensor, *,
                   act: int = L.ACT_NONE, dx0_into: torch.Tensor | None = None, want_dbias: bool = True,
                   fold_direct: bool = False, beta: float = 1.0, u_upper: torch.Tensor | None = None,
                   want_dx0: bool = True):
    """krs_gemm_cross_bwd: G = A @ Bt^T + beta * R (the data gradient of a cross layer = dL/dy of the layer below it)
    and, from G as stored, the elementwise backward of that layer below -- dz = G x0 act'(u), dx0 = [dx0_into +] G u,
    dbias = column sums of dz -- in ONE launch (fold_direct: the layer below is fed x0 itself, its direct term G joins
    dx0; u_upper: the saved activation output of the layer ABOVE, whose own term R * u_upper then starts dx0 here instead
    of in a matrix that layer would have written; want_dx0=False, without R only: no dL/dx0 from this launch -- `u` is
    handed to the next one as ITS u_upper).  Returns (G, dz, dx0, dbias).  a: [M, K], bt: [N, K] (K-contiguous
    weight), r / x0 / u: [M, N] row-major of a's dtype."""
    a, bt = L.rowmajor(a, "gemm_cross_bwd A"), L.rowmajor(bt, "gemm_cross_bwd Bt")
    x0, u = (L.rowmajor(t, "gemm_cross_bwd operand").contiguous() for t in (x0, u))
    r = None if r is None else L.rowmajor(r, "gemm_cross_bwd R").contiguous()      # (None: no residual term)
    m, k = a.shape
    n = bt.shape[0]
    if bt.shape[1] != k or (r is not None and tuple(r.shape) != (m, n)) or tuple(x0.shape) != (m, n) or tuple(u.shape) != (m, n):
        raise L.KrsError("gemm_cross_bwd: shapes do not fit")
    if not (a.dtype == bt.dtype == x0.dtype == u.dtype) or (r is not None and r.dtype != a.dtype):
        raise L.KrsError("gemm_cross_bwd: one dtype for every operand")
    g = torch.empty((m, n), dtype=a.dtype, device=a.device)
    dz = torch.empty_like(g)
    if not want_dx0 and (r is not None or dx0_into is not None or u_upper is not None or fold_direct):
        raise L.KrsError("gemm_cross_bwd: want_dx0=False is the form without R, dx0_into, u_upper and fold_direct")
    dx0 = None if not want_dx0 else (dx0_into if dx0_into is not None else torch.empty_like(g))
    if dx0 is not None and (not dx0.is_contiguous() or dx0.dtype != a.dtype or tuple(dx0.shape) != (m, n)):
        raise L.KrsError("gemm_cross_bwd: dx0 buffer must be a contiguous [M, N] matrix of the operands' dtype")
    if u_upper is not None:
        u_upper = L.rowmajor(u_upper, "gemm_cross_bwd u_upper").contiguous()
        if dx0_into is not None or r is None or beta != 1.0 or u_upper.dtype != a.dtype or tuple(u_upper.shape) != (m, n):
            raise L.KrsError("gemm_cross_bwd: u_upper needs R (beta = 1), no dx0 to accumulate into, and the operands' shape / dtype")
    dbias = torch.empty(n, dtype=torch.float32, device=a.device) if want_dbias else None
    nbytes = int(L.lib().krs_gemm_cross_bwd_workspace_bytes(m, n)) if want_dbias else 0
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=a.device) if want_dbias else None
    # (its own span: the launch is a product AND five to seven [M, N] streams of elementwise work)
    with probe.span("gemm_cross_bwd", 2.0 * m * n * k):
        rc = L.lib().krs_gemm_cross_bwd(
            L.ptr(a), a.stride(0), L.ptr(bt), bt.stride(0), L.ptr(r), r.stride(0) if r is not None else n, beta,
            L.ptr(g), n, L.ptr(x0), L.ptr(u), L.ptr(dz), L.ptr(dx0), n, int(dx0_into is not None), L.ptr(u_upper),
            int(fold_direct), L.ptr(dbias), m, n, k, act, L.fdtype(a), L.ptr(ws), nbytes, L.stream_ptr())
    L.check(rc, "krs_gemm_cross_bwd")
    return g, dz, dx0, dbias


def gemm_dense_bwd(a: torch.Tensor, bt: torch.Tensor, y: torch.Tensor, act: int, want_dbias: bool = True,
                   want_g: bool = False):
    """krs_gemm_dense_bwd: dz = (A @ Bt^T) * act'(y) and dbias = column sums of dz in ONE launch -- the
    data-gradient product of a Dense layer running the activation backward of the Dense layer BELOW it (whose saved output
    is y) in its epilogue.  want_g: the product G = A @ Bt^T (rounded once; dz is computed from it as stored) is written
    too -- the true dL/dy of that output; otherwise it is never stored.  a: [M, K], bt: [N, K], y: [M, N].
    Returns (dz, dbias, G or None)."""
    a, bt = L.rowmajor(a, "gemm_dense_bwd A"), L.rowmajor(bt, "gemm_dense_bwd Bt")
    y = L.rowmajor(y, "gemm_dense_bwd y").contiguous()
    m, k = a.shape
    n = bt.shape[0]
    if bt.shape[1] != k or tuple(y.shape) != (m, n) or not (a.dtype == bt.dtype == y.dtype):
        raise L.KrsError("gemm_dense_bwd: shapes / dtypes do not fit")
    dz = torch.empty((m, n), dtype=a.dtype, device=a.device)
    g = torch.empty_like(dz) if want_g else None
    dbias = torch.empty(n, dtype=torch.float32, device=a.device) if want_dbias else None
    nbytes = int(L.lib().krs_gemm_cross_bwd_workspace_bytes(m, n)) if want_dbias else 0
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=a.device) if want_dbias else None
    with probe.span("gemm_dense_bwd", 2.0 * m * n * k):
        rc = L.lib().krs_gemm_dense_bwd(L.ptr(a), a.stride(0), L.ptr(bt), bt.stride(0), L.ptr(g), n, L.ptr(y),
                                        L.ptr(dz), n, L.ptr(dbias), m, n, k, act, L.fdtype(a), L.ptr(ws), nbytes,
                                        L.stream_ptr())
    L.check(rc, "krs_gemm_dense_bwd")
    return dz, dbias, g


CROSS_BWD_ROUTES = {0: None, 1: "two_call", 2: "pp64", 3: "pp256"}


def last_cross_bwd_route():
    """(route, epilogue) of the calling thread's last krs_gemm_cross_bwd / krs_gemm_dense_bwd (gemm_cross_bwd /
    gemm_dense_bwd): route is "two_call", "pp64" or "pp256" (fused, on that ring kernel), None when no launch was made;
    epilogue is the fused epilogue number (3 .. 10), 0 otherwise.  A diagnostic for tests: it reads a host-side record,
    no device sync."""
    ep = C.c_int(0)
    route = int(L.lib().krs_gemm_cross_bwd_last_route(C.byref(ep)))
    return CROSS_BWD_ROUTES[route], int(ep.value)


GEMM_KERNELS = {0: None, 1: "generic", 2: "mfma", 3: "glds", 4: "tn_glds", 5: "pp256", 6: "pp256_kstrided", 7: "pp64",
                8: "thin", 9: "rowdot", 10: "smallk"}
GEMM_REDUCES = {0: None, 1: "scalar", 2: "vec4", 3: "vec8"}


def _route_dict(rt) -> dict:
    return dict(kernel=GEMM_KERNELS[rt.kernel], splits=int(rt.splits), reduce=GEMM_REDUCES[rt.reduce],
                epilogue=int(rt.epilogue), ep_vec=bool(rt.ep_vec), thin_width=int(rt.thin_width),
                thin_is_a=bool(rt.thin_is_a))


def last_gemm_route() -> dict:
    """Where the calling thread's last krs_gemm ran (krs_gemm_last_route): kernel (a GEMM_KERNELS name, None when no
    launch was made), splits (1 = no split-K), reduce (a GEMM_REDUCES name), epilogue (the tile kernel's build: 0, 1, 2),
    ep_vec, and for gemm_thin_kernel thin_width (1, 4, 8, 16) and thin_is_a.  A diagnostic for tests: it reads a host-side
    record, no device sync."""
    rt = L.GemmRoute()
    L.lib().krs_gemm_last_route(C.byref(rt))
    return _route_dict(rt)


def _schedule_set(rt) -> frozenset:
    names = ((L.GEMM_SCHED_LDS_LANDING, "lds_landing"), (L.GEMM_SCHED_STAGGER, "stagger"), (L.GEMM_SCHED_X_IS_X0, "x_is_x0"))
    return frozenset(name for bit, name in names if rt.schedule & bit)


def last_gemm_schedule() -> frozenset:
    """The epilogue schedule of the calling thread's last krs_gemm (the `schedule` field of krs_gemm_last_route): a subset
    of {"lds_landing", "stagger", "x_is_x0"}, empty off gemm_pp64_kernel's cross / residual builds and under
    KRS_GEMM_OPT_EPI_SCHEDULE 0.  Kept out of last_gemm_route(): the record of WHERE a product ran does not depend on
    the schedule option."""
    rt = L.GemmRoute()
    L.lib().krs_gemm_last_route(C.byref(rt))
    return _schedule_set(rt)


def plan_gemm_schedule(a, lda, a_is_km, b, ldb, b_is_nk, c, ldc, m, n, k, in_dtype, out_dtype, epilogue=None,
                       workspace_bytes=0) -> frozenset:
    """last_gemm_schedule() of the call plan_gemm_route() describes, from krs_gemm_plan_route (no GPU)."""
    rt = L.GemmRoute()
    L.lib().krs_gemm_plan_route(a, lda, int(a_is_km), b, ldb, int(b_is_nk), c, ldc, m, n, k, in_dtype, out_dtype,
                                C.byref(epilogue) if epilogue is not None else None, int(workspace_bytes), C.byref(rt))
    return _schedule_set(rt)


def plan_gemm_route(a, lda, a_is_km, b, ldb, b_is_nk, c, ldc, m, n, k, in_dtype, out_dtype, epilogue=None,
                    workspace_bytes=0):
    """(status, route) a krs_gemm with these arguments would have (krs_gemm_plan_route; needs no GPU): a, b, c are
    addresses (ints: only their alignment is read), epilogue a GemmEpilogue or None; status is what krs_gemm returns
    before its first launch, route the dict of last_gemm_route()."""
    rt = L.GemmRoute()
    rc = L.lib().krs_gemm_plan_route(a, lda, int(a_is_km), b, ldb, int(b_is_nk), c, ldc, m, n, k, in_dtype, out_dtype,
                                     C.byref(epilogue) if epilogue is not None else None, int(workspace_bytes), C.byref(rt))
    return int(rc), _route_dict(rt)


# ---- K18: Dense / FeatureCross products in int8 -----------------------------------------------------------------------
GEMM_Q8_KERNELS = {0: None, 1: "generic", 2: "tile128", 3: "ring"}


def _q8_route_dict(rt) -> dict:
    return dict(kernel=GEMM_Q8_KERNELS[rt.kernel], ep_vec=bool(rt.ep_vec), k_tail=bool(rt.k_tail), epilogue=int(rt.epilogue))


def last_gemm_q8_route() -> dict:
    """Where the calling thread's last krs_gemm_q8 ran (krs_gemm_q8_last_route): kernel (a GEMM_Q8_KERNELS name, None when
    no launch was made), ep_vec, k_tail, epilogue (the ring's build: 0 general, 1 cross).  Reads a host-side record, no
    device sync."""
    rt = L.GemmQ8Route()
    L.lib().krs_gemm_q8_last_route(C.byref(rt))
    return _q8_route_dict(rt)


def plan_gemm_q8_route(aq, lda, astep, wq, ldw, wstep, c, ldc, m, n, k, out_dtype, epilogue=None):
    """(status, route) a krs_gemm_q8 with these arguments would have (krs_gemm_q8_plan_route; needs no GPU): the operands
    are addresses (ints: only their alignment and nullness are read), epilogue a GemmEpilogue or None."""
    rt = L.GemmQ8Route()
    rc = L.lib().krs_gemm_q8_plan_route(aq, lda, astep, wq, ldw, wstep, c, ldc, m, n, k, out_dtype,
                                        C.byref(epilogue) if epilogue is not None else None, C.byref(rt))
    return int(rc), _q8_route_dict(rt)


def gemm_q8_prequantized(aq: torch.Tensor, astep: torch.Tensor, wq: torch.Tensor, wstep: torch.Tensor, *,
                         bias: torch.Tensor | None = None, act: int = L.ACT_NONE, x0: torch.Tensor | None = None,
                         x_res: torch.Tensor | None = None, diag_scale: float = 0.0,
                         out_dtype: torch.dtype = torch.float32, u_out: bool = False, r: torch.Tensor | None = None,
                         beta: float = 1.0, out: torch.Tensor | None = None):
    """krs_gemm_q8 on operands that are int8 already: aq [M, K] with astep [M], wq [N, K] with wstep [N] (row strides
    taken from the tensors).  Returns (C, u_or_None)."""
    aq, wq = L.rowmajor(aq, "gemm_q8 aq"), L.rowmajor(wq, "gemm_q8 wq")
    if aq.dtype != torch.int8 or wq.dtype != torch.int8:
        raise L.KrsError("gemm_q8: aq and wq must be int8")
    (m, k), (n, kw) = aq.shape, wq.shape
    if k != kw or tuple(astep.shape) != (m,) or tuple(wstep.shape) != (n,):
        raise L.KrsError(f"gemm_q8: shapes do not fit (aq {tuple(aq.shape)}, astep {tuple(astep.shape)}, "
                         f"wq {tuple(wq.shape)}, wstep {tuple(wstep.shape)})")
    if astep.dtype != torch.float32 or wstep.dtype != torch.float32 or not astep.is_contiguous() or not wstep.is_contiguous():
        raise L.KrsError("gemm_q8: steps are contiguous float32 vectors")
    c = out if out is not None else torch.empty((m, n), dtype=out_dtype, device=aq.device)
    odt = c.dtype
    ep = L.GemmEpilogue()
    keep = []
    if bias is not None:
        bias = bias.float().contiguous()
        keep.append(bias)
        ep.bias = bias.data_ptr()
    ep.act = act
    ep.diag_scale = float(diag_scale or 0.0)
    if x0 is not None:
        x0, x_res = L.rowmajor(x0, "gemm_q8 x0"), L.rowmajor(x_res, "gemm_q8 x_res")
        if x0.stride(0) != x_res.stride(0):
            x0, x_res = x0.contiguous(), x_res.contiguous()
        if x0.dtype != odt or x_res.dtype != odt or tuple(x0.shape) != (m, n) or tuple(x_res.shape) != (m, n):
            raise L.KrsError("gemm_q8: x0 / x_res must have the output's shape and dtype")
        keep += [x0, x_res]
        ep.x0, ep.x, ep.ldx = x0.data_ptr(), x_res.data_ptr(), x0.stride(0) if m > 1 else n
    u = None
    if u_out:
        u = torch.empty((m, n), dtype=odt, device=aq.device)
        ep.u_out, ep.ldu = u.data_ptr(), n
    if r is not None:
        r = L.rowmajor(r, "gemm_q8 R")
        if r.dtype != odt or tuple(r.shape) != (m, n):
            raise L.KrsError("gemm_q8: R must have the output's shape and dtype")
        keep.append(r)
        ep.r, ep.ldr, ep.beta = r.data_ptr(), r.stride(0) if m > 1 else n, float(beta)
    name = "gemm_q8 %dx%dx%d" % (m, n, k) if probe.ACTIVE is not None else "gemm_q8"
    with probe.span(name, 2.0 * m * n * k):
        rc = L.lib().krs_gemm_q8(L.ptr(aq), aq.stride(0) if m > 1 else k, L.ptr(astep), L.ptr(wq),
                                 wq.stride(0) if n > 1 else k, L.ptr(wstep), L.ptr(c), c.stride(0) if m > 1 else n, m, n, k,
                                 L.fdtype(c), C.byref(ep), L.stream_ptr())
    L.check(rc, "krs_gemm_q8")
    return c, u


def gemm_q8(x: torch.Tensor, wq: torch.Tensor, wstep: torch.Tensor, *, bias: torch.Tensor | None = None,
            act: int = L.ACT_NONE, x0: torch.Tensor | None = None, x_res: torch.Tensor | None = None,
            diag_scale: float = 0.0, out_dtype: torch.dtype | None = None, u_out: bool = False):
    """C = epilogue(scale(quantize(x) . wq^T)) (include/krs.h, K18): x [M, K] fp32 / bf16 is quantized per row
    (embedding_ops.quantize_rows: Keras' dynamic input quantization), then ONE krs_gemm_q8 against the stored weight
    wq [N, K] int8 / wstep [N] with the fused bias, activation and cross form.  Two launches, no error word read, no host
    wait.  A row of x with a NaN or an infinity comes back as a row of NaNs.  Returns (C, u_or_None)."""
    from keras_rs_amd.embedding_ops import quantize_rows

    L.require_device(x, "gemm_q8 x")
    if x.dim() != 2:
        raise L.KrsError(f"gemm_q8: expected a matrix, got shape {tuple(x.shape)}")
    aq, astep = quantize_rows(x.contiguous())
    return gemm_q8_prequantized(aq, astep, wq, wstep, bias=bias, act=act, x0=x0, x_res=x_res, diag_scale=diag_scale,
                                out_dtype=out_dtype or x.dtype, u_out=u_out)


def colsum(a: torch.Tensor) -> torch.Tensor:
    a = L.rowmajor(a, "colsum")
    out = torch.empty(a.shape[1], dtype=torch.float32, device=a.device)
    ws, ws_ptr, ws_bytes = _colsum_ws(a.shape[0], a.shape[1], a.device)
    rc = L.lib().krs_colsum(L.ptr(a), a.stride(0), a.shape[0], a.shape[1],
                            L.fdtype(a), L.ptr(out), ws_ptr, ws_bytes, L.stream_ptr())
    L.check(rc, "krs_colsum")
    return out


def dense_act_bwd(g: torch.Tensor, y: torch.Tensor | None, act: int, want_dbias: bool = True):
    """(dz, dbias) of a Dense layer's bias + activation epilogue: dz = g * act'(y) from the saved output y
    (None without an activation), dbias = fp32 column sums of dz (None if not wanted); krs_dense_act_bwd."""
    g = L.rowmajor(g, "dense_act_bwd g")
    m, n = g.shape
    if y is not None:
        y = L.rowmajor(y, "dense_act_bwd y")
        if y.dtype != g.dtype or tuple(y.shape) != (m, n):
            raise L.KrsError("dense_act_bwd: y must have the shape and dtype of g")
    need_dz = act != L.ACT_NONE
    dz = torch.empty((m, n), dtype=g.dtype, device=g.device) if need_dz else None
    db = torch.empty(n, dtype=torch.float32, device=g.device) if want_dbias else None
    if need_dz or want_dbias:
        ws, ws_ptr, ws_bytes = _colsum_ws(m, n, g.device) if want_dbias else (None, None, 0)
        rc = L.lib().krs_dense_act_bwd(L.ptr(g), g.stride(0), L.ptr(y if need_dz else None),
                                       y.stride(0) if (y is not None and need_dz) else n,
                                       L.ptr(dz), n, L.ptr(db), m, n, act,
                                       L.fdtype(g), ws_ptr, ws_bytes, L.stream_ptr())
        L.check(rc, "krs_dense_act_bwd")
    return (dz if need_dz else g), db


def _cast_cache_key(w: torch.Tensor, dtype: torch.dtype):
    return (w.data_ptr(), w._version, tuple(w.shape), w.dtype, dtype)


def cast_transpose(w: torch.Tensor, dtype: torch.dtype, want_plain: bool = True, want_t: bool = True):
    """(w.to(dtype), w.to(dtype).t().contiguous()) of a 2-D weight in ONE launch (krs_cast_transpose); an output
    that is not wanted is None; the plain one is `w` itself when it already has the dtype and is row-major.

    Parameters remember that they were asked for (`_krs_cast_want`): `refresh_casts` -- called by
    keras_rs_amd.optim.Adagrad(prepare_casts=True) right behind its update -- then prepares the copies of ALL such
    weights for the next step in one launch and leaves them on the parameter (`_krs_cast`), where this function finds
    them ONCE (keyed by storage address, torch version, shape and dtypes)."""
    w = L.rowmajor(w, "cast_transpose")
    if isinstance(w, torch.nn.Parameter) and w.dtype != dtype and want_plain and want_t and w.is_contiguous():
        hit = getattr(w, "_krs_cast", None)
        if hit is not None:
            w._krs_cast = None        # one use: the first forward behind the optimizer step that prepared it
            if hit[0] == _cast_cache_key(w, dtype):
                return hit[1], hit[2]
        w._krs_cast_want = dtype
    rows, cols = w.shape
    plain = None
    if want_plain:
        plain = w if w.dtype == dtype else torch.empty((rows, cols), dtype=dtype, device=w.device)
    wt = torch.empty((cols, rows), dtype=dtype, device=w.device) if want_t else None
    write_plain = plain is not None and plain is not w
    if write_plain or want_t:
        rc = L.lib().krs_cast_transpose(L.ptr(w), rows, cols, w.stride(0),
                                        L.fdtype(w), L.ptr(plain) if write_plain else None,
                                        cols, L.ptr(wt), rows,
                                        L.fdtype(plain if plain is not None else wt), L.stream_ptr())
        L.check(rc, "krs_cast_transpose")
    return plain, wt


def refresh_casts(params) -> int:
    """Cast + transposed copies of every parameter that a layer has asked `cast_transpose` for, in ONE launch
    (krs_cast_transpose_many); to be called when the weights have just changed (behind the optimizer step: the C-ABI
    update does not go through torch, so the copies are keyed by storage and version AFTER it).  Returns the count."""
    todo = [p for p in params if getattr(p, "_krs_cast_want", None) is not None and p.is_cuda and p.dim() == 2
            and p.is_contiguous()]
    by_dtype: dict = {}
    for p in todo:
        by_dtype.setdefault((p.dtype, p._krs_cast_want), []).append(p)
    for (sdt, ddt), ps in by_dtype.items():
        n = len(ps)
        # the copies live in buffers that belong to the parameter and are rewritten in place, step after step (stream
        # order puts the rewrite behind the last reader: the backward pass of the step whose update precedes it) --
        # fixed addresses, so a step captured in a graph (torch.cuda.graph) keeps reading what its replays write
        plains, trans = [], []
        for p in ps:
            buf = getattr(p, "_krs_cast_buf", None)
            if buf is None or buf[0].dtype != ddt or buf[0].device != p.device or tuple(buf[0].shape) != tuple(p.shape):
                buf = p._krs_cast_buf = (torch.empty(tuple(p.shape), dtype=ddt, device=p.device),
                                         torch.empty((p.shape[1], p.shape[0]), dtype=ddt, device=p.device))
            plains.append(buf[0])
            trans.append(buf[1])
        ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
        rc = L.lib().krs_cast_transpose_many(
            n, ptrs(ps), (C.c_int64 * n)(*[p.shape[0] for p in ps]), (C.c_int64 * n)(*[p.shape[1] for p in ps]),
            L.fdtype(ps[0]), ptrs(plains), ptrs(trans), L.fdtype(plains[0]), L.stream_ptr())
        L.check(rc, "krs_cast_transpose_many")
        for p, a, b in zip(ps, plains, trans):
            # the C ABI rewrote these buffers behind torch's back: bump their version counters (host-side bookkeeping,
            # no kernel), so that a backward pass that still holds them from an EARLIER forward -- a retained graph,
            # two forwards before one backward across an optimizer step, a teacher / EMA forward -- fails autograd's
            # saved-tensor check loudly instead of differentiating against the new weights' copies
            torch.autograd.graph.increment_version(a)
            torch.autograd.graph.increment_version(b)
            p._krs_cast = (_cast_cache_key(p, ddt), a, b)
    return len(todo)


def _ptr_table(ts: Sequence[torch.Tensor]):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), (C.c_int64 * len(ts))(*[t.stride(0) for t in ts])


def dot_out_cols(n_feats: int, self_interaction: bool, skip_gather: bool) -> int:
    if skip_gather:
        return n_feats * n_feats
    return n_feats * (n_feats + 1) // 2 if self_interaction else n_feats * (n_feats - 1) // 2


def dot_interaction_fwd(feats: Sequence[torch.Tensor], self_interaction=False, skip_gather=False):
    feats = [L.rowmajor(f, "dot_interaction feature") for f in feats]
    batch, dim = feats[0].shape
    out = torch.empty((batch, dot_out_cols(len(feats), self_interaction, skip_gather)), dtype=feats[0].dtype,
                      device=feats[0].device)
    ptrs, lds = _ptr_table(feats)
    rc = L.lib().krs_dot_interaction_fwd(ptrs, lds, len(feats), batch, dim,
                                         L.fdtype(feats[0]), int(self_interaction),
                                         int(skip_gather), L.ptr(out), out.stride(0),
                                         L.stream_ptr())
    L.check(rc, "krs_dot_interaction_fwd")
    return out


def dot_interaction_bwd(feats: Sequence[torch.Tensor], grad_out: torch.Tensor, self_interaction=False,
                        skip_gather=False, into: torch.Tensor | None = None, accumulate_mask: int = 0):
    """Gradients of the features, as column views of one [B, F*dim] buffer.

    into / accumulate_mask (krs_dot_interaction_bwd_accumulate): `into` is a [B, F*dim] row-major matrix that
    already holds gradients of the features; feature f with bit f of the mask set is ADDED there (its returned
    gradient is None: the caller hands `into` on), the others are written to a fresh buffer as usual."""
    feats = [L.rowmajor(f, "dot_interaction feature") for f in feats]
    grad_out = L.rowmajor(grad_out, "dot_interaction grad")
    batch, dim = feats[0].shape
    n = len(feats)
    # one buffer, per-feature column views: a consumer that wants the gradients side by side
    # (the embedding backward) can take the buffer as it is
    if into is None or not accumulate_mask:
        accumulate_mask = 0
        gbuf = torch.empty((batch, n * dim), dtype=feats[0].dtype, device=feats[0].device)
        grads = [gbuf[:, i * dim:(i + 1) * dim] for i in range(n)]
        outs = grads
    else:
        if tuple(into.shape) != (batch, n * dim) or into.dtype != feats[0].dtype or into.stride(1) != 1:
            raise L.KrsError("dot_interaction_bwd: `into` must be a row-major [batch, F*dim] matrix of the features' dtype")
        fresh = [i for i in range(n) if not (accumulate_mask >> i) & 1]
        gbuf = torch.empty((batch, max(len(fresh), 1) * dim), dtype=feats[0].dtype, device=feats[0].device)
        slot = {f: k for k, f in enumerate(fresh)}
        outs = [into[:, i * dim:(i + 1) * dim] if i not in slot else gbuf[:, slot[i] * dim:(slot[i] + 1) * dim]
                for i in range(n)]
        grads = [None if i not in slot else outs[i] for i in range(n)]
    ptrs, lds = _ptr_table(feats)
    gptrs, glds = _ptr_table(outs)
    rc = L.lib().krs_dot_interaction_bwd_accumulate(ptrs, lds, n, batch, dim,
                                                    L.fdtype(feats[0]), int(self_interaction),
                                                    int(skip_gather), L.ptr(grad_out),
                                                    grad_out.stride(0), gptrs, glds,
                                                    int(accumulate_mask), L.stream_ptr())
    L.check(rc, "krs_dot_interaction_bwd_accumulate")
    return grads


DOT_KERNELS = {0: None, 1: "fwd_mfma", 2: "fwd_generic", 3: "fwd_block", 4: "bwd_mfma", 5: "bwd_valu", 6: "bwd_generic",
               7: "bwd_block"}
DOT_DTYPES = {L.F32: "f32", L.BF16: "bf16"}


def _dot_route_dict(rt) -> dict:
    d = {name: int(getattr(rt, name)) for name, _ in L.DotRoute._fields_}
    d["kernel"] = DOT_KERNELS[rt.kernel]
    d["dtype"] = DOT_DTYPES[rt.dtype] if rt.kernel else None
    return d


def dot_last_route() -> dict:
    """Where the calling thread's last krs_dot_interaction_* ran (krs_dot_interaction_last_route): the fields of
    krs_dot_route, kernel as a DOT_KERNELS name and dtype as "f32" / "bf16" (both None when no launch was made).  Reads a
    host-side record, no device sync."""
    rt = L.DotRoute()
    L.lib().krs_dot_interaction_last_route(C.byref(rt))
    return _dot_route_dict(rt)


def dot_plan_route(backward, feat_ptrs, lds, batch, dim, dtype, self_interaction, skip_gather, out, out_ld,
                   grad_ptrs=None, grad_lds=None, accumulate_mask=0):
    """(status, route) a krs_dot_interaction_fwd (backward false) / _bwd_accumulate with these arguments would have
    (krs_dot_interaction_plan_route; needs no GPU).  feat_ptrs / grad_ptrs are sequences of addresses (ints: only
    nullness and alignment are read) or None, lds / grad_lds the row strides, out the address of the output (forward) or
    of the incoming gradient; route is the dict of dot_last_route()."""
    def table(values, ctype):
        return None if values is None else (ctype * len(values))(*values)

    n = len(feat_ptrs) if feat_ptrs is not None else (len(lds) if lds is not None else 0)
    rt = L.DotRoute()
    rc = L.lib().krs_dot_interaction_plan_route(int(bool(backward)), table(feat_ptrs, C.c_void_p), table(lds, C.c_int64), n,
                                                int(batch), int(dim), int(dtype), int(self_interaction), int(skip_gather),
                                                out, int(out_ld), table(grad_ptrs, C.c_void_p),
                                                table(grad_lds, C.c_int64), int(accumulate_mask), C.byref(rt))
    return int(rc), _dot_route_dict(rt)


def mod_bucketize(ids: torch.Tensor, n_shards: int):
    """Stable grouping of ids by id % n_shards.  Returns (local_ids, perm, bucket_counts[int64])."""
    L.require_device(ids, "ids")
    ids = ids.contiguous().reshape(-1)
    nnz = ids.numel()
    local = torch.empty_like(ids)
    perm = torch.empty(nnz, dtype=torch.int32, device=ids.device)
    counts = torch.empty(n_shards, dtype=torch.int64, device=ids.device)
    wsb = L.lib().krs_mod_bucketize_workspace_bytes(nnz, n_shards)
    ws = torch.empty(max(int(wsb), 1), dtype=torch.uint8, device=ids.device)
    rc = L.lib().krs_mod_bucketize(L.ptr(ids), L.itype(ids), nnz, n_shards,
                                   L.ptr(local), L.ptr(perm), L.ptr(counts), L.ptr(ws), ws.numel(),
                                   L.stream_ptr())
    L.check(rc, "krs_mod_bucketize")
    return local, perm, counts


def bce_fwd_bwd(pred: torch.Tensor, labels: torch.Tensor, epsilon: float = 1e-7, grad_scale: float = 1.0,
                want_grad: bool = True):
    """(loss [] fp32, dL/dpred | None): binary cross-entropy of probabilities, mean reduction, forward and backward in
    one pass (krs_bce_fwd_bwd; keras.losses.BinaryCrossentropy() of examples/ml_perf/main.py:201-210)."""
    L.require_device(pred, "bce pred")
    p = pred.reshape(-1)
    if not p.is_contiguous():
        p = p.contiguous()
    y = labels.reshape(-1).to(torch.float32)
    if not y.is_contiguous():
        y = y.contiguous()
    if y.numel() != p.numel():
        raise L.KrsError(f"bce: {p.numel()} predictions but {y.numel()} labels")
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    dp = torch.empty_like(p) if want_grad else None
    scratch = torch.empty(64, dtype=torch.float32, device=pred.device)     # KRS_BCE_MAX_BLOCKS partial sums
    rc = L.lib().krs_bce_fwd_bwd(L.ptr(p), L.fdtype(p), L.ptr(y), p.numel(), epsilon,
                                 grad_scale, L.ptr(loss), L.ptr(dp), L.ptr(scratch), L.stream_ptr())
    L.check(rc, "krs_bce_fwd_bwd")
    return loss, (None if dp is None else dp.reshape(pred.shape))
