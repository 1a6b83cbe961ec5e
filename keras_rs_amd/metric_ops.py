"""Host side of K10 and K12: thin torch wrappers over krs_ranking_metrics, krs_ranking_metrics_accumulate and
krs_binary_metrics (include/krs.h).

All run on the current stream and never wait for the device, so a metric update can be captured in a HIP graph.
"""

from __future__ import annotations

import ctypes as C

import torch

from keras_rs_amd import _lib as L

MAX_LIST = L.MAX_LIST
MAX_SPECS = 8     # KRS_METRIC_MAX_SPECS
MAX_AUCS = 4            # KRS_BINARY_METRIC_MAX_AUCS
MAX_THRESHOLDS = 2048   # KRS_BINARY_METRIC_MAX_THRESHOLDS
BINARY_CHUNK = 1024     # KRS_BINARY_METRIC_CHUNK
METRIC_KINDS = {"dcg": 0, "ndcg": 1, "map": 2, "mrr": 3, "precision": 4, "recall": 5}   # krs_metric_kind


def _int_array(xs):
    return (C.c_int * len(xs))(*xs)


def _full(t, name, shape, device, dtype, what):
    if t is None:
        return None
    t = t.to(device=device, dtype=dtype).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise L.KrsError(f"{what}: {name} shape {tuple(t.shape)} where {tuple(shape)} is expected")
    return t


def ranking_metrics(specs, scores: torch.Tensor, labels: torch.Tensor, mask: torch.Tensor | None = None,
                    weights: torch.Tensor | float | None = None, *, gain: torch.Tensor | None = None,
                    discount: torch.Tensor | None = None, shuffle_ties: bool = False, seed: int = 0,
                    draw: torch.Tensor | None = None, want_order: bool = False):
    """Stage A.  specs: up to 8 (kind, k) with kind a METRIC_KINDS key and k an int or None.  scores [B, L] fp32 /
    bf16; labels, gain [B, L]; weights [B, L], [B] (one weight per list) or a Python number (every item's weight):
    the last two reach the kernel as they are, no [B, L] copy is made; mask [B, L] bool; discount [>= every DCG /
    NDCG k]; draw a device int64 tensor of one element (read, not advanced).  Returns (values [n, B], sums [5, B],
    order [B, L] int32 or None): see include/krs.h for each."""
    what = "ranking_metrics"
    scores = L.rowmajor(scores, what, "[batch, list] scores")
    b, n = scores.shape
    ld = scores.stride(0) if b > 1 else n
    dev = scores.device
    y = _full(labels, "labels", (b, n), dev, torch.float32, what)
    m = _full(mask, "mask", (b, n), dev, torch.bool, what)
    m = None if m is None else m.view(torch.uint8)
    w, w_strides, w_scalar = None, (0, 0), 1.0
    if isinstance(weights, (int, float)):
        w_scalar = float(weights)
    elif weights is not None and weights.dim() == 1:
        w, w_strides = _full(weights, "weights", (b,), dev, torch.float32, what), (1, 0)
    elif weights is not None:
        w, w_strides = _full(weights, "weights", (b, n), dev, torch.float32, what), (n, 1)
    g = _full(gain, "gain", (b, n), dev, torch.float32, what)
    d = None if discount is None else discount.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    if draw is not None and (draw.dtype != torch.int64 or draw.device != dev or draw.numel() != 1):
        raise L.KrsError(f"{what}: draw must be one int64 on {dev}")
    kinds = _int_array([METRIC_KINDS[kind] for kind, _ in specs])
    ks = _int_array([0 if k is None else int(k) for _, k in specs])
    values = torch.empty((len(specs), b), dtype=torch.float32, device=dev)
    sums = torch.empty((5, b), dtype=torch.float32, device=dev)
    order = torch.empty((b, n), dtype=torch.int32, device=dev) if want_order else None
    rc = L.lib().krs_ranking_metrics(L.ptr(scores), ld, L.fdtype(scores), L.ptr(y), L.ptr(m), L.ptr(w), w_strides[0],
                                     w_strides[1], w_scalar, L.ptr(g), L.ptr(d), 0 if d is None else d.numel(),
                                     int(bool(shuffle_ties)),
                                     int(seed) & (2 ** 64 - 1), L.ptr(draw), kinds, ks, len(specs), b, n,
                                     L.ptr(values), L.ptr(sums), L.ptr(order), L.stream_ptr())
    L.check(rc, "krs_ranking_metrics")
    return values, sums, order


def ranking_metrics_accumulate(kinds, values: torch.Tensor, sums: torch.Tensor, states, *,
                               draw: torch.Tensor | None = None, want_lists: bool = False):
    """Stage B.  kinds: the METRIC_KINDS keys of the rows of `values`; states: one fp32 device tensor {total, count}
    per row, updated in place; draw is advanced by one.  Returns (per-list values, per-list weights), both [n, B],
    or (None, None)."""
    what = "ranking_metrics_accumulate"
    L.require_device(values, what)
    n, b = values.shape
    if len(kinds) != n or len(states) != n or tuple(sums.shape) != (5, b):
        raise L.KrsError(f"{what}: {len(kinds)} kinds, {len(states)} states and sums {tuple(sums.shape)} for values "
                         f"{tuple(values.shape)}")
    for s in states:
        if s.dtype != torch.float32 or s.numel() != 2 or s.device != values.device or not s.is_contiguous():
            raise L.KrsError(f"{what}: a state must be two contiguous fp32 values on {values.device}")
    out_v = torch.empty_like(values) if want_lists else None
    out_w = torch.empty_like(values) if want_lists else None
    ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in states])
    ws_bytes = L.lib().krs_ranking_metrics_accumulate_workspace_bytes(b)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=values.device) if ws_bytes else None
    rc = L.lib().krs_ranking_metrics_accumulate(L.ptr(values), L.ptr(sums),
                                                _int_array([METRIC_KINDS[k] for k in kinds]), n, b, ptrs,
                                                L.ptr(out_v), L.ptr(out_w), L.ptr(draw), L.ptr(ws), ws_bytes,
                                                L.stream_ptr())
    L.check(rc, "krs_ranking_metrics_accumulate")
    return out_v, out_w


def binary_metrics(pred: torch.Tensor, labels: torch.Tensor, weights: torch.Tensor | float | None = None, *,
                   accuracy=None, aucs=()) -> None:
    """K12.  pred [n] fp32 / bf16 and labels [n] (any shapes of n elements); weights [n] or a Python number (every
    sample's weight).  accuracy: None or (threshold, state) with state two fp32 device values {total, count}.  aucs:
    up to 4 (thresholds, T, from_logits, state): thresholds None (the even set, T >= 3) or T ascending fp32 values
    on the device, state [4, T] fp32 (tp, fp, tn, fn).  Every state is updated in place."""
    what = "binary_metrics"
    L.require_device(pred, what)
    dev = pred.device
    pred = pred.contiguous().reshape(-1)
    n = pred.numel()
    y = _full(labels.reshape(-1), "labels", (n,), dev, torch.float32, what)
    w, w_scalar = None, 1.0
    if isinstance(weights, (int, float)):
        w_scalar = float(weights)
    elif weights is not None:
        w = _full(weights.reshape(-1), "weights", (n,), dev, torch.float32, what)
    aucs = list(aucs)

    def state_ok(s, numel):
        return s.dtype == torch.float32 and s.numel() == numel and s.device == dev and s.is_contiguous()

    acc_threshold, acc_state = 0.0, None
    if accuracy is not None:
        acc_threshold, acc_state = float(accuracy[0]), accuracy[1]
        if not state_ok(acc_state, 2):
            raise L.KrsError(f"{what}: the accuracy state must be two contiguous fp32 values on {dev}")
    for th, t, _, state in aucs:
        if not state_ok(state, 4 * int(t)):
            raise L.KrsError(f"{what}: an AUC state must be [4, {t}] contiguous fp32 on {dev}")
        if th is not None and (th.dtype != torch.float32 or th.numel() != int(t) or th.device != dev
                               or not th.is_contiguous()):
            raise L.KrsError(f"{what}: thresholds must be {t} contiguous fp32 values on {dev}")
    ts = _int_array([int(t) for _, t, _, _ in aucs])
    logits = _int_array([int(bool(fl)) for _, _, fl, _ in aucs])
    th_ptrs = (C.c_void_p * len(aucs))(*[L.ptr(th) for th, _, _, _ in aucs])
    st_ptrs = (C.c_void_p * len(aucs))(*[s.data_ptr() for _, _, _, s in aucs])
    ws_bytes = L.lib().krs_binary_metrics_workspace_bytes(n, len(aucs), ts)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    rc = L.lib().krs_binary_metrics(L.ptr(pred), L.fdtype(pred), L.ptr(y), L.ptr(w), w_scalar, n, acc_threshold,
                                    L.ptr(acc_state), len(aucs), th_ptrs, ts, logits, st_ptrs, L.ptr(ws), ws_bytes,
                                    L.stream_ptr())
    L.check(rc, "krs_binary_metrics")
