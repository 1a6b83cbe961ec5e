"""Host side of K8: thin torch wrappers over krs_topk_rows and krs_retrieval_topk (include/krs.h).

Both run on the current stream, allocate their workspace from torch's caching allocator and never wait for the
device, so a call can be captured into a HIP graph.
"""

from __future__ import annotations

import torch

from keras_rs_amd import _lib as L

# HardNegativeMining's boost (hard_negative_mining.py: MAX_FLOAT = finfo(float32).max / 100)
MAX_FLOAT = float(torch.finfo(torch.float32).max) / 100.0


def _rowmajor(t: torch.Tensor, what: str) -> torch.Tensor:
    L.require_device(t, what)
    if t.dim() != 2:
        raise L.KrsError(f"{what}: expected a matrix, got shape {tuple(t.shape)}")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        return t.contiguous()
    return t


def topk_rows_workspace_bytes(rows: int, cols: int, k: int) -> int:
    return int(L.lib().krs_topk_rows_workspace_bytes(rows, cols, k))


def retrieval_topk_workspace_bytes(b: int, n: int, d: int, k: int, dtype: torch.dtype) -> int:
    dt = L.BF16 if dtype == torch.bfloat16 else L.F32
    return int(L.lib().krs_retrieval_topk_workspace_bytes(b, n, d, k, dt))


def topk_rows(x: torch.Tensor, k: int, *, boost: torch.Tensor | None = None, boost_scale: float = 0.0,
              want_keys: bool = False):
    """Top-k column indices of each row of x [R, C] (fp32 / bf16) on the key x + boost_scale * boost (fp32), in the
    order key descending, index ascending.  Returns int32 indices [R, k], or (indices, fp32 keys) with want_keys."""
    x = _rowmajor(x, "topk_rows x")
    if boost is not None:
        boost = _rowmajor(boost, "topk_rows boost")
        if boost.dtype != x.dtype:
            boost = boost.to(x.dtype)
        if tuple(boost.shape) != tuple(x.shape):
            raise L.KrsError(f"topk_rows: boost shape {tuple(boost.shape)} differs from x {tuple(x.shape)}")
        if boost.stride(0) != x.stride(0):
            x, boost = x.contiguous(), boost.contiguous()
    rows, cols = x.shape
    idx = torch.empty((rows, k), dtype=torch.int32, device=x.device)
    keys = torch.empty((rows, k), dtype=torch.float32, device=x.device) if want_keys else None
    ws = torch.empty(max(1, topk_rows_workspace_bytes(rows, cols, k)), dtype=torch.uint8, device=x.device)
    rc = L.lib().krs_topk_rows(L.ptr(x), L.ptr(boost), boost_scale, x.stride(0) if rows else cols, L.fdtype(x), rows,
                               cols, k, L.ptr(idx), L.ptr(keys), L.ptr(ws), ws.numel(), L.stream_ptr())
    L.check(rc, "krs_topk_rows")
    return (idx, keys) if want_keys else idx


def retrieval_topk(query: torch.Tensor, candidates: torch.Tensor, k: int, *, ids: torch.Tensor | None = None,
                   want_scores: bool = True):
    """Top-k of query [B, D] . candidates [N, D]^T per query row (one dtype, fp32 / bf16).  Returns
    (scores [B, k] in the input dtype or None, int32 ids [B, k]); ids = ids[index] when ids (int32 [N]) is given."""
    q = _rowmajor(query, "retrieval_topk query")
    c = _rowmajor(candidates, "retrieval_topk candidates")
    if q.dtype != c.dtype:
        raise L.KrsError("retrieval_topk: query and candidates must share a dtype")
    b, d = q.shape
    n = c.shape[0]
    if c.shape[1] != d:
        raise L.KrsError(f"retrieval_topk: query width {d} differs from candidate width {c.shape[1]}")
    if ids is not None:
        L.require_device(ids, "retrieval_topk ids")
        if ids.dtype != torch.int32 or ids.dim() != 1 or ids.shape[0] != n or not ids.is_contiguous():
            raise L.KrsError("retrieval_topk: ids must be a contiguous int32 vector of one id per candidate")
    scores = torch.empty((b, k), dtype=q.dtype, device=q.device) if want_scores else None
    out_ids = torch.empty((b, k), dtype=torch.int32, device=q.device)
    ws = torch.empty(max(1, retrieval_topk_workspace_bytes(b, n, d, k, q.dtype)), dtype=torch.uint8, device=q.device)
    rc = L.lib().krs_retrieval_topk(L.ptr(q), q.stride(0) if b else d, L.ptr(c), c.stride(0),
                                    L.ptr(ids), L.fdtype(q), b, n, d,
                                    k, L.ptr(scores), L.ptr(out_ids), L.ptr(ws), ws.numel(),
                                    L.stream_ptr())
    L.check(rc, "krs_retrieval_topk")
    return scores, out_ids
