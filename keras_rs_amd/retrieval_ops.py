"""Host side of K8, K11, K13, K14, K15, K17, K21 and K23: thin torch wrappers over krs_topk_rows and krs_retrieval_topk (serving and
mining), over krs_retrieval_topk_q8 (serving from an int8 index), over krs_retrieval_ivf (serving from a partitioned
index), over krs_ah_encode, krs_retrieval_ivf_ah and krs_retrieval_rescore (serving from 4-bit codes, with exact rescoring), over krs_softmax_xent, krs_sampling_correction and krs_remove_accidental_hits (the training head on stored
scores), over krs_retrieval_xent_fwd / krs_retrieval_xent_bwd (the in-batch softmax loss that never stores the scores),
over krs_retrieval_mine (the same loss on each row's hardest negatives) and over krs_retrieval_rank (the positive's
rank among all candidates, for evaluation), all of include/krs.h.

All run on the current stream, allocate from torch's caching allocator and never wait for the device, so a call can
be captured into a HIP graph.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from keras_rs_amd import _lib as L

# HardNegativeMining's boost (hard_negative_mining.py: MAX_FLOAT = finfo(float32).max / 100)
MAX_FLOAT = float(torch.finfo(torch.float32).max) / 100.0
# RemoveAccidentalHits' constant (remove_accidental_hits.py: finfo(float32).smallest_normal / 100): 1.1754944e-40, a
# positive fp32 subnormal
SMALLEST_FLOAT = float(np.float32(np.finfo(np.float32).tiny) / np.float32(100.0))


def topk_rows_workspace_bytes(rows: int, cols: int, k: int) -> int:
    return int(L.lib().krs_topk_rows_workspace_bytes(rows, cols, k))


def retrieval_topk_workspace_bytes(b: int, n: int, d: int, k: int, dtype: torch.dtype) -> int:
    dt = L.BF16 if dtype == torch.bfloat16 else L.F32
    return int(L.lib().krs_retrieval_topk_workspace_bytes(b, n, d, k, dt))


def topk_rows(x: torch.Tensor, k: int, *, boost: torch.Tensor | None = None, boost_scale: float = 0.0,
              want_keys: bool = False):
    """Top-k column indices of each row of x [R, C] (fp32 / bf16) on the key x + boost_scale * boost (fp32), in the
    order key descending, index ascending.  Returns int32 indices [R, k], or (indices, fp32 keys) with want_keys."""
    x = L.rowmajor(x, "topk_rows x")
    if boost is not None:
        boost = L.rowmajor(boost, "topk_rows boost")
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
    q = L.rowmajor(query, "retrieval_topk query")
    c = L.rowmajor(candidates, "retrieval_topk candidates")
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


RETR_KERNELS = {0: None, 1: "fused", 2: "slab", 3: "rows"}               # KRS_RETR_*
RETR_VARIANTS = {0: None, 1: "topk", 2: "q8", 3: "mine", 4: "rows"}       # KRS_RETR_VARIANT_*
RETR_SELECTS = {0: None, 1: "lds", 2: "radix", 3: "radix_merge"}          # KRS_SELECT_*
_VARIANT_CODES = {name: code for code, name in RETR_VARIANTS.items() if name}


def _route_dict(rt) -> dict:
    d = {name: int(getattr(rt, name)) for name, _ in L.RetrievalRoute._fields_}
    d["kernel"] = RETR_KERNELS[rt.kernel]
    d["variant"] = RETR_VARIANTS[rt.variant]
    d["select"] = RETR_SELECTS[rt.select]
    return d


def last_route() -> dict:
    """Where the calling thread's last topk_rows / retrieval_topk / retrieval_topk_q8 / retrieval_mine ran
    (krs_retrieval_last_route): the fields of krs_retrieval_route with kernel, variant and select as names (None when no
    launch was made).  Reads a host-side record, no device sync."""
    rt = L.RetrievalRoute()
    L.lib().krs_retrieval_last_route(C.byref(rt))
    return _route_dict(rt)


def plan_route(variant: str, b: int, n: int, d: int, k: int, dtype: torch.dtype, *, ldq: int | None = None,
               ldc: int | None = None, q: int | None = 0x7F0000100000, c: int | None = 0x7E0000100000):
    """(status, route) the entry `variant` ("topk", "q8", "mine", "rows") would have with these arguments
    (krs_retrieval_plan_route; needs no GPU).  q and c are addresses (ints: only nullness and alignment are read), ldq /
    ldc the row strides (default: d, or n for "rows", where b is rows, n is cols and c stands for x); route is the dict
    of last_route().  KRS_RETRIEVAL_SLAB_BYTES is honoured as the entry honours it."""
    width = n if variant == "rows" else d
    rt = L.RetrievalRoute()
    rc = L.lib().krs_retrieval_plan_route(_VARIANT_CODES[variant], q, width if ldq is None else ldq, c,
                                          width if ldc is None else ldc, L.BF16 if dtype == torch.bfloat16 else L.F32,
                                          b, n, d, k, C.byref(rt))
    return int(rc), _route_dict(rt)


# ---- K17: the same over an int8 candidate index ------------------------------------------------------------------------
Q8_MAX_K = 128             # most results per query of krs_retrieval_topk_q8 (there is no slab path)
Q8_MAX_D = 512             # its widest embedding


def retrieval_topk_q8_workspace_bytes(b: int, n: int, d: int, k: int) -> int:
    return int(L.lib().krs_retrieval_topk_q8_workspace_bytes(b, n, d, k))


def retrieval_topk_q8(query: torch.Tensor, cand_q: torch.Tensor, cand_step: torch.Tensor, k: int, *,
                      ids: torch.Tensor | None = None, want_scores: bool = True,
                      err_flag: torch.Tensor | None = None):
    """Top-k of query [B, D] (fp32 / bf16) against the int8 index cand_q [N, D], cand_step [N] fp32 (the output of
    embedding_ops.quantize_rows): the query rows are quantized on the way in and the scores are
    (qq . cq) * cand_step * query_step (include/krs.h, K17).  Returns (scores [B, k] in the query's dtype or None, int32
    ids [B, k]); ids = ids[index] when ids (int32 [N]) is given.  err_flag (int32 [1], optional) gets
    FLAG_NONFINITE_ROW or-ed in when a query row holds a NaN or an infinity; such a row scores +0.0 everywhere."""
    q = L.rowmajor(query, "retrieval_topk_q8 query")
    c = L.rowmajor(cand_q, "retrieval_topk_q8 cand_q")
    L.require_device(cand_step, "retrieval_topk_q8 cand_step")
    if q.dtype not in (torch.float32, torch.bfloat16):
        raise L.KrsError(f"retrieval_topk_q8: unsupported query dtype {q.dtype} (float32 / bfloat16)")
    b, d = q.shape
    n = c.shape[0]
    if c.dtype != torch.int8 or c.shape[1] != d:
        raise L.KrsError(f"retrieval_topk_q8: cand_q must be int8 [N, {d}], got {c.dtype} {tuple(c.shape)}")
    if cand_step.dtype != torch.float32 or tuple(cand_step.shape) != (n,) or not cand_step.is_contiguous():
        raise L.KrsError("retrieval_topk_q8: cand_step must be a contiguous float32 vector of one step per candidate")
    if ids is not None:
        L.require_device(ids, "retrieval_topk_q8 ids")
        if ids.dtype != torch.int32 or ids.dim() != 1 or ids.shape[0] != n or not ids.is_contiguous():
            raise L.KrsError("retrieval_topk_q8: ids must be a contiguous int32 vector of one id per candidate")
    if err_flag is not None:
        L.require_device(err_flag, "retrieval_topk_q8 err_flag")
        if err_flag.dtype != torch.int32 or err_flag.numel() < 1:
            raise L.KrsError("retrieval_topk_q8: err_flag must be an int32 tensor of at least one element")
    scores = torch.empty((b, k), dtype=q.dtype, device=q.device) if want_scores else None
    out_ids = torch.empty((b, k), dtype=torch.int32, device=q.device)
    ws = torch.empty(max(1, retrieval_topk_q8_workspace_bytes(b, n, d, k)), dtype=torch.uint8, device=q.device)
    rc = L.lib().krs_retrieval_topk_q8(L.ptr(q), q.stride(0) if b > 1 else d, L.fdtype(q), L.ptr(c),
                                       c.stride(0) if n > 1 else d, L.ptr(cand_step), L.ptr(ids), b, n, d, k,
                                       L.ptr(scores), L.fdtype(q), L.ptr(out_ids), L.ptr(err_flag), L.ptr(ws),
                                       ws.numel(), L.stream_ptr())
    L.check(rc, "krs_retrieval_topk_q8")
    return scores, out_ids


# ---- K21: K8 over the best few leaves of a partitioned index ------------------------------------------------------------
IVF_MAX_K = 128            # most results per query of krs_retrieval_ivf (there is no slab path)
IVF_MAX_D = 512            # its widest embedding
IVF_MAX_PROBES = 128       # most leaves searched per query


def retrieval_ivf_workspace_bytes(b: int, n: int, d: int, leaves: int, probes: int, k: int, dtype: torch.dtype) -> int:
    dt = L.BF16 if dtype == torch.bfloat16 else L.F32
    return int(L.lib().krs_retrieval_ivf_workspace_bytes(b, n, d, leaves, probes, k, dt))


def _int32_vector(t: torch.Tensor, length: int, what: str) -> None:
    L.require_device(t, what)
    if t.dtype != torch.int32 or tuple(t.shape) != (length,) or not t.is_contiguous():
        raise L.KrsError(f"{what} must be a contiguous int32 vector of {length} entries, got {t.dtype} {tuple(t.shape)}")


def retrieval_ivf(query: torch.Tensor, centroids: torch.Tensor, rows: torch.Tensor, leaf_offsets: torch.Tensor,
                  row_index: torch.Tensor, k: int, probes: int, *, ids: torch.Tensor | None = None,
                  want_scores: bool = True, want_leaves: bool = False):
    """Top-k of query [B, D] over the candidates of its `probes` best leaves (include/krs.h, K21).  centroids
    [leaves, D] and rows [N, D] (the candidates regrouped leaf by leaf) share the query's dtype (fp32 / bf16);
    leaf_offsets int32 [leaves + 1], row_index int32 [N] (original index of a stored row, ascending inside a leaf), ids
    int32 [N] by original index or None.  Returns (scores [B, k] in the input dtype or None, int32 ids [B, k]), and the
    probed leaves int32 [B, probes] as a third item with want_leaves.  A query whose leaves hold fewer than k candidates
    ends in id -1, score -inf."""
    q = L.rowmajor(query, "retrieval_ivf query")
    m = L.rowmajor(centroids, "retrieval_ivf centroids")
    c = L.rowmajor(rows, "retrieval_ivf rows")
    if q.dtype != c.dtype or q.dtype != m.dtype:
        raise L.KrsError("retrieval_ivf: query, centroids and rows must share a dtype")
    b, d = q.shape
    n, leaves = c.shape[0], m.shape[0]
    if c.shape[1] != d or m.shape[1] != d:
        raise L.KrsError(f"retrieval_ivf: query width {d} differs from the index width ({m.shape[1]} centroids, "
                         f"{c.shape[1]} rows)")
    _int32_vector(leaf_offsets, leaves + 1, "retrieval_ivf: leaf_offsets")
    _int32_vector(row_index, n, "retrieval_ivf: row_index")
    if ids is not None:
        _int32_vector(ids, n, "retrieval_ivf: ids")
    scores = torch.empty((b, k), dtype=q.dtype, device=q.device) if want_scores else None
    out_ids = torch.empty((b, k), dtype=torch.int32, device=q.device)
    out_leaves = torch.empty((b, probes), dtype=torch.int32, device=q.device) if want_leaves else None
    ws = torch.empty(max(1, retrieval_ivf_workspace_bytes(b, n, d, leaves, probes, k, q.dtype)), dtype=torch.uint8,
                     device=q.device)
    rc = L.lib().krs_retrieval_ivf(L.ptr(q), q.stride(0) if b > 1 else d, L.ptr(m), m.stride(0) if leaves > 1 else d,
                                   L.ptr(c), c.stride(0) if n > 1 else d, L.ptr(leaf_offsets), L.ptr(row_index),
                                   L.ptr(ids), L.fdtype(q), b, n, d, leaves, probes, k, L.ptr(scores), L.ptr(out_ids),
                                   L.ptr(out_leaves), L.ptr(ws), ws.numel(), L.stream_ptr())
    L.check(rc, "krs_retrieval_ivf")
    return (scores, out_ids, out_leaves) if want_leaves else (scores, out_ids)


# ---- K23: asymmetric hashing over K21's partition, and the reorder stage ---------------------------------------------------
AH_MAX_R = 128             # most candidates handed to the reorder stage
AH_BLOCK_DIMS = (2, 4, 8)  # dimensions per block


def ah_code_bytes(d: int, m: int) -> int:
    """Bytes of a code row: one nibble per block of m columns, rounded up to whole 4-byte words (0: unsupported d, m)."""
    return int(L.lib().krs_ah_code_bytes(d, m))


def _dt(dtype: torch.dtype) -> int:
    return L.BF16 if dtype == torch.bfloat16 else L.F32


def _codebooks(codebooks: torch.Tensor, d: int, what: str) -> int:
    """Checks codebooks bf16 [blocks, 16, m] against d; returns m."""
    L.require_device(codebooks, what)
    m = codebooks.shape[2] if codebooks.dim() == 3 else 0
    if (codebooks.dtype != torch.bfloat16 or m not in AH_BLOCK_DIMS or not codebooks.is_contiguous()
            or tuple(codebooks.shape) != (-(-d // m), 16, m)):
        raise L.KrsError(f"{what} must be contiguous bfloat16 [ceil({d} / m), 16, m] with m in {AH_BLOCK_DIMS}, got "
                         f"{codebooks.dtype} {tuple(codebooks.shape)}")
    return m


def _codes(codes: torch.Tensor, n: int, d: int, m: int, what: str) -> None:
    L.require_device(codes, what)
    if (codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[0] != n or codes.shape[1] != ah_code_bytes(d, m)
            or codes.stride(1) != 1 or (n > 1 and (codes.stride(0) < codes.shape[1] or codes.stride(0) % 4))):
        raise L.KrsError(f"{what} must be uint8 [{n}, {ah_code_bytes(d, m)}] with a row stride that is a multiple of 4, "
                         f"got {codes.dtype} {tuple(codes.shape)} strides {tuple(codes.stride())}")


def ah_encode(x: torch.Tensor, row_leaf: torch.Tensor, centroids: torch.Tensor, codebooks: torch.Tensor, *,
              row_index: torch.Tensor | None = None) -> torch.Tensor:
    """The 4-bit codes uint8 [N, ah_code_bytes(D, m)] of N stored rows (include/krs.h, K23): stored row s is
    x[row_index[s]] (x[s] without row_index; x [N, D] fp32 / bf16) and belongs to leaf row_leaf[s] (int32 [N]); what is
    coded is its residual against centroids[leaf] (the dtype of x), block by block against codebooks bf16
    [blocks, 16, m]: the nearest centre, the lowest code on a tie."""
    x = L.rowmajor(x, "ah_encode x")
    cen = L.rowmajor(centroids, "ah_encode centroids")
    if x.dtype != cen.dtype:
        raise L.KrsError("ah_encode: x and centroids must share a dtype")
    n, d = x.shape
    if cen.shape[1] != d:
        raise L.KrsError(f"ah_encode: x has {d} columns, centroids {cen.shape[1]}")
    m = _codebooks(codebooks, d, "ah_encode: codebooks")
    _int32_vector(row_leaf, n, "ah_encode: row_leaf")
    if row_index is not None:
        _int32_vector(row_index, n, "ah_encode: row_index")
    codes = torch.empty((n, ah_code_bytes(d, m)), dtype=torch.uint8, device=x.device)
    rc = L.lib().krs_ah_encode(L.ptr(x), x.stride(0) if n > 1 else d, L.ptr(row_index), L.ptr(row_leaf), L.ptr(cen),
                               cen.stride(0) if cen.shape[0] > 1 else d, L.fdtype(x), L.ptr(codebooks), n, d,
                               cen.shape[0], m, L.ptr(codes), codes.shape[1], L.stream_ptr())
    L.check(rc, "krs_ah_encode")
    return codes


def retrieval_rescore_workspace_bytes(b: int, r: int, k: int) -> int:
    return int(L.lib().krs_retrieval_rescore_workspace_bytes(b, r, k))


def retrieval_rescore(query: torch.Tensor, rows: torch.Tensor, idx: torch.Tensor, k: int, *,
                      ids: torch.Tensor | None = None, want_scores: bool = True):
    """The k best of each query's listed candidates by exact score (include/krs.h, K23): idx int32 [B, R] holds
    candidate indices into rows [N, D] (the query's dtype), -1 is padding.  Returns (scores [B, k] in the input dtype or
    None, int32 ids [B, k]) in BruteForceRetrieval's order, with K8's score bits; -1 / -inf where fewer than k are real."""
    q = L.rowmajor(query, "retrieval_rescore query")
    c = L.rowmajor(rows, "retrieval_rescore rows")
    if q.dtype != c.dtype:
        raise L.KrsError("retrieval_rescore: query and rows must share a dtype")
    b, d = q.shape
    n = c.shape[0]
    if c.shape[1] != d:
        raise L.KrsError(f"retrieval_rescore: query width {d} differs from row width {c.shape[1]}")
    L.require_device(idx, "retrieval_rescore idx")
    if idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != b or (idx.shape[1] > 1 and idx.stride(1) != 1):
        raise L.KrsError(f"retrieval_rescore: idx must be int32 [{b}, R] with contiguous rows, got {idx.dtype} "
                         f"{tuple(idx.shape)}")
    r = idx.shape[1]
    if ids is not None:
        _int32_vector(ids, n, "retrieval_rescore: ids")
    scores = torch.empty((b, k), dtype=q.dtype, device=q.device) if want_scores else None
    out_ids = torch.empty((b, k), dtype=torch.int32, device=q.device)
    ws = torch.empty(max(1, retrieval_rescore_workspace_bytes(b, r, k)), dtype=torch.uint8, device=q.device)
    rc = L.lib().krs_retrieval_rescore(L.ptr(q), q.stride(0) if b > 1 else d, L.ptr(c), c.stride(0) if n > 1 else d,
                                       L.ptr(idx), idx.stride(0) if b > 1 else r, L.ptr(ids), L.fdtype(q), b, n, d, r, k,
                                       L.ptr(scores), L.ptr(out_ids), L.ptr(ws), ws.numel(), L.stream_ptr())
    L.check(rc, "krs_retrieval_rescore")
    return scores, out_ids


def retrieval_ivf_ah_workspace_bytes(b: int, n: int, d: int, leaves: int, probes: int, k: int, r: int, m: int,
                                     reorder: bool, dtype: torch.dtype) -> int:
    return int(L.lib().krs_retrieval_ivf_ah_workspace_bytes(b, n, d, leaves, probes, k, r, m, int(reorder), _dt(dtype)))


def retrieval_ivf_ah(query: torch.Tensor, centroids: torch.Tensor, codebooks: torch.Tensor, codes: torch.Tensor,
                     leaf_offsets: torch.Tensor, row_index: torch.Tensor, k: int, probes: int, *,
                     rows: torch.Tensor | None = None, num_reordering_candidates: int | None = None,
                     ids: torch.Tensor | None = None, want_scores: bool = True, want_leaves: bool = False):
    """Top-k of query [B, D] over the 4-bit codes of its `probes` best leaves (include/krs.h, K23).  centroids
    [leaves, D] share the query's dtype; codebooks bf16 [blocks, 16, m]; codes uint8 [N, ah_code_bytes(D, m)] in stored
    order; leaf_offsets, row_index and ids as retrieval_ivf's.  Without `rows` the scores are AH scores,
    q . decode(code) + q . centroid.  With rows [N, D] (ORIGINAL order, the query's dtype) the best
    `num_reordering_candidates` (default k) by AH score are rescored exactly and the k best of those returned.  Returns
    retrieval_ivf's tuple."""
    q = L.rowmajor(query, "retrieval_ivf_ah query")
    cen = L.rowmajor(centroids, "retrieval_ivf_ah centroids")
    if q.dtype != cen.dtype:
        raise L.KrsError("retrieval_ivf_ah: query and centroids must share a dtype")
    b, d = q.shape
    leaves, n = cen.shape[0], codes.shape[0]
    if cen.shape[1] != d:
        raise L.KrsError(f"retrieval_ivf_ah: query width {d} differs from the centroids' {cen.shape[1]}")
    m = _codebooks(codebooks, d, "retrieval_ivf_ah: codebooks")
    _codes(codes, n, d, m, "retrieval_ivf_ah: codes")
    _int32_vector(leaf_offsets, leaves + 1, "retrieval_ivf_ah: leaf_offsets")
    _int32_vector(row_index, n, "retrieval_ivf_ah: row_index")
    if ids is not None:
        _int32_vector(ids, n, "retrieval_ivf_ah: ids")
    r = k if num_reordering_candidates is None else num_reordering_candidates
    c = None
    if rows is not None:
        c = L.rowmajor(rows, "retrieval_ivf_ah rows")
        if c.dtype != q.dtype or tuple(c.shape) != (n, d):
            raise L.KrsError(f"retrieval_ivf_ah: rows must be {q.dtype} [{n}, {d}], got {c.dtype} {tuple(c.shape)}")
    elif r != k:
        raise L.KrsError("retrieval_ivf_ah: num_reordering_candidates needs the float rows")
    scores = torch.empty((b, k), dtype=q.dtype, device=q.device) if want_scores else None
    out_ids = torch.empty((b, k), dtype=torch.int32, device=q.device)
    out_leaves = torch.empty((b, probes), dtype=torch.int32, device=q.device) if want_leaves else None
    ws = torch.empty(max(1, retrieval_ivf_ah_workspace_bytes(b, n, d, leaves, probes, k, r, m, c is not None, q.dtype)),
                     dtype=torch.uint8, device=q.device)
    rc = L.lib().krs_retrieval_ivf_ah(L.ptr(q), q.stride(0) if b > 1 else d, L.ptr(cen),
                                      cen.stride(0) if leaves > 1 else d, L.ptr(codebooks), m, L.ptr(codes),
                                      codes.stride(0) if n > 1 else codes.shape[1], L.ptr(leaf_offsets), L.ptr(row_index),
                                      L.ptr(c), 0 if c is None else (c.stride(0) if n > 1 else d), L.ptr(ids),
                                      L.fdtype(q), b, n, d, leaves, probes, k, r, L.ptr(scores), L.ptr(out_ids),
                                      L.ptr(out_leaves), L.ptr(ws), ws.numel(), L.stream_ptr())
    L.check(rc, "krs_retrieval_ivf_ah")
    return (scores, out_ids, out_leaves) if want_leaves else (scores, out_ids)


# ---- K11: the training head ---------------------------------------------------------------------------------------
def _rows2d(t: torch.Tensor, what: str):
    """(a [rows, cols] view of t over its last axis whose rows are `ld` elements apart, ld): no copy where the last
    axis is contiguous and the rows are evenly spaced, a contiguous copy otherwise."""
    L.require_device(t, what)
    if t.dim() == 0:
        raise L.KrsError(f"{what}: expected at least one axis, got a scalar")
    cols = t.shape[-1]
    if t.dim() <= 2 and (cols == 1 or t.stride(-1) == 1) and (t.dim() == 1 or t.shape[0] <= 1 or t.stride(0) >= cols):
        t2 = t.reshape(1, cols) if t.dim() == 1 else t
        return t2, (t2.stride(0) if t2.shape[0] > 1 else cols)
    return t.contiguous().view(-1, cols), cols


def _float_logits(logits: torch.Tensor) -> torch.Tensor:
    return logits if logits.dtype in (torch.float32, torch.bfloat16) else logits.to(torch.float32)


def sampling_correction(logits: torch.Tensor, probs: torch.Tensor, epsilon: float = 1e-6) -> torch.Tensor:
    """logits - log(clip(probs, epsilon, 1)) in the logits' dtype (fp32 / bf16, computed in fp32).  probs' shape is
    the last probs.dim() axes of logits': it is broadcast over the leading ones inside the kernel."""
    L.require_device(probs, "sampling_correction probs")
    x, ld = _rows2d(_float_logits(logits), "sampling_correction logits")
    rows, cols = x.shape
    if probs.dim() > logits.dim() or tuple(probs.shape) != tuple(logits.shape[logits.dim() - probs.dim():]) \
            or probs.dim() == 0:
        raise L.KrsError(f"sampling_correction: probs shape {tuple(probs.shape)} is not the last axes of logits "
                         f"{tuple(logits.shape)}")
    p = probs.to(torch.float32).contiguous().view(-1, cols)
    out = torch.empty((rows, cols), dtype=x.dtype, device=x.device)
    rc = L.lib().krs_sampling_correction(L.ptr(x), ld, L.fdtype(x), L.ptr(p), max(1, p.shape[0]), float(epsilon),
                                         rows, cols, L.ptr(out), cols, L.stream_ptr())
    L.check(rc, "krs_sampling_correction")
    return out.view(logits.shape)


def remove_accidental_hits(logits: torch.Tensor, labels: torch.Tensor, ids: torch.Tensor,
                           value: float = SMALLEST_FLOAT) -> torch.Tensor:
    """logits + ((ids == ids[argmax(labels)]) - labels) * value, row by row in fp32 with each operation rounded on its
    own, in the logits' dtype.  labels has logits' shape; ids' shape (int32 / int64) is its last ids.dim() axes."""
    L.require_device(labels, "remove_accidental_hits labels")
    L.require_device(ids, "remove_accidental_hits ids")
    if tuple(labels.shape) != tuple(logits.shape):
        raise L.KrsError(f"remove_accidental_hits: labels shape {tuple(labels.shape)} differs from logits "
                         f"{tuple(logits.shape)}")
    if ids.dim() == 0 or ids.dim() > logits.dim() or tuple(ids.shape) != tuple(logits.shape[logits.dim() - ids.dim():]):
        raise L.KrsError(f"remove_accidental_hits: ids shape {tuple(ids.shape)} is not the last axes of logits "
                         f"{tuple(logits.shape)}")
    x, ld = _rows2d(_float_logits(logits), "remove_accidental_hits logits")
    y, ldy = _rows2d(labels.to(torch.float32), "remove_accidental_hits labels")
    rows, cols = x.shape
    if ids.dtype not in (torch.int32, torch.int64):
        ids = ids.to(torch.int64)
    i2 = ids.contiguous().view(-1, cols)
    out = torch.empty((rows, cols), dtype=x.dtype, device=x.device)
    rc = L.lib().krs_remove_accidental_hits(L.ptr(x), ld, L.fdtype(x), L.ptr(y), ldy, L.ptr(i2), L.itype(i2),
                                            max(1, i2.shape[0]), float(value), rows, cols, L.ptr(out), cols,
                                            L.stream_ptr())
    L.check(rc, "krs_remove_accidental_hits")
    return out.view(logits.shape)


def softmax_xent(logits: torch.Tensor, labels: torch.Tensor | None = None, label_index: torch.Tensor | None = None, *,
                 label_smoothing: float = 0.0, g: torch.Tensor | None = None, g_scale: float = 1.0,
                 want_loss: bool = True, want_grad: bool = True):
    """Row softmax cross-entropy of logits [R, C] (fp32 / bf16) against dense labels [R, C] or label_index [R]
    (exactly one of them): (fp32 loss [R] or None, d(sum_r g_r loss_r)/dlogits [R, C] in logits' dtype or None) with
    g_r = g_scale * g[r] (g broadcast to [R]; None = g_scale)."""
    if logits.dim() != 2:
        raise L.KrsError(f"softmax_xent: expected [rows, cols] logits, got shape {tuple(logits.shape)}")
    if (labels is None) == (label_index is None):
        raise L.KrsError("softmax_xent: give exactly one of labels and label_index")
    x, ld = _rows2d(logits, "softmax_xent logits")
    rows, cols = x.shape
    y, ldy, idx = None, 0, None
    if labels is not None:
        if tuple(labels.shape) != (rows, cols):
            raise L.KrsError(f"softmax_xent: labels shape {tuple(labels.shape)} differs from logits {(rows, cols)}")
        y, ldy = _rows2d(labels.to(torch.float32), "softmax_xent labels")
    else:
        L.require_device(label_index, "softmax_xent label_index")
        if tuple(label_index.shape) != (rows,):
            raise L.KrsError(f"softmax_xent: label_index shape {tuple(label_index.shape)} is not ({rows},)")
        # (an index beyond int32 stays out of range after the clamp: it marks its row NaN like any other)
        idx = label_index if label_index.dtype == torch.int32 else label_index.clamp(-1, 2**31 - 1).to(torch.int32)
        idx = idx.contiguous()
    gw = None if g is None else g.to(device=x.device, dtype=torch.float32).expand((rows,)).contiguous()
    loss = torch.empty((rows,), dtype=torch.float32, device=x.device) if want_loss else None
    dx = torch.empty((rows, cols), dtype=x.dtype, device=x.device) if want_grad else None
    rc = L.lib().krs_softmax_xent(L.ptr(x), ld, L.fdtype(x), L.ptr(y), ldy, L.ptr(idx), float(label_smoothing),
                                  L.ptr(gw), float(g_scale), rows, cols, L.ptr(loss), L.ptr(dx), cols, L.stream_ptr())
    L.check(rc, "krs_softmax_xent")
    return loss, dx


class SoftmaxCrossentropyFn(torch.autograd.Function):
    """Softmax cross-entropy of logits [R, C] with its Keras reduction, in ranking_ops.RankingLossFn's scheme: a scalar
    reduction knows every row's share g = weight / divisor of the result before the launch and takes loss and gradient
    from ONE launch, the backward only scales that gradient by the incoming scalar; reduction "none" computes the
    losses alone and its backward runs a second launch with g = upstream * weight.  `weight` is None, a scalar tensor
    or [R]; exactly one of `labels` [R, C] and `index` [R] is a tensor."""

    @staticmethod
    def forward(ctx, logits, labels, index, weight, label_smoothing, reduction):
        ctx.meta = (label_smoothing, reduction)
        if reduction == "none":
            v, _ = softmax_xent(logits, labels, index, label_smoothing=label_smoothing, want_grad=False)
            ctx.save_for_backward(logits, labels, index, weight)
            return v if weight is None else v * weight
        rows = logits.shape[0]
        g, scale = weight, 1.0
        if reduction == "mean_with_sample_weight" and weight is not None:
            div = weight.expand((rows,)).sum()
            g = torch.where(div != 0, weight / div, torch.zeros_like(weight))   # divide_no_nan
        elif reduction != "sum":
            scale = 1.0 / rows if rows else 0.0
        v, dx = softmax_xent(logits, labels, index, label_smoothing=label_smoothing, g=g, g_scale=scale,
                             want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(dx)
        return (v.sum() if g is None else (v * g).sum()) * scale

    @staticmethod
    def backward(ctx, up):
        label_smoothing, reduction = ctx.meta
        if reduction != "none":
            (dx,) = ctx.saved_tensors
            return (dx.float() * up).to(dx.dtype), None, None, None, None, None
        logits, labels, index, weight = ctx.saved_tensors
        g = up.to(torch.float32)
        if weight is not None:
            g = g * weight
        _, dx = softmax_xent(logits, labels, index, label_smoothing=label_smoothing, g=g, want_loss=False)
        return dx, None, None, None, None, None


class _LogitCorrectionFn(torch.autograd.Function):
    """A K11 logit correction: out = logits + (a term that does not depend on the logits), so the backward hands the
    upstream gradient to the logits unchanged and nothing to the other operands."""

    @staticmethod
    def forward(ctx, logits, op, *operands):
        ctx.in_dtype, ctx.n_operands = logits.dtype, len(operands)
        return op(logits, *operands)

    @staticmethod
    def backward(ctx, up):
        return (up.to(ctx.in_dtype), None) + (None,) * ctx.n_operands


def corrected(op, logits: torch.Tensor, *operands):
    """op(logits, *operands) (sampling_correction or remove_accidental_hits) with the identity gradient to logits."""
    return _LogitCorrectionFn.apply(logits, op, *operands)


# ---- K13: the in-batch softmax loss from the embeddings, scores never stored -----------------------------------------
SLAB_BYTES = 256 << 20     # default budget of the slab path's fp32 score slab
XENT_MAX_D = 256           # widest embedding of the fused kernels (bf16 only)


def retrieval_xent_workspace_bytes(b: int, n: int, d: int, dtype: torch.dtype = torch.bfloat16) -> int:
    dt = L.BF16 if dtype == torch.bfloat16 else L.F32
    return int(L.lib().krs_retrieval_xent_workspace_bytes(b, n, d, dt))


def _xent_operands(query, candidates, positive_index, cand_bias, cand_ids):
    """The operands of K13 checked and in the form the C ABI takes: (q, c, pos int32 [B] or None, bias fp32 [N] or
    None, ids int32 / int64 [N] or None)."""
    q = L.rowmajor(query, "retrieval_xent query")
    c = L.rowmajor(candidates, "retrieval_xent candidates")
    if q.dtype != c.dtype or q.dtype not in (torch.float32, torch.bfloat16):
        raise L.KrsError(f"retrieval_xent: query ({q.dtype}) and candidates ({c.dtype}) must share a dtype, float32 or "
                         "bfloat16")
    b, d = q.shape
    n = c.shape[0]
    if c.shape[1] != d or n < 1 or d < 1:
        raise L.KrsError(f"retrieval_xent: query {tuple(q.shape)} against candidates {tuple(c.shape)}: the widths must "
                         "agree and there must be at least one candidate and one column")
    pos = bias = ids = None
    if positive_index is not None:
        L.require_device(positive_index, "retrieval_xent positive_index")
        if tuple(positive_index.shape) != (b,) or positive_index.dtype.is_floating_point:
            raise L.KrsError(f"retrieval_xent: positive_index must be {b} integers, got {tuple(positive_index.shape)} "
                             f"{positive_index.dtype}")
        # (an index beyond int32 stays out of range after the clamp: it marks its row NaN like any other)
        pos = positive_index if positive_index.dtype == torch.int32 else \
            positive_index.clamp(-1, 2**31 - 1).to(torch.int32)
        pos = pos.contiguous()
    if cand_bias is not None:
        L.require_device(cand_bias, "retrieval_xent cand_bias")
        if tuple(cand_bias.shape) != (n,):
            raise L.KrsError(f"retrieval_xent: cand_bias must have shape ({n},), got {tuple(cand_bias.shape)}")
        bias = cand_bias.detach().to(torch.float32).contiguous()
    if cand_ids is not None:
        L.require_device(cand_ids, "retrieval_xent cand_ids")
        if tuple(cand_ids.shape) != (n,) or cand_ids.dtype.is_floating_point:
            raise L.KrsError(f"retrieval_xent: cand_ids must be {n} integers, got {tuple(cand_ids.shape)} "
                             f"{cand_ids.dtype}")
        ids = cand_ids if cand_ids.dtype in (torch.int32, torch.int64) else cand_ids.to(torch.int64)
        ids = ids.contiguous()
    return q, c, pos, bias, ids


def _xent_workspace(b, n, d, device):
    size = retrieval_xent_workspace_bytes(b, n, d)
    return torch.empty(max(1, size), dtype=torch.uint8, device=device), size


def retrieval_xent_fwd(q, c, pos, bias, ids, hit_value: float, label_smoothing: float):
    """krs_retrieval_xent_fwd on checked operands: (fp32 loss [B], fp32 log-sum-exp [B])."""
    b, d = q.shape
    n = c.shape[0]
    loss = torch.empty((b,), dtype=torch.float32, device=q.device)
    lse = torch.empty((b,), dtype=torch.float32, device=q.device)
    ws, size = _xent_workspace(b, n, d, q.device)
    rc = L.lib().krs_retrieval_xent_fwd(L.ptr(q), q.stride(0) if b > 1 else d, L.ptr(c), c.stride(0) if n > 1 else d,
                                        L.fdtype(q), b, n, d, L.ptr(pos), L.ptr(bias), L.ptr(ids),
                                        L.itype(ids) if ids is not None else L.I32, float(hit_value),
                                        float(label_smoothing), L.ptr(loss), L.ptr(lse), L.ptr(ws), size,
                                        L.stream_ptr())
    L.check(rc, "krs_retrieval_xent_fwd")
    return loss, lse


def retrieval_xent_bwd(q, c, pos, bias, ids, hit_value: float, label_smoothing: float, lse, g, *, want_dq: bool = True,
                       want_dc: bool = True):
    """krs_retrieval_xent_bwd on checked operands with the per-row factor g (fp32 [B]): (dq, dc) in the inputs'
    dtype, None where not wanted."""
    b, d = q.shape
    n = c.shape[0]
    dq = torch.empty((b, d), dtype=q.dtype, device=q.device) if want_dq else None
    dc = torch.empty((n, d), dtype=c.dtype, device=c.device) if want_dc else None
    if b == 0:
        return dq, (None if dc is None else dc.zero_())
    ws, size = _xent_workspace(b, n, d, q.device)
    rc = L.lib().krs_retrieval_xent_bwd(L.ptr(q), q.stride(0) if b > 1 else d, L.ptr(c), c.stride(0) if n > 1 else d,
                                        L.fdtype(q), b, n, d, L.ptr(pos), L.ptr(bias), L.ptr(ids),
                                        L.itype(ids) if ids is not None else L.I32, float(hit_value),
                                        float(label_smoothing), L.ptr(lse), L.ptr(g), 1.0, L.ptr(dq), d, L.ptr(dc), d,
                                        L.ptr(ws), size, L.stream_ptr())
    L.check(rc, "krs_retrieval_xent_bwd")
    return dq, dc


# The slab path: the same loss from existing entry points only (krs_gemm with its bias epilogue for the sampling
# correction, krs_remove_accidental_hits, krs_softmax_xent), a slab of query rows at a time, everything in fp32.
def _slabs(b: int, n: int, slab_bytes: int):
    rows = max(1, min(b, int(slab_bytes) // (4 * n)))
    return [(r0, min(b, r0 + rows)) for r0 in range(0, b, rows)]


def _slab_scores(q32, c32, r0, r1, pos, bias, ids, hit_value):
    """(corrected fp32 scores [r1 - r0, N], int32 positives of the slab)"""
    from keras_rs_amd import dense_ops

    n = c32.shape[0]
    scores, _ = dense_ops.gemm(q32[r0:r1], c32, b_is_nk=True, out_dtype=torch.float32, bias=bias)
    idx = pos[r0:r1] if pos is not None else torch.arange(r0, r1, dtype=torch.int32, device=q32.device)
    if ids is not None:
        ok = (idx >= 0) & (idx < n)
        labels = torch.zeros((r1 - r0, n), dtype=torch.float32, device=q32.device)
        labels.scatter_(1, idx.clamp(0, n - 1).to(torch.int64)[:, None], ok.to(torch.float32)[:, None])
        scores = remove_accidental_hits(scores, labels, ids, hit_value)
    return scores, idx


def retrieval_xent_slab_fwd(q, c, pos, bias, ids, hit_value: float, label_smoothing: float,
                            slab_bytes: int = SLAB_BYTES) -> torch.Tensor:
    """The fp32 row losses [B] by the slab path."""
    b, n = q.shape[0], c.shape[0]
    q32, c32 = q.to(torch.float32), c.to(torch.float32)
    loss = torch.empty((b,), dtype=torch.float32, device=q.device)
    for r0, r1 in _slabs(b, n, slab_bytes):
        scores, idx = _slab_scores(q32, c32, r0, r1, pos, bias, ids, hit_value)
        loss[r0:r1], _ = softmax_xent(scores, label_index=idx, label_smoothing=label_smoothing, want_grad=False)
    return loss


def retrieval_xent_slab_bwd(q, c, pos, bias, ids, hit_value: float, label_smoothing: float, g,
                            slab_bytes: int = SLAB_BYTES):
    """(dq [B, D], dc [N, D]) in fp32 by the slab path: each slab's scores are recomputed, its logit gradient feeds
    two more krs_gemm calls, and dc is accumulated across slabs in fp32."""
    from keras_rs_amd import dense_ops

    b, d = q.shape
    n = c.shape[0]
    q32, c32 = q.to(torch.float32), c.to(torch.float32)
    dq = torch.empty((b, d), dtype=torch.float32, device=q.device)
    dc = None
    for r0, r1 in _slabs(b, n, slab_bytes):
        scores, idx = _slab_scores(q32, c32, r0, r1, pos, bias, ids, hit_value)
        _, dx = softmax_xent(scores, label_index=idx, label_smoothing=label_smoothing, g=g[r0:r1], want_loss=False)
        dense_ops.gemm(dx, c32, out=dq[r0:r1])
        dc, _ = dense_ops.gemm(dx, q32[r0:r1], a_is_km=True, r=dc)
    if dc is None:
        dc = torch.zeros((n, d), dtype=torch.float32, device=q.device)
    return dq, dc


class RetrievalXentFn(torch.autograd.Function):
    """The in-batch softmax loss of query [B, D] against candidates [N, D] with its Keras reduction.  The forward keeps
    q, c, the log-sum-exp per row (fused path) and the small operands; the backward recomputes the scores with the
    per-row factor g = upstream * weight / divisor.  `weight` is None, a scalar tensor or [B]."""

    @staticmethod
    def forward(ctx, q, c, pos, bias, ids, weight, hit_value, label_smoothing, reduction, fused, slab_bytes):
        if fused:
            v, lse = retrieval_xent_fwd(q, c, pos, bias, ids, hit_value, label_smoothing)
        else:
            v, lse = retrieval_xent_slab_fwd(q, c, pos, bias, ids, hit_value, label_smoothing, slab_bytes), None
        rows = q.shape[0]
        g, scale = weight, 1.0
        if reduction == "mean_with_sample_weight" and weight is not None:
            div = weight.expand((rows,)).sum()
            g = torch.where(div != 0, weight / div, torch.zeros_like(weight))   # divide_no_nan
        elif reduction not in ("none", "sum"):
            scale = 1.0 / rows if rows else 0.0
        ctx.meta = (hit_value, label_smoothing, reduction, fused, slab_bytes, scale)
        ctx.save_for_backward(q, c, lse, pos, bias, ids, g)
        if reduction == "none":
            return v if weight is None else v * weight
        return (v.sum() if g is None else (v * g).sum()) * scale

    @staticmethod
    def backward(ctx, up):
        hit_value, label_smoothing, reduction, fused, slab_bytes, scale = ctx.meta
        q, c, lse, pos, bias, ids, g = ctx.saved_tensors
        rows = q.shape[0]
        gv = up.to(torch.float32) if scale == 1.0 else up.to(torch.float32) * scale
        if g is not None:
            gv = gv * g
        gv = gv.expand((rows,)).contiguous()
        want_dq, want_dc = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if fused:
            dq, dc = retrieval_xent_bwd(q, c, pos, bias, ids, hit_value, label_smoothing, lse, gv, want_dq=want_dq,
                                        want_dc=want_dc)
        else:
            dq, dc = retrieval_xent_slab_bwd(q, c, pos, bias, ids, hit_value, label_smoothing, gv, slab_bytes)
            dq, dc = (dq.to(q.dtype) if want_dq else None), (dc.to(c.dtype) if want_dc else None)
        return (dq, dc) + (None,) * 9


# ---- K14: the in-batch softmax loss on each row's positive and its k hardest negatives ----------------------------------
MINE_MAX_K = 128           # most negatives per row of the fused mining kernel
MINE_MAX_D = 512           # its widest embedding


def retrieval_mine_workspace_bytes(b: int, n: int, d: int, k: int, dtype: torch.dtype = torch.bfloat16) -> int:
    dt = L.BF16 if dtype == torch.bfloat16 else L.F32
    return int(L.lib().krs_retrieval_mine_workspace_bytes(b, n, d, k, dt))


def retrieval_mine(q, c, k: int, pos, bias, ids, hit_value: float):
    """krs_retrieval_mine on checked operands: (int32 indices [B, k] of the k hardest negatives of each row in the
    total order, their corrected fp32 scores [B, k], the positive's fp32 score [B], NaN for a positive outside
    [0, N))."""
    b, d = q.shape
    n = c.shape[0]
    idx = torch.empty((b, k), dtype=torch.int32, device=q.device)
    val = torch.empty((b, k), dtype=torch.float32, device=q.device)
    pos_score = torch.empty((b,), dtype=torch.float32, device=q.device)
    size = retrieval_mine_workspace_bytes(b, n, d, k, q.dtype)
    ws = torch.empty(max(1, size), dtype=torch.uint8, device=q.device)
    rc = L.lib().krs_retrieval_mine(L.ptr(q), q.stride(0) if b > 1 else d, L.ptr(c), c.stride(0) if n > 1 else d,
                                    L.fdtype(q), b, n, d, k, L.ptr(pos), L.ptr(bias), L.ptr(ids),
                                    L.itype(ids) if ids is not None else L.I32, float(hit_value), L.ptr(idx), L.ptr(val),
                                    L.ptr(pos_score), L.ptr(ws), ws.numel(), L.stream_ptr())
    L.check(rc, "krs_retrieval_mine")
    return idx, val, pos_score


def retrieval_mine_slab(q, c, k: int, pos, bias, ids, hit_value: float, slab_bytes: int = SLAB_BYTES):
    """What retrieval_mine returns, from existing entry points only: per slab of query rows the corrected fp32 scores
    (krs_gemm, krs_remove_accidental_hits), then HardNegativeMining's selection top_k(scores + labels * MAX_FLOAT,
    k + 1) by krs_topk_rows, whose first column is the positive."""
    b, n = q.shape[0], c.shape[0]
    q32, c32 = q.to(torch.float32), c.to(torch.float32)
    idx = torch.empty((b, k), dtype=torch.int32, device=q.device)
    val = torch.empty((b, k), dtype=torch.float32, device=q.device)
    pos_score = torch.empty((b,), dtype=torch.float32, device=q.device)
    for r0, r1 in _slabs(b, n, slab_bytes):
        scores, p = _slab_scores(q32, c32, r0, r1, pos, bias, ids, hit_value)
        ok = (p >= 0) & (p < n)
        p64 = p.clamp(0, n - 1).to(torch.int64)[:, None]
        labels = torch.zeros_like(scores).scatter_(1, p64, ok.to(torch.float32)[:, None])
        sel = topk_rows(scores, k + 1, boost=labels, boost_scale=MAX_FLOAT)
        # (a row without a positive has no boosted column: its k hardest candidates are the first k columns)
        neg = torch.where(ok[:, None], sel[:, 1:], sel[:, :k])
        idx[r0:r1] = neg
        val[r0:r1] = scores.gather(1, neg.to(torch.int64))
        pos_score[r0:r1] = torch.where(ok, scores.gather(1, p64)[:, 0], torch.full_like(scores[:, 0], float("nan")))
    return idx, val, pos_score


def _mined_bags(c):
    """The candidate matrix as the one table of a K1 / K2 call: one dense feature, combiner sum."""
    from keras_rs_amd import embedding_ops

    return embedding_ops.FusedBags([c.contiguous()], [(0, "sum", 0)])


class MinedRetrievalXentFn(torch.autograd.Function):
    """The in-batch softmax loss on the positive and the k hardest negatives of each row (include/krs.h, K14), with
    RetrievalXentFn's reduction scheme.  The forward keeps q, c, the index list [B, k + 1] (positive first) and the
    logits [B, k + 1]; the backward takes P = d(sum_i g_i loss_i)/dlogits from K11 (fp32, never rounded to bf16) and
    forms dq = sum_m P_im c[idx_im] with K1 and dc_j = sum_{idx_im = j} P_im q_i with K2's sort plan and dense form, or,
    on the slab path, scatters P into a zeroed slab of query rows and runs the slab path's two krs_gemm calls."""

    @staticmethod
    def forward(ctx, q, c, pos, bias, ids, weight, k, hit_value, label_smoothing, reduction, fused, slab_bytes):
        rows, n = q.shape[0], c.shape[0]
        if fused:
            idx, val, pos_score = retrieval_mine(q, c, k, pos, bias, ids, hit_value)
        else:
            idx, val, pos_score = retrieval_mine_slab(q, c, k, pos, bias, ids, hit_value, slab_bytes)
        logits = torch.cat((pos_score[:, None], val), dim=1)
        zeros = torch.zeros((rows,), dtype=torch.int32, device=q.device)
        v, _ = softmax_xent(logits, label_index=zeros, label_smoothing=label_smoothing, want_grad=False)
        bad = torch.isnan(pos_score)                      # (scores are finite: only a positive outside [0, N))
        v = torch.where(bad, pos_score, v)
        first = pos.clamp(0, n - 1) if pos is not None else \
            torch.arange(rows, dtype=torch.int32, device=q.device).clamp(max=n - 1)
        index = torch.cat((first[:, None], idx), dim=1)
        g, scale = weight, 1.0
        if reduction == "mean_with_sample_weight" and weight is not None:
            div = weight.expand((rows,)).sum()
            g = torch.where(div != 0, weight / div, torch.zeros_like(weight))   # divide_no_nan
        elif reduction not in ("none", "sum"):
            scale = 1.0 / rows if rows else 0.0
        ctx.meta = (label_smoothing, fused, slab_bytes, scale)
        ctx.save_for_backward(q, c, index, logits, g)
        if reduction == "none":
            return v if weight is None else v * weight
        return (v.sum() if g is None else (v * g).sum()) * scale

    @staticmethod
    def backward(ctx, up):
        from keras_rs_amd import dense_ops

        label_smoothing, fused, slab_bytes, scale = ctx.meta
        q, c, index, logits, g = ctx.saved_tensors
        rows, d = q.shape
        n, k1 = c.shape[0], index.shape[1]
        want_dq, want_dc = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dq = torch.empty((rows, d), dtype=q.dtype, device=q.device) if want_dq else None
        dc = torch.zeros((n, d), dtype=torch.float32, device=q.device) if want_dc else None
        if rows == 0:
            return (dq, None if dc is None else dc.to(c.dtype)) + (None,) * 10
        gv = up.to(torch.float32) if scale == 1.0 else up.to(torch.float32) * scale
        if g is not None:
            gv = gv * g
        gv = gv.expand((rows,)).contiguous()
        zeros = torch.zeros((rows,), dtype=torch.int32, device=q.device)
        _, P = softmax_xent(logits, label_index=zeros, label_smoothing=label_smoothing, g=gv, want_loss=False)
        # a row without a positive: NaN on its k mined candidates, and nothing on slot 0, whose index is a stand-in
        bad = torch.isnan(logits[:, :1])
        slot0 = torch.arange(k1, device=q.device)[None, :] == 0
        P = torch.where(bad, torch.where(slot0, torch.zeros_like(P), torch.full_like(P, float("nan"))), P)
        if fused:
            bags = _mined_bags(c)
            flat, w = index.reshape(-1), P.reshape(-1)
            if want_dq:
                bags.forward(flat, rows, hots=[k1], weights=w, out=dq)
            if want_dc:
                plan = bags.plan_backward(flat, rows, hots=[k1])
                bags.backward_dense(plan, q, rows, flat.numel(), hots=[k1], weights=w, out=[dc])
        else:
            q32, c32 = q.to(torch.float32), c.to(torch.float32)
            dq32 = torch.empty((rows, d), dtype=torch.float32, device=q.device)
            acc = None
            for r0, r1 in _slabs(rows, n, slab_bytes):
                dx = torch.zeros((r1 - r0, n), dtype=torch.float32, device=q.device)
                dx.scatter_add_(1, index[r0:r1].to(torch.int64), P[r0:r1])
                if want_dq:
                    dense_ops.gemm(dx, c32, out=dq32[r0:r1])
                if want_dc:
                    acc, _ = dense_ops.gemm(dx, q32[r0:r1], a_is_km=True, r=acc)
            dq = dq32.to(q.dtype) if want_dq else None
            dc = acc if want_dc else None
        return (dq, None if dc is None else dc.to(c.dtype)) + (None,) * 10


def _retrieval_xent_mined(query, candidates, positive_index, cand_bias, cand_ids, hit_value, label_smoothing, path,
                          sample_weight, reduction, slab_bytes, num_hard_negatives):
    if isinstance(num_hard_negatives, bool) or not isinstance(num_hard_negatives, (int, np.integer)) \
            or num_hard_negatives < 1:
        raise L.KrsError(f"retrieval_xent: num_hard_negatives must be an integer >= 1 or None, got "
                         f"{num_hard_negatives!r}")
    if path not in ("auto", "fused", "slab"):
        raise L.KrsError(f"retrieval_xent: path must be 'auto', 'fused' or 'slab', got {path!r}")
    if not 0.0 <= label_smoothing < 1.0:
        raise L.KrsError(f"retrieval_xent: label_smoothing {label_smoothing} outside [0, 1)")
    q, c, pos, bias, ids = _xent_operands(query, candidates, positive_index, cand_bias, cand_ids)
    n, d = c.shape
    k = min(int(num_hard_negatives), n - 1)
    if k == 0:     # one candidate: nothing to mine, the loss over (positive) alone is the unmined loss
        return retrieval_xent(query, candidates, positive_index=positive_index, cand_bias=cand_bias, cand_ids=cand_ids,
                              hit_value=hit_value, label_smoothing=label_smoothing, path=path,
                              sample_weight=sample_weight, reduction=reduction, slab_bytes=slab_bytes)
    fused = path == "fused" or (path == "auto" and k <= MINE_MAX_K and d <= MINE_MAX_D)
    w = None
    if sample_weight is not None:
        w = sample_weight.detach().to(device=q.device, dtype=torch.float32)
        if w.dim() > 0:
            w = w.expand((q.shape[0],)).contiguous()
    reduction = "none" if reduction is None else reduction
    return MinedRetrievalXentFn.apply(q, c, pos, bias, ids, w, k, float(hit_value), float(label_smoothing), reduction,
                                      fused, int(slab_bytes))



def retrieval_xent(query: torch.Tensor, candidates: torch.Tensor, *, positive_index: torch.Tensor | None = None,
                   cand_bias: torch.Tensor | None = None, cand_ids: torch.Tensor | None = None,
                   hit_value: float = SMALLEST_FLOAT, label_smoothing: float = 0.0, path: str = "auto",
                   sample_weight: torch.Tensor | None = None, reduction: str | None = "none",
                   slab_bytes: int = SLAB_BYTES, num_hard_negatives: int | None = None) -> torch.Tensor:
    """Softmax cross-entropy of the scores query [B, D] . candidates [N, D]^T + cand_bias (+ hit_value on the
    accidental hits given by cand_ids) against the positives positive_index (None: candidate i for query i), with
    gradients to both embeddings (include/krs.h, K13).  The [B, N] scores are never stored.

    path: "fused" -- the K13 kernels (bf16, D <= 256); "slab" -- krs_gemm + K11 on slabs of query rows whose fp32
    scores stay under slab_bytes, in fp32; "auto" -- fused wherever it is eligible, whatever the shape: its contract
    is memory, not speed.  reduction / sample_weight follow SoftmaxCrossentropyFn: "none" / None returns the fp32
    losses [B] (times the weight), the others a scalar.

    num_hard_negatives (an integer >= 1): the softmax runs over each row's positive and its k = min(num_hard_negatives,
    N - 1) highest-scoring other candidates only (include/krs.h, K14: HardNegativeMining in front of the loss, ties
    to the lowest index), and label_smoothing spreads over those k + 1 logits.  Then path "fused" is krs_retrieval_mine
    (fp32 or bf16, k <= 128, D <= 512), K11 on the [B, k + 1] logits, and K1 / K2 for the gradients; "slab" mines on
    slabs of stored fp32 scores with krs_topk_rows; "auto" is fused wherever it is eligible."""
    if num_hard_negatives is not None:
        return _retrieval_xent_mined(query, candidates, positive_index, cand_bias, cand_ids, hit_value, label_smoothing,
                                     path, sample_weight, reduction, slab_bytes, num_hard_negatives)
    if path not in ("auto", "fused", "slab"):
        raise L.KrsError(f"retrieval_xent: path must be 'auto', 'fused' or 'slab', got {path!r}")
    if not 0.0 <= label_smoothing < 1.0:
        raise L.KrsError(f"retrieval_xent: label_smoothing {label_smoothing} outside [0, 1)")
    q, c, pos, bias, ids = _xent_operands(query, candidates, positive_index, cand_bias, cand_ids)
    fused = path == "fused" or (path == "auto" and q.dtype == torch.bfloat16 and q.shape[1] <= XENT_MAX_D)
    w = None
    if sample_weight is not None:
        w = sample_weight.detach().to(device=q.device, dtype=torch.float32)
        if w.dim() > 0:
            w = w.expand((q.shape[0],)).contiguous()
    reduction = "none" if reduction is None else reduction
    return RetrievalXentFn.apply(q, c, pos, bias, ids, w, float(hit_value), float(label_smoothing), reduction, fused,
                                 int(slab_bytes))


# ---- K15: the positive's rank among all candidates, scores never stored -----------------------------------------------
def retrieval_rank_workspace_bytes(b: int, n: int, d: int, dtype: torch.dtype = torch.bfloat16) -> int:
    dt = L.BF16 if dtype == torch.bfloat16 else L.F32
    return int(L.lib().krs_retrieval_rank_workspace_bytes(b, n, d, dt))


def retrieval_rank_fused(q, c, pos, ids):
    """krs_retrieval_rank on checked operands: (int32 rank [B], fp32 score of the positive [B])."""
    b, d = q.shape
    n = c.shape[0]
    rank = torch.empty((b,), dtype=torch.int32, device=q.device)
    pos_score = torch.empty((b,), dtype=torch.float32, device=q.device)
    size = retrieval_rank_workspace_bytes(b, n, d, q.dtype)
    ws = torch.empty(max(1, size), dtype=torch.uint8, device=q.device)
    rc = L.lib().krs_retrieval_rank(L.ptr(q), q.stride(0) if b > 1 else d, L.ptr(c), c.stride(0) if n > 1 else d,
                                    L.fdtype(q), b, n, d, L.ptr(pos), L.ptr(ids),
                                    L.itype(ids) if ids is not None else L.I32, L.ptr(rank), L.ptr(pos_score),
                                    L.ptr(ws), size, L.stream_ptr())
    L.check(rc, "krs_retrieval_rank")
    return rank, pos_score


def rank_in_scores(scores: torch.Tensor, pos: torch.Tensor, ids: torch.Tensor | None = None):
    """(int32 rank [R], fp32 score of the positive [R]) from stored fp32 scores [R, N] with plain torch ops (any
    device): the number of candidates other than pos that precede it in K8's total order -- score descending, then
    index ascending, -0.0 as +0.0, NaN above +inf -- leaving out those that carry the positive's id.  A pos outside
    [0, N) gives -1 and NaN."""
    n = scores.shape[1]
    ok = (pos >= 0) & (pos < n)
    p64 = pos.clamp(0, n - 1).to(torch.int64)[:, None]
    sp = scores.gather(1, p64)
    nan_s, nan_p = torch.isnan(scores), torch.isnan(sp)
    above = (scores > sp) | (nan_s & ~nan_p)
    level = (scores == sp) | (nan_s & nan_p)
    col = torch.arange(n, device=scores.device)[None, :]
    counts = (above | (level & (col < p64))) & (col != p64)
    if ids is not None:
        ids64 = ids.to(torch.int64)
        counts &= ids64[None, :] != ids64[p64[:, 0]][:, None]
    rank = torch.where(ok, counts.sum(dim=1), torch.full_like(p64[:, 0], -1)).to(torch.int32)
    return rank, torch.where(ok, sp[:, 0], torch.full_like(sp[:, 0], float("nan")))


def retrieval_rank_slab(q, c, pos, ids, slab_bytes: int = SLAB_BYTES):
    """What retrieval_rank_fused returns, from krs_gemm into an fp32 slab of query rows and rank_in_scores on it."""
    from keras_rs_amd import dense_ops

    b, n = q.shape[0], c.shape[0]
    q32, c32 = q.to(torch.float32), c.to(torch.float32)
    rank = torch.empty((b,), dtype=torch.int32, device=q.device)
    pos_score = torch.empty((b,), dtype=torch.float32, device=q.device)
    for r0, r1 in _slabs(b, n, slab_bytes):
        scores, _ = dense_ops.gemm(q32[r0:r1], c32, b_is_nk=True, out_dtype=torch.float32)
        idx = pos[r0:r1] if pos is not None else torch.arange(r0, r1, dtype=torch.int32, device=q.device)
        rank[r0:r1], pos_score[r0:r1] = rank_in_scores(scores, idx, ids)
    return rank, pos_score


def retrieval_rank(query: torch.Tensor, candidates: torch.Tensor, positive_index: torch.Tensor | None = None,
                   cand_ids: torch.Tensor | None = None, path: str = "auto", *, slab_bytes: int = SLAB_BYTES):
    """The rank of each query's positive among all candidates by the score query [B, D] . candidates [N, D]^T
    (include/krs.h, K15): (int32 rank [B], fp32 score of the positive [B]).  rank is the number of candidates other
    than the positive that precede it in K8's order (score descending, then index ascending), i.e. the column at which
    BruteForceRetrieval(k = N) returns it; with cand_ids, candidates that carry the positive's id are not counted.
    positive_index None: candidate i for query i; an index outside [0, N) gives rank -1 and score NaN.  No autograd.

    path: "fused" -- krs_retrieval_rank (bf16, D <= 256), the [B, N] scores never stored; "slab" -- krs_gemm into fp32
    slabs of query rows under slab_bytes and the count with torch ops; "auto" -- fused wherever it is eligible,
    whatever the shape: its contract is memory, not speed."""
    if path not in ("auto", "fused", "slab"):
        raise L.KrsError(f"retrieval_rank: path must be 'auto', 'fused' or 'slab', got {path!r}")
    q, c, pos, _, ids = _xent_operands(query.detach(), candidates.detach(), positive_index, None, cand_ids)
    fused = path == "fused" or (path == "auto" and q.dtype == torch.bfloat16 and q.shape[1] <= XENT_MAX_D)
    if fused:
        return retrieval_rank_fused(q, c, pos, ids)
    return retrieval_rank_slab(q, c, pos, ids, int(slab_bytes))
