"""K23 (krs_ah_encode, krs_retrieval_ivf_ah, krs_retrieval_rescore; AsymmetricHashingRetrieval) restated in plain numpy
-- the reference of tests/test_retrieval_ah_gpu.py and tests/test_retrieval_ah_host.py.  It shares nothing with the
kernels.

    residual  e = float32(x) - float32(centroid[leaf(x)])                      one rounded fp32 subtraction per element
    encode    per block j (m columns) and centre c: dist = 0; for t in 0 .. m-1: u = e_t - c_t; dist = dist + u * u,
              every operation rounded to fp32; code = the least dist, the LOWEST code on a tie; columns from D on: 0
    layout    a code row is 4 * ceil(blocks / 8) bytes; block j is nibble j, nibble j sits in byte j // 2, the even j
              in the low four bits; the nibbles from `blocks` on are zero
    decode    block j of the row = codebooks[j][code_j]
    AH score  float32( bf16(q) . decode(code) ) + float32( q . centroid[leaf] ), the sum rounded once to fp32
    scan      pool_i = the candidates of the probed leaves; the first r of pool_i by AH score descending, then the
              ORIGINAL index ascending (r = k without reordering: that is the result, with AH scores)
    reorder   the k best of those r by the exact score q . x descending, then the original index ascending
    short     fewer than k real entries leave id -1 (also with ids) and score -inf
On the integer data of tests/retrieval_ah_cases.py (|x| <= 8, D <= 512) every product and sum above is an integer below
2^24: exact in fp32 in any order, so the kernels must return these ids and these score bits, with no tolerance.
"""

import numpy as np

from tests.retrieval_ivf_restatement import layout, order, probe, scores   # noqa: F401  (re-exported for the tests)
from tests.retrieval_q8_restatement import to_bf16


def blocks_of(d, m):
    return -(-d // m)


def code_bytes(d, m):
    return 4 * (-(-blocks_of(d, m) // 8))


def encode(x, leaf, centroids, codebooks):
    """int64 [N, blocks]: the code of every block of every row.  x [N, D] and centroids [leaves, D] hold the values the
    kernel reads (bf16 ones widened exactly), leaf [N] the leaf of each row, codebooks [blocks, 16, m] bf16 values."""
    x, centroids = np.asarray(x, np.float32), np.asarray(centroids, np.float32)
    cb = np.asarray(codebooks, np.float32)
    blocks, _, m = cb.shape
    n, d = x.shape
    assert blocks == blocks_of(d, m)
    e = np.zeros((n, blocks * m), np.float32)
    e[:, :d] = x - centroids[np.asarray(leaf)]                           # float32 - float32: one rounding
    e = e.reshape(n, blocks, m)
    cb = cb.copy().reshape(blocks, 16 * m)
    col = np.arange(blocks)[:, None] * m + np.tile(np.arange(m), 16)[None, :]
    cb[col >= d] = 0.0                                                   # columns from D on read as zero
    cb = cb.reshape(blocks, 16, m)
    dist = np.zeros((n, blocks, 16), np.float32)
    for t in range(m):
        u = e[:, :, None, t] - cb[None, :, :, t]
        dist = dist + u * u                                              # float32 product, then float32 sum
    return np.argmin(dist, axis=2)                                       # the first minimum: the lowest code


def pack(nibbles, d, m):
    """uint8 [N, code_bytes]: the stored form of int codes [N, blocks]."""
    nibbles = np.asarray(nibbles)
    n, blocks = nibbles.shape
    assert blocks == blocks_of(d, m) and nibbles.min(initial=0) >= 0 and nibbles.max(initial=0) <= 15
    wide = np.zeros((n, 2 * code_bytes(d, m)), np.uint8)
    wide[:, :blocks] = nibbles
    return (wide[:, 0::2] | (wide[:, 1::2] << 4)).astype(np.uint8)


def unpack(codes, d, m):
    """int64 [N, blocks] from the stored form."""
    codes = np.asarray(codes, np.uint8)
    wide = np.stack((codes & 15, codes >> 4), axis=2).reshape(codes.shape[0], -1)
    return wide[:, :blocks_of(d, m)].astype(np.int64)


def decode(nibbles, codebooks, d):
    """float32 [N, D]: the reconstructed residuals."""
    cb = np.asarray(codebooks, np.float32)
    blocks, _, m = cb.shape
    nibbles = np.asarray(nibbles)
    out = cb[np.arange(blocks)[None, :], nibbles]                       # [N, blocks, m]
    return out.reshape(len(nibbles), blocks * m)[:, :d].copy()


def rescore_select(query, rows, idx, k, ids=None, out_bf16=False):
    """What krs_retrieval_rescore returns: {"ids", "scores", "index"}.  idx int [B, R], entries outside [0, N) are
    padding."""
    query, rows, idx = np.asarray(query, np.float32), np.asarray(rows, np.float32), np.asarray(idx, np.int64)
    b, n = len(query), len(rows)
    index = np.full((b, k), -1, np.int64)
    top = np.full((b, k), -np.inf, np.float32)
    for i in range(b):
        pool = idx[i][(idx[i] >= 0) & (idx[i] < n)]
        if len(pool) == 0:
            continue
        s = scores(query[i:i + 1], rows[pool])[0]
        sel = order(s, pool, k)
        index[i, :len(sel)] = pool[sel]
        top[i, :len(sel)] = s[sel] + np.float32(0.0)
    if out_bf16:
        top = np.where(np.isfinite(top), to_bf16(np.where(np.isfinite(top), top, 0)), top).astype(np.float32)
    out_ids = index.copy()
    if ids is not None:
        out_ids = np.where(index >= 0, np.asarray(ids, np.int64)[np.maximum(index, 0)], -1)
    return {"ids": out_ids.astype(np.int32), "scores": top, "index": index}


def ah_scores(query, centroids, recon, assignments):
    """float32 [B, N]: the AH score of every (query, candidate) pair, whether probed or not.  recon [N, D] is
    decode(...) in ORIGINAL order."""
    chain = scores(to_bf16(np.asarray(query, np.float32)), recon)                  # bf16(q) . decode, rounded to fp32
    probe_score = scores(query, centroids)[:, np.asarray(assignments)]            # q . centroid[leaf], fp32
    return (chain + probe_score).astype(np.float32)                                # float32 + float32: one rounding


def restate(query, centroids, codebooks, nibbles, assignments, probes, k, r=None, rows=None, ids=None, out_bf16=False):
    """What krs_retrieval_ivf_ah returns for candidates in their ORIGINAL order: nibbles int [N, blocks] their codes,
    assignments [N] their leaves, rows [N, D] their float rows (None: no reordering, r must be None or k).
    {"ids", "scores", "leaves", "index", "count" (candidates in each query's pool), "merged" (int64 [B, r], the scan's
    r best by AH score, -1 padded)}."""
    query = np.asarray(query, np.float32)
    assignments = np.asarray(assignments)
    r = k if r is None else r
    assert rows is not None or r == k
    d = query.shape[1]
    leaves = probe(query, centroids, probes)
    s_all = ah_scores(query, centroids, decode(nibbles, codebooks, d), assignments)
    b = query.shape[0]
    merged = np.full((b, r), -1, np.int64)
    merged_s = np.full((b, r), -np.inf, np.float32)
    count = np.zeros((b,), np.int64)
    for i in range(b):
        pool = np.flatnonzero(np.isin(assignments, leaves[i]))
        count[i] = len(pool)
        if len(pool) == 0:
            continue
        sel = order(s_all[i, pool], pool, r)
        merged[i, :len(sel)] = pool[sel]
        merged_s[i, :len(sel)] = s_all[i, pool][sel] + np.float32(0.0)
    if rows is not None:
        out = rescore_select(query, rows, merged, k, ids=ids, out_bf16=out_bf16)
        out.update({"leaves": leaves, "count": count, "merged": merged})
        return out
    top = merged_s
    if out_bf16:
        top = np.where(np.isfinite(top), to_bf16(np.where(np.isfinite(top), top, 0)), top).astype(np.float32)
    out_ids = merged.copy()
    if ids is not None:
        out_ids = np.where(merged >= 0, np.asarray(ids, np.int64)[np.maximum(merged, 0)], -1)
    return {"ids": out_ids.astype(np.int32), "scores": top, "leaves": leaves, "index": merged, "count": count,
            "merged": merged}
