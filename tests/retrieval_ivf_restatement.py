"""K21 (krs_retrieval_ivf, the partitioned index of PartitionedRetrieval) restated in plain numpy -- the reference of
tests/test_retrieval_ivf_gpu.py and tests/test_retrieval_ivf_host.py.  It shares nothing with the kernel.

    leaves_i  = K8's top `probes` of q_i . centroid_l: score descending (-0.0 as +0.0), leaf index ascending
    pool_i    = the candidates j whose leaf is in leaves_i
    result_i  = the first k of pool_i by q_i . c_j descending (-0.0 as +0.0), then the ORIGINAL index j ascending
    short     = a pool of m < k candidates leaves id -1 (also with ids) and score -inf in slots m .. k-1
Scores are float64 dot products rounded to float32: on the integer data of the tests (|x| <= 8, D <= 512) every dot
product is an integer below 2^24, so it is exact in fp32 in any summation order and the kernel must return these ids and
these score bits, with no tolerance.
"""

import numpy as np

from tests.retrieval_q8_restatement import to_bf16


def scores(query, rows):
    """[B, M] float32: query . rows^T, formed in float64 and rounded once (exact on the tests' integer data)."""
    return (np.asarray(query, np.float64) @ np.asarray(rows, np.float64).T).astype(np.float32)


def order(s, index, k):
    """Positions into `index` of the first k entries of one row in K8's total order: the score descending with -0.0 as
    +0.0, then the index ascending."""
    s = np.asarray(s, np.float32) + np.float32(0.0)
    assert np.isfinite(s).all()
    return np.lexsort((np.asarray(index), -s.astype(np.float64)))[:k]


def probe(query, centroids, probes):
    """int32 [B, probes]: the probed leaves of every query, best first."""
    s = scores(query, centroids)
    leaves = np.arange(s.shape[1])
    return np.stack([leaves[order(row, leaves, probes)] for row in s]).astype(np.int32).reshape(len(s), probes)


def restate(query, centroids, cand, assignments, probes, k, ids=None, out_bf16=False):
    """What krs_retrieval_ivf returns for candidates `cand` [N, D] in their ORIGINAL order with leaf `assignments` [N]:
    {"ids": int32 [B, k], "scores": float32 [B, k] (rounded to bf16 when out_bf16), "leaves": int32 [B, probes],
     "index": the original candidate indices (-1 in padding slots), "count": candidates in each query's pool}."""
    query, cand = np.asarray(query, np.float32), np.asarray(cand, np.float32)
    assignments = np.asarray(assignments)
    assert assignments.shape == (cand.shape[0],) and 1 <= probes <= len(centroids)
    leaves = probe(query, centroids, probes)
    b = query.shape[0]
    index = np.full((b, k), -1, np.int64)
    top = np.full((b, k), -np.inf, np.float32)
    count = np.zeros((b,), np.int64)
    for i in range(b):
        pool = np.flatnonzero(np.isin(assignments, leaves[i]))          # ascending original index
        count[i] = len(pool)
        if len(pool) == 0:
            continue
        s = scores(query[i:i + 1], cand[pool])[0]
        sel = order(s, pool, k)
        index[i, :len(sel)] = pool[sel]
        top[i, :len(sel)] = s[sel] + np.float32(0.0)
    if out_bf16:
        top = np.where(np.isfinite(top), to_bf16(np.where(np.isfinite(top), top, 0)), top).astype(np.float32)
    out_ids = index.copy()
    if ids is not None:
        out_ids = np.where(index >= 0, np.asarray(ids, np.int64)[np.maximum(index, 0)], -1)
    return {"ids": out_ids.astype(np.int32), "scores": top, "leaves": leaves, "index": index, "count": count}


def layout(assignments, leaves):
    """The stored layout of a partition: (row_index int32 [N], leaf_offsets int32 [leaves + 1]); row_index is a stable
    sort of the original indices by leaf."""
    assignments = np.asarray(assignments, np.int64)
    row_index = np.argsort(assignments, kind="stable").astype(np.int32)
    offsets = np.zeros((leaves + 1,), np.int32)
    offsets[1:] = np.cumsum(np.bincount(assignments, minlength=leaves))
    return row_index, offsets
