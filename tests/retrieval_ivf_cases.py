"""The case table of K21 (krs_retrieval_ivf): tests/test_retrieval_ivf_gpu.py runs every case through the C ABI against
tests/retrieval_ivf_restatement.py, and tests/test_retrieval_ivf_host.py asserts that the table covers what the kernel
can get wrong (leaf sizes around the 128-candidate step, tiles of 1 / 32 / 33 / more than 64 queries, an unprobed and
an empty leaf, the queue cut, short results on both merge routes, both dtypes and load paths, strides, ids).

All values are small integers (|x| <= 8): every dot product with D <= 512 is exact in fp32 in any summation order, bf16
holds the values exactly, and ties are frequent -- which is where the order can go wrong.
"""

import numpy as np


def _ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float32)


def _routed(rng, sets, leaves, d):
    """Queries and centroids with CHOSEN probes: centroid l = 4 e_l, and query i scores 3, 2, 1 ... on the leaves of
    sets[i] (in that order) and 0 on the others; the columns from `leaves` on are random on the queries and zero on
    the centroids, so they move the candidate scores only."""
    assert d > leaves
    centroids = np.zeros((leaves, d), np.float32)
    centroids[np.arange(leaves), np.arange(leaves)] = 4.0
    query = _ints(rng, (len(sets), d))
    query[:, :leaves] = 0.0
    for i, chosen in enumerate(sets):
        for rank, leaf in enumerate(chosen):
            query[i, leaf] = float(len(chosen) - rank)
    return query, centroids


def _routing_sets():
    """70 queries, 3 probes each: leaf 0 is probed by all 70, leaf 1 by 33, leaf 2 by 32, leaf 3 by one, leaf 7 by none;
    leaves 4 (empty), 5 (450 rows) and 6 fill the third slot."""
    sets = []
    for i in range(70):
        fill = 4 + i % 3
        if i < 33:
            sets.append((0, 1, fill))
        elif i < 65:
            sets.append((0, 2, fill))
        elif i == 65:
            sets.append((0, 3, fill))
        else:
            sets.append((0, 5, 6) if i % 2 else (0, 6, 4))
    return sets


#      name              dtype   d    leaf sizes                                 b   probes k   ids    ld - d  routed
CASES = [
    ("routing",          "bf16", 32,  [129, 128, 127, 1, 0, 450, 5, 60],         70, 3,     8,  True,  0,      True),
    ("b1_probe1_k1",     "f32",  16,  [3, 200, 1, 0, 40],                        1,  1,     1,  False, 0,      False),
    ("b33_full_probe",   "bf16", 100, [129, 300, 0, 1, 127, 128],                33, 6,     128, True, 0,      False),
    ("fp32_d512_stride", "f32",  512, [130, 10, 0, 60],                          5,  2,     10, False, 8,      False),
    ("short_radix",      "bf16", 32,  [3] * 60,                                  9,  20,    128, True, 0,      False),
    ("short_small",      "f32",  8,   [2, 0, 5, 1, 3, 0, 4, 150],                12, 2,     16, False, 0,      False),
    ("stride_vec",       "bf16", 32,  [40, 129, 7, 260],                         34, 2,     5,  True,  8,      False),
    ("stride_odd",       "bf16", 32,  [40, 129, 7, 260],                         34, 2,     5,  False, 1,      False),
    ("radix_full",       "bf16", 64,  [50] * 32,                                 3,  32,    100, False, 0,     False),
    ("queue_cut_ties",   "f32",  4,   [500, 20],                                 33, 1,     3,  False, 0,      False),
]
NAMES = [c[0] for c in CASES]


def make(name):
    """The operands of a case, in numpy: {"query" [b, d], "centroids" [leaves, d], "cand" [n, d] in original order,
    "assignments" int64 [n], "ids" int32 [n] or None, "dtype", "probes", "k", "pad" (row stride minus d), "sizes"}."""
    i = NAMES.index(name)
    _, dtype, d, sizes, b, probes, k, with_ids, pad, routed = CASES[i]
    rng = np.random.default_rng(2100 + i)
    leaves, n = len(sizes), int(sum(sizes))
    assignments = rng.permutation(np.repeat(np.arange(leaves), sizes))     # original order: leaves interleaved
    cand = _ints(rng, (n, d))
    if routed:
        query, centroids = _routed(rng, _routing_sets(), leaves, d)
        assert b == len(query)
    else:
        query, centroids = _ints(rng, (b, d)), _ints(rng, (leaves, d))
    ids = (rng.permutation(n) * 3 + 7).astype(np.int32) if with_ids else None
    return {"name": name, "query": query, "centroids": centroids, "cand": cand, "assignments": assignments, "ids": ids,
            "dtype": dtype, "probes": probes, "k": k, "pad": pad, "sizes": list(sizes)}
