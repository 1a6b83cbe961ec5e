"""The case table of K23 (krs_ah_encode, krs_retrieval_ivf_ah): tests/test_retrieval_ah_gpu.py runs every case through the
C ABI against tests/retrieval_ah_restatement.py, and tests/test_retrieval_ah_host.py asserts that the table covers what
the kernels can get wrong (leaf sizes around the 128-candidate step, tiles of 1 / 32 / 33 pairs, an unprobed and an empty
probed leaf, every block width, a padded last block, short results against k and against r, reordering on and off, both
query dtypes, strides, ids).

All values are small integers: rows, centroids and codebooks with |x| <= 8 and bf16-exact queries with |q| <= 8.  Every
dot product with D <= 512 (q . decode, q . centroid, q . x) is an integer below 2^16 and every encoder distance an integer
below 2^24, exact in fp32 in any summation order -- and ties are everywhere, in the encoder and in the ranking.
"""

import functools

import numpy as np

from tests import retrieval_ah_restatement as RA
from tests.retrieval_ivf_cases import _ints, _routed, _routing_sets

ROUTING_SIZES = [129, 128, 127, 1, 0, 450, 5, 60]

#      name               dtype   d    m  leaf sizes                    b   probes k    r     ids    ld - d  routed
CASES = [
    ("routing",           "bf16", 32,  2, ROUTING_SIZES,                70, 3,     8,   None, True,  0,      True),
    ("routing_reorder",   "bf16", 32,  4, ROUTING_SIZES,                70, 3,     8,   128,  True,  0,      True),
    ("b1_probe1_k1",      "f32",  32,  8, [3, 200, 1, 0, 40],           1,  1,     1,   None, False, 0,      False),
    ("b33_d100_m8",       "bf16", 100, 8, [129, 300, 0, 1, 127, 128],   33, 6,     10,  100,  True,  0,      False),
    ("fp32_d512_stride",  "f32",  512, 2, [130, 10, 0, 60],             5,  2,     10,  10,   False, 8,      False),
    ("short_reorder",     "bf16", 32,  4, [2, 0, 5, 1, 3, 0, 4, 150],   12, 2,     16,  128,  False, 0,      False),
    ("short_scan",        "f32",  32,  2, [3] * 20,                     9,  4,     16,  None, True,  0,      False),
    ("d100_m4_odd",       "bf16", 100, 4, [40, 129, 7, 260],            34, 2,     5,   64,   False, 1,      False),
    ("d100_m2_scan",      "f32",  100, 2, [40, 129, 7, 260],            3,  2,     5,   None, False, 0,      False),
    ("queue_cut_ties",    "bf16", 32,  2, [500, 20],                    33, 1,     3,   None, False, 0,      False),
    ("k128_r128",         "bf16", 32,  8, [300, 200],                   3,  2,     128, 128,  False, 0,      False),
]
NAMES = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def make(name):
    """The operands of a case, in numpy: {"query" [b, d], "centroids" [leaves, d], "cand" [n, d] in original order,
    "assignments" int64 [n], "codebooks" [blocks, 16, m] (zero in the columns from d on), "nibbles" int64 [n, blocks] (the
    restatement's codes of the candidates, original order), "ids" int32 [n] or None, "dtype" (of queries, centroids and
    float rows), "m", "probes", "k", "r" (None: no reordering), "pad" (row stride minus d), "sizes"}."""
    i = NAMES.index(name)
    _, dtype, d, m, sizes, b, probes, k, r, with_ids, pad, routed = CASES[i]
    rng = np.random.default_rng(2300 + i)
    leaves, n = len(sizes), int(sum(sizes))
    assignments = rng.permutation(np.repeat(np.arange(leaves), sizes))     # original order: leaves interleaved
    cand = _ints(rng, (n, d))
    if routed:
        query, centroids = _routed(rng, _routing_sets(), leaves, d)
        assert b == len(query)
    else:
        query, centroids = _ints(rng, (b, d)), _ints(rng, (leaves, d))
    blocks = RA.blocks_of(d, m)
    codebooks = _ints(rng, (blocks, 16, m)).reshape(blocks * 16 * m)
    col = (np.arange(blocks)[:, None, None] * m + np.arange(m)[None, None, :] + np.zeros((1, 16, 1), int)).reshape(-1)
    codebooks[col >= d] = 0.0
    codebooks = codebooks.reshape(blocks, 16, m)
    ids = (rng.permutation(n) * 3 + 7).astype(np.int32) if with_ids else None
    nibbles = RA.encode(cand, assignments, centroids, codebooks)
    return {"name": name, "query": query, "centroids": centroids, "cand": cand, "assignments": assignments,
            "codebooks": codebooks, "nibbles": nibbles, "ids": ids, "dtype": dtype, "m": m, "probes": probes, "k": k,
            "r": r, "pad": pad, "sizes": list(sizes)}
