"""The case table of the K8 route tests: one case per row, with the krs_retrieval_route record the call must have.
tests/test_retrieval_routes_host.py checks the records against the planner without a GPU and that the table names every
stage-1 build, every selection route and a multi-chunk slab run; tests/test_retrieval_matrix_gpu.py runs every case,
asserts the record against what ran and compares the result with tests/retrieval_restatement.py.

The records are written from the kernels' own constants (32 query rows and 128 candidates per stage-1 step, a queue of
256 pairs, 2048 pairs per LDS sort); the slice geometry (S, slice) of every candidate count and the launch counts of the
merged selections are given by hand, not taken from the planner.
"""

import functools
import zlib
from dataclasses import dataclass

import numpy as np

ES = {"f32": 4, "bf16": 2}
DTYPES = ("f32", "bf16")
FIELDS = ("kernel", "variant", "es", "vec", "S", "qtiles", "row_bytes", "lds_bytes", "select", "select_launches", "slice",
          "blocks", "select_len", "select_p", "chunks", "chunk_rows")
B = 33                                   # two query tiles, the second with one row
# (S, slice) of stage 1 for B = 33 queries: the fewest slices of >= 8192 candidates, rounded up to 8 slices of whole
# 128-candidate steps
GEOMETRY = {130: (8, 128), 255: (8, 128), 700: (8, 128), 3000: (8, 384), 40000: (8, 5120), 65537: (16, 4224),
            131073: (24, 5504)}
# launches of a selection merged in global memory: select, the block sort, per level its global steps and a block pass, emit
MERGE_LAUNCHES = {4096: 2 + (1 + 1) + 1, 8192: 2 + (1 + 1) + (2 + 1) + 1}


def R(**kw):
    rt = dict.fromkeys(FIELDS, 0)
    rt.update(kernel=None, variant=None, select=None)
    rt.update(**kw)
    return rt


def cdiv(a, b):
    return -(-a // b)


def pow2(v):
    p = 1
    while p < v:
        p *= 2
    return p


def selection(length, k):
    if length <= 2048:
        return dict(select="lds", select_len=length, select_p=pow2(length), select_launches=1)
    p = pow2(k)
    if p <= 2048:
        return dict(select="radix", select_len=length, select_p=p, select_launches=3)
    return dict(select="radix_merge", select_len=length, select_p=p, select_launches=MERGE_LAUNCHES[p])


def fused(dtype, n, d, k, vec, b=B):
    S, slice_ = GEOMETRY[n]
    row_bytes = cdiv(d * ES[dtype], 32) * 32
    # the query tile (rows padded by 16 bytes), the row queues, the counts and the thresholds
    lds = 32 * (row_bytes + 16) + 32 * 256 * 8 + 32 * 4 + 32 * 4
    return R(kernel="fused", variant="topk", es=ES[dtype], vec=int(vec), S=S, qtiles=cdiv(b, 32), slice=slice_,
             row_bytes=row_bytes, lds_bytes=lds, blocks=S * cdiv(b, 32), **selection(S * k, k))


def slab(dtype, n, k, chunks, chunk_rows):
    return R(kernel="slab", variant="topk", es=ES[dtype], chunks=chunks, chunk_rows=chunk_rows, **selection(n, k))


def rows_route(dtype, cols, k):
    return R(kernel="rows", variant="rows", es=ES[dtype], **selection(cols, k))


@dataclass(frozen=True)
class Case:
    name: str
    group: str              # the item of the test plan: "build", "order", "special", "merge", "chunks", "rows", "normal"
    entry: str              # "topk" (retrieval_topk) | "rows" (topk_rows)
    dtype: str
    b: int                  # query rows / rows
    n: int                  # candidates / columns
    d: int
    k: int
    data: str               # what inputs() builds
    layout: str             # "plain" | "col_slice" (wide[:, 1:1 + d] of [n, d + 3]) | "odd_stride" (parent[:, :d] of [n, d + 1])
    ids: str                # "none" | "reversed" | "signed" (negatives and duplicates)
    nan: int                # "special": NaN candidates at the highest indices
    budget: int             # KRS_RETRIEVAL_SLAB_BYTES, 0 = unset
    route: dict

    @property
    def ld(self):
        return {"plain": self.d, "col_slice": self.d + 3, "odd_stride": self.d + 1}[self.layout]

    @property
    def base_offset(self):
        """bytes from a 16-byte boundary to the first candidate element"""
        return ES[self.dtype] if self.layout == "col_slice" else 0


CASES = []


def _add(group, entry, dtype, b, n, d, k, data, route, layout="plain", ids="none", nan=0, budget=0):
    name = f"{group}-{entry}-{dtype}-b{b}-n{n}-d{d}-k{k}-{data}"
    for tag, on in ((layout, layout != "plain"), (f"ids_{ids}", ids != "none"), (f"nan{nan}", nan), (f"budget{budget}", budget)):
        if on:
            name += f"-{tag}"
    CASES.append(Case(name, group, entry, dtype, b, n, d, k, data, layout, ids, nan, budget, route))


# a. every stage-1 build, both dtypes: 16-byte loads need rows of whole 16-byte chunks on a 16-byte boundary
VEC_D = {"bf16": (8, 72, 128, 136, 512), "f32": (4, 20, 64, 68, 100, 512)}
ELEM_D = {"bf16": (1, 7, 9, 100, 129, 511), "f32": (1, 3, 5, 63, 65, 509)}
LAYOUT_D = {"bf16": 128, "f32": 64}
for dt in DTYPES:
    for d_ in VEC_D[dt]:
        _add("build", "topk", dt, B, 255, d_, 10, "ints", fused(dt, 255, d_, 10, True), ids="reversed")
    for d_ in ELEM_D[dt]:
        _add("build", "topk", dt, B, 255, d_, 10, "ints", fused(dt, 255, d_, 10, False), ids="reversed")
    for lay in ("col_slice", "odd_stride"):
        _add("build", "topk", dt, B, 255, LAYOUT_D[dt], 10, "ints", fused(dt, 255, LAYOUT_D[dt], 10, False), layout=lay,
             ids="reversed")
    _add("build", "topk", dt, B, 255, LAYOUT_D[dt], 10, "ints", fused(dt, 255, LAYOUT_D[dt], 10, True), ids="signed")

# b. score order in stage 1: ascending, descending and all-tied rows in one tile; a sawtooth, whose ties straddle step and
# queue boundaries; and a late arrival exactly at the k-th place right after the first queue cut, which a threshold picked
# even one place too high loses (random and monotone scores do not notice such a threshold: the slices' tails rarely matter)
for dt in DTYPES:
    for data_ in ("ramp", "saw", "late"):
        for k_ in (1, 2, 3, 5, 64, 127, 128):
            _add("order", "topk", dt, B, 40000, 2, k_, data_, fused(dt, 40000, 2, k_, False))

# c. NaN and +-inf scores through four routes, fewer and more NaN candidates than k
for dt in DTYPES:
    for n_, d_, k_, nans in ((700, 4, 10, (3, 15)), (131073, 4, 86, (3, 100)), (700, 4, 129, (3, 140)), (700, 513, 10, (3, 15))):
        for nan_ in nans:
            if k_ <= 128 and d_ <= 512:
                rt = fused(dt, n_, d_, k_, dt == "f32")      # d = 4: 16 bytes of fp32, 8 of bf16
            else:
                rt = slab(dt, n_, k_, 1, B)
            _add("special", "topk", dt, B, n_, d_, k_, "special", rt, nan=nan_)

# d. the merge of the slice lists on both sides of 2048 pairs, and slices with fewer than k candidates or none
for dt in DTYPES:
    for n_, k_ in ((131073, 85), (131073, 86), (65537, 128), (130, 10)):
        _add("merge", "topk", dt, B, n_, 4, k_, "ints", fused(dt, n_, 4, k_, dt == "f32"), ids="reversed")

# e. the two-step path in chunks: a row costs 3000 * 4 slab bytes + 256 * 8 list bytes = 14048
for dt in DTYPES:
    _add("chunks", "topk", dt, 70, 3000, 16, 200, "ints", slab(dt, 3000, 200, 1, 70))
    _add("chunks", "topk", dt, 70, 3000, 16, 200, "ints", slab(dt, 3000, 200, 3, 32), budget=450000)   # 32, 32, 6 rows
    _add("chunks", "topk", dt, 70, 3000, 16, 200, "ints", slab(dt, 3000, 200, 70, 1), budget=20000)

# f. the row selection
for cols_, k_, data_ in ((2048, 10, "ints50"), (2049, 10, "ints50"), (5000, 2048, "ints50"), (5000, 2049, "ints50"),
                         (5000, 4097, "ints50"), (5000, 300, "bucket")):
    _add("rows", "rows", "f32", 3, cols_, 0, k_, data_, rows_route("f32", cols_, k_))
for k_ in (1, 255, 256, 257, 2048, 4999, 5000):
    _add("rows", "rows", "f32", 3, 5000, 0, k_, "equal", rows_route("f32", 5000, k_))
_add("rows", "rows", "bf16", 3, 5000, 0, 4097, "ints50", rows_route("bf16", 5000, 4097))
_add("rows", "rows", "bf16", 3, 2048, 0, 10, "ints50", rows_route("bf16", 2048, 10))

# g. random normal data, one case per stage-1 build
for dt, d_, vec_ in (("bf16", 128, True), ("bf16", 100, False), ("f32", 64, True), ("f32", 63, False)):
    _add("normal", "topk", dt, B, 3000, d_, 16, "normal", fused(dt, 3000, d_, 16, vec_))

BY_NAME = {c.name: c for c in CASES}
SCALES = (1.0, -1.0, 2.0, -2.0, 0.0)


@functools.lru_cache(maxsize=4)
def inputs(name):
    """Host inputs of a case, fp32 values that the case's dtype holds exactly (but "normal"): q [b, d], c [n, d] and ids
    (int32 [n] or None) for "topk"; x [rows, cols] for "rows".  Cached: treat as read-only."""
    c = BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if c.entry == "rows":
        if c.data == "ints50":
            x = rng.integers(-50, 50, size=(c.b, c.n)).astype(np.float32)           # many ties
        elif c.data == "equal":
            x = np.full((c.b, c.n), 7.0, np.float32)    # all keys equal: the select runs down to the index bytes
        else:
            # "bucket": exactly k values in [2, 4) (the first byte of their keys is 0xc0), the rest in [0.5, 1) (0xbf):
            # the k-th pair's bucket is taken whole at the first digit
            x = (0.5 + rng.integers(0, 128, size=(c.b, c.n)) / 256.0).astype(np.float32)
            for r in range(c.b):
                at = rng.choice(c.n, size=c.k, replace=False)
                x[r, at] = (2.0 + rng.integers(0, 128, size=c.k) / 64.0).astype(np.float32)
        return {"x": x}
    if c.data == "ints":
        q = rng.integers(-2, 3, size=(c.b, c.d)).astype(np.float32)
        cand = rng.integers(-2, 3, size=(c.n, c.d)).astype(np.float32)
    elif c.data in ("ramp", "saw", "late"):
        # score(r, i) = s_r * v_i with v_i = i (ramp), i % 300 (saw) or (late) 2000 + 2 (255 - i) over the first two steps,
        # whose cut keeps candidates 0 .. k - 1 and sets the threshold, then small values but for candidate 300, which
        # scores between candidates k - 2 and k - 1: exact in fp32, every operand exact in bf16
        s = np.array([SCALES[r % len(SCALES)] for r in range(c.b)], np.float32)
        q = s[:, None] * np.array([[256.0, 1.0]], np.float32)
        i = np.arange(c.n)
        if c.data == "saw":
            i = i % 300
        elif c.data == "late":
            i = np.where(i < 256, 2000 + 2 * (255 - i), i % 251)
            i[300] = 2000 + 2 * (255 - (c.k - 1)) + 1
        assert i.max() < 65536
        cand = np.stack([i >> 8, i & 255], 1).astype(np.float32)
    elif c.data == "special":
        s = np.array([(1.0, -1.0, 2.0, -2.0, 3.0)[r % 5] for r in range(c.b)], np.float32)
        s[-1] = 0.0                                     # one all-zero query row
        q = np.zeros((c.b, c.d), np.float32)
        q[:, 0] = s
        col = rng.integers(-20, 21, size=c.n).astype(np.float32)
        kind = rng.random(c.n)
        col[kind < 0.05] = np.inf
        col[kind > 0.95] = -np.inf
        col[c.n - c.nan:] = np.nan                      # NaN at the highest indices: they must displace a full queue
        cand = np.zeros((c.n, c.d), np.float32)
        cand[:, 0] = col
    else:
        q = rng.normal(size=(c.b, c.d)).astype(np.float32)
        cand = rng.normal(size=(c.n, c.d)).astype(np.float32)
    ids = None
    if c.ids == "reversed":
        ids = (c.n - 1 - np.arange(c.n)).astype(np.int32)
    elif c.ids == "signed":
        ids = ((np.arange(c.n) % 50 - 25) * 40000001).astype(np.int32)       # negatives and duplicates: passed through
    return {"q": q, "c": cand, "ids": ids}
