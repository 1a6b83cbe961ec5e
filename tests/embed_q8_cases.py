"""The case table of tests/test_embed_q8_gpu.py (krs_embed_bag_fwd_q8 on every kernel instantiation and branch of
keras_rs_amd/csrc/embed_bag_fwd_q8.hip) and of its coverage check, tests/test_embed_q8_host.py.

A case fixes one krs_embed_bag_fwd_q8 call: the output dtype, dim, batch, the features (table, combiner) over two tables
(vocab 300 and 37; the three-feature form shares table 0), dense `hots` or CSR bag lengths, weights, the id and offset
types, the out-of-range ids planted in the buffer, the layout of the output slab -- and the route record
krs_embed_bag_fwd_q8_last_route must report for it.  The expected routes are asserted on the host against the planner
(keras_rs_amd/csrc/embed_fwd_q8_plan.h through krs_embed_bag_fwd_q8_plan_route) and on the device against what ran.

The tables are set directly, not through the quantizer: q[r, c] = ((131 r + 7 c) mod 255) - 127, so the 16 bytes of a
piece all differ and half of them are negative (a byte-order or sign-extension slip cannot cancel); row 1 is all -128, row
2 all +127; the steps span 1e-6 .. 10; step[0] is NaN on every table and no valid id is 0, so a masked stand-in read that
leaks shows as NaN.
"""

import dataclasses
import functools
import zlib

import numpy as np

from tests.embed_q8_restatement import MEAN, SQRTN, SUM

OUTS = ("f32", "bf16")
ES = {"f32": 4, "bf16": 2}
LPRS = (8, 16, 32, 64)
# per LPR: dims on the vector path (whole 16-byte pieces, at most 1024); the first leaves lanes of the group idle
VEC_DIMS = {8: (16, 48, 128), 16: (208, 256), 32: (400, 512), 64: (1024,)}
GENERIC_DIMS = {20: 32, 1040: 64, 1: 1}      # dim -> lanes per bag of the generic kernel
VOCABS = (300, 37)
ONE = ((0, MEAN),)
THREE = ((0, SUM), (1, MEAN), (0, SQRTN))    # table 0 is shared
BAD = (-1, "vocab")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    odt: str
    dim: int
    batch: int
    route: dict                        # what embedding_ops.embed_fwd_q8_last_route() must return
    feats: tuple = THREE               # (table index, combiner) per feature
    hots: tuple = None                 # dense form: ids per bag, per feature
    lens: tuple = None                 # CSR form: the length of every bag, feature-major
    weights: str = None                # None | "uniform" (0.25 .. 1) | "mixed" (zeros and negatives, see inputs())
    id64: bool = False
    off64: bool = False
    bad: tuple = ()                    # out-of-range ids planted in the buffer ("vocab": the vocab of that lookup's table)
    lead: int = 8                      # NaN columns before the first slot (a non-zero first out_col), between two slots, after
    gap: int = 8
    tail: int = 8

    @property
    def csr(self):
        return self.lens is not None

    @property
    def n_feats(self):
        return len(self.feats)

    @property
    def nnz(self):
        return int(sum(self.lens)) if self.csr else self.batch * int(sum(self.hots))

    @property
    def out_cols(self):
        return [self.lead + f * (self.dim + self.gap) for f in range(self.n_feats)]

    @property
    def width(self):
        """columns of the output slab (out_ld): more than n_feats * dim"""
        return self.lead + self.n_feats * (self.dim + self.gap) - self.gap + self.tail

    @property
    def flag(self):
        return 1 if self.bad else 0


def cdiv(a, b):
    return -(-a // b)


def R(kernel, odt=None, lpr=0, has_w=False, bpg=0, blocks=0):
    """An expected route record, in the form embedding_ops.embed_fwd_q8_last_route() returns."""
    if kernel is None:
        return dict(kernel=None, lpr=0, has_w=False, stream=False, hot_rows=0, bpg=0, table_dtype=None, out_dtype=None,
                    blocks=0)
    return dict(kernel=kernel, lpr=lpr, has_w=has_w, stream=False, hot_rows=0, bpg=bpg, table_dtype="i8", out_dtype=odt,
                blocks=blocks)


CASES = []


def case(name, odt, dim, batch, kernel, lpr, *, bpg=0, **kw):
    """Appends a case.  kernel / lpr / bpg are the expected route, stated by the caller; has_w follows from the weights and
    the block count from the launch geometry the route implies: a wave per 64 / lpr groups of bpg bags, four waves per
    workgroup (vec); 256 / lpr bags per workgroup (generic)."""
    c = Case(name, odt, dim, batch, None, **kw)
    nf = c.n_feats
    blocks = cdiv(cdiv(batch, (64 // lpr) * bpg) * nf, 4) if kernel == "vec" else cdiv(batch * nf, 256 // lpr)
    c = dataclasses.replace(c, route=R(kernel, odt, lpr, c.weights is not None, bpg, blocks))
    assert (c.hots is None) != (c.lens is None) and (c.lens is None or len(c.lens) == nf * batch), name
    assert c.hots is None or len(c.hots) == nf, name
    CASES.append(c)
    return c


def tiled(pattern, n, seed):
    """n bag lengths: `pattern` repeated, then shuffled"""
    lens = np.resize(np.asarray(pattern, np.int64), n)
    np.random.default_rng(seed).shuffle(lens)
    return tuple(int(v) for v in lens)


POOL_LENS = (4, 2, 3, 0, 1, 5, 3, 2)       # mean 2.5, nnz // bags == 2: bpg 16

# ---- embed_bag_fwd_q8_vec: every (out dtype, LPR, HAS_W); every vector dim; batch 1, 5, 67; dense and CSR ---------------
k = 0
for oi, odt in enumerate(OUTS):
    for li, lpr in enumerate(LPRS):
        for has_w in (False, True):
            for di, dim in enumerate(VEC_DIMS[lpr]):
                batch = (67, 5, 1)[(k + di) % 3] if dim < 1024 else (5, 67)[has_w]
                feats = ONE if (k + di) % 4 == 3 else THREE
                csr = (k + di) % 2 == 1
                kw = dict(feats=feats, weights=("uniform", "mixed")[(oi + li) % 2] if has_w else None, id64=k % 3 == 0,
                          off64=csr and k % 2 == 0)
                if csr:
                    kw["lens"] = tiled(POOL_LENS, len(feats) * batch, k + di) if batch > 1 else (3, 0, 4)[:len(feats)]
                    mean = int(sum(kw["lens"])) // (len(feats) * batch)
                    bpg = min(16, 32 // max(mean, 1))
                else:
                    kw["hots"] = ((2,), (1, 2, 33))[len(feats) == 3]
                    bpg = 16 if len(feats) == 1 else 2          # mean 12: bpg 2
                case(f"vec-{odt}-lpr{lpr}-w{int(has_w)}-d{dim}-b{batch}-{'csr' if csr else 'dense'}-f{len(feats)}", odt,
                     dim, batch, "vec", lpr, bpg=bpg, **kw)
            k += 1
# one lookup per bag, unweighted (the pure gather runs on the pooled kernel): bpg 16
for odt in OUTS:
    case(f"vec-{odt}-hot1-d128", odt, 128, 67, "vec", 8, bpg=16, hots=(1, 1, 1))
    case(f"vec-{odt}-hot1-d1024", odt, 1024, 5, "vec", 64, bpg=16, hots=(1, 1, 1), id64=True)
case("vec-f32-hot33-d48", "f32", 48, 67, "vec", 8, bpg=1, feats=ONE, hots=(33,), weights="uniform")
# output slots off their 16-byte alignment: the element-store branch, per output type
for odt in OUTS:
    case(f"vec-{odt}-unaligned-slots", odt, 48, 67, "vec", 8, bpg=16, hots=(2, 2, 2), weights="uniform", lead=1, gap=3, tail=2)


def _edge_lens(n):
    """n >= 8 CSR bags: a first empty bag, one bag of 200 lookups (it crosses the id window: 64 ids at LPR 8, 128 at LPR
    16), an empty bag behind it, short bags, a last empty bag"""
    return (0, 200, 0, 3, 1) + tuple((2, 0, 5, 1)[i % 4] for i in range(n - 6)) + (0,)


# nnz // bags = 222 // 15 = 14 -> bpg 2 (batch 5, 3 features); 326 // 67 = 4 -> bpg 8 (batch 67, one feature)
case("csr-edges-lpr8-b5", "f32", 128, 5, "vec", 8, bpg=2, lens=_edge_lens(15), weights="uniform", off64=True)
case("csr-edges-lpr16-b67", "bf16", 256, 67, "vec", 16, bpg=8, feats=ONE, lens=_edge_lens(67), id64=True)
# zero denominators: mean bags whose weights cancel, sqrtn bags whose weights are all zero -> exactly 0
case("den0-mixed-dense", "f32", 128, 67, "vec", 8, bpg=16, hots=(2, 2, 2), weights="mixed")
case("den0-mixed-generic", "bf16", 20, 67, "generic", 32, hots=(2, 2, 2), weights="mixed")
# out-of-range ids (-1 and vocab), both id types, both kernels
case("oob-vec-i32", "f32", 128, 67, "vec", 8, bpg=16, hots=(2, 2, 2), bad=BAD)
case("oob-vec-i64-csr", "bf16", 48, 67, "vec", 8, bpg=16, lens=tiled(POOL_LENS, 201, 5), weights="uniform", id64=True,
     off64=True, bad=BAD)
case("oob-generic-i32", "f32", 20, 67, "generic", 32, hots=(1, 2, 33), bad=BAD)
case("oob-generic-i64", "bf16", 1, 67, "generic", 1, hots=(2, 2, 2), id64=True, bad=BAD)

# ---- embed_bag_fwd_q8_generic: both out dtypes, every generic dim, dense and CSR ------------------------------------------
k = 0
for odt in OUTS:
    for dim, lpr in GENERIC_DIMS.items():
        for csr in (False, True):
            batch = (67, 5, 1)[k % 3] if dim < 1000 else (5, 1)[csr]
            feats = ONE if k % 4 == 1 else THREE
            kw = dict(feats=feats, weights=(None, "uniform", "mixed")[k % 3], id64=k % 2 == 1, off64=csr and k % 4 < 2,
                      lead=(8, 1)[csr], gap=(8, 3)[csr])
            if csr:
                kw["lens"] = tiled(POOL_LENS, len(feats) * batch, k) if batch > 1 else (3, 0, 4)[:len(feats)]
            else:
                kw["hots"] = ((2,), (1, 2, 33))[len(feats) == 3]
            case(f"generic-{odt}-d{dim}-b{batch}-{'csr' if csr else 'dense'}-f{len(feats)}", odt, dim, batch, "generic", lpr,
                 **kw)
            k += 1

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
LARGEST = max(CASES, key=lambda c: c.nnz * c.dim).name


# ---- the inputs of a case ----------------------------------------------------------------------------------------------

MIXED = (0.5, -0.5, 0.0, 0.0, 0.75, -0.25, 0.0, 1.0)     # bags of two: mean den 0 | all zero | 0.5 | one zero weight


def q_table(vocab, dim):
    r, c = np.arange(vocab, dtype=np.int64)[:, None], np.arange(dim, dtype=np.int64)[None, :]
    q = ((131 * r + 7 * c) % 255 - 127).astype(np.int8)
    q[1], q[2] = -128, 127
    return q


def step_array(vocab, seed):
    step = np.logspace(-6, 1, vocab).astype(np.float32)
    np.random.default_rng(seed).shuffle(step)
    step[0] = np.nan
    return step


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Host inputs of a case: q_tables (int8), steps (float32), ids, offsets | None, weights | None.  Deterministic in the
    case name."""
    c = BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n_tables = max(t for t, _ in c.feats) + 1
    q_tables = [q_table(VOCABS[t], c.dim) for t in range(n_tables)]
    steps = [step_array(VOCABS[t], 11 + t) for t in range(n_tables)]
    if c.csr:
        lens = np.asarray(c.lens, np.int64)
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64 if c.off64 else np.int32)
    else:
        lens = np.repeat(np.asarray(c.hots, np.int64), c.batch)
        offsets = None
    feat_of = np.repeat(np.arange(c.n_feats), c.batch)
    vocab_of = np.repeat(np.array([VOCABS[c.feats[f][0]] for f in feat_of], np.int64), lens)
    nnz = int(lens.sum())
    assert nnz == c.nnz
    ids = (rng.integers(0, 2 ** 31, nnz) % (vocab_of - 1) + 1).astype(np.int64)          # never 0
    ids[: min(nnz, 2)] = (1, 2)[: min(nnz, 2)]                                            # the -128 and the +127 row
    if c.bad:
        assert nnz > 8, name
        pos = rng.choice(np.arange(2, nnz), size=max(4, nnz // 16), replace=False)
        for i, p in enumerate(pos):
            ids[p] = vocab_of[p] if c.bad[i % 2] == "vocab" else c.bad[i % 2]
    ids = ids.astype(np.int64 if c.id64 else np.int32)
    if c.weights == "uniform":
        weights = rng.uniform(0.25, 1.0, nnz).astype(np.float32)
    elif c.weights == "mixed":
        weights = np.resize(np.asarray(MIXED, np.float32), nnz)
    else:
        weights = None
    return dict(q_tables=q_tables, steps=steps, ids=ids, offsets=offsets, weights=weights)
