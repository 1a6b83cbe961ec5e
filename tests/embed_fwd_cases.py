"""The case table of tests/test_embed_fwd_matrix_gpu.py (krs_embed_bag_fwd on every kernel instantiation and route of
keras_rs_amd/csrc/embed_bag_fwd.hip) and of its coverage check, tests/test_embed_fwd_routes_host.py.

A case fixes one krs_embed_bag_fwd call: the dtype pair, dim, batch, the features (table, combiner), dense `hots` or CSR
bag lengths, weights, the id and offset types, the out-of-range ids planted in the buffer, the layout of the output
buffer (lead / gap / tail sentinel columns, an element offset of its base) and the KRS_EMBED_OPT_HOTROWS value -- and the
route record krs_embed_bag_fwd_last_route must report for it.  The expected routes are asserted on the host against the
planner (keras_rs_amd/csrc/embed_fwd_plan.h through krs_embed_bag_fwd_plan_route) and on the device against what ran, so
a dispatch change shows up as a failing case, not as lost coverage.  Shapes stay tiny: batch <= 200, vocab <= 300,
n_feats <= 4 (one case has 129 features: the limit of the sample-major gather).
"""

import dataclasses
import functools
import zlib

import numpy as np

from tests.embed_fwd_restatement import MEAN, SQRTN, SUM

PAIRS = (("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f32", "bf16"))
ES = {"f32": 4, "bf16": 2}
LPRS = (8, 16, 32, 64)
# per table dtype and LPR: a dim that leaves lanes of the group idle, and one that fills it (pieces == LPR)
DIMS = {"f32": {8: (12, 32), 16: (40, 64), 32: (96, 128), 64: (160, 256)},
        "bf16": {8: (24, 64), 16: (80, 128), 32: (192, 256), 64: (320, 512)}}
MORE_IDLE_DIMS = {"f32": {8: 20}}      # (a second LPR 8 dim with idle lanes: 5 pieces)
GENERIC_DIMS = {"f32": (7, 260, 320), "bf16": (12, 20)}      # rows that are not whole 16-byte pieces, or exceed 1024 bytes
VOCABS = (300, 37, 150)
ALL3 = ((0, SUM), (1, MEAN), (2, SQRTN))
BAD32 = (-1, "vocab")
BAD64 = (-1, "vocab", 2 ** 32 + 3, -2 ** 40)
FLAG_ID_OUT_OF_RANGE = 1


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    tdt: str
    odt: str
    dim: int
    batch: int
    route: dict                        # what embedding_ops.embed_fwd_last_route() must return
    feats: tuple = ALL3                # (table index, combiner) per feature
    hots: tuple = None                 # dense form: ids per bag, per feature
    lens: tuple = None                 # CSR form: the length of every bag, feature-major
    weights: str = None                # None | "uniform" (0.25 .. 1) | "pm_half" (+0.5, -0.5, +0.5, ...)
    id64: bool = False
    off64: bool = False
    bad: tuple = ()                    # out-of-range ids planted in the buffer ("vocab": the vocab of that lookup's table)
    poison: bool = True                # row 0 of every table is NaN and no valid id is 0
    specials: bool = False             # gather cases: +-inf, subnormals, NaN and bf16 halfway values in the table rows
    lead: int = 8                      # sentinel columns before the first slot, between two slots, after the last
    gap: int = 8
    tail: int = 8
    base_off: int = 0                  # `out` starts this many elements into its buffer row (buf[:, base_off:])
    hot_opt: int = 0                   # krs_embed_set_option(KRS_EMBED_OPT_HOTROWS, .)
    vocabs: tuple = VOCABS

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
        """columns of the output BUFFER (the leading dimension of `out`)"""
        return self.base_off + self.lead + self.n_feats * (self.dim + self.gap) - self.gap + self.tail

    @property
    def flag(self):
        return FLAG_ID_OUT_OF_RANGE if self.bad else 0


def cdiv(a, b):
    return -(-a // b)


def R(kernel, tdt=None, odt=None, lpr=0, has_w=False, stream=False, hot_rows=0, bpg=0, blocks=0):
    """An expected route record, in the form embedding_ops.embed_fwd_last_route() returns."""
    if kernel is None:
        return dict(kernel=None, lpr=0, has_w=False, stream=False, hot_rows=0, bpg=0, table_dtype=None, out_dtype=None,
                    blocks=0)
    return dict(kernel=kernel, lpr=lpr, has_w=has_w, stream=stream, hot_rows=hot_rows, bpg=bpg, table_dtype=tdt,
                out_dtype=odt, blocks=blocks)


CASES = []


def case(name, tdt, odt, dim, batch, kernel, lpr, *, bpg=0, stream=False, hot_rows=0, ld_mult=None, **kw):
    """Appends a case.  kernel / lpr / bpg / stream / hot_rows are the expected route, stated by the caller; has_w follows
    from the weights, and the block count from the launch geometry the route implies: a wave per 64 / lpr groups of bpg
    bags (pooled), per 64 bags of a feature (hot1), per 64 (sample, feature) units (hot1_rows), 256 / lpr bags per
    workgroup (generic), four waves per workgroup.  ld_mult: the tail grows until the buffer width is a multiple of it."""
    c = Case(name, tdt, odt, dim, batch, None, **kw)
    if ld_mult:
        c = dataclasses.replace(c, tail=c.tail + (-c.width) % ld_mult)
    nf = c.n_feats
    blocks = {"vec": lambda: cdiv(cdiv(batch, (64 // lpr) * bpg) * nf, 4), "hot1": lambda: cdiv(cdiv(batch, 64) * nf, 4),
              "hot1_rows": lambda: cdiv(cdiv(batch * nf, 64), 4), "generic": lambda: cdiv(batch * nf, 256 // lpr)}[kernel]()
    has_w = c.weights is not None and kernel in ("vec", "generic")
    c = dataclasses.replace(c, route=R(kernel, tdt, odt, lpr, has_w, stream, hot_rows, bpg, blocks))
    assert (c.hots is None) != (c.lens is None) and (c.lens is None or len(c.lens) == nf * batch), name
    assert not c.specials or all(h == 1 for h in c.hots), name
    assert c.id64 or all(isinstance(b, str) or -2 ** 31 <= b < 2 ** 31 for b in c.bad), name
    CASES.append(c)
    return c


def tiled(pattern, n, seed):
    """n bag lengths: `pattern` repeated, then shuffled"""
    lens = np.resize(np.asarray(pattern, np.int64), n)
    np.random.default_rng(seed).shuffle(lens)
    return tuple(int(v) for v in lens)


STREAM_LENS = (0, 1, 2, 1, 1, 2, 0, 2)     # lengths in {0, 1, 2}, mean 9 / 8: nnz < 2 * bags
POOL_LENS = (4, 2, 3, 0, 1, 5, 3, 2)       # mean 2.5 (every prefix of a repetition keeps nnz >= 2 * bags): bpg 16

# ---- embed_bag_fwd_vec: every (dtype pair, LPR, HAS_W, STREAM); dense and CSR, the three combiners in each call --------
for pi, (tdt, odt) in enumerate(PAIRS):
    for li, lpr in enumerate(LPRS):
        for has_w in (False, True):
            for stream in (False, True):
                k = pi * 16 + li * 4 + has_w * 2 + stream
                dim = DIMS[tdt][lpr][(has_w + stream + li) % 2]
                csr = (has_w + stream + pi) % 2 == 0
                batch = (70, 37, 130, 200)[(li + pi) % 4]
                kw = dict(weights="uniform" if has_w else None, id64=k % 3 == 0, off64=csr and (k // 2) % 2 == 0)
                if csr:
                    kw["lens"] = tiled(STREAM_LENS if stream else POOL_LENS, 3 * batch, k)
                elif stream:
                    kw["hots"] = (1, 1, 1) if has_w else (1, 1, 0)      # (unweighted (1, 1, 1) is the pure gather)
                else:
                    kw["hots"] = (2, 5, 1)                              # mean 2: bpg 16
                case(f"vec-{tdt}-{odt}-lpr{lpr}-w{int(has_w)}-s{int(stream)}-{'csr' if csr else 'dense'}-d{dim}", tdt, odt,
                     dim, batch, "vec", lpr, bpg=16, stream=stream, **kw)
case("vec-f32-f32-lpr8-d20-5-pieces", "f32", "f32", MORE_IDLE_DIMS["f32"][8], 70, "vec", 8, bpg=16, hots=(2, 5, 1),
     weights="uniform")
# output slots off their vector alignment: the element-store branch of store_row_piece, per output type and piece width
for tdt, odt in PAIRS:
    case(f"vec-{tdt}-{odt}-unaligned-slots", tdt, odt, DIMS[tdt][8][1], 37, "vec", 8, bpg=10, hots=(3, 4, 3),
         weights="uniform", lead=1, gap=3, tail=2)
    case(f"vec-{tdt}-{odt}-out-base-off-1", tdt, odt, DIMS[tdt][16][0], 37, "vec", 16, bpg=16, stream=True,
         lens=tiled(STREAM_LENS, 111, 7), base_off=1)

# ---- bags per group: mean bag lengths 1, 2, 3, 5, 9, 40 give bpg 16, 16, 10, 6, 3, 1; batch 1, one full wave, one more --
for mean, bpg, (tdt, odt), lpr in ((1, 16, PAIRS[1], 8), (2, 16, PAIRS[0], 16), (3, 10, PAIRS[2], 32),
                                   (5, 6, PAIRS[3], 64), (9, 3, PAIRS[0], 8), (40, 1, PAIRS[1], 16)):
    wave = (64 // lpr) * bpg
    for bi, batch in enumerate((1, wave, wave + 1)):
        kw = dict(weights="uniform", id64=bi == 1)
        if bi == 1:      # CSR around the mean: (+1, 0, -1) repeated keeps nnz // bags == mean
            kw.update(lens=tuple(mean + (1, 0, -1)[i % 3] for i in range(3 * batch)), off64=mean % 2 == 1)
        else:
            kw["hots"] = (mean, mean, mean)
        case(f"bpg{bpg}-mean{mean}-batch{batch}-lpr{lpr}", tdt, odt, DIMS[tdt][lpr][0], batch, "vec", lpr, bpg=bpg,
             stream=mean == 1, **kw)

# ---- window edges: a group's stream of WIN - 1, WIN and WIN + 1 lookups (WIN = 8 * LPR), mean and sqrtn with weights ---
for lpr, (tdt, odt) in ((8, PAIRS[0]), (64, PAIRS[1])):
    for hot in (8 * lpr - 1, 8 * lpr, 8 * lpr + 1):
        case(f"window-lpr{lpr}-hot{hot}", tdt, odt, DIMS[tdt][lpr][1], 3, "vec", lpr, bpg=1, feats=((0, MEAN), (2, SQRTN)),
             hots=(hot, hot), weights="uniform", id64=hot % 2 == 0)


def _edge_group(win):
    """Six bags for one group of bpg = 6: the second ends on the last slot of a window, an empty bag, the next starts on
    slot 0 of the next window, one spans three windows, the last is empty."""
    return (win - 24, 24, 0, 10, 2 * win + 22, 0)


for lpr, (tdt, odt), batch in ((8, PAIRS[0], 96), (16, PAIRS[1], 200)):
    win, group = 8 * lpr, _edge_group(8 * lpr)
    # the other bags are short, so that nnz // bags == 5 and the planner groups six bags
    fill = 5 * batch - sum(group) + 3
    rest = np.full(batch - 6, fill // (batch - 6), np.int64)
    rest[:fill - int(rest.sum())] += 1
    lens = (group + tuple(int(v) for v in rest)) * 2
    assert sum(lens) // (2 * batch) == 5
    case(f"window-csr-edges-lpr{lpr}", tdt, odt, DIMS[tdt][lpr][0], batch, "vec", lpr, bpg=6,
         feats=((0, MEAN), (2, SQRTN)), lens=lens, weights="uniform", off64=lpr == 16)

# a mean bag whose weights cancel: den is exactly 0, the output and the scale are exactly 0
case("den0-pm-half-dense", "f32", "f32", 32, 37, "vec", 8, bpg=16, hots=(2, 2, 2), weights="pm_half")
case("den0-pm-half-generic", "f32", "f32", 7, 37, "generic", 8, hots=(2, 2, 2), weights="pm_half")

# ---- hot rows staged in LDS (KRS_EMBED_OPT_HOTROWS 64 | 128): bf16 / bf16, 256-byte rows, unweighted -------------------
# table 1 is shorter than either window; batch 200 gives workgroups on one feature (staging) and, where a feature's
# waves are no multiple of four, workgroups that straddle two (no staging); batch 70 straddles in the first workgroup
for hr in (64, 128):
    for stream in (False, True):
        for csr in (False, True):
            batch = 200 if csr == stream else 70
            kw = (dict(lens=tiled(STREAM_LENS if stream else (3, 4, 0, 5, 3, 3), 3 * batch, hr + csr), off64=hr == 128)
                  if csr else dict(hots=(1, 1, 0) if stream else (3, 4, 3)))
            case(f"hotrows{hr}-s{int(stream)}-{'csr' if csr else 'dense'}", "bf16", "bf16", 128, batch, "vec", 16,
                 bpg=16 if stream else 10, stream=stream, hot_rows=hr, hot_opt=hr, id64=hr == 64 and csr, **kw)
# the option set where the gate refuses it: weights, another dim, another dtype pair
case("hotrows128-refused-weights", "bf16", "bf16", 128, 70, "vec", 16, bpg=10, hots=(3, 4, 3), weights="uniform",
     hot_opt=128)
case("hotrows64-refused-dim80", "bf16", "bf16", 80, 70, "vec", 16, bpg=10, hots=(3, 4, 3), hot_opt=64)
case("hotrows64-refused-f32out", "bf16", "f32", 128, 70, "vec", 16, bpg=10, hots=(3, 4, 3), hot_opt=64)

# ---- embed_gather_hot1_rows (sample-major): both table types x four LPR; aligned slots, slots off by 1 and by N - 1 ----
for tdt in ("f32", "bf16"):
    n_vec = 16 // ES[tdt]
    for li, lpr in enumerate(LPRS):
        dim_idle, dim_full = DIMS[tdt][lpr]
        case(f"rows-{tdt}-lpr{lpr}-aligned", tdt, tdt, dim_idle, 70, "hot1_rows", lpr, hots=(1, 1, 1), specials=True,
             id64=li % 2 == 1, bad=BAD64 if li == 1 else (BAD32 if li == 2 else ()))
        # slot 0 off by one element, slot 1 by N - 1, on 16-byte rows: the element-store branch
        case(f"rows-{tdt}-lpr{lpr}-slots-off-1-and-{n_vec - 1}", tdt, tdt, dim_full if li % 2 else dim_idle, 37,
             "hot1_rows", lpr, hots=(1, 1, 1), lead=1, gap=n_vec - 2, tail=1, ld_mult=n_vec, id64=li % 2 == 0,
             bad=BAD32 if li == 0 else ())
    case(f"rows-{tdt}-mixed-hots-2-0-1", tdt, tdt, DIMS[tdt][16][1], 70, "hot1_rows", 16, hots=(2, 0, 1),
         feats=((0, MEAN), (1, SUM), (2, SQRTN)), bad=BAD32)
    case(f"rows-{tdt}-mixed-hots-0-1-2-int64", tdt, tdt, DIMS[tdt][8][0], 37, "hot1_rows", 8, hots=(0, 1, 2),
         feats=((0, MEAN), (1, SQRTN), (2, SQRTN)), id64=True, bad=BAD64, lead=1, gap=n_vec - 2, tail=1, ld_mult=n_vec)
    case(f"rows-{tdt}-batch1", tdt, tdt, DIMS[tdt][32][1], 1, "hot1_rows", 32, hots=(1, 1, 1))
    case(f"rows-{tdt}-128-features", tdt, tdt, 16 // ES[tdt], 3, "hot1_rows", 8, feats=((0, SUM),) * 128, hots=(1,) * 128,
         gap=0)

# ---- embed_gather_hot1 (feature-major): four pairs x four LPR; batch 1, 64, 70 -----------------------------------------
for pi, (tdt, odt) in enumerate(PAIRS):
    n_vec = 16 // ES[odt]
    for li, lpr in enumerate(LPRS):
        dim_idle, dim_full = DIMS[tdt][lpr]
        batch = (1, 64, 70)[(pi + li) % 3]
        if tdt != odt:       # reached by the dtype pair alone: aligned and unaligned stores
            bad = BAD64 if li == 0 else (BAD32 if li == 3 else ())
            case(f"hot1-{tdt}-{odt}-lpr{lpr}-aligned", tdt, odt, dim_idle, 70 if bad and batch == 1 else batch, "hot1", lpr,
                 hots=(1, 1, 1), specials=True, id64=li % 2 == 0, bad=bad)
            case(f"hot1-{tdt}-{odt}-lpr{lpr}-slots-off-1", tdt, odt, dim_full, (70, 1, 64)[(pi + li) % 3], "hot1", lpr,
                 hots=(1, 1, 1), specials=True, lead=1, gap=3, tail=2)
        else:                # equal types: only an unaligned output base or row stride leaves the sample-major kernel
            case(f"hot1-{tdt}-{odt}-lpr{lpr}-out-base-off-1", tdt, odt, dim_idle, batch, "hot1", lpr, hots=(1, 1, 1),
                 specials=True, base_off=1, ld_mult=n_vec, id64=li % 2 == 1, bad=BAD64 if li == 1 else ())
            case(f"hot1-{tdt}-{odt}-lpr{lpr}-odd-row-stride", tdt, odt, dim_full, (64, 70, 1)[(pi + li) % 3], "hot1",
                 lpr, hots=(1, 1, 1), tail=9, bad=BAD32 if li == 3 else ())
    # a feature whose hot is not 1 in a call with one lookup per bag on average: the slow loop
    case(f"hot1-{tdt}-{odt}-mixed-hots-1-2-0", tdt, odt, DIMS[tdt][16][0], 70, "hot1", 16, hots=(1, 2, 0),
         feats=((0, SQRTN), (1, MEAN), (2, MEAN)), base_off=1, bad=BAD32, id64=pi % 2 == 0)
case("hot1-f32-f32-129-features-dim4", "f32", "f32", 4, 70, "hot1", 8, feats=((0, SUM),) * 129, hots=(1,) * 129, gap=0,
     bad=BAD32)

# ---- embed_bag_fwd_generic: four pairs, dense and CSR -------------------------------------------------------------------
GENERIC_LPR = {7: 8, 260: 64, 320: 64, 12: 16, 20: 32}
for pi, (tdt, odt) in enumerate(PAIRS):
    for di, dim in enumerate(GENERIC_DIMS[tdt]):
        for csr in (False, True):
            k = pi * 8 + di * 2 + csr
            batch = 37 if dim > 100 else 70
            kw = dict(lens=tiled((0, 1, 3, 2, 6, 0, 4, 1), 3 * batch, k), off64=k % 3 == 0) if csr else dict(hots=(3, 1, 4))
            case(f"generic-{tdt}-{odt}-d{dim}-{'csr' if csr else 'dense'}", tdt, odt, dim, batch, "generic",
                 GENERIC_LPR[dim], weights="uniform" if (di + csr) % 2 else None, id64=k % 2 == 1,
                 bad=(BAD64 if k % 2 else BAD32) if di == 0 else (), lead=(8, 1)[csr], gap=(8, 3)[csr], **kw)
case("generic-f32-f32-d7-one-lookup-per-bag", "f32", "f32", 7, 70, "generic", 8, hots=(1, 1, 1))

# ---- ids: both types with out-of-range ids on the pooled kernel (the gather and generic families carry theirs above) --
for pi, (tdt, odt) in enumerate(PAIRS):
    for id64 in (False, True):
        for stream in (False, True):
            lpr = LPRS[(pi + id64 * 2 + stream) % 4]
            csr = (pi + stream) % 2 == 0
            kw = (dict(lens=tiled(STREAM_LENS if stream else POOL_LENS, 210, pi), off64=id64) if csr
                  else dict(hots=(1, 1, 1) if stream else (2, 5, 1), weights="uniform"))
            case(f"ids-{tdt}-{odt}-{'i64' if id64 else 'i32'}-s{int(stream)}-lpr{lpr}", tdt, odt, DIMS[tdt][lpr][0], 70,
                 "vec", lpr, bpg=16, stream=stream, id64=id64, bad=BAD64 if id64 else BAD32, **kw)
# valid id 0 and a finite row 0 (every other case keeps its ids off the poisoned row)
case("row0-valid-vec", "bf16", "bf16", 128, 70, "vec", 16, bpg=16, hots=(2, 5, 1), poison=False)
case("row0-valid-rows", "f32", "f32", 64, 70, "hot1_rows", 16, hots=(1, 1, 1), poison=False)
case("row0-valid-hot1", "f32", "bf16", 64, 70, "hot1", 16, hots=(1, 1, 1), poison=False)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- the inputs of a case ----------------------------------------------------------------------------------------------

def _round_to(a, dt):
    """float32 values rounded to the dtype `dt` ("f32" | "bf16", round to nearest even), as float32"""
    if dt == "f32":
        return a
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


def _special_values():
    """float32 values for the gather kernels: signed zeros, +-inf, NaN, fp32 and bf16 subnormals, exact ties between two
    bf16 numbers (to even both ways), the largest finite values (which round to inf in bf16), ordinary neighbours"""
    bits = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x00000001, 0x807fffff, 0x00010000,
                     0x80008000, 0x00018000, 0x3f808000, 0x3f818000, 0xbf808000, 0x3f808001, 0x3f807fff, 0x7f7fffff,
                     0xff7f8000, 0x7f7f7fff, 0x3f800000, 0xc0490fdb], np.uint32)
    return bits.view(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Host inputs of a case: tables (float32 arrays whose values are exact in the table dtype), ids, offsets | None,
    weights | None.  Deterministic in the case name."""
    c = BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n_tables = max(t for t, _ in c.feats) + 1
    tables = []
    for t in range(n_tables):
        tab = _round_to(rng.uniform(-1, 1, (c.vocabs[t], c.dim)).astype(np.float32), c.tdt)
        if c.specials:
            sp = _special_values()
            flat = tab.reshape(-1)
            pos = rng.choice(flat.shape[0] - c.dim, size=4 * sp.shape[0], replace=False) + c.dim
            flat[pos] = np.tile(sp, 4)
            tab = _round_to(tab, c.tdt)
        if c.poison:
            tab[0] = np.nan
        tables.append(tab)
    if c.csr:
        lens = np.asarray(c.lens, np.int64)
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64 if c.off64 else np.int32)
    else:
        lens = np.repeat(np.asarray(c.hots, np.int64), c.batch)
        offsets = None
    feat_of = np.repeat(np.arange(c.n_feats), c.batch)
    vocab_of = np.repeat(np.array([c.vocabs[c.feats[f][0]] for f in feat_of], np.int64), lens)
    nnz = int(lens.sum())
    assert nnz == c.nnz
    ids = (rng.integers(0, 2 ** 31, nnz) % (vocab_of - c.poison) + c.poison).astype(np.int64)
    if c.specials:      # every row is looked up somewhere, the planted values included
        for f in range(c.n_feats):
            sl = slice(f * c.batch, (f + 1) * c.batch)
            v = c.vocabs[c.feats[f][0]]
            ids[sl] = (np.arange(c.batch) * 7 + rng.integers(0, v)) % (v - c.poison) + c.poison
    if c.bad:
        assert nnz > len(c.bad), name           # every value is planted, a valid lookup remains
        pos = rng.choice(nnz, size=min(nnz - 1, max(2 * len(c.bad), nnz // 16)), replace=False)
        for i, p in enumerate(pos):
            b = c.bad[i % len(c.bad)]
            ids[p] = vocab_of[p] if b == "vocab" else b
    ids = ids.astype(np.int64 if c.id64 else np.int32)
    if c.weights == "uniform":
        weights = rng.uniform(0.25, 1.0, nnz).astype(np.float32)
    elif c.weights == "pm_half":
        weights = np.where(np.arange(nnz) % 2 == 0, 0.5, -0.5).astype(np.float32)
    else:
        weights = None
    return dict(tables=tables, ids=ids, offsets=offsets, weights=weights)
