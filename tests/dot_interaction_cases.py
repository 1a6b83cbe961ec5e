"""The case table of the DotInteraction (K4) route tests: one case per row, with the krs_dot_route record the call must
have.  tests/test_dot_interaction_routes_host.py checks the records against the planner without a GPU and that the table
names every one of the 40 kernel builds of keras_rs_amd/csrc/dot_interaction.hip;
tests/test_dot_interaction_matrix_gpu.py runs every case and asserts the record against what ran.

The records are written from the kernels' own constants (the grid caps, the NG and LDS layout formulas of
dot_bwd_valu_kernel and dot_bwd_mfma_kernel), and the build parameters fr / multi / lps_log2 / spw of every vector-ALU
case are given by hand, not taken from the planner.
"""

import functools
import itertools
import zlib
from dataclasses import dataclass

import numpy as np

ES = {"f32": 4, "bf16": 2}
FIELDS = ("kernel", "dtype", "ks", "fr", "self", "multi", "acc", "ng", "lps_log2", "spw", "launches", "lds_bytes", "blocks")
MODES = ((False, False), (True, False), (False, True), (True, True))     # (self_interaction, skip_gather)


def R(kernel=None, dtype=None, **kw):
    rt = dict.fromkeys(FIELDS, 0)
    rt.update(kernel=kernel, dtype=dtype, **kw)
    return rt


def tri(rows, self_i):
    return rows * (rows + 1) // 2 if self_i else rows * (rows - 1) // 2


def cdiv(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class Case:
    name: str
    direction: str          # "fwd" | "bwd"
    dtype: str
    F: int
    D: int
    B: int
    self_i: bool
    skip: bool
    mask: int               # accumulate_mask (backward)
    off: int                # byte offset of every feature base from a 16-byte boundary
    layout: str             # "concat": views of one buffer | "separate": one tensor per feature, its own row stride
    odd_ld: bool            # separate tensors with odd row strides (plain kernels only)
    route: dict

    @property
    def cols(self):
        return self.F * self.F if self.skip else tri(self.F, self.self_i)


CASES = []


def _add(name, direction, dtype, F, D, B, mode, route, mask=0, off=0, layout="concat", odd_ld=False):
    tag = f"{direction}-{route['kernel'].split('_', 1)[1]}-{dtype}-F{F}-D{D}-B{B}-s{int(mode[0])}g{int(mode[1])}"
    if mask:
        tag += f"-m{mask:x}"
    if off or layout != "concat":
        tag += f"-{layout}{'-odd' if odd_ld else ''}-off{off}"
    CASES.append(Case(f"{name}:{tag}", direction, dtype, F, D, B, mode[0], mode[1], mask, off, layout, odd_ld, route))


def fwd_mfma(dt, D, B):
    ks = {("bf16", 128): 8, ("bf16", 64): 4}.get((dt, D), 0)
    return R("fwd_mfma", dt, ks=ks, fr=32, launches=1, blocks=min(cdiv(B, 4), 2048))


def bwd_mfma(self_i, skip, acc, B):
    # LDS: pointer table, then per wave an 8 KB X image, a 2 KB Gs image and a [32][36] fp32 staging block
    return R("bwd_mfma", "bf16", fr=32, self=int(self_i), acc=int(acc), ng=16 if skip else 9, launches=1,
             lds_bytes=1024 + 2 * (8192 + 2048 + 32 * 36 * 4), blocks=min(cdiv(B, 2), 2048))


def bwd_valu(dt, fr, self_i, multi, acc, lps_log2, spw, B):
    # LDS: pointer table, then [2][spw][tri_cols(FR, SELF) + 1] floats
    return R("bwd_valu", dt, fr=fr, self=int(self_i), multi=int(multi), acc=int(acc),
             ng=16 if multi else cdiv(tri(fr, self_i), 64), lps_log2=lps_log2, spw=spw, launches=1,
             lds_bytes=1024 + 2 * spw * (tri(fr, self_i) + 1) * 4, blocks=min(cdiv(B, spw), 16384))


def generic(direction, dt, F, D, B):
    return R(direction + "_generic", dt, fr=64, launches=1, blocks=min(cdiv(B * F * (D if direction == "bwd" else F), 256), 65536))


def block(direction, dt, F, D, B, skip):
    launches = blocks = 0
    for i0 in range(0, F, 32):
        ni = min(32, F - i0)
        j_end = i0 + ni if direction == "fwd" and not skip else F
        for j0 in range(0, j_end, 128):
            nj = min(128, j_end - j0)
            launches += 1
            blocks += min(cdiv(B * ni * (D if direction == "bwd" else nj), 256), 65536)
    return R(direction + "_block", dt, launches=launches, blocks=blocks)


FULL, ONE, ALT = (1 << 64) - 1, 1 << 1, 0xAAAAAAAAAAAAAAAA
_masks = itertools.cycle((FULL, ONE, ALT, 0x5))


def _low(mask, F):
    return mask & ((1 << min(F, 64)) - 1)


# ---- forward on the matrix cores: dot_fwd_mfma_kernel<ES, KS> -------------------------------------------------------
FWD_MFMA_DIMS = (("bf16", 128), ("bf16", 64), ("bf16", 8), ("bf16", 72), ("f32", 4), ("f32", 12))
_modes = itertools.cycle(MODES)
for (dt, D), F in itertools.product(FWD_MFMA_DIMS, (1, 2, 27, 32)):
    _add("fwd-mfma", "fwd", dt, F, D, 6, next(_modes), fwd_mfma(dt, D, 6))
for (dt, D), mode in zip(FWD_MFMA_DIMS, itertools.cycle(MODES)):      # the other layouts of the output, separate tensors
    _add("fwd-mfma-separate", "fwd", dt, 5, D, 9, mode, fwd_mfma(dt, D, 9), layout="separate")
    _add("fwd-mfma-modes", "fwd", dt, 5, D, 9, MODES[(MODES.index(mode) + 2) % 4], fwd_mfma(dt, D, 9))
for (dt, D), mode in zip((("bf16", 128), ("bf16", 64), ("bf16", 72), ("f32", 12)), MODES):   # the prefetched sample is used
    _add("fwd-mfma-second-turn", "fwd", dt, 2, D, 2048 * 4 + 3, mode, fwd_mfma(dt, D, 2048 * 4 + 3))

# ---- backward on the matrix cores: dot_bwd_mfma_kernel<SELF, ACC, NG, 4> ---------------------------------------------
_shapes = itertools.cycle(((2, 32), (5, 64), (27, 96), (32, 128), (5, 32), (2, 128), (32, 64)))
for _round in range(2):
    for (self_i, skip), acc in itertools.product(MODES, (False, True)):
        F, D = next(_shapes)
        mask = _low(next(_masks), F) if acc else 0
        _add("bwd-mfma", "bwd", "bf16", F, D, 7, (self_i, skip), bwd_mfma(self_i, skip, acc, 7), mask=mask,
             layout="separate" if _round else "concat")
for mode, mask in itertools.product(MODES, (FULL, ONE, ALT)):       # full, one bit, alternating under every mode
    _add("bwd-mfma-masks", "bwd", "bf16", 5, 32, 3, mode, bwd_mfma(mode[0], mode[1], True, 3), mask=_low(mask, 5))
for acc in (False, True):                                             # the next sample's loads are used
    _add("bwd-mfma-second-turn", "bwd", "bf16", 2, 32, 2048 * 2 + 3, (acc, False), bwd_mfma(acc, False, acc, 4099),
         mask=0b11 if acc else 0)

# ---- backward on the vector ALU: dot_bwd_valu_kernel<ES, FR, SELF, MULTI, ACC> ---------------------------------------
# (dtype, F, D, B, mode, fr, multi, lps_log2, spw): lps_log2 = the smallest l with 2 << l >= min(D, 128); spw = what the
# lanes hold (64 >> l), what 1024 gradient elements cover (1024 // cols), what 64 KiB of LDS hold (15 with SELF, else 16)
for dt, (self_i, acc) in itertools.product(("f32", "bf16"), itertools.product((False, True), (False, True))):
    m = lambda F: _low(next(_masks), F) if acc else 0       # noqa: E731
    # one sample per wave, 28 rows: F <= 28 without skip_gather
    _add("bwd-valu-fr28", "bwd", dt, 27, 130, 3, (self_i, False), bwd_valu(dt, 28, self_i, False, acc, 6, 1, 3), mask=m(27))
    # one sample per wave, 32 rows: F = 29 (gathered) and F = 22 ([F, F] layout, 484 columns)
    _add("bwd-valu-fr32", "bwd", dt, 29, 72, 3, (self_i, False), bwd_valu(dt, 32, self_i, False, acc, 6, 1, 3), mask=m(29))
    _add("bwd-valu-fr32", "bwd", dt, 22, 72, 3, (self_i, True), bwd_valu(dt, 32, self_i, False, acc, 6, 1, 3), mask=m(22),
         layout="separate")
    # several samples per wave: D = 16 -> 8 lanes per sample, 8 samples
    _add("bwd-valu-multi", "bwd", dt, 5, 16, 19, (self_i, False), bwd_valu(dt, 32, self_i, True, acc, 3, 8, 19), mask=m(5))
    _add("bwd-valu-multi", "bwd", dt, 5, 16, 19, (self_i, True), bwd_valu(dt, 32, self_i, True, acc, 3, 8, 19), mask=m(5),
         layout="separate")
# the [F, F] layout around the columns a one-sample build loads (512 without SELF, 576 with): F = 23 and 24 without SELF
# were sent to the one-sample build, which never read columns 512 and up
for dt, F, D, self_i, multi in (("f32", 22, 160, False, False), ("f32", 23, 256, False, True), ("bf16", 23, 130, False, True),
                                ("f32", 24, 130, False, True), ("bf16", 24, 160, False, True), ("f32", 24, 6, True, False),
                                ("bf16", 24, 72, True, False), ("f32", 25, 4, True, True), ("bf16", 25, 130, False, True),
                                ("f32", 32, 256, False, True), ("bf16", 32, 130, True, True)):
    lps = {4: 1, 6: 2}.get(D, 6)
    _add("bwd-valu-ff-columns", "bwd", dt, F, D, 3, (self_i, True), bwd_valu(dt, 32, self_i, multi, False, lps, 1, 3))
for dt, F, D, self_i, fr in (("f32", 28, 130, False, 28), ("bf16", 28, 256, True, 28), ("f32", 29, 160, True, 32),
                             ("bf16", 32, 160, False, 32), ("f32", 32, 256, True, 32), ("bf16", 25, 72, False, 28)):
    _add("bwd-valu-rows", "bwd", dt, F, D, 3, (self_i, False), bwd_valu(dt, fr, self_i, False, False, 6, 1, 3))
# small D: the sample count is capped so that the MULTI build's 2 * spw rows of tri_cols(32, SELF) + 1 floats fit 64 KiB
for dt, F, D, mode, lps, spw in (("f32", 6, 2, (False, False), 0, 16), ("bf16", 6, 2, (True, False), 0, 15),
                                 ("f32", 4, 2, (True, True), 0, 15), ("bf16", 8, 4, (False, False), 1, 16),
                                 ("f32", 8, 4, (True, False), 1, 15), ("bf16", 5, 4, (False, True), 1, 16),
                                 ("f32", 10, 6, (True, False), 2, 15), ("bf16", 10, 8, (True, False), 2, 15),
                                 ("f32", 10, 8, (False, False), 2, 16), ("bf16", 5, 6, (False, False), 2, 16),
                                 ("f32", 10, 6, (True, True), 2, 10)):
    _add("bwd-valu-small-dim", "bwd", dt, F, D, 37, mode, bwd_valu(dt, 32, mode[0], True, False, lps, spw, 37))
for mode, mask in itertools.product(MODES, (FULL, ONE, ALT)):       # full, one bit, alternating under every mode
    _add("bwd-valu-masks", "bwd", "f32", 5, 16, 11, mode, bwd_valu("f32", 32, mode[0], True, True, 3, 8, 11), mask=_low(mask, 5))
# bf16 rows 4 bytes off a 16-byte boundary, fp32 rows 8 bytes off: the vector ALU where the matrix cores refuse
_add("bwd-valu-off", "bwd", "bf16", 5, 64, 5, (False, False), bwd_valu("bf16", 32, False, True, False, 5, 2, 5), off=4)
_add("bwd-valu-off", "bwd", "f32", 5, 8, 5, (True, False), bwd_valu("f32", 32, True, True, False, 2, 15, 5), off=8)
# a workgroup takes a second group of samples: B = 16384 * spw + 5, one case per MULTI value
_add("bwd-valu-second-turn", "bwd", "f32", 2, 2, 16384 * 16 + 5, (False, False),
     bwd_valu("f32", 32, False, True, False, 0, 16, 16384 * 16 + 5))
_add("bwd-valu-second-turn", "bwd", "bf16", 2, 130, 16384 + 5, (False, False),
     bwd_valu("bf16", 28, False, False, True, 6, 1, 16384 + 5), mask=0b10)

# ---- the plain kernels: odd D, a base 4 bytes off, odd row strides, F = 33 and 64 ------------------------------------
for direction, dt in itertools.product(("fwd", "bwd"), ("f32", "bf16")):
    mode = next(_modes)
    mask = 0b101 if direction == "bwd" else 0
    _add("generic-odd-dim", direction, dt, 3, 5, 7, mode, generic(direction, dt, 3, 5, 7), mask=mask)
    _add("generic-off", direction, dt, 4, 8, 7, next(_modes), generic(direction, dt, 4, 8, 7), off=4 if dt == "f32" else 2)
    _add("generic-odd-ld", direction, dt, 4, 8, 7, next(_modes), generic(direction, dt, 4, 8, 7), layout="separate", odd_ld=True)
    _add("generic-33", direction, dt, 33, 8, 3, next(_modes), generic(direction, dt, 33, 8, 3), mask=mask << 30)
    _add("generic-64", direction, dt, 64, 4, 2, next(_modes), generic(direction, dt, 64, 4, 2), mask=mask << 61)
# one feature, no pair: the gradient is zero (or what was there); the vector-ALU kernel has no column to clamp its loads to
_add("generic-no-pair", "bwd", "f32", 1, 8, 5, (False, False), generic("bwd", "f32", 1, 8, 5))
_add("generic-no-pair", "bwd", "bf16", 1, 32, 5, (False, False), generic("bwd", "bf16", 1, 32, 5), mask=1)
# more than 65536 x 256 items: the grid-stride loop takes a second turn
_add("generic-wrap", "fwd", "bf16", 33, 1, 15407, (False, False), generic("fwd", "bf16", 33, 1, 15407))
_add("generic-wrap", "bwd", "bf16", 2, 2047, 4099, (True, False), generic("bwd", "bf16", 2, 2047, 4099))

# ---- more than 64 features: the block kernels; masks on bits 0, 31, 32 and 63 ----------------------------------------
BLOCK_MASK = (1 << 0) | (1 << 31) | (1 << 32) | (1 << 63)
for direction, (F, dt) in itertools.product(("fwd", "bwd"), ((65, "f32"), (65, "bf16"), (129, "bf16"), (130, "f32"), (130, "bf16"))):
    for mode in MODES:
        mask = BLOCK_MASK if direction == "bwd" and mode[0] == mode[1] else 0
        _add("block", direction, dt, F, 3, 3, mode, block(direction, dt, F, 3, 3, mode[1]), mask=mask)
_add("block-mask-separate", "bwd", "bf16", 65, 4, 3, (False, True), block("bwd", "bf16", 65, 4, 3, True), mask=BLOCK_MASK,
     layout="separate")
_add("block-mask-separate", "bwd", "f32", 129, 2, 3, (True, False), block("bwd", "f32", 129, 2, 3, False), mask=BLOCK_MASK | ALT,
     layout="separate", odd_ld=True)
_add("block-wrap", "fwd", "bf16", 65, 1, 8193, (False, False), block("fwd", "bf16", 65, 1, 8193, False))
# (the block backward wraps only past 32 * B * D > 2^24 items of 65 and more products each: its float64 reference takes
# seconds, so there is no such case)

BY_NAME = {c.name: c for c in CASES}


def feature_layout(c):
    """(lead, column of every feature, row stride of every feature) in elements, of the buffers the GPU test builds for
    case c.  `concat`: views of one buffer [lead | f0 | gap | f1 | gap ... | tail]; `separate`: one buffer per feature
    [lead | f | tail], each with its own width.  lead carries the case's byte offset from a 16-byte boundary; gaps and
    widths are whole 16-byte pieces (so every feature keeps that offset) unless the case asks for odd row strides."""
    piece = 16 // ES[c.dtype]
    lead = piece + c.off // ES[c.dtype]
    if c.layout == "concat":
        width = -(-(lead + c.F * (c.D + piece) + piece) // 8) * 8 + int(c.odd_ld)
        return lead, [lead + f * (c.D + piece) for f in range(c.F)], [width] * c.F
    return lead, [lead] * c.F, [(-(-(lead + c.D) // 8) * 8 + 8 * (1 + f % 3)) + int(c.odd_ld) for f in range(c.F)]


@functools.lru_cache(maxsize=8)
def inputs(name):
    """The host inputs of a case, stored values widened to float32: X [B, F, D], G [B, cols] (backward), existing
    [B, F, D] (backward with a mask).  Values differ from sample to sample, feature to feature and column to column, and G
    has no symmetry, so a swapped sample, feature, column or triangle half shows."""
    from tests.dot_interaction_restatement import to_storage

    c = BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    bf16 = c.dtype == "bf16"
    h = {"X": to_storage(rng.uniform(-1.0, 1.0, (c.B, c.F, c.D)).astype(np.float32), bf16)}
    if c.direction == "bwd":
        h["G"] = to_storage(rng.uniform(-1.0, 1.0, (c.B, c.cols)).astype(np.float32), bf16)
        h["existing"] = to_storage(rng.uniform(-2.0, 2.0, (c.B, c.F, c.D)).astype(np.float32), bf16) if c.mask else None
    return h
