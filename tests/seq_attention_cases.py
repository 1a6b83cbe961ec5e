"""The case table of K19 (krs_seq_attn_fwd / _bwd), shared by tests/test_seq_attention_host.py (no GPU) and
tests/test_seq_attention_matrix_gpu.py.

Every case has B <= 3 and H <= 3.  The table covers L in {1, 31, 32, 33, 64, 65, 127, 128, 129, 200}; bf16 at
Dh in {8, 32, 33, 50, 64, 65, 128} (the fast route, every DPAD with and without whole 16-byte rows) and at Dh = 160 (the
generic route); fp32 at Dh in {8, 50, 64, 160, 256}; causal on and off; the masks none / right-padded / left-padded
(fully masked rows under causal) / one all-padding sequence / only key 0 valid; dropout_p in {0, 0.2}; and q, k, v as
column slices of one packed buffer with a stride of its own.  The fast route is taken through every
(DPAD, causal, masked, dropout) combination, the generic route through every (dtype, causal, masked, dropout).

Bounds.  fp32 cases: the project's standing rtol = atol = 1e-5 against float64.  bf16 cases, per element, from the
float64 reference alone (tests/seq_attention_restatement.py, `magnitudes`):
    out   C 2^-8 sum_j P~_ij |v_jd|                 + 2^-8 |out|     (the second term: the output's own half ulp)
    dv    C 2^-8 sum_i P~_ij |dO_id|                + 2^-8 |dv|
    dq    C 2^-8 scale sum_j A_ij |k_jd|            + 2^-8 |dq|      A_ij = P_ij (keep_ij / (1 - p) |dP~_ij|
    dk    C 2^-8 scale sum_i A_ij |q_id|            + 2^-8 |dk|                   + sum_d |dO_id o_id|)
    lse   2^-18 (1 + scale max_j sum_d |q_id k_jd|)
(P~ and dS are rounded to bf16, relative error 2^-9 each, and delta is formed from the rounded output: every term of
the sums carries an error of that size relative to its magnitude, never relative to the cancelled sum.  lse is fp32:
a score of magnitude x carries about x 2^-24 from its accumulation and x 2^-24 from the exponent's argument, and the
sum and logarithm a few ulp more; 2^-18 leaves a factor of ten.)
C = 1.76: over the whole table the restatement that rounds where the fast path rounds reaches at most
OBSERVED_MAX = 0.8755 of the C = 1 bound (rounded up to 0.88; the test recomputes it and asserts it stays at or under
C / 2); doubled for the summation order.
"""

import math
from typing import NamedTuple

import numpy as np

from tests import seq_attention_restatement as R

C = 1.76
OBSERVED_MAX = 0.8755
FP32_TOL = 1e-5

LENGTHS = (1, 31, 32, 33, 64, 65, 127, 128, 129, 200)
BF16_FAST_DH = (8, 32, 33, 50, 64, 65, 128)
BF16_GENERIC_DH = (160,)
FP32_DH = (8, 50, 64, 160, 256)
MASKS = ("none", "right", "left", "allpad", "key0")
FAST, GENERIC = 1, 2


class Case(NamedTuple):
    name: str
    dtype: str          # "bf16" | "fp32"
    b: int
    h: int
    l: int
    dh: int
    causal: bool
    mask: str
    p: float
    pad: int            # -1: q, k, v are separate contiguous tensors; >= 0: one packed [B L, 3 H Dh + pad] buffer
    route: int          # claimed: FAST | GENERIC
    dpad: int           # claimed: 32 | 64 | 128, 0 on the generic route
    vec: int            # claimed: whole 16-byte rows on 16-byte boundaries (fast route)


def _claim(dtype, h, dh, pad):
    if dtype == "bf16" and dh <= 128:
        ld = h * dh if pad < 0 else 3 * h * dh + pad
        aligned = ld % 8 == 0 and (h * dh) % 8 == 0          # (bases: allocations are on 256 bytes; k, v start at H Dh)
        return FAST, 32 if dh <= 32 else 64 if dh <= 64 else 128, int(aligned and dh % 8 == 0)
    return GENERIC, 0, 0


def _build():
    cases, n = [], 0

    def add(dtype, dh, causal, masked, drop, pad=-1):
        nonlocal n
        l = LENGTHS[n % len(LENGTHS)]
        mask = MASKS[1 + (n // 2) % 4] if masked else "none"
        b, h = 1 + n % 3, 1 + (n // 3) % 3
        if mask == "allpad":
            b = max(b, 2)
        p = 0.2 if drop else 0.0
        route, dpad, vec = _claim(dtype, h, dh, pad)
        name = f"{dtype}-b{b}h{h}l{l}d{dh}-{'causal' if causal else 'full'}-{mask}-p{p}" + (f"-packed{pad}" if pad >= 0 else "")
        cases.append(Case(name, dtype, b, h, l, dh, bool(causal), mask, p, pad, route, dpad, vec))
        n += 1

    flags = [(c, m, d) for c in (0, 1) for m in (0, 1) for d in (0, 1)]
    for dh in BF16_FAST_DH:
        for c, m, d in flags:
            add("bf16", dh, c, m, d)
    for c, m, d in flags:
        add("bf16", 160, c, m, d)
    for rep in range(2):
        for x, (c, m, d) in enumerate(flags):
            add("fp32", FP32_DH[(x + 3 * rep) % len(FP32_DH)], c, m, d)
    add("fp32", 256, 1, 1, 0)
    add("fp32", 160, 0, 1, 1)
    # packed q | k | v buffers: stride 3 H Dh + pad
    add("bf16", 64, 1, 1, 1, pad=0)      # whole chunks
    add("bf16", 64, 1, 1, 0, pad=8)      # whole chunks, a stride that is not the width
    add("bf16", 8, 0, 1, 1, pad=4)       # DPAD 32 on a stride that is not whole chunks
    add("bf16", 128, 1, 0, 1, pad=3)     # DPAD 128 on an odd stride
    add("fp32", 50, 1, 1, 1, pad=5)
    return tuple(cases)


CASES = _build()
SHARED_FAST_GENERIC = Case("bf16-shared-d128-vs-d160", "bf16", 2, 2, 129, 128, True, "right", 0.2, -1, FAST, 128, 1)


def key_valid_of(case: Case):
    """uint8 [B, L] or None."""
    b, l = case.b, case.l
    if case.mask == "none":
        return None
    kv = np.zeros((b, l), dtype=np.uint8)
    for x in range(b):
        length = max(1, l - ((x + 1) * l) // 4)
        if case.mask == "right":
            kv[x, :length] = 1
        elif case.mask == "left":
            kv[x, l - length:] = 1
        elif case.mask == "allpad":
            if x > 0:
                kv[x, :length] = 1
        elif case.mask == "key0":
            kv[x, 0] = 1
    return kv


def inputs_of(case: Case, index: int | None = None):
    """float64 arrays the dtype of the case represents exactly: q, k, v, dout [B, L, H, Dh]; key_valid; scale (the fp32
    value of 1 / sqrt(Dh)); seed; draw."""
    if index is None:
        index = [c.name for c in CASES].index(case.name) if case in CASES else 977
    rng = np.random.default_rng(1900 + index)
    shape = (case.b, case.l, case.h, case.dh)
    t = {name: rng.standard_normal(shape) for name in ("q", "k", "v", "dout")}
    for name in t:
        t[name] = R.round_bf16(t[name]) if case.dtype == "bf16" else t[name].astype(np.float32).astype(np.float64)
    t["key_valid"] = key_valid_of(case)
    t["scale"] = float(np.float32(1.0 / math.sqrt(case.dh)))
    t["seed"] = 0x1234_5678_9ABC_DEF0 + index
    t["draw"] = 3 + index
    return t


def kwargs_of(case: Case, t: dict):
    return dict(key_valid=t["key_valid"], causal=case.causal, scale=t["scale"], dropout_p=case.p, seed=t["seed"],
                draw=t["draw"])


def reference(case: Case, t: dict):
    """float64: out, lse, dq, dk, dv."""
    kw = kwargs_of(case, t)
    f = R.forward(t["q"], t["k"], t["v"], **kw)
    g = R.backward(t["q"], t["k"], t["v"], t["dout"], fwd=f, **kw)
    return {"out": f["out"], "lse": f["lse"], **g}


def bounds(case: Case, t: dict, ref: dict, c: float = C):
    """Per-element bounds of out, lse, dq, dk, dv (lse: where it is finite; -inf must be matched exactly)."""
    if case.dtype == "fp32":
        return {key: FP32_TOL + FP32_TOL * np.abs(np.where(np.isfinite(ref[key]), ref[key], 0.0)) for key in ref}
    mag = R.magnitudes(t["q"], t["k"], t["v"], t["dout"], **kwargs_of(case, t))
    out = {key: c * 2.0 ** -8 * mag[key] + 2.0 ** -8 * np.abs(ref[key]) for key in ("out", "dq", "dk", "dv")}
    out["lse"] = 2.0 ** -18 * mag["lse"]
    return out


def worst_ratio(got: dict, ref: dict, bound: dict):
    """max over outputs and elements of |got - ref| / bound (0 / 0 = 0; a non-finite mismatch = inf)."""
    worst = 0.0
    for key in ("out", "lse", "dq", "dk", "dv"):
        g, r, bd = np.asarray(got[key], dtype=np.float64), ref[key], bound[key]
        fin = np.isfinite(r)
        if not np.array_equal(g[~fin], r[~fin]) or not np.isfinite(g[fin]).all():
            return math.inf
        err = np.abs(g[fin] - r[fin])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / bd[fin])
        if ratio.size:
            worst = max(worst, float(ratio.max()))
    return worst
