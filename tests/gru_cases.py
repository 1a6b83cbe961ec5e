"""The case table of K20 (krs_gru_fwd / _bwd), shared by tests/test_gru_host.py (no GPU) and tests/test_gru_matrix_gpu.py.

Every case has B <= 65.  The table covers B in {1, 3, 31, 32, 33, 65} (a ragged last slab, more than one workgroup),
L in {1, 2, 7, 33}; bf16 at U in {8, 31, 32, 33, 50, 64, 65, 128} (the fast route, every UPAD) and at U in {160, 256}
(the generic route); fp32 at U in {8, 50, 128, 200}; the masks none / right-padded / left-padded / one all-padding
sequence / holes in the middle / first step masked; initial_state given and absent (given with the first step
masked); gradients arriving at the sequence output, at the final state, or at both; no recurrent bias; xz as a strided
view of a wider buffer; and one "sticky" case whose update gate sits near 1, so that a step changes the state by less
than a bf16 ulp (what keeping the carried state in fp32 is for).

Bounds.  fp32 cases: the project's standing rtol = atol = 1e-5 against float64.  bf16 cases: for each case and output,
E is the largest distance between the restatement that rounds where the fast path rounds (tests/gru_restatement.py,
bf16=True) and the exact one; a result must be within
    2 E + 2^-8 |ref|
of the exact restatement, element by element (the factor 2 for the summation order, the second term the output's own
half ulp).  Nothing here is measured on a GPU: E is computed on the CPU when this module is imported.  E divided by
the output's largest magnitude reaches OBSERVED_MAX_E = 0.056 over the whole table (the assertion at the end of this
module and the host test recompute it).  That maximum is the sticky case's d recurrent_kernel: z ~ 0.9975 stored in
the bf16 reserve is 1 or 0.9961, so the backward's factor 1 - z is off by up to its own size.  Without that case the
maximum is 0.020 (a gradient too); the forward's outputs stay at 0.0032 everywhere, the sticky case included.
The rounding restatement leaves unrounded what nothing reads back (the final state, dxz, dh0, the weight gradients), so
that an output's own half ulp enters its bound once, as the second term; hs is rounded there because the backward reads
h_{t-1} from it.
"""

from typing import NamedTuple

import numpy as np

from tests import gru_restatement as R

FP32_TOL = 1e-5
OBSERVED_MAX_E = 0.056

BATCHES = (1, 3, 31, 32, 33, 65)
LENGTHS = (1, 2, 7, 33)
BF16_FAST_U = (8, 31, 32, 33, 50, 64, 65, 128)
BF16_GENERIC_U = (160, 256)
FP32_U = (8, 50, 128, 200)
MASKS = ("none", "right", "left", "allpad", "holes", "first")
GRADS = ("seq", "last", "both")
FAST, GENERIC = 1, 2
OUTPUTS = ("hs", "h_last", "dxz", "dh0", "drk", "drb")


class Case(NamedTuple):
    name: str
    dtype: str          # "bf16" | "fp32"
    b: int
    l: int
    u: int
    mask: str
    h0: bool            # an initial state is given
    grad: str           # where gradients arrive: "seq" | "last" | "both"
    bias: bool          # a recurrent bias is given
    pad: int            # -1: xz is contiguous; >= 0: a view of a [B L, 3U + pad] buffer
    sticky: bool        # xz_z shifted by +6: z ~ 0.9975
    route: int          # claimed: FAST | GENERIC
    upad: int           # claimed: 32 | 64 | 128, 0 on the generic route


def _claim(dtype, u):
    if dtype == "bf16" and u <= 128:
        return FAST, 32 if u <= 32 else 64 if u <= 64 else 128
    return GENERIC, 0


def _build():
    cases, n = [], 0

    def add(dtype, u, *, b=None, l=None, mask=None, h0=None, grad=None, bias=True, pad=-1, sticky=False):
        nonlocal n
        b = BATCHES[n % len(BATCHES)] if b is None else b
        l = LENGTHS[(n // 2) % len(LENGTHS)] if l is None else l
        mask = MASKS[(n + n // len(MASKS)) % len(MASKS)] if mask is None else mask
        if mask == "allpad":
            b = max(b, 3)
        if mask in ("holes", "first"):
            l = max(l, 7)
        h0 = (mask == "first" or n % 3 == 0) if h0 is None else h0
        grad = GRADS[n % 3] if grad is None else grad
        route, upad = _claim(dtype, u)
        name = f"{dtype}-b{b}l{l}u{u}-{mask}-{'h0' if h0 else 'zero'}-{grad}" + ("" if bias else "-nobias") \
            + (f"-pad{pad}" if pad >= 0 else "") + ("-sticky" if sticky else "")
        cases.append(Case(name, dtype, b, l, u, mask, bool(h0), grad, bool(bias), pad, bool(sticky), route, upad))
        n += 1

    for u in BF16_FAST_U:
        for _ in range(3):
            add("bf16", u)
    n += 1      # (shifts the cycles, so that the generic routes meet other batch sizes and masks)
    for u in BF16_GENERIC_U:
        for _ in range(3):
            add("bf16", u)
    for u in FP32_U:
        for _ in range(3):
            add("fp32", u)
    add("bf16", 64, b=65, l=33, mask="first", h0=True, grad="both")
    add("bf16", 128, b=33, l=33, mask="holes", h0=True, grad="both")
    add("bf16", 32, b=65, l=7, mask="left", h0=True, grad="both", bias=False)
    add("bf16", 50, b=33, l=7, mask="right", grad="seq", pad=5)          # a stride that is no whole chunk
    add("bf16", 64, b=32, l=2, mask="none", grad="last", pad=8)
    add("bf16", 256, b=31, l=7, mask="allpad", grad="both", bias=False, pad=2)
    add("fp32", 200, b=33, l=33, mask="holes", h0=True, grad="both", pad=3)
    add("fp32", 8, b=65, l=7, mask="first", h0=True, grad="seq", bias=False)
    add("bf16", 128, b=65, l=7, mask="none", grad="both")                # no mask on several workgroups, every route
    add("bf16", 64, b=33, l=2, mask="none", h0=True, grad="seq")
    add("bf16", 160, b=33, l=7, mask="none", grad="last")
    add("fp32", 50, b=65, l=2, mask="none", h0=True, grad="both")
    add("bf16", 32, b=33, l=33, mask="none", h0=True, grad="both", sticky=True)
    return tuple(cases)


CASES = _build()


def valid_of(case: Case):
    """uint8 [B, L] or None."""
    b, l = case.b, case.l
    if case.mask == "none":
        return None
    v = np.zeros((b, l), dtype=np.uint8)
    for x in range(b):
        length = max(1, l - ((x % 4 + 1) * l) // 5)
        if case.mask == "right":
            v[x, :length] = 1
        elif case.mask == "left":
            v[x, l - length:] = 1
        elif case.mask == "allpad":
            if x != 1:
                v[x, :length] = 1
        elif case.mask == "holes":
            v[x, :] = 1
            v[x, 1 + x % 3:l - 1:3] = 0
        elif case.mask == "first":
            v[x, 1 + x % 2:] = 1
    return v


def inputs_of(case: Case, index: int | None = None):
    """float64 arrays the dtype of the case represents exactly: xz [B, L, 3U], rk [U, 3U], rb [3U] (fp32 values) or
    None, h0 [B, U] or None, dhs [B, L, U] or None, dh_last [B, U] or None; valid."""
    if index is None:
        index = [c.name for c in CASES].index(case.name) if case in CASES else 977
    rng = np.random.default_rng(2000 + index)
    b, l, u = case.b, case.l, case.u
    rep = R.round_bf16 if case.dtype == "bf16" else (lambda x: x.astype(np.float32).astype(np.float64))
    xz = rng.standard_normal((b, l, 3 * u))
    if case.sticky:
        xz[:, :, :u] += 6.0
    t = {"xz": rep(xz), "rk": rep(rng.standard_normal((u, 3 * u)) / np.sqrt(u))}
    rb = rng.standard_normal(3 * u) * 0.5
    t["rb"] = rb.astype(np.float32).astype(np.float64) if case.bias else None
    h0 = rep(rng.standard_normal((b, u)))
    t["h0"] = h0 if case.h0 else None
    dhs, dh_last = rep(rng.standard_normal((b, l, u))), rep(rng.standard_normal((b, u)))
    t["dhs"] = dhs if case.grad in ("seq", "both") else None
    t["dh_last"] = dh_last if case.grad in ("last", "both") else None
    t["valid"] = valid_of(case)
    return t


def compute(case: Case, t: dict, *, bf16=False, defect=None):
    """hs, h_last, dxz, dh0, drk, drb of the restatement."""
    f = R.forward(t["xz"], t["rk"], t["rb"], t["valid"], t["h0"], bf16=bf16, defect=defect)
    g = R.backward(t["rk"], t["valid"], t["h0"], f, t["dhs"], t["dh_last"], bf16=bf16)
    return {"hs": f["hs"], "h_last": f["h_last"], **g}


def reference(case: Case, t: dict):
    return compute(case, t)


def rounding_distance(case: Case, t: dict, ref: dict):
    """E per output: max |rounding restatement - exact restatement| (bf16 cases)."""
    rounded = compute(case, t, bf16=True)
    return {key: float(np.abs(rounded[key] - ref[key]).max(initial=0.0)) for key in OUTPUTS}


def bounds(case: Case, t: dict, ref: dict):
    """Per-element bounds of every output."""
    if case.dtype == "fp32":
        return {key: FP32_TOL + FP32_TOL * np.abs(ref[key]) for key in OUTPUTS}
    e = rounding_distance(case, t, ref)
    return {key: 2.0 * e[key] + 2.0 ** -8 * np.abs(ref[key]) for key in OUTPUTS}


def worst_ratio(got: dict, ref: dict, bound: dict, keys=OUTPUTS):
    """max over outputs and elements of |got - ref| / bound (0 / 0 = 0; anything non-finite = inf)."""
    worst = 0.0
    for key in keys:
        g = np.asarray(got[key], dtype=np.float64)
        if g.shape != ref[key].shape or not np.isfinite(g).all():
            return float("inf")
        err = np.abs(g - ref[key])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / bound[key])
        if ratio.size:
            worst = max(worst, float(ratio.max()))
    return worst


def _table():
    """(inputs, reference, bounds, E / max |ref|) of every case, computed once when the table is imported."""
    out = []
    for index, case in enumerate(CASES):
        t = inputs_of(case, index)
        ref = reference(case, t)
        rel = 0.0
        if case.dtype == "bf16":
            e = rounding_distance(case, t, ref)
            rel = max(e[key] / max(float(np.abs(ref[key]).max(initial=0.0)), 1e-30) for key in OUTPUTS if e[key] > 0.0)
        out.append((t, ref, bounds(case, t, ref), rel))
    return tuple(out)


TABLE = _table()
MAX_E = max(row[3] for row in TABLE)
assert MAX_E <= OBSERVED_MAX_E <= 1.05 * MAX_E, f"OBSERVED_MAX_E = {OBSERVED_MAX_E} but the table gives {MAX_E:.5f}"
