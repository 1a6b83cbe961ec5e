"""The case table of K22 (krs_ln_fwd / _bwd), shared by tests/test_layer_norm_host.py (no GPU) and
tests/test_layer_norm_matrix_gpu.py.

Every case has n <= 257 rows.  The table covers n in {1, 7, 8, 9, 63, 64, 65, 257} (257 rows are several workgroups of
the weight-gradient partials at every d); d in {1, 2, 7, 8, 50, 64, 100, 128, 129, 256, 1000, 1024, 1999, 2048, 4096}
(every lanes_per_row boundary and every count of registers a lane holds: 8, 16, 32, 64); bf16 and fp32; the three
forms (norm, add-norm, add) with and without residual, gamma, beta; p in {0, 0.2}; eps in {1e-8, 1e-5, 1e-3}; row
strides wider than d that keep and that break the 16-byte claim; a constant row (variance 0: y = beta exactly, its
value 1.5 and the row sums of its multiples being exact in fp32); gamma with zero entries.  Each dtype takes both routes
through every (form, dropout) combination.

Bounds, from the float64 reference alone (tests/layer_norm_restatement.py, `magnitudes`).
fp32 cases: the project's standing rtol = atol = 1e-5; dgamma and dbeta, which sum over rows, relative to their largest
entry: 1e-5 (1 + max |ref|).
bf16 cases.  s is rounded to bf16 once: |ds_ij| <= delta_ij = 2^-8 |s_ij| (half an ulp of bf16 is at most
2^-8 / (1 + 2^-8) of the value).  Everything else follows from an error e, |e_ij| <= delta_ij, in s, to first
order.  With xh = (s - mean) rstd:  d mean = mean_j e;  d var = 2 mean_j((s - mean) e), so d rstd = -rstd^2 mean_j(xh e);
    |d xh_ij| <= A_ij = rstd_i ( delta_ij + mean_j delta_i. + |xh_ij| mean_j(|xh_i.| delta_i.) )
    |d rstd_i| / rstd_i <= rho_i = rstd_i mean_j(|xh_i.| delta_i.)
    s      2^-8 |s|
    y      C [ |gamma_j| A_ij + 2^-8 |y_ij| ]                         (the second term: the output's own rounding)
    mean   C mean_j delta_i. + fp32        rstd   C rstd_i rho_i + fp32          (fp32: 1e-5 (1 + |ref|), they are fp32)
The backward reloads the rounded s with the mean and rstd made from it; dy and dsum are given exactly.  With
g = dy gamma, m2 = mean_j(g xh) and T = rstd (g - mean_j g - xh m2) the norm's share of ds:
    d T_ij = (d rstd / rstd) T_ij - rstd ( d xh_ij m2 + xh_ij mean_j(g_i. d xh_i.) )
    dres   C [ rho_i |T_ij| + rstd_i ( A_ij |m2_i| + |xh_ij| mean_j(|g_i.| A_i.) ) + 2^-8 |dres_ij| ]
    dx     the same bracket times keep_ij / (1 - p), with 2^-8 |dx_ij|
    dgamma C sum_i |dy_ij| A_ij + 1e-5 (1 + max |ref|)                 dbeta   1e-5 (1 + max |ref|)   (no s in it)
The add form takes no statistics: sum and dx carry their own rounding only, dres is dsum exactly.
1 / (1 - p) is the contract's fp32 quotient in the reference too, and s is one fused multiply-add: the 2^-8 |s| holds
however residual and x cancel (the largest relative half ulp of bf16 is 2^-8 / (1 + 2^-8)).
C = 1.952: over the whole table the restatement that rounds where the kernel rounds reaches at most
OBSERVED_MAX = 0.976 of the C = 1 bounds that carry C (s does not; it reaches 0.9961 of its own); the host test
recomputes it and asserts it stays at or under C / 2.  Doubled for the fp32 sums and their order, which the restatement
does not restate, and for the second-order terms.
"""

import functools
from typing import NamedTuple

import numpy as np

from tests import layer_norm_restatement as R

C = 1.952
OBSERVED_MAX = 0.976
FP32_TOL = 1e-5

ROWS = (1, 7, 8, 9, 63, 64, 65, 257)
WIDTHS = (1, 2, 7, 8, 50, 64, 100, 128, 129, 256, 1000, 1024, 1999, 2048, 4096)
EPS = (1e-8, 1e-5, 1e-3)
FORMS = ("norm", "addnorm", "add")
VEC, ELEM = 1, 2
KEYS = ("s", "y", "mean", "rstd", "dres", "dx", "dgamma", "dbeta")


class Case(NamedTuple):
    name: str
    dtype: str          # "bf16" | "fp32"
    n: int
    d: int
    form: str           # "norm" | "addnorm" | "add"
    res: bool           # a residual is given (never in the norm form)
    gamma: bool
    beta: bool
    p: float
    eps: float
    pad: int            # every matrix is the first d columns of an [n, d + pad] buffer
    special: str        # "" | "const" (row 0 of s is 1.5 everywhere) | "gamma0" (every third gamma is 0)
    route: int          # claimed: VEC | ELEM
    lanes: int          # claimed lanes_per_row
    vec: int            # claimed


def lanes_of(d):
    return 8 if d <= 64 else 16 if d <= 128 else 32 if d <= 256 else 64


def per_lane_of(d):
    return 8 if d <= 512 else 16 if d <= 1024 else 32 if d <= 2048 else 64


def _claim(dtype, d, pad):
    chunk = 8 if dtype == "bf16" else 4
    vec = int(d % chunk == 0 and (d + pad) % chunk == 0)       # (bases: allocations are on 256 bytes)
    return (VEC if vec else ELEM), lanes_of(d), vec


def _build():
    cases, k = [], 0

    def add(dtype, d, form, res, p, *, n=None, gamma=None, beta=None, eps=None, pad=0, special=""):
        nonlocal k
        n = ROWS[k % len(ROWS)] if n is None else n
        if d >= 1999 and n > 65 and (k % 5):
            n = 65                                             # (the widest rows: 257 of them only now and then)
        gamma = (k % 4 != 3) if gamma is None else gamma
        beta = (k % 3 != 2) if beta is None else beta
        eps = EPS[k % 3] if eps is None else eps
        if form == "add":
            gamma = beta = False
        route, lanes, vec = _claim(dtype, d, pad)
        name = (f"{dtype}-n{n}d{d}-{form}-{'res' if res else 'nores'}-{'g' if gamma else ''}{'b' if beta else ''}"
                f"-p{p}-eps{eps}" + (f"-pad{pad}" if pad else "") + (f"-{special}" if special else ""))
        cases.append(Case(name, dtype, n, d, form, bool(res), bool(gamma), bool(beta), p, eps, pad, special, route, lanes, vec))
        k += 1

    combos = [("norm", False, 0.0), ("addnorm", True, 0.0), ("addnorm", True, 0.2), ("addnorm", False, 0.2),
              ("add", True, 0.0), ("add", True, 0.2), ("add", False, 0.2)]
    for dtype in ("bf16", "fp32"):
        # both routes through every (form, dropout) combination: d = 64 in whole chunks, d = 50 element-wise
        for d in (64, 50):
            for form, res, p in combos:
                add(dtype, d, form, res, p)
        # every width, two forms each, the combination moving on with the width
        for x, d in enumerate(WIDTHS):
            add(dtype, d, *combos[(2 * x) % 4])
            add(dtype, d, *combos[(2 * x + 1) % len(combos)])
        # 257 rows at the widths of the sequence models and at the widest: several workgroups of partials
        for d in (50, 64, 128, 256, 4096):
            add(dtype, d, "addnorm", True, 0.2, n=257, gamma=True, beta=True)
        # strides: wider than d and still whole chunks; wider and not; an odd stride under an odd width
        add(dtype, 64, "addnorm", True, 0.2, n=65, pad=8)
        add(dtype, 128, "norm", False, 0.0, n=9, pad=16)
        add(dtype, 64, "addnorm", True, 0.0, n=63, pad=3)
        add(dtype, 1024, "add", True, 0.2, n=7, pad=2)
        add(dtype, 50, "addnorm", True, 0.2, n=64, pad=5)
        add(dtype, 4096, "addnorm", True, 0.2, n=9, pad=1)     # the widest row element-wise
        add(dtype, 100, "norm", False, 0.0, n=63, pad=1)       # 16 lanes a row element-wise in fp32 too
        # a constant row, with and without beta; gamma with zero entries
        add(dtype, 64, "norm", False, 0.0, n=8, gamma=True, beta=True, eps=1e-5, special="const")
        add(dtype, 50, "addnorm", True, 0.0, n=7, gamma=True, beta=False, eps=1e-8, special="const")
        add(dtype, 100, "addnorm", True, 0.2, n=9, gamma=True, beta=True, special="gamma0")
        add(dtype, 256, "norm", False, 0.0, n=65, gamma=True, beta=False, special="gamma0")
    return tuple(cases)


CASES = _build()
# one shape on both routes: whole chunks, and the same matrices on a stride that breaks the claim
SHARED_VEC = Case("bf16-shared-vec", "bf16", 65, 128, "addnorm", True, True, True, 0.2, 1e-5, 0, "", VEC, 16, 1)
SHARED_ELEM = SHARED_VEC._replace(name="bf16-shared-elem", pad=1, route=ELEM, vec=0)


def inputs_of(case: Case, index: int | None = None):
    """float64 arrays the dtype of the case represents exactly: x, residual, dy, dsum [n, d] (residual None without one;
    dy None in the add form); gamma, beta fp32-exact [d] or None; seed; draw."""
    if index is None:
        index = [c.name for c in CASES].index(case.name) if case in CASES else 977
    rng = np.random.default_rng(2200 + index)
    n, d = case.n, case.d
    t = {name: R.round_to(rng.standard_normal((n, d)), case.dtype) for name in ("x", "residual", "dy", "dsum")}
    if not case.res:
        t["residual"] = None
    if case.form == "add":
        t["dy"] = None
    if case.form == "norm":
        t["dsum"] = None
    t["gamma"] = R.round_to(1.0 + 0.5 * rng.standard_normal(d), "fp32") if case.gamma else None
    t["beta"] = R.round_to(0.5 * rng.standard_normal(d), "fp32") if case.beta else None
    if case.special == "const":
        assert case.p == 0
        t["x"][0] = 1.5 if t["residual"] is None else 2.0
        if t["residual"] is not None:
            t["residual"][0] = -0.5
    if case.special == "gamma0":
        t["gamma"][::3] = 0.0
    t["seed"] = 0x0FED_CBA9_8765_4321 + index
    t["draw"] = 5 + index
    return t


def _run(case: Case, t: dict, dtype):
    kw = dict(p=case.p, seed=t["seed"], draw=t["draw"])
    f = R.forward(t["x"], t["residual"], t["gamma"], t["beta"], eps=case.eps, norm=case.form != "add", dtype=dtype, **kw)
    g = R.backward(f["s"], f.get("mean"), f.get("rstd"), t["gamma"], t["dy"], t["dsum"], dtype=dtype, **kw)
    return {**f, **g}


def reference(case: Case, t: dict):
    """float64: s, y, mean, rstd, dres, dx, dgamma, dbeta (those the form has)."""
    return _run(case, t, None)


def rounded(case: Case, t: dict):
    """The restatement that rounds where the kernel rounds."""
    return _run(case, t, case.dtype)


@functools.lru_cache(maxsize=None)
def reference_of(index: int):
    """(inputs, reference, bounds) of CASES[index], computed once and shared; treat them as read-only."""
    case = CASES[index]
    t = inputs_of(case, index)
    ref = reference(case, t)
    return t, ref, bounds(case, t, ref)


def bounds(case: Case, t: dict, ref: dict, c: float = C):
    """Per-element bounds of every output in ref."""
    fp32_tol = lambda key: FP32_TOL + FP32_TOL * (np.abs(ref[key]).max() if key in ("dgamma", "dbeta") else np.abs(ref[key]))
    if case.dtype == "fp32":
        return {key: fp32_tol(key) + np.zeros_like(ref[key]) for key in ref}
    mag = R.magnitudes(ref, True, t["gamma"], t["dy"], p=case.p, seed=t["seed"], draw=t["draw"])
    out = {}
    for key in ref:
        if key == "s":
            out[key] = 2.0 ** -8 * np.abs(ref[key])
        elif key in ("mean", "rstd", "dgamma", "dbeta"):
            out[key] = c * mag[key] + fp32_tol(key)
        else:
            out[key] = c * (mag[key] + 2.0 ** -8 * np.abs(ref[key]))
    return out


def worst_ratio(got: dict, ref: dict, bound: dict):
    """(max over outputs and elements of |got - ref| / bound, the output it is at); 0 / 0 = 0, a non-finite value = inf."""
    worst, where = 0.0, ""
    for key in ref:
        g, r, bd = np.asarray(got[key], dtype=np.float64), ref[key], bound[key]
        if not np.isfinite(g).all():
            return np.inf, key
        err = np.abs(g - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / bd)
        if ratio.size and float(ratio.max()) > worst:
            worst, where = float(ratio.max()), key
    return worst, where
