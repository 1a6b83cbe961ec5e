"""K2 apply stage, kernel by kernel and mode by mode, against float64.

`run_apply` (keras_rs_amd/csrc/embed_bag_bwd.hip:832-854) sends a call to the vector kernels when the gradient
row is a whole number of 16-byte pieces of at most 1024 bytes, the dtype pair is not fp32 gradients into bf16
tables in a fused mode, and there are at most 512 features and tables (:839-840); `launch_apply_lpr`
(:785-829) then picks LPR = 8 / 16 / 32 / 64 lanes per row from the piece count (:786) and HAS_W x HAS_SCALE
from the call (:792-794), and adds bag_apply_long_kernel for segments longer than 128 lookups (:803) and
bag_apply_finish_kernel for segments longer than 2048 (:818).  Everything else runs bag_apply_generic (:846-851).
Every case below runs all seven modes: dense, compact, SGD, Adagrad, Adam, FTRL (three learning-rate powers),
row-wise Adagrad.  `test_the_cases_cover_the_apply_matrix` checks the table against the dispatch rule.

  case                 pair (table / grad)   dim  reaches                                      W  S
  fast_f32_d20         f32 / f32              20  fast LPR 8 (3 of 8 lanes idle)               y  y
  fast_f32_d36         f32 / f32              36  fast LPR 16 (7 idle)                         -  -
  fast_f32_d128        f32 / f32             128  fast LPR 32                                  y  -
  fast_f32_d132        f32 / f32             132  fast LPR 64 (31 idle)                        -  y
  fast_f32_d256        f32 / f32             256  fast LPR 64                                  y  y
  fast_bf16_d64        bf16 / bf16            64  fast LPR 8                                   y  y
  fast_bf16_d128       bf16 / bf16           128  fast LPR 16                                  -  -
  fast_bf16_d200       bf16 / bf16           200  fast LPR 32 (7 idle)                         y  -
  fast_bf16_d512       bf16 / bf16           512  fast LPR 64                                  -  y
  fast_mixed_d64       f32 / bf16             64  fast LPR 8                                   y  y
  fast_mixed_d264      f32 / bf16            264  fast LPR 64 (31 idle)                        -  y
  fast_f32_d36_desc    f32 / f32              36  fast LPR 16, row_base descending             y  y
  hot_f32_d32_b30000   f32 / f32              32  fast + long + finish LPR 8 (~15 chunks)      y  y
  hot_f32_d128_b4000   f32 / f32             128  fast + long + finish LPR 32                  -  y
  hot_bf16_d64_b4000   bf16 / bf16            64  fast + long + finish LPR 8                   y  -
  hot_mixed_d64_b4000  f32 / bf16             64  fast + long + finish LPR 8                   y  y
  gen_f32_d7           f32 / f32               7  generic (28-byte rows)                       y  y
  gen_f32_d260         f32 / f32             260  generic (1040-byte rows)                     -  -
  gen_f32_d320         f32 / f32             320  generic (1280-byte rows)                     y  y
  gen_bf16_d12         bf16 / bf16            12  generic (24-byte rows)                       y  -
  gen_mixed_d12        f32 / bf16             12  generic (24-byte rows)                       -  y
  gen_bf16tab_d64      bf16 / f32             64  fused: generic; dense / compact: fast LPR 16 y  y
  gen_520_tables       f32 / f32               8  generic (521 features, 520 tables)           y  y
  gen_f32_d7_desc      f32 / f32               7  generic, row_base descending                 y  y

W = per-lookup weights, S = bag_scale given (without it the call is the all-`sum` form, HAS_SCALE = false).
The long kernel reads weights as HAS_W and the scale at run time; the finish kernel reads neither.

The float64 references:
  * gradient: coef = w[p] * scale[bag] (either factor absent = 1); dE[row] += coef * grad[b, col] over the
    dtype-rounded gradient, M[row] = sum |coef * grad|, n = lookups of the row.  The kernels sum one fp32 fma
    chain per lane group in ascending position (fast, generic), or interleaved chains, their partial rows and the
    chunk partials (long, finish): every product passes through at most n roundings, plus one for coef, so
    |got - dE| <= gamma(n + 3) * M, gamma(k) = k u / (1 - k u), u = 2^-24.
  * updates: the Keras rules in float64 (_sgd ... _rowwise below), fed with the kernel's own fp32 summed gradient
    (the dense form on the same plan) and the device's tables and slots before the step: the check is then
    independent of summation order.  That SGD, Adagrad, Adam and FTRL sum exactly like the dense form is checked
    per case by `test_fused_forms_sum_exactly_like_the_dense_form`; row-wise Adagrad has no such identity and takes
    the float64 gradient with its bound instead.  Each tolerance is 2 x (first-order error bound): u per rounding
    times the magnitude of the rounded quantity, errors of inputs carried forward; bf16 tables add one rounding of
    the result (2^-8 relative).
"""

import functools
import math
import zlib
from dataclasses import dataclass

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24     # fp32 unit roundoff
UB = 2.0 ** -8     # bf16 unit roundoff
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
MODES = ["sgd", "adagrad", "adam", "ftrl", "adagrad_rowwise"]
ADAM = (0.85, 0.99, 1e-3)                  # beta_1, beta_2, epsilon (large enough that its placement shows)
# FTRL (learning_rate_power, l1, l2, beta) and initial accumulator.  A zero accumulator only with l2 or beta > 0:
# Keras's own rule divides 0 / 0 when n = g = 0 and l2 = beta = 0.
FTRL = [((-0.5, 0.5, 0.01, 0.1), 0.1), ((-0.25, 0.3, 0.02, 0.0), 0.0), ((0.0, 0.5, 0.0, 0.2), 0.1)]


@dataclass(frozen=True)
class Case:
    tdt: str
    gdt: str
    dim: int
    vocabs: tuple
    tix: tuple             # table of every feature
    hots: tuple            # ids per bag of every feature
    batch: int
    use_w: bool
    use_scale: bool
    lead: int = 2          # first gradient column (2: feature slots are not 16-byte aligned)
    desc: bool = False     # row_base descending with the table index


_SMALL = dict(vocabs=(37, 60, 5), tix=(0, 1, 2, 0), hots=(3, 1, 4, 2), batch=41)
_HOT = dict(vocabs=(3, 5, 20, 400), tix=(0, 1, 2, 3, 0), hots=(2, 1, 1, 1, 1), batch=4000)
_rng520 = np.random.default_rng(520)
_WIDE = dict(vocabs=tuple(int(v) for v in _rng520.integers(3, 12, 520)), tix=tuple(range(520)) + (0,),
             hots=tuple(int(h) for h in _rng520.integers(1, 4, 521)), batch=7)

CASES = {
    "fast_f32_d20": Case("f32", "f32", 20, use_w=True, use_scale=True, **_SMALL),
    "fast_f32_d36": Case("f32", "f32", 36, use_w=False, use_scale=False, lead=0, **_SMALL),
    "fast_f32_d128": Case("f32", "f32", 128, use_w=True, use_scale=False, **_SMALL),
    "fast_f32_d132": Case("f32", "f32", 132, use_w=False, use_scale=True, **_SMALL),
    "fast_f32_d256": Case("f32", "f32", 256, use_w=True, use_scale=True, lead=0, **_SMALL),
    "fast_bf16_d64": Case("bf16", "bf16", 64, use_w=True, use_scale=True, **_SMALL),
    "fast_bf16_d128": Case("bf16", "bf16", 128, use_w=False, use_scale=False, **_SMALL),
    "fast_bf16_d200": Case("bf16", "bf16", 200, use_w=True, use_scale=False, lead=0, **_SMALL),
    "fast_bf16_d512": Case("bf16", "bf16", 512, use_w=False, use_scale=True, **_SMALL),
    "fast_mixed_d64": Case("f32", "bf16", 64, use_w=True, use_scale=True, **_SMALL),
    "fast_mixed_d264": Case("f32", "bf16", 264, use_w=False, use_scale=True, **_SMALL),
    "fast_f32_d36_desc": Case("f32", "f32", 36, use_w=True, use_scale=True, desc=True, **_SMALL),
    "hot_f32_d32_b30000": Case("f32", "f32", 32, vocabs=(3, 6), tix=(0, 1, 0), hots=(2, 1, 1), batch=30000,
                               use_w=True, use_scale=True),
    "hot_f32_d128_b4000": Case("f32", "f32", 128, use_w=False, use_scale=True, lead=0, **_HOT),
    "hot_bf16_d64_b4000": Case("bf16", "bf16", 64, use_w=True, use_scale=False, **_HOT),
    "hot_mixed_d64_b4000": Case("f32", "bf16", 64, use_w=True, use_scale=True, **_HOT),
    "gen_f32_d7": Case("f32", "f32", 7, use_w=True, use_scale=True, **_SMALL),
    "gen_f32_d260": Case("f32", "f32", 260, use_w=False, use_scale=False, **_SMALL),
    "gen_f32_d320": Case("f32", "f32", 320, use_w=True, use_scale=True, lead=0, **_SMALL),
    "gen_bf16_d12": Case("bf16", "bf16", 12, use_w=True, use_scale=False, **_SMALL),
    "gen_mixed_d12": Case("f32", "bf16", 12, use_w=False, use_scale=True, **_SMALL),
    "gen_bf16tab_d64": Case("bf16", "f32", 64, use_w=True, use_scale=True, **_SMALL),
    "gen_520_tables": Case("f32", "f32", 8, use_w=True, use_scale=True, **_WIDE),
    "gen_f32_d7_desc": Case("f32", "f32", 7, use_w=True, use_scale=True, desc=True, **_SMALL),
}


def _gamma(k):
    return k * U / (1.0 - k * U)


def _bf16_round(a: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


@functools.lru_cache(maxsize=None)
def _host(name):
    """Inputs of a case (host copies) and its float64 gradient reference, in FLAT row order (the tables one after
    the other in index order, whatever their row_base)."""
    c = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    D, nt, nf = c.dim, len(c.vocabs), len(c.tix)
    vocabs = np.array(c.vocabs, np.int64)
    flat_base = np.concatenate([[0], np.cumsum(vocabs)[:-1]]).astype(np.int64)
    R = int(vocabs.sum())
    row_bases = (R - flat_base - vocabs) if c.desc else flat_base.copy()
    ids = np.concatenate([rng.integers(0, c.vocabs[c.tix[f]], c.batch * c.hots[f]) for f in range(nf)]).astype(np.int32)
    nnz = ids.size
    w = rng.uniform(0.1, 1.0, nnz).astype(np.float32) if c.use_w else None
    scale = rng.uniform(0.2, 1.5, nf * c.batch).astype(np.float32) if c.use_scale else None
    out_col = np.array([c.lead + f * D for f in range(nf)], np.int64)
    cols = c.lead + nf * D + (0 if c.lead == 0 else 3)
    grad = rng.uniform(-1, 1, (c.batch, cols)).astype(np.float32)
    if c.gdt == "bf16":
        grad = _bf16_round(grad)
    init = rng.uniform(-1, 1, (R, D)).astype(np.float32)
    if c.tdt == "bf16":
        init = _bf16_round(init)
    # per lookup: feature, sample, bag, coefficient, flat row
    n_per_f = np.array([c.batch * h for h in c.hots], np.int64)
    feat = np.repeat(np.arange(nf), n_per_f)
    start = np.concatenate([[0], np.cumsum(n_per_f)[:-1]])
    sample = (np.arange(nnz) - start[feat]) // np.array(c.hots, np.int64)[feat]
    bag = feat * c.batch + sample
    coef = np.ones(nnz)
    if w is not None:
        coef *= w.astype(np.float64)
    if scale is not None:
        coef *= scale.astype(np.float64)[bag]
    tab = np.array(c.tix, np.int64)[feat]
    row = flat_base[tab] + ids
    contrib = coef[:, None] * grad.astype(np.float64)[sample[:, None], out_col[feat][:, None] + np.arange(D)[None, :]]
    dE = np.zeros((R, D))
    M = np.zeros((R, D))
    np.add.at(dE, row, contrib)
    np.add.at(M, row, np.abs(contrib))
    n_row = np.bincount(row, minlength=R)
    # table / learning rate of every flat row; flat row of every global row
    tab_of_row = np.repeat(np.arange(nt), vocabs)
    lrs = np.array([0.05 * (1 + t % 3) for t in range(nt)], np.float32)
    flat_of_global = np.empty(R, np.int64)
    for t in range(nt):
        flat_of_global[row_bases[t]:row_bases[t] + vocabs[t]] = flat_base[t] + np.arange(vocabs[t])
    return dict(c=c, vocabs=vocabs, flat_base=flat_base, R=R, row_bases=row_bases, ids=ids, w=w, scale=scale,
                out_col=out_col, grad=grad, init=init, dE=dE, M=M, n_row=n_row, touched=n_row > 0,
                lr_row=lrs[tab_of_row].astype(np.float64)[:, None], lrs=lrs, flat_of_global=flat_of_global)


class _Run:
    """Device state of one case: tables (views of one [R, D] buffer), slots, descriptors and the plan."""

    def __init__(self, name, mode=None, table_fill=None, lrs=None, ftrl_init=0.1):
        from keras_rs_amd.embedding_ops import FusedBags

        h = self.h = _host(name)
        c = self.c = h["c"]
        dev = self.dev = torch.device("cuda:0")
        D, R = c.dim, h["R"]
        init = h["init"] if table_fill is None else np.full((R, D), table_fill, np.float32)
        self.flat = torch.from_numpy(init).to(dev).to(TORCH_DT[c.tdt])
        spans = [(int(o), int(v)) for o, v in zip(h["flat_base"], h["vocabs"])]
        tables = [self.flat[o:o + v] for o, v in spans]
        self.slot = None
        slots = None
        if mode == "adagrad":
            self.slot = torch.full((R, D), 0.1, dtype=torch.float32, device=dev)
            slots = [self.slot[o:o + v] for o, v in spans]
        elif mode == "adagrad_rowwise":
            self.slot = torch.full((R,), 0.1, dtype=torch.float32, device=dev)
            slots = [self.slot[o:o + v] for o, v in spans]
        elif mode in ("adam", "ftrl"):
            self.slot = torch.zeros(2 * R * D, dtype=torch.float32, device=dev)
            slots = [self.slot[2 * o * D:2 * (o + v) * D].view(2, v, D) for o, v in spans]
            if mode == "ftrl":
                for s in slots:
                    s[0].fill_(ftrl_init)
        lrs = [float(x) for x in (h["lrs"] if lrs is None else lrs)]
        self.fb = FusedBags(tables, [(c.tix[f], "sum", int(h["out_col"][f])) for f in range(len(c.tix))],
                            slots=slots, lrs=lrs)
        self.fb.row_bases[:-1] = h["row_bases"]
        self.ids = torch.from_numpy(h["ids"]).to(dev)
        self.grad = torch.from_numpy(h["grad"]).to(TORCH_DT[c.gdt]).to(dev)
        self.w = None if h["w"] is None else torch.from_numpy(h["w"]).to(dev)
        self.scale = None if h["scale"] is None else torch.from_numpy(h["scale"]).to(dev)
        self.ws = self.fb.plan_backward(self.ids, c.batch, hots=list(c.hots))
        self.kw = dict(hots=list(c.hots), weights=self.w, bag_scale=self.scale)

    def dense(self):
        h = self.h
        buf = torch.zeros((h["R"], self.c.dim), dtype=torch.float32, device=self.dev)
        out = [buf[int(o):int(o) + int(v)] for o, v in zip(h["flat_base"], h["vocabs"])]
        self.fb.backward_dense(self.ws, self.grad, self.c.batch, self.ids.numel(), out=out, **self.kw)
        return buf.cpu().numpy()

    def fused(self, kind, hyper=None):
        self.fb.backward_fused(kind, self.ws, self.grad, self.c.batch, self.ids.numel(), hyper=hyper, **self.kw)

    def table(self):
        """(values as float64, raw bits) of the flat table buffer."""
        t = self.flat.detach().cpu()
        bits = t.view(torch.int16).numpy().copy() if t.dtype == torch.bfloat16 else t.numpy().view(np.int32).copy()
        return t.float().numpy().astype(np.float64), bits

    def planes(self):
        """Slot planes in flat row order: [R, D] (Adagrad), [R] (row-wise), or two [R, D] (Adam m, v / FTRL n, z)."""
        s = self.slot.cpu().numpy()
        if s.ndim == 2 or s.size == self.h["R"]:
            return (s.copy(),)
        D = self.c.dim
        p0, p1 = [], []
        for o, v in zip(self.h["flat_base"], self.h["vocabs"]):
            blk = s[2 * o * D:2 * (o + v) * D].reshape(2, v, D)
            p0.append(blk[0])
            p1.append(blk[1])
        return np.concatenate(p0), np.concatenate(p1)


def _check_grad(got, h, rows):
    """|got - dE| <= gamma(n + 3) * M on the flat rows `rows`."""
    tol = _gamma(h["n_row"][rows] + 3)[:, None] * h["M"][rows]
    err = np.abs(got.astype(np.float64) - h["dE"][rows])
    bad = err > tol
    assert not bad.any(), (f"{int(bad.sum())} gradient elements out of bound; worst err/tol "
                           f"{float(np.max(err / np.maximum(tol, 1e-300))):.3g}")


def _close(name, got, ref, tol):
    err = np.abs(got - ref)
    bad = ~(err <= tol)
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} out of bound; worst err/tol "
                           f"{float(np.max(err / np.maximum(tol, 1e-300))):.3g}")


# ---- float64 Keras rules; each returns the new values and their tolerances (2 x the first-order bound) ----------
def _sgd(w, g, lr):
    step = lr * g
    return (w - step,), (2 * (U * (np.abs(w) + np.abs(step)) + U * np.abs(step)),)


def _adagrad(w, a, g, lr):
    """acc += g^2 (one fmaf); w -= lr * g / sqrt(acc), no epsilon: lr * g, the square root of an input that is u off,
    the square root, the quotient, the difference."""
    a1 = a + g * g
    step = lr * g / np.sqrt(a1)
    return (w - step, a1), (2 * (U * (np.abs(w) + np.abs(step)) + 3.5 * U * np.abs(step)), 2 * U * a1)


def _adam(w, m, v, g, lr, hp, t):
    """Keras Adam (lazy): m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2); w -= lr * corr * m / (sqrt(v) + eps),
    corr = sqrt(1 - b2^t) / (1 - b1^t) (in fp32, as the call passes it).  1 - b is exact in fp32 (Sterbenz)."""
    b1, b2, eps = (float(np.float32(x)) for x in hp)
    corr = float(np.float32(math.sqrt(1 - hp[1] ** t) / (1 - hp[0] ** t)))
    e1, e2 = 1.0 - b1, 1.0 - b2
    alpha = lr * corr
    m1 = m + (g - m) * e1
    v1 = v + (g * g - v) * e2
    den = np.sqrt(v1) + eps
    step = alpha * m1 / den
    tol_m = 3 * U * (np.abs(m) + e1 * (np.abs(g) + np.abs(m)))
    tol_v = 4 * U * (v + e2 * (g * g + v))
    tol_den = np.where(v1 > 0, tol_v / np.sqrt(np.where(v1 > 0, v1, 1)), np.sqrt(tol_v)) + U * np.sqrt(v1) + U * den
    tol_step = np.abs(step) * (3 * U + tol_den / den) + alpha * tol_m / den
    tol_w = U * (np.abs(w) + np.abs(step)) + tol_step
    return (w - step, m1, v1), (2 * tol_w, 2 * tol_m, 2 * tol_v)


def _ftrl(w, n, z, g, lr, hp):
    """Keras Ftrl without l2 shrinkage: n' = n + g^2; z += g - (n'^-p - n^-p) / lr * w;
    w = (clip(z, -l1, l1) - z) / (n'^-p / lr + 2 (l2 + beta / (2 lr))).  n'^-p - n^-p cancels: its error is bounded
    by the magnitudes of both powers (sqrtf is correctly rounded; powf is allowed 4 ulp = 8 u), carried through
    / lr * w into z; clip(z) - z is 1-Lipschitz in z, so w inherits z's error / quad."""
    p, l1, l2, beta = (float(np.float32(x)) for x in hp)
    c_pow = 1.0 if p == -0.5 else 8.0
    n1 = n + g * g
    pn, po = n1 ** -p, n ** -p
    t = (pn - po) / lr * w
    z1 = z + g - t
    quad = pn / lr + 2 * (l2 + beta / (2 * lr))
    zc = np.clip(z1, -l1, l1)
    w1 = (zc - z1) / quad
    e_pn = (2 * abs(p) + c_pow) * U
    err_t = (e_pn * pn + c_pow * U * po + U * (pn + po)) / lr * np.abs(w) + 2 * U * np.abs(t)
    tol_z = 2 * U * (np.abs(z) + np.abs(g) + np.abs(t)) + err_t
    tol_w = (tol_z + U * np.abs(zc - z1)) / quad + (e_pn + 6 * U) * np.abs(w1)
    return (w1, n1, z1), (2 * tol_w, 2 * 2 * U * n1, 2 * tol_z), (np.abs(z1) + tol_z < l1)


def _rowwise(w, a, g, g_err, lr, dim):
    """acc[row] += mean_j g_j^2; w -= lr * g / sqrt(acc).  The sum of squares of non-negative terms passes through
    at most 8 products per lane, 6 butterfly levels, the division by dim and the add: 16 u * acc'.  No identity
    pins this mode's summed gradient to the dense form's, so g is the float64 gradient and carries its own bound
    g_err (the gradient check's) into both outputs."""
    a1 = a + (g * g).sum(axis=1) / dim
    inv = lr[:, 0] / np.sqrt(a1)
    step = inv[:, None] * g
    tol_a = 16 * U * a1 + 2 * (np.abs(g) * g_err).sum(axis=1) / dim
    rel_inv = tol_a / (2 * a1) + 2 * U
    tol_w = U * (np.abs(w) + np.abs(step)) + np.abs(step) * (rel_inv[:, None] + U) + inv[:, None] * g_err
    return (w - step, a1), (2 * tol_w, 2 * tol_a)


def _check_table(run, before, after, ref_w, tol_w, touched):
    vals, bits = after
    if run.c.tdt == "bf16":
        tol_w = tol_w + UB * (np.abs(ref_w) + tol_w)
    _close("table", vals[touched], ref_w, tol_w)
    assert np.array_equal(bits[~touched], before[1][~touched]), "an untouched table row changed"


# ---- the tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_dense_and_compact_gradients_match_float64(name):
    run = _Run(name)
    h = run.h
    touched = h["touched"]
    got = run.dense()
    _check_grad(got[touched], h, np.nonzero(touched)[0])
    assert np.all(got[~touched] == 0), "dense form wrote an untouched row"
    rows, vals = run.fb.backward_sparse(run.ws, run.grad, run.c.batch, run.ids.numel(), **run.kw)
    rows, vals = rows.cpu().numpy(), vals.cpu().numpy()
    exp_rows = np.sort(np.nonzero(touched[h["flat_of_global"]])[0])   # touched GLOBAL rows, ascending
    assert np.array_equal(rows, exp_rows)
    _check_grad(vals, h, h["flat_of_global"][rows])


@pytest.mark.parametrize("name", list(CASES))
def test_fused_forms_sum_exactly_like_the_dense_form(name):
    """The update checks feed the kernel's dense gradient g into the float64 rules; that holds only if each fused form
    sums the segment exactly as the dense form does.  On a zero table: SGD with lr = 1 leaves -g; Adagrad from a zero
    accumulator leaves fl(g * g); Adam with beta_1 = 0 leaves m = g; FTRL with w = z = 0 leaves z = g."""
    g = _Run(name).dense()
    touched = _host(name)["touched"]
    g32 = g.astype(np.float32)
    for kind, hyper in [("sgd", None), ("adagrad", None), ("adam", (0.0, 0.99, 1e-3, 1.0)),
                        ("ftrl", (-0.5, 0.5, 0.01, 0.1))]:
        run = _Run(name, kind, table_fill=0.0, lrs=[1.0] * len(_host(name)["vocabs"]) if kind == "sgd" else None,
                   ftrl_init=0.1)
        if kind == "adagrad":
            run.slot.zero_()
        run.fused(kind, hyper)
        if kind == "sgd":
            vals = run.table()[0]
            exp = -g32 if run.c.tdt == "f32" else _bf16_round(-g32)
            assert np.array_equal(vals[touched], exp[touched].astype(np.float64)), kind
        elif kind == "adagrad":
            assert np.array_equal(run.planes()[0][touched], (g32 * g32)[touched]), kind
        else:
            plane = run.planes()[0 if kind == "adam" else 1]
            assert np.array_equal(plane[touched], g32[touched]), kind


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_fused_update_matches_the_float64_rule(name, mode):
    """One update (two for Adam and FTRL, the second from the device's state after the first) against the Keras rule in
    float64; untouched rows keep the bits of table and every slot plane."""
    h = _host(name)
    touched = h["touched"]
    ftrl_runs = FTRL if mode == "ftrl" else [(None, 0.1)]
    n_clipped = 0
    for hp, init in ftrl_runs:
        run = _Run(name, mode, ftrl_init=init)
        g = run.dense()[touched].astype(np.float64)
        lr = h["lr_row"][touched]
        for step in (1, 2) if mode in ("adam", "ftrl") else (1,):
            before = run.table()
            w = before[0][touched]
            pl = run.planes() if run.slot is not None else ()
            hyper = None
            if mode == "sgd":
                ref, tol = _sgd(w, g, lr)
            elif mode == "adagrad":
                ref, tol = _adagrad(w, pl[0][touched].astype(np.float64), g, lr)
            elif mode == "adagrad_rowwise":
                g_err = _gamma(h["n_row"][touched] + 3)[:, None] * h["M"][touched]
                ref, tol = _rowwise(w, pl[0][touched].astype(np.float64), h["dE"][touched], g_err, lr, run.c.dim)
            elif mode == "adam":
                hyper = ADAM + (float(math.sqrt(1 - ADAM[1] ** step) / (1 - ADAM[0] ** step)),)
                ref, tol = _adam(w, pl[0][touched].astype(np.float64), pl[1][touched].astype(np.float64), g, lr,
                                 ADAM, step)
            else:
                hyper = hp
                ref, tol, inside = _ftrl(w, pl[0][touched].astype(np.float64), pl[1][touched].astype(np.float64), g,
                                         lr, hp)
            run.fused(mode, hyper)
            after = run.table()
            _check_table(run, before, after, ref[0], tol[0], touched)
            new = run.planes() if run.slot is not None else ()
            for k, (a, b) in enumerate(zip(pl, new)):
                _close(f"slot plane {k}", b[touched].astype(np.float64), ref[1 + k], tol[1 + k])
                assert np.array_equal(a[~touched], b[~touched]), f"slot plane {k} of an untouched row changed"
            if mode == "ftrl":
                # |z| < l1 with room to spare: the weight is exactly zero
                assert np.all(after[0][touched][inside] == 0.0)
                n_clipped += int(inside.sum())
    if mode == "ftrl" and not name.startswith("hot_"):
        assert n_clipped > 0, "no weight was clipped to zero: l1 too small for this case"


def _routes(name, mode):
    """The apply kernels a case reaches in `mode`, restated from run_apply / launch_apply_lpr."""
    c, h = CASES[name], _host(name)
    fused = mode not in ("dense", "compact")
    gbytes = c.dim * (2 if c.gdt == "bf16" else 4)
    n_tables = 0 if mode == "compact" else len(c.vocabs)
    vec_pair = not (c.gdt == "f32" and c.tdt == "bf16" and fused)
    if gbytes % 16 or gbytes > 1024 or not vec_pair or len(c.tix) > 512 or n_tables > 512:
        return {("generic", 0)}
    pieces = gbytes // 16
    lpr = 8 if pieces <= 8 else 16 if pieces <= 16 else 32 if pieces <= 32 else 64
    out = {("fast", lpr)}
    if (h["n_row"] > 128).any():
        out.add(("long", lpr))
    if (h["n_row"] > 2048).any():
        out.add(("finish", lpr))
    return out


def test_the_cases_cover_the_apply_matrix():
    """Every mode meets every kernel, every fast LPR and every HAS_W x HAS_SCALE instance; every dtype pair meets every
    mode on each kernel it can reach (the dense / compact forms write fp32: only the gradient dtype names their pair);
    both row_base orders reach the fast and the generic kernel."""
    seen = set()
    for name, c in CASES.items():
        for mode in ["dense", "compact"] + MODES:
            pair = (c.tdt if mode not in ("dense", "compact") else "-", c.gdt)
            for kern, lpr in _routes(name, mode):
                seen.add((kern, mode, pair))
                seen.add((kern, mode, c.desc))
                if kern == "fast":
                    seen.add(("lpr", lpr, mode))
                    seen.add(("w_scale", c.use_w, c.use_scale, mode))
    for mode in ["dense", "compact"] + MODES:
        pairs = [("-", "f32"), ("-", "bf16")] if mode in ("dense", "compact") else \
            [("f32", "f32"), ("bf16", "bf16"), ("f32", "bf16")]
        for kern in ("fast", "long", "finish", "generic"):
            for pair in pairs + ([("bf16", "f32")] if kern == "generic" and mode not in ("dense", "compact") else []):
                assert (kern, mode, pair) in seen, (kern, mode, pair)
        for kern in ("fast", "generic"):
            assert (kern, mode, True) in seen and (kern, mode, False) in seen, (kern, mode)
        for lpr in (8, 16, 32, 64):
            assert ("lpr", lpr, mode) in seen, (lpr, mode)
        for ws in [(a, b) for a in (False, True) for b in (False, True)]:
            assert ("w_scale",) + ws + (mode,) in seen, (ws, mode)
