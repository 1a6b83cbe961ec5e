"""The case table of the dense elementwise walks (krs_cross_epilogue_fwd / _bwd, krs_dense_act_bwd, krs_colsum,
krs_bce_fwd_bwd): one case per row, with the route it claims, its float64 inputs (already rounded to the case's dtype,
so the restatement sees what the kernel sees), the restatement's outputs and the bound of every output.  Needs no GPU:
tests/test_dense_walk_host.py checks the table and the bounds, tests/test_dense_walk_matrix_gpu.py runs it.

The claimed geometry is restated here (`claim`), not asked of the planner: strips of 64 threads over n / v columns, at
most ceil(4096 / strips) row chunks, one chunk per wave and four waves per workgroup on the vector kernels.

Bounds, with u = 2^-24 and M the restatement's magnitude (tests/dense_walk_restatement.py).  An elementwise output is
within C * u * M, C = the roundings on the output's longest path, counted without fused multiply-adds (the compiler may
contract, which only removes roundings), plus one:
    y    diag*x (1), u + . (2), x0 * . (3), . + x (4)                                            C = 5
    dz   cross: g*x0 (1) beside act' = 1 - u (1), u * . (2) [sigmoid] or u*u (1), 1 - . (2) [tanh]; their product (3)
         Dense: act' (2), g * . (3)                                                              C = 4
    dxd  g*x0 (1), diag * . (2), g + . (3)                                                       C = 4
    dx0  scalar kernel: diag*x (1), u + . (2), g * . (3), init + . (4), + direct term [3 roundings of its own] (5)
         (the vector kernel's two fused multiply-adds make it 4)                                 C = 6
A bf16 output adds its own rounding, 2^-8 |ref| (the project's convention for one bf16 rounding).  Column sums
(dbias, colsum; fp32) are within (depth + 4) * u * M, depth the longest chain of additions of the route: two-stage
rows_per_block + 2 + ceil(grid_y / 32) + 32 (the chunk's rows, the four waves, a slice's run of groups, the 32 slices),
atomics rows_per_block + chunks.  The BCE loss is within (chain + 9) * u * M with chain = ceil(n / (blocks * 1024)) +
10 + blocks (a thread's stride, the LDS tree, the workgroups in order) and 9 = logf at 2 ulp (4 u) + the product with
the label (1) + the sum of the two terms (1) + 1 / n and the product with it (2) + one; dpred is within 5 * u * M:
1 - p (1), the quotient (2), the difference (3), times scale / n (4), plus one."""

import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests import dense_walk_restatement as R

U = 2.0 ** -24
C = {"y": 5, "dz": 4, "dxd": 4, "dx0": 6, "dpred": 5}
C_SUM, C_BCE = 4, 9
NONE, VEC, SCALAR = 0, 1, 2
ENTRIES = ("cross_fwd", "cross_bwd", "dense_act_bwd", "colsum", "bce")
TINY = ((1, 8), (5, 3), (37, 24), (33, 1))
BCE_N = (1, 1023, 1024, 1025, 65536, 65537, 200000)
BCE_MAX_BLOCKS, BCE_THREADS = 64, 1024


@dataclass(frozen=True)
class Case:
    name: str
    entry: str
    dtype: str                      # "fp32" | "bf16"
    m: int
    n: int
    ld: tuple = ()                  # one leading dimension; krs_dense_act_bwd: (g, y, dz).  () = n
    off: int = 0                    # elements the base of every operand is off its 16-byte-aligned allocation
    act: int = R.NONE
    diag: float = 0.0
    acc: bool = False               # dx0 arrives holding the terms of the layers above (dx0_accumulate)
    fold: bool = False              # dxd == dx0
    outs: tuple = ()
    u_null: bool = False
    ws: str = ""                    # "two_stage" | "atomics" | "" (no column sums)
    form: str = ""                  # the entry of tests/test_autograd_handoffs_host.py's table this case restates

    @property
    def lds(self):
        return self.ld or (self.n,) * (3 if self.entry == "dense_act_bwd" else 1)

    @property
    def live_lds(self):
        """The leading dimensions of the call's non-null matrices (the ones the vector test reads)."""
        if self.entry != "dense_act_bwd":
            return () if self.entry == "colsum" else self.lds
        ldg, ldy, ldz = self.lds
        return (ldg,) + ((ldy,) if self.act != R.NONE else ()) + ((ldz,) if "dz" in self.outs else ())

    @property
    def v(self):
        return 8 if self.dtype == "bf16" else 4


def claim(case):
    """(kernel, v, acc, two_stage, rows_per_block, strips, chunks, grid_y) the case says it runs on."""
    if case.entry == "bce" or case.m == 0 or case.n == 0:
        return (NONE, 0, 0, 0, 0, 0, 0, 0)
    v = case.v
    vec = case.entry != "colsum" and case.n % v == 0 and case.off == 0 and all(l % v == 0 for l in case.live_lds)
    if case.entry == "cross_fwd":
        return (VEC if vec else SCALAR, v if vec else 1, 0, 0, 0, 0, 0, 0)
    w = v if vec else 1
    strips = math.ceil(case.n // w / 64)
    rows = math.ceil(case.m / min(math.ceil(4096 / strips), case.m))
    chunks = math.ceil(case.m / rows)
    return (VEC if vec else SCALAR, w, int(vec and case.acc and "dx0" in case.outs), int(case.ws == "two_stage"), rows, strips,
            chunks, math.ceil(chunks / 4) if vec else chunks)


# ---- the table ------------------------------------------------------------------------------------------------------
# the forms of _cross_elementwise (entries "b" to "l" of tests/test_autograd_handoffs_host.py's table)
FORMS = {
    "b": dict(act=R.TANH, acc=True, fold=True, outs=("dz", "dx0", "dbias")),
    "c": dict(act=R.TANH, acc=True, outs=("dz", "dx0", "dxd", "dbias")),
    "d": dict(act=R.TANH, outs=("dz", "dx0", "dxd", "dbias")),
    "e": dict(acc=True, fold=True, outs=("dx0",)),
    "f": dict(acc=True, fold=True, outs=("dz", "dx0", "dbias")),
    "g": dict(acc=True, outs=("dz", "dx0", "dbias")),
    "h": dict(acc=True, outs=("dx0",)),
    "i": dict(fold=True, outs=("dz", "dx0", "dbias")),
    "j": dict(outs=("dz", "dx0", "dbias")),
    "k": dict(outs=("dz", "dbias")),
    "l": dict(u_null=True, outs=("dz", "dbias")),
}
ALL = ("dz", "dx0", "dxd", "dbias")
# (m, n) of the forms: vector with a partial last strip, scalar with several strips -- three rows a chunk on all four
FORM_SHAPES = {("fp32", VEC): (2750, 516), ("fp32", SCALAR): (2100, 250), ("bf16", VEC): (4100, 776), ("bf16", SCALAR): (2750, 130)}


def _table():
    t = []

    def add(entry, dtype, m, n, tag="", **kw):
        if entry in ("cross_bwd", "dense_act_bwd") and "outs" not in kw:
            kw["outs"] = ALL if entry == "cross_bwd" else ("dz", "dbias")
        if entry == "colsum":
            kw.setdefault("outs", ("colsum",))
        if entry == "cross_fwd":
            kw["outs"] = ("y",)
        if ("dbias" in kw.get("outs", ()) or entry == "colsum") and "ws" not in kw:
            kw["ws"] = "two_stage"
        t.append(Case(f"{entry}-{dtype}-{m}x{n}{'-' + tag if tag else ''}", entry, dtype, m, n, **kw))

    for dtype in ("fp32", "bf16"):
        v = 8 if dtype == "bf16" else 4
        # every form of the cross backward on the vector and on the scalar route
        for route in (VEC, SCALAR):
            m, n = FORM_SHAPES[dtype, route]
            for k, (letter, form) in enumerate(FORMS.items()):
                kw = dict(form)
                kw["diag"] = 0.5 if (k + route) % 2 else 0.0
                if "dbias" in kw["outs"]:
                    kw["ws"] = "atomics" if k % 3 == 1 else "two_stage"
                add("cross_bwd", dtype, m, n, "form_" + letter, form=letter, **kw)
        # vector walk: three rows a chunk, several strips, a short last chunk, idle waves in the last group
        big = ((700, 4096), (1100, 2048)) if dtype == "fp32" else ((1300, 4096), (700, 8192))
        add("cross_bwd", dtype, *big[0], act=R.SIGMOID, diag=0.25, acc=True)
        add("cross_bwd", dtype, *big[1], act=R.RELU, outs=("dz", "dx0", "dbias"), ws="atomics")
        add("dense_act_bwd", dtype, *big[1], act=R.RELU)
        # ... one strip, deep chunks (2734 of them, the last of one row)
        deep = (8200, 256) if dtype == "fp32" else (8200, 512)
        add("cross_bwd", dtype, *deep, act=R.RELU, diag=-0.5, fold=True, outs=("dz", "dx0", "dbias"))
        add("dense_act_bwd", dtype, *deep, act=R.SIGMOID)
        # ... a partial last strip (idle lanes)
        part = FORM_SHAPES[dtype, VEC]
        add("dense_act_bwd", dtype, *part, act=R.TANH, ws="atomics")
        add("dense_act_bwd", dtype, *part, "dz_only", act=R.RELU, outs=("dz",))
        # scalar walk, several rows and strips
        for m, n in ((2100, 250), (2750, 130)):
            add("dense_act_bwd", dtype, m, n, act=R.SIGMOID if n == 250 else R.RELU, ws="two_stage" if n == 250 else "atomics")
            add("colsum", dtype, m, n, ld=(n + 6,), ws="two_stage" if n == 130 else "atomics")
        add("cross_bwd", dtype, *((2750, 130) if dtype == "fp32" else (2100, 250)), "sigmoid", act=R.SIGMOID, diag=0.5)
        # a vector-eligible shape pushed to the scalar kernel: ld = n + 1, a base one element off, (bf16) n % 8 == 4
        m, n = part
        add("cross_bwd", dtype, m, n, "ld_n+1", ld=(n + 1,), act=R.RELU, diag=0.5, acc=True)
        add("cross_bwd", dtype, m, n, "base_off", off=1, act=R.TANH, ws="atomics")
        add("dense_act_bwd", dtype, m, n, "base_off", off=1, act=R.RELU)
        add("dense_act_bwd", dtype, m, n, "ld_n+1", ld=(n + 1,) * 3, act=R.NONE)
        if dtype == "bf16":
            add("cross_bwd", dtype, 2750, 516, "n%8==4", act=R.RELU, diag=0.5)
            add("dense_act_bwd", dtype, 2750, 516, "n%8==4", act=R.SIGMOID)
        # leading dimensions: n + v stays on the vector route, n + 3 leaves it; three different ones for the Dense backward
        add("cross_bwd", dtype, m, n, "ld_n+v", ld=(n + v,), act=R.SIGMOID, diag=0.5, fold=True, outs=("dz", "dx0", "dbias"))
        add("cross_bwd", dtype, m, n, "ld_n+3", ld=(n + 3,), act=R.SIGMOID, outs=("dz", "dx0", "dxd"))
        add("dense_act_bwd", dtype, m, n, "three_lds", ld=(n + v, n + 3 * v, n + 2 * v), act=R.SIGMOID)
        add("dense_act_bwd", dtype, m, n, "three_lds_scalar", ld=(n + 3, n, n + v), act=R.RELU, outs=("dz",))
        add("cross_fwd", dtype, m, n, "ld_n+v", ld=(n + v,), diag=0.5)
        add("cross_fwd", dtype, m, n, "ld_n+3", ld=(n + 3,), diag=0.5)
        add("cross_fwd", dtype, m, n, "base_off", off=1)
        add("cross_fwd", dtype, 300, 4096, diag=-0.25)
        # colsum_finish_kernel: >= 128 groups with an unrolled run and a tail (fp32: 263 groups on the vector kernel,
        # bf16: 420 chunks on the scalar one); 32 .. 127 groups are the `big` shapes, < 32 the tiny ones
        add("cross_bwd", dtype, 2100, 532, act=R.NONE, outs=("dz", "dbias"), u_null=True)
        add("dense_act_bwd", dtype, 2100, 532, act=R.NONE, outs=("dbias",))
        # the shapes of the tests before these
        for k, (m, n) in enumerate(TINY):
            act = (R.NONE, R.RELU, R.SIGMOID, R.TANH)[k]
            add("cross_fwd", dtype, m, n, diag=0.5 if k % 2 else 0.0)
            add("cross_bwd", dtype, m, n, act=act, diag=0.0 if k % 2 else 0.5, acc=k >= 2)
            add("colsum" if k % 2 else "dense_act_bwd", dtype, m, n, **({} if k % 2 else {"act": act}))
            add("dense_act_bwd" if k % 2 else "colsum", dtype, m, n, "atomics", ws="atomics", **({"act": act} if k % 2 else {}))
        for n in BCE_N:
            t.append(Case(f"bce-{dtype}-{n}", "bce", dtype, 1, n, outs=("loss", "dpred")))
    return tuple(t)


CASES = _table()


# ---- inputs, reference, bounds --------------------------------------------------------------------------------------
def round_to(x, dtype):
    """float64 -> the dtype's nearest value (ties to even) -> float64."""
    f = np.asarray(x, dtype=np.float64).astype(np.float32)
    if dtype == "fp32":
        return f.astype(np.float64)
    bits = f.view(np.uint32).astype(np.uint64)
    bits = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16
    return bits.astype(np.uint32).view(np.float32).astype(np.float64).reshape(f.shape)


def inputs_of(index):
    """The float64 operands of a case, exactly representable in its dtype.  Uniform in (-1, 1) (u / y in (0, 1) under a
    sigmoid), with exact special points: u = +0, -0 and 1, g = 0."""
    case = CASES[index]
    rng = np.random.default_rng(1000 + index)
    if case.entry == "bce":
        n = case.n
        pred = rng.uniform(0.01, 0.99, n)
        lo, hi = R.bce_bounds(1e-7)
        for k, value in enumerate((0.0, 1.0, 5e-8, hi, lo)):
            pred[(k * 7919) % n if n > 8 else k % n] = value
        labels = (rng.uniform(0, 1, n) < 0.4).astype(np.float64)
        if n > 8:
            labels[3::11] = rng.uniform(0, 1, labels[3::11].shape)       # a few soft labels
        return {"pred": round_to(pred, case.dtype), "labels": round_to(labels, "fp32")}
    shape = (case.m, case.n)
    draw = lambda lo=-1.0: round_to(rng.uniform(lo, 1.0, shape), case.dtype)
    t = {"g": draw()}
    size = case.m * case.n
    spots = rng.choice(size, size=min(size, max(4, size // 50)), replace=False)
    if case.entry == "colsum":
        return {"a": t["g"]}
    sig = case.act == R.SIGMOID
    if case.entry == "dense_act_bwd":
        t["y"] = draw(0.0 if sig else -1.0)
        special = t["y"]
    else:
        t["u"], t["x0"], t["x"] = draw(0.0 if sig else -1.0), draw(), draw()
        special = t["u"]
        if case.acc:
            t["init"] = draw()
    for k, value in enumerate((0.0, -0.0, 1.0)):
        special.flat[spots[k::4]] = value
    if case.entry != "cross_fwd":
        t["g"].flat[spots[3::4]] = 0.0
    if case.entry == "cross_fwd":
        del t["g"]
    return t


def run(case, t):
    """The restatement on a case's inputs -> (outputs, magnitudes)."""
    if case.entry == "cross_fwd":
        return R.cross_fwd(t["u"], t["x0"], t["x"], case.diag)
    if case.entry == "cross_bwd":
        return R.cross_bwd(t["g"], None if case.u_null else t["u"], t["x0"], t["x"], case.diag, case.act, t.get("init"),
                           case.fold, case.outs)
    if case.entry == "dense_act_bwd":
        return R.dense_act_bwd(t["g"], t["y"], case.act, case.outs)
    if case.entry == "colsum":
        return R.colsum(t["a"])
    return R.bce(t["pred"], t["labels"], BCE_EPS, BCE_SCALE)


BCE_EPS, BCE_SCALE = 1e-7, 0.5


def bce_blocks(n, partials=True):
    return min(BCE_MAX_BLOCKS, math.ceil(n / BCE_THREADS)) if partials else 1


def sum_depth(route, ws):
    _, _, _, _, rows, _, chunks, grid_y = route
    return rows + 2 + math.ceil(grid_y / 32) + 32 if ws == "two_stage" else rows + chunks


def bounds(case, ref, mag, route=None, partials=True):
    """name -> the bound of |kernel - ref| (an array of the output's shape)."""
    route = claim(case) if route is None else route
    b = {}
    for name, m in mag.items():
        if name in ("dbias", "colsum"):
            b[name] = (sum_depth(route, case.ws) + C_SUM) * U * m
        elif name == "loss":
            blocks = bce_blocks(case.n, partials)
            b[name] = (math.ceil(case.n / (blocks * BCE_THREADS)) + 10 + blocks + C_BCE) * U * m
        else:
            b[name] = C[name] * U * m + (2.0 ** -8 * np.abs(ref[name]) if case.dtype == "bf16" else 0.0)
    return b


@lru_cache(maxsize=2)
def reference_of(index):
    """(inputs, outputs, magnitudes, bounds) of a case; the arrays are shared: do not write to them."""
    case = CASES[index]
    t = inputs_of(index)
    ref, mag = run(case, t)
    return t, ref, mag, bounds(case, ref, mag)


def worst_ratio(got, ref, bound):
    """max over the outputs of |got - ref| / bound (inf where an error meets a zero bound or is not a number)."""
    worst, where = 0.0, ""
    for name in ref:
        err = np.abs(np.asarray(got[name], dtype=np.float64) - ref[name])
        bad = ~(err <= bound[name])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound[name])
        ratio = np.where(bad & ~(ratio > 1.0), np.inf, ratio)
        r = float(np.max(ratio)) if np.size(ratio) else 0.0
        if r > worst:
            worst, where = r, f"{name}{np.unravel_index(int(np.argmax(ratio)), np.shape(ratio)) if np.ndim(ratio) else ''}"
    return worst, where
