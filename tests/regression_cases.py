"""The case table of K24 (krs_regression_fwd_bwd), shared by tests/test_regression_host.py (no GPU) and
tests/test_regression_gpu.py.

A case names a call; `tensors(case)` makes its inputs, already rounded to the case's dtype, from the case's name alone.
The table reaches every kind x reduction x {weights, none} x {fp32, bf16} x {vector route, element route} at small
shapes (GRID), and the edges at which this kernel can go wrong (EDGES):
  * b in {0, 1, 63, 64, 65} on both routes;
  * one workgroup filled exactly and one item more: 1024 / 1025 rows on the element route, 4096 / 4097 (fp32) and
    8192 / 8193 (bf16) rows on the vector route;
  * every partial of the two-stage sum with a ragged last stride: 256 * 1024 + 1 items, i.e. 262145 rows on the element
    route and 4 * 262145 + 3 fp32 rows on the vector route (with a tail), once with weights under
    mean_with_sample_weight (the W pass at full width);
  * c in {1, 3, 5, 300} (5 is the listwise example's list; the element build has no per-row limit, 300 stands for "long");
  * ld > c for pred and target (`pad`), a pred base off 16 bytes (`offset` elements);
  * in EVERY case with at least 6 elements: e = +delta, e = -delta, e = 0, e just above delta, e just below delta, and
    under weights a zero and a negative weight;
  * all-zero weights under mean_with_sample_weight; one NaN and one inf prediction.

Bounds (tests/regression_restatement.py, `bounds`): dpred has none, it is bit for bit.  The loss and the batch sums:
depth of the summation x fp32 unit round-off x sum |terms|, from the order include/krs.h states; nothing in it comes
from what the kernel returns.
"""

import zlib
from typing import NamedTuple

import numpy as np

from tests import regression_restatement as R

VEC, ELEM = 1, 2
DELTA = 0.5           # a bf16 value, so |e| == delta is reachable exactly in both dtypes


class Case(NamedTuple):
    name: str
    kind: str           # "mse" | "mae" | "huber"
    reduction: str      # one of R.REDUCTIONS
    weights: str        # "" | "mixed" (a zero and a negative weight among positive ones) | "zero" (all zero)
    dtype: str          # "fp32" | "bf16"
    b: int
    c: int
    pad: int = 0        # ld = c + pad for pred and target
    offset: int = 0     # elements between a 16-byte boundary and pred's base
    special: str = ""   # "" | "nan" | "inf"

    @property
    def route(self):    # claimed; the planner is asked in the host test and the kernel in the GPU test
        if self.b == 0:
            return 0
        return VEC if self.c == 1 and self.pad == 0 and self.offset == 0 else ELEM


def _grid():
    out = []
    for kind in R.KINDS:
        for reduction in R.REDUCTIONS:
            for weights in ("", "mixed"):
                for dtype in ("fp32", "bf16"):
                    tag = f"{kind}-{reduction}-{weights or 'now'}-{dtype}"
                    out.append(Case(f"grid-vec-{tag}", kind, reduction, weights, dtype, 67, 1))
                    out.append(Case(f"grid-elem-{tag}", kind, reduction, weights, dtype, 13, 3, pad=2))
    return out


GRID = _grid()
S, M = "sum_over_batch_size", "mean_with_sample_weight"
EDGES = (
    [Case(f"b{b}-vec", "mse", S, "mixed", "fp32", b, 1) for b in (0, 1, 63, 64, 65)]
    + [Case(f"b{b}-elem", "huber", M, "mixed", "bf16", b, 1, offset=1) for b in (0, 1, 63, 64, 65)]
    + [Case(f"fill-elem-{b}", "mae", S, "", "fp32", b, 1, pad=1) for b in (1024, 1025)]
    + [Case(f"fill-vec-fp32-{b}", "mse", "sum", "", "fp32", b, 1) for b in (4096, 4097)]
    + [Case(f"fill-vec-bf16-{b}", "huber", "none", "mixed", "bf16", b, 1) for b in (8192, 8193)]
    + [Case("two-stage-elem", "mse", S, "", "fp32", 256 * 1024 + 1, 1, offset=1),
       Case("two-stage-vec", "huber", S, "", "fp32", 4 * (256 * 1024 + 1) + 3, 1),
       Case("two-stage-elem-weighted", "mse", M, "mixed", "bf16", 256 * 1024 + 1, 1, offset=3),
       Case("c5", "mse", S, "mixed", "fp32", 129, 5),
       Case("c5-bf16-none", "mae", "none", "mixed", "bf16", 129, 5, pad=3),
       Case("c300", "huber", "sum", "", "bf16", 7, 300, offset=1),
       Case("c1-ld2", "mse", M, "mixed", "fp32", 100, 1, pad=1),
       Case("zero-weights", "mse", M, "zero", "fp32", 70, 1),
       Case("zero-weights-elem", "huber", M, "zero", "bf16", 70, 3)]
    + [Case(f"{special}-{kind}-{route}", kind, S, "", "fp32", 70, c, special=special)
       for special in ("nan", "inf") for kind in R.KINDS for route, c in (("vec", 1), ("elem", 3))]
)
CASES = GRID + list(EDGES)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def tensors(case: Case):
    """{"pred" [b, c] fp32 values of the case's dtype, "target" [b, c] fp32, "weight" [b] fp32 or None, "g" [b] fp32}"""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    b, c = case.b, case.c
    target = (rng.integers(-4, 5, size=(b, c)) * 0.5).astype(np.float32)
    pred = (target + rng.uniform(-1.5, 1.5, size=(b, c))).astype(np.float32)
    if case.dtype == "bf16":
        pred = R.round_bf16(pred)
    flat_p, flat_y = pred.reshape(-1), target.reshape(-1)      # (views)
    if b * c >= 6:      # e = +delta, -delta, 0, just above and just below delta (bf16 values all)
        flat_y[:5] = 0.0
        flat_p[:5] = [DELTA, -DELTA, 0.0, DELTA * (1 + 2.0 ** -7), -DELTA * (1 - 2.0 ** -8)]
        if case.special:
            flat_p[5] = np.nan if case.special == "nan" else np.inf
    weight = None
    if case.weights == "mixed":
        weight = rng.uniform(0.25, 2.0, size=b).astype(np.float32)
        if b >= 3:
            weight[b // 2] = 0.0
            weight[b - 1] = -0.75
    elif case.weights == "zero":
        weight = np.zeros(b, dtype=np.float32)
    g = rng.uniform(-2.0, 2.0, size=b).astype(np.float32)
    return {"pred": pred, "target": target, "weight": weight, "g": g}
