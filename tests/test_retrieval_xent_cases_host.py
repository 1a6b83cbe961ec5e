"""The K13 case table (tests/retrieval_xent_cases.py), checked without a GPU.  The slice planner's invariants are walked
by a stand-alone program built with the sanitizers (tests/host/xent_plan_check.cpp, which includes
keras_rs_amd/csrc/retrieval_xent_plan.h and nothing else of the project); the same program prints the plans of the
table's shapes, which must equal what the table claims; the table, with the shapes tests/test_retrieval_xent_gpu.py
already compares with float64, must reach every (DPAD, VEC) instantiation of xent_kernel on a sliced and on an unsliced
sweep of either owner; and the float64 reference of every case must be one its own bounds can tell from a wrong result:

    * the median over the non-zero elements of bound / |reference| is at most 0.05, for dq and for dc;
    * the reference dc with two adjacent rows swapped, and the reference dq with two columns swapped, lie outside the
      bounds (matrix cases).

tests/test_retrieval_xent_matrix_gpu.py runs the same inputs on the device."""

import os
import shutil
import subprocess

import pytest
import torch

from tests import retrieval_xent_cases as T
from tests import retrieval_xent_restatement as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEDIAN_CAP = 0.05        # of bound / |reference|, fixed before any kernel result was seen: a case that breaks it changes, not the cap


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """runs the plan program: planner(tuples of (owner, streamed, b, n)) -> [(oblocks, S, slice)]"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("xent_plan") / "xent_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "xent_plan_check.cpp"), "-o", exe],
                   check=True)

    def ask(tuples):
        args = [str(v) for t in tuples for v in t]
        run = subprocess.run([exe] + args, capture_output=True, text=True)
        assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
        lines = run.stdout.strip().splitlines()
        assert "0 failed checks" in lines[-1] and len(lines) == len(tuples) + 1
        return [tuple(int(v) for v in line.split()) for line in lines[:-1]]

    return ask


def _plans(planner, shapes):
    """{(b, n): ((fwd/dq oblocks, S, slice), (dc oblocks, S, slice))}"""
    shapes = sorted(set(shapes))
    got = planner([t for (b, n) in shapes for t in ((b, n, b, n), (n, b, b, n))])
    return {s: (got[2 * i], got[2 * i + 1]) for i, s in enumerate(shapes)}


def test_the_planner_keeps_its_invariants_over_the_grid_under_the_sanitizers(planner):
    assert planner([]) == []


def test_the_table_is_the_stated_matrix_and_is_well_formed():
    assert len({c.name for c in T.CASES}) == len(T.CASES) == len(T.WIDTHS) * len(T.PLANS)
    assert {(c.b, c.n, c.d) for c in T.CASES} == {(b, n, d) for d in (5, 31, 32, 33, 40, 64, 65, 72, 129, 136, 255)
                                                  for (b, n) in ((40, 161), (161, 40))}
    for c in T.CASES:
        assert c.d <= c.dpad and (c.dpad == 32 or c.d > c.dpad // 2) and c.vec == (c.d % 8 == 0), c.name
    # both sides of every DPAD step
    assert {(c.d, c.dpad) for c in T.CASES} >= {(32, 32), (33, 64), (64, 64), (65, 128), (129, 256)}
    assert {(b, n, d) for (b, n, d) in T.TESTED_BEFORE if d == 128}        # (128 itself stays with the older tests)


def test_the_claimed_slice_plans_are_the_planners(planner):
    plans = _plans(planner, [(c.b, c.n) for c in T.CASES])
    for c in T.CASES:
        fwd, dc = plans[(c.b, c.n)]
        assert fwd[:2] == c.fwd and dc[:2] == c.dc, c.name
        assert all(p[2] == T.SLICE_ROWS for p in (fwd, dc)), c.name
    # what the module's docstring says of the two shapes: a last slice of one full tile and a one-row tile; an owner
    # block of 33 rows; an unsliced dc sweep whose streamed side is a full tile and one of 8 rows
    assert 161 - 2 * T.SLICE_ROWS == 33 and 161 - 128 == 33 and 40 == 32 + 8
    # the structured orders stream n in slices, the last of them ending in a partial tile that holds row n - 1
    for (b, n, d), (fwd, _) in zip(T.ORDER_SHAPES, (_plans(planner, [(b, n)])[(b, n)] for (b, n, d) in T.ORDER_SHAPES)):
        assert fwd[1] > 1 and (n - (fwd[1] - 1) * fwd[2]) % 32 != 0, (b, n, d)


def test_every_instantiation_is_reached_sliced_and_unsliced_on_both_owners(planner):
    shapes = [(c.b, c.n, c.d) for c in T.CASES] + list(T.TESTED_BEFORE)
    plans = _plans(planner, [(b, n) for (b, n, _) in shapes])
    reached = set()                                           # (dpad, vec, sweep, sliced)
    for (b, n, d) in shapes:
        fwd, dc = plans[(b, n)]
        reached.add((T.dpad_of(d), d % 8 == 0, "fwd/dq", fwd[1] > 1))
        reached.add((T.dpad_of(d), d % 8 == 0, "dc", dc[1] > 1))
    missing = [(p, v, s, sl) for p in (32, 64, 128, 256) for v in (True, False) for s in ("fwd/dq", "dc")
               for sl in (True, False) if (p, v, s, sl) not in reached]
    assert missing == []
    # the table alone names every (DPAD, VEC) pair: none rests on the older shapes only
    table = {(c.dpad, c.vec) for c in T.CASES}
    assert table == {(p, v) for p in (32, 64, 128, 256) for v in (True, False)}
    # several queries share a positive, and a dc sweep is sliced while the dq sweep is not, where b > n
    big_b = [c for c in T.CASES if c.b > c.n]
    assert big_b and all(c.dc[1] > 1 and c.fwd[1] == 1 for c in big_b)
    assert all(len(set(T.matrix_inputs(c)[2].tolist())) < c.b for c in big_b)


# ---- the references are ones their bounds can tell from a wrong result -------------------------------------------------

def _reference(case, builder):
    q, c, pos, bias, w = builder(case)
    return X.reference(q, c, pos, bias, ls=T.LS, g=w)


def _median_ratio(ref, key):
    value, tol = ref[key], ref[key + "_tol"]
    live = value.abs() > 0
    assert bool(live.any())
    return float((tol[live] / value[live].abs()).median())


@pytest.mark.parametrize("case", T.CASES, ids=[c.name for c in T.CASES])
def test_the_bounds_of_a_matrix_case_would_not_hide_a_failure(case):
    ref = _reference(case, T.matrix_inputs)
    for key in ("dq", "dc"):
        ratio = _median_ratio(ref, key)
        print(f"{case.name} {key}: median bound / |reference| = {ratio:.4f}")
        assert ratio <= MEDIAN_CAP, (case.name, key, ratio)
    # two adjacent rows of dc exchanged (a kernel that stored a row at its neighbour's place), for every pair of rows;
    # two columns of dq exchanged, for every adjacent pair: each such result leaves the bounds
    dc, dq = ref["dc"], ref["dq"]
    for r in range(case.n - 1):
        assert bool(((dc[r] - dc[r + 1]).abs() > torch.minimum(ref["dc_tol"][r], ref["dc_tol"][r + 1])).any()), (case.name, r)
    for k in range(case.d - 1):
        assert bool(((dq[:, k] - dq[:, k + 1]).abs() > torch.minimum(ref["dq_tol"][:, k], ref["dq_tol"][:, k + 1])).any()), \
            (case.name, k)


@pytest.mark.parametrize("case", T.ORDERS, ids=[c.name for c in T.ORDERS])
def test_the_bounds_of_a_structured_order_would_not_hide_a_failure(case):
    assert case.n >= 2
    ref = _reference(case, T.order_inputs)
    for key in ("dq", "dc"):
        ratio = _median_ratio(ref, key)
        print(f"{case.name} {key}: median bound / |reference| = {ratio:.4f}")
        assert ratio <= MEDIAN_CAP, (case.name, key, ratio)
    # the order is what its name says: every query's float64 scores without the bias rise, fall, or peak at the end
    q, c, pos, bias, w = T.order_inputs(case)
    s = q.double() @ c.double().T
    tiles = s.unfold(1, 32, 32).amax(-1)                    # the maximum of each whole tile of 32 streamed rows
    if case.order == "ascending":
        assert bool((tiles[:, 1:] > tiles[:, :-1]).all())
    elif case.order == "descending":
        assert bool((tiles[:, 1:] < tiles[:, :-1]).all())
    else:
        assert bool((s.argmax(-1) == case.n - 1).all()) and bool((s[:, -1] - s[:, :-1].amax(-1) > 50).all())
    if case.extreme_bias:
        assert sorted(set(round(float(v), 1) for v in bias)) == [0.0, 13.8]
