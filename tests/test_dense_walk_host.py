"""The dense elementwise walks without a GPU: the restatement against hand-computed rows and float64 torch autograd; the
case table's coverage; the host planner under the sanitizers and the routes the table claims; the ABI rows and every
refusal of the five entries (they come before the first launch, so made-up pointers do); and the bounds' teeth: eight
mistakes a kernel could make, applied to the restatement, leave the bound of every case they can be expressed on."""

import ctypes as C
import dataclasses
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from tests import dense_walk_cases as T
from tests import dense_walk_restatement as R
from tests.test_capi_symbols import _header, header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"cross_fwd": L.WALK_CROSS_FWD, "cross_bwd": L.WALK_CROSS_BWD, "dense_act_bwd": L.WALK_DENSE_ACT_BWD,
         "colsum": L.WALK_COLSUM}
FIELDS = ("kernel", "v", "acc", "two_stage", "rows_per_block", "strips", "chunks", "grid_y")
INVALID, UNSUPPORTED = -1, -2


def route_tuple(rt):
    assert rt.reserved == 0
    return tuple(int(getattr(rt, f)) for f in FIELDS)


def last_route():
    rt = L.DenseWalkRoute()
    assert L.lib().krs_dense_walk_last_route(C.byref(rt)) == rt.kernel
    return route_tuple(rt)


def planned(case):
    """krs_dense_walk_plan_route for a case's call: one operand address stands for all (they share their alignment)."""
    item = 2 if case.dtype == "bf16" else 4
    lds = (C.c_int64 * max(1, len(case.live_lds)))(*case.live_lds)
    ptrs = (C.c_void_p * 2)(4096 + case.off * item, None)
    rt = L.DenseWalkRoute()
    rc = L.lib().krs_dense_walk_plan_route(ENTRY[case.entry], case.m, case.n, L.BF16 if case.dtype == "bf16" else L.F32, lds,
                                           len(case.live_lds), ptrs, 2, int("dbias" in case.outs), int(case.ws == "two_stage"),
                                           int(case.acc and "dx0" in case.outs), C.byref(rt))
    assert rc == 0, case.name
    return route_tuple(rt)


# ---- (a) the restatement --------------------------------------------------------------------------------------------
def test_restatement_on_two_hand_computed_rows():
    # g = (2, -1), u = (.5, 0), x0 = (3, 4), x = (1, 2), diag = .5, tanh: act' = (.75, 1)
    g, u, x0, x = (np.array([v]) for v in ([2.0, -1.0], [0.5, 0.0], [3.0, 4.0], [1.0, 2.0]))
    y, my = R.cross_fwd(u, x0, x, 0.5)
    assert np.array_equal(y["y"], [[4.0, 6.0]]) and np.array_equal(my["y"], [[4.0, 6.0]])       # 3 (.5 + .5) + 1, 4 (0 + 1) + 2
    out, mag = R.cross_bwd(g, u, x0, x, 0.5, R.TANH, init=np.array([[10.0, 20.0]]))
    assert np.array_equal(out["dz"], [[4.5, -4.0]]) and np.array_equal(out["dbias"], [4.5, -4.0])    # 6 * .75, -4 * 1
    assert np.array_equal(out["dx0"], [[12.0, 19.0]])                                              # 10 + 2 (1), 20 - 1 (1)
    assert np.array_equal(out["dxd"], [[5.0, -3.0]])                                               # 2 + .5 * 6, -1 + .5 * -4
    assert np.array_equal(mag["dz"], [[6 * 1.25, 4.0]]) and np.array_equal(mag["dx0"], [[12.0, 21.0]])
    assert np.array_equal(mag["dxd"], [[5.0, 3.0]])
    fold, mfold = R.cross_bwd(g, u, x0, x, 0.5, R.TANH, init=np.array([[10.0, 20.0]]), fold=True)
    assert "dxd" not in fold and np.array_equal(fold["dx0"], [[17.0, 16.0]]) and np.array_equal(mfold["dx0"], [[17.0, 24.0]])
    # second row: a Dense epilogue under a sigmoid and a relu, the column sum, and BCE at p = .5 / outside the clip
    g2, y2 = np.array([[2.0, -1.0], [4.0, 8.0]]), np.array([[0.5, 0.25], [0.0, 1.0]])
    d, md = R.dense_act_bwd(g2, y2, R.SIGMOID)
    assert np.array_equal(d["dz"], [[0.5, -0.1875], [0.0, 0.0]]) and np.array_equal(d["dbias"], [0.5, -0.1875])
    assert np.array_equal(md["dz"], [[1.5, 0.3125], [0.0, 16.0]])
    assert np.array_equal(R.dense_act_bwd(g2, y2 - 0.25, R.RELU)[0]["dz"], [[2.0, 0.0], [0.0, 8.0]])     # relu'(0) = 0
    assert np.array_equal(R.colsum(g2)[0]["colsum"], [6.0, 7.0]) and np.array_equal(R.colsum(g2)[1]["colsum"], [6.0, 9.0])
    b, _ = R.bce(np.array([0.5, 0.5, 0.0, 1.0]), np.array([1.0, 0.0, 0.0, 1.0]), 1e-7, 2.0)
    lo, hi = R.bce_bounds(1e-7)
    assert lo == float(np.float32(1e-7)) and hi == 1.0 - 2.0 ** -23
    assert abs(b["loss"] - (2 * math.log(2) - math.log1p(-lo) - math.log(hi)) / 4) < 1e-15
    assert np.array_equal(b["dpred"], [-1.0, 1.0, 0.0, 0.0])                                       # 2 / 4 * (-1 / .5), ...


SMALL = [i for i, c in enumerate(T.CASES) if c.m * c.n <= 1000 and c.entry in ("cross_bwd", "dense_act_bwd")]


@pytest.mark.parametrize("index", SMALL, ids=[T.CASES[i].name for i in SMALL])
def test_restatement_agrees_with_float64_autograd(index):
    case = T.CASES[index]
    t, ref, _, _ = T.reference_of(index)
    act = {R.NONE: lambda z: z, R.RELU: torch.relu, R.SIGMOID: torch.sigmoid, R.TANH: torch.tanh}[case.act]
    inv = {R.NONE: lambda u: u, R.RELU: lambda u: u, R.SIGMOID: torch.logit, R.TANH: torch.atanh}[case.act]
    tt = {k: torch.from_numpy(v.copy()) for k, v in t.items()}
    close = lambda a, b: np.abs(a.numpy() - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
    if case.entry == "dense_act_bwd":
        # interior points only: at y = 0 / 1 the pre-activation is at infinity (sigmoid) or on the kink (relu)
        y = tt["y"].clamp(0.01, 0.99) if case.act in (R.SIGMOID, R.TANH) else tt["y"]
        y = torch.where(y == 0, torch.full_like(y, 0.5), y) if case.act == R.RELU else y
        z = inv(y).clone().requires_grad_(True)
        y = torch.relu(y) if case.act == R.RELU else y          # (a relu's saved output: the draw is its pre-activation)
        bias = torch.zeros(case.n, dtype=torch.float64, requires_grad=True)
        dz, db = torch.autograd.grad(act(z + bias), [z, bias], tt["g"])
        want, _ = R.dense_act_bwd(t["g"], y.numpy(), case.act)
        assert close(dz, want["dz"]) and close(db, want["dbias"])
        return
    u = tt["u"].clamp(0.01, 0.99) if case.act in (R.SIGMOID, R.TANH) else tt["u"]
    u = torch.where(u == 0, torch.full_like(u, 0.5), u) if case.act == R.RELU else u
    z = inv(u).clone().requires_grad_(True)
    u = torch.relu(u) if case.act == R.RELU else u              # (a relu's saved output: the draw is its pre-activation)
    x0, x = tt["x0"].clone().requires_grad_(True), tt["x"].clone().requires_grad_(True)
    y = x0 * (act(z) + case.diag * x) + x
    fwd, _ = R.cross_fwd(u.numpy(), t["x0"], t["x"], case.diag)
    assert close(y.detach(), fwd["y"])
    dz, dx0, dx = torch.autograd.grad(y, [z, x0, x], tt["g"])
    want, _ = R.cross_bwd(t["g"], u.numpy(), t["x0"], t["x"], case.diag, case.act, t.get("init"))
    assert close(dz, want["dz"]) and close(dz.sum(0), want["dbias"]) and close(dx, want["dxd"])
    assert close(dx0 + (tt["init"] if case.acc else 0.0), want["dx0"])
    folded, _ = R.cross_bwd(t["g"], u.numpy(), t["x0"], t["x"], case.diag, case.act, t.get("init"), fold=True)
    assert close(dx0 + dx + (tt["init"] if case.acc else 0.0), folded["dx0"])       # x is x0: both gradients land in one


def test_restatement_agrees_with_torch_binary_cross_entropy():
    for index, case in enumerate(T.CASES):
        if case.entry != "bce" or case.n > 1025:
            continue
        t, ref, _, _ = T.reference_of(index)
        lo, hi = R.bce_bounds(T.BCE_EPS)
        pred = torch.from_numpy(t["pred"].copy()).requires_grad_(True)
        loss = torch.nn.functional.binary_cross_entropy(pred.clamp(lo, hi), torch.from_numpy(t["labels"]))
        (grad,) = torch.autograd.grad(loss * T.BCE_SCALE, pred)
        assert abs(loss.item() - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
        assert np.abs(grad.numpy() - ref["dpred"]).max() <= 1e-9 * np.abs(ref["dpred"]).max()
        assert (ref["dpred"][(t["pred"] < lo) | (t["pred"] > hi)] == 0).all()


# ---- (b) the table --------------------------------------------------------------------------------------------------
def test_the_table_is_the_stated_matrix():
    names = [c.name for c in T.CASES]
    assert len(set(names)) == len(names) <= 150
    item = {"fp32": 4, "bf16": 2}
    assert all(c.m * max(c.lds) * item[c.dtype] <= 32 * 2 ** 20 for c in T.CASES)           # every operand below 32 MB
    for dtype in ("fp32", "bf16"):
        own = [(c, dict(zip(FIELDS, T.claim(c)))) for c in T.CASES if c.dtype == dtype]
        walk = [(c, r) for c, r in own if c.entry in ("cross_bwd", "dense_act_bwd")]
        last = lambda c, r: c.m - (r["chunks"] - 1) * r["rows_per_block"]
        for entry in ("cross_bwd", "dense_act_bwd"):
            mine = [(c, r) for c, r in walk if c.entry == entry]
            # vector walk: >= 3 rows a chunk, several strips, a short last chunk, idle waves in the last group
            assert any(r["kernel"] == T.VEC and r["rows_per_block"] >= 3 and r["strips"] >= 8 and r["chunks"] % 4 and
                       last(c, r) < r["rows_per_block"] for c, r in mine), (dtype, entry)
            # ... one strip, deep chunks, the last of one row
            assert any(r["kernel"] == T.VEC and r["strips"] == 1 and r["rows_per_block"] >= 3 and r["chunks"] > 2000 and
                       last(c, r) == 1 for c, r in mine)
            # ... a partial last strip
            assert any(r["kernel"] == T.VEC and (c.n // r["v"]) % 64 and r["strips"] >= 2 and r["rows_per_block"] >= 3 for c, r in mine)
            # scalar walk: several rows and strips
            assert {(c.m, c.n) for c, r in mine if r["kernel"] == T.SCALAR and r["rows_per_block"] >= 3 and r["strips"] >= 3} >= \
                {(2100, 250), (2750, 130)}
            # a vector-eligible shape on the scalar kernel: ld = n + 1, a base one element off, (bf16) n % 8 == 4
            pushed = [(c, r) for c, r in mine if r["kernel"] == T.SCALAR and c.n % 4 == 0 and r["rows_per_block"] >= 3]
            assert any(c.lds[0] == c.n + 1 and c.n % c.v == 0 for c, r in pushed) and any(c.off == 1 and c.n % c.v == 0 for c, r in pushed)
            assert dtype == "fp32" or any(c.n % 8 == 4 and c.off == 0 and c.lds[0] == c.n for c, r in pushed)
            assert {c.act for c, r in mine if r["kernel"] == T.VEC} == {0, 1, 2, 3} == {c.act for c, r in mine if r["kernel"] == T.SCALAR}
            # column sums absent, two-stage and by atomics, on both kernels
            assert {(r["kernel"], c.ws) for c, r in mine} >= {(k, w) for k in (T.VEC, T.SCALAR) for w in ("", "two_stage", "atomics")}
        # leading dimensions
        cross = [(c, r) for c, r in walk if c.entry == "cross_bwd"]
        assert any(c.lds[0] == c.n + c.v and r["kernel"] == T.VEC for c, r in cross)
        assert any(c.lds[0] == c.n + 3 and c.n % c.v == 0 and r["kernel"] == T.SCALAR for c, r in cross)
        dense = [(c, r) for c, r in walk if c.entry == "dense_act_bwd"]
        assert {r["kernel"] for c, r in dense if len(set(c.lds)) == 3} == {T.VEC, T.SCALAR}
        assert any("dz" not in c.outs for c, r in dense) and any("dbias" not in c.outs for c, r in dense)
        # the shapes of the earlier tests
        for entry in ("cross_fwd", "cross_bwd", "dense_act_bwd", "colsum"):
            assert {(c.m, c.n) for c, r in own if c.entry == entry} >= set(T.TINY)
        # colsum_finish_kernel: empty slices, the tail loop alone, the unrolled loop and a tail
        groups = {r["grid_y"] for c, r in own if r["two_stage"]}
        assert any(g < 32 for g in groups) and any(32 <= g < 128 for g in groups)
        assert any(g >= 128 and math.ceil(g / 32) % 4 for g in groups)
        if dtype == "fp32":
            assert 263 in groups
        # the forms of the cross backward, each on both kernels
        for kernel in (T.VEC, T.SCALAR):
            mine = [c for c, r in cross if r["kernel"] == kernel]
            forms = {c.form: c for c in mine if c.form}
            assert set(forms) == set("bcdefghijkl")
            for letter, c in forms.items():
                f = T.FORMS[letter]
                assert (c.act, c.acc, c.fold, c.u_null, c.outs) == (f.get("act", 0), f.get("acc", False), f.get("fold", False),
                                                                    f.get("u_null", False), f["outs"])
            assert any(c.u_null and c.act == R.NONE and "dx0" not in c.outs for c in mine)
            with_dx0 = [c for c in mine if "dx0" in c.outs]
            assert {c.diag == 0 for c in with_dx0} == {True, False} == {c.acc for c in with_dx0}
            # dxd absent, separate, aliased to dx0
            assert {(c.fold, "dxd" in c.outs) for c in with_dx0} == {(False, False), (False, True), (True, False)}
            assert {c.ws for c in mine} == {"", "two_stage", "atomics"}
        assert {r["acc"] for c, r in cross if r["kernel"] == T.VEC and "dx0" in c.outs} == {0, 1}
        # the forward and the column sum on their kernels; BCE at every n
        assert {r["kernel"] for c, r in own if c.entry == "cross_fwd"} == {T.VEC, T.SCALAR}
        assert {c.ws for c, r in own if c.entry == "colsum" and r["rows_per_block"] >= 3 and c.lds[0] > c.n} == {"two_stage", "atomics"}
        assert tuple(c.n for c, r in own if c.entry == "bce") == T.BCE_N
    assert T.BCE_N == (1, 1023, 1024, 1025, 65536, 65537, 200000)


def test_the_inputs_hold_the_special_points():
    for index, case in enumerate(T.CASES):
        if case.m * case.n > 300000 and case.entry != "bce":
            continue
        t = T.inputs_of(index)
        for k, v in t.items():
            assert np.array_equal(T.round_to(v, case.dtype if k != "labels" else "fp32"), v), (case.name, k)
        if case.entry == "bce":
            lo, hi = R.bce_bounds(T.BCE_EPS)
            want = {0.0, 1.0} if case.n < 8 or case.dtype == "bf16" else {0.0, 1.0, float(np.float32(5e-8)), hi}
            assert case.n < 2 or want <= set(t["pred"].tolist()), case.name
            assert t["pred"].min() >= 0 and t["pred"].max() <= 1
        elif case.entry in ("cross_bwd", "dense_act_bwd"):
            s = t["u" if case.entry == "cross_bwd" else "y"]
            assert (s == 1).any() and (t["g"] == 0).any() and np.signbit(s[s == 0]).any() and (~np.signbit(s[s == 0])).any()
            assert np.abs(t["g"]).max() <= 1 and (case.act != R.SIGMOID or s.min() >= 0)


# ---- (c) the planner ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tests/host/dense_walk_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("dense_walk_plan") / "dense_walk_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "dense_walk_plan_check.cpp"),
                    "-o", exe], check=True)

    def ask(args):
        run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
        lines = run.stdout.strip().splitlines()
        assert " 0 failed checks" in lines[-1]
        return [list(map(int, line.split())) for line in lines[:-1]]

    return ask


def test_the_planner_keeps_its_invariants_over_the_grid_under_the_sanitizers_and_knows_the_stated_geometry(planner):
    B = L.WALK_CROSS_BWD
    # (status kernel v acc two_stage rows_per_block strips chunks grid_y workspace) of "entry m n dtype ld misalign dbias ws acc"
    asked = [(B, 700, 4096, 0, 4096, 0, 1, 1, 0), (B, 1100, 2048, 0, 2048, 0, 1, 1, 1), (B, 1300, 4096, 1, 4096, 0, 1, 1, 0),
             (B, 700, 8192, 1, 8192, 0, 1, 0, 0), (B, 8200, 256, 0, 256, 0, 0, 1, 0), (B, 2750, 516, 0, 516, 0, 1, 1, 0),
             (B, 4100, 776, 1, 776, 0, 1, 1, 0), (B, 2100, 250, 0, 250, 0, 1, 1, 0), (B, 2750, 130, 1, 130, 0, 1, 1, 0),
             (B, 2100, 532, 0, 532, 0, 1, 1, 0), (B, 16384, 3456, 1, 3456, 0, 1, 1, 1), (B, 2750, 516, 0, 516, 4, 1, 1, 1),
             (L.WALK_COLSUM, 2100, 256, 0, 256, 0, 0, 1, 0), (L.WALK_CROSS_FWD, 2100, 256, 0, 256, 0, 1, 1, 1)]
    lines = planner([a for row in asked for a in row])
    got = [line[:9] for line in lines]
    assert got == [
        [0, 1, 4, 0, 1, 3, 16, 234, 59], [0, 1, 4, 1, 1, 3, 8, 367, 92], [0, 1, 8, 0, 1, 3, 8, 434, 109],
        [0, 1, 8, 0, 0, 3, 16, 234, 59], [0, 1, 4, 0, 0, 3, 1, 2734, 684], [0, 1, 4, 0, 1, 3, 3, 917, 230],
        [0, 1, 8, 0, 1, 3, 2, 1367, 342], [0, 2, 1, 0, 1, 3, 4, 700, 700], [0, 2, 1, 0, 1, 3, 3, 917, 917],
        [0, 1, 4, 0, 1, 2, 3, 1050, 263], [0, 1, 8, 1, 1, 28, 7, 586, 147],      # the ml_perf backward: 28 rows a wave
        [0, 2, 1, 0, 1, 7, 9, 393, 393],                                        # off 16 bytes: scalar, and never ACC
        [0, 2, 1, 0, 1, 3, 4, 700, 700], [0, 1, 4, 0, 0, 0, 0, 0, 0]]
    assert 234 % 4 == 2 and 367 % 4 == 3 and 434 % 4 == 2 and 917 % 4 == 1 and 700 - 233 * 3 == 1 and 8200 - 2733 * 3 == 1
    # the workspace is the widest route's: (2750, 516) walks 393 scalar chunks (9 strips of 64 columns, 7 rows a chunk)
    assert lines[5][9] == 393 * 516 * 4 and lines[7][9] == 700 * 250 * 4


def test_every_claimed_route_is_the_planners_and_the_workspace_is_its_too():
    ws = L.lib().krs_colsum_workspace_bytes
    for case in T.CASES:
        if case.entry == "bce":
            continue
        claimed = T.claim(case)
        assert planned(case) == claimed, case.name
        if claimed[3]:
            # the entry's workspace covers this route and every other the shape can take
            assert ws(case.m, case.n) >= claimed[7] * case.n * 4, case.name
            shape = dataclasses.replace(case, entry="cross_bwd", ld=(), off=0)
            routes = [dataclasses.replace(shape, off=1), dataclasses.replace(shape, dtype="fp32"), dataclasses.replace(shape, dtype="bf16")]
            assert ws(case.m, case.n) == max(T.claim(c)[7] for c in routes) * case.n * 4, case.name
    assert ws(0, 8) == 0 and ws(8, 0) == 0 and ws(-1, 8) == 0 and ws(1, 1) == 4
    assert ws(2100, 250) == 700 * 250 * 4 and ws(700, 4096) == 88 * 4096 * 4        # the bf16 vector route: 350 chunks of 2 rows


# ---- (d) the ABI and the refusals -----------------------------------------------------------------------------------
WALK_ENTRIES = ("krs_colsum_workspace_bytes", "krs_cross_epilogue_fwd", "krs_cross_epilogue_bwd", "krs_dense_act_bwd", "krs_colsum",
                "krs_dense_walk_last_route", "krs_dense_walk_plan_route", "krs_bce_fwd_bwd")


def test_abi_prototypes_match_the_header():
    declared = header_prototypes(_header())
    for name in WALK_ENTRIES:
        assert name in declared and name in L.PROTOTYPES, name
        restype, argtypes = L.PROTOTYPES[name]
        assert (restype, list(argtypes)) == (declared[name][0], list(declared[name][1])), name
        assert hasattr(L.lib(), name)
    assert C.sizeof(L.DenseWalkRoute) == 48 and len(L.PROTOTYPES["krs_dense_walk_plan_route"][1]) == 12
    text = _header()
    assert "KRS_DENSE_WALK_NONE = 0, KRS_DENSE_WALK_VEC, KRS_DENSE_WALK_SCALAR" in text
    assert "KRS_DENSE_WALK_CROSS_FWD = 0, KRS_DENSE_WALK_CROSS_BWD, KRS_DENSE_WALK_DENSE_ACT_BWD, KRS_DENSE_WALK_COLSUM" in text
    assert (L.WALK_NONE, L.WALK_VEC, L.WALK_SCALAR) == (T.NONE, T.VEC, T.SCALAR) == (0, 1, 2)
    for name, value in (("KRS_ERR_INVALID", INVALID), ("KRS_ERR_UNSUPPORTED", UNSUPPORTED)):
        assert f"{name} = {value}" in text, name


def _fwd(**kw):
    a = dict(u=16, x0=16, x=16, y=16, m=4, n=8, ld=8, diag=0.0, dtype=L.F32)
    a.update(kw)
    return L.lib().krs_cross_epilogue_fwd(*a.values(), None)


def _bwd(**kw):
    a = dict(g=16, u=16, x0=16, x=16, du=16, dx0=16, acc=0, dxd=None, dbias=None, m=4, n=8, ld=8, diag=0.0, act=0, dtype=L.F32,
             ws=None, ws_bytes=0)
    a.update(kw)
    return L.lib().krs_cross_epilogue_bwd(*a.values(), None)


def _dense(**kw):
    a = dict(g=16, ldg=8, y=16, ldy=8, dz=16, lddz=8, dbias=None, m=4, n=8, act=1, dtype=L.F32, ws=None, ws_bytes=0)
    a.update(kw)
    return L.lib().krs_dense_act_bwd(*a.values(), None)


def _colsum(**kw):
    a = dict(a=16, lda=8, m=4, n=8, dtype=L.F32, out=16, ws=None, ws_bytes=0)
    a.update(kw)
    return L.lib().krs_colsum(*a.values(), None)


def _bce(**kw):
    a = dict(pred=16, dtype=L.F32, labels=16, n=4, eps=1e-7, scale=1.0, loss=16, dpred=None, partials=None)
    a.update(kw)
    return L.lib().krs_bce_fwd_bwd(*a.values(), None)


REFUSALS = [
    (_fwd, dict(u=None), INVALID, "cross_epilogue_fwd: null operand"), (_fwd, dict(y=None), INVALID, "cross_epilogue_fwd: null operand"),
    (_fwd, dict(m=-1), INVALID, "cross_epilogue_fwd: bad sizes"), (_fwd, dict(n=-1), INVALID, "cross_epilogue_fwd: bad sizes"),
    (_fwd, dict(ld=7), INVALID, "cross_epilogue_fwd: bad sizes"), (_fwd, dict(dtype=2), INVALID, "cross_epilogue_fwd: dtype must be f32 or bf16"),
    (_fwd, dict(m=2 ** 31), UNSUPPORTED, "cross_epilogue_fwd: m <= 2^31 - 1"),
    (_bwd, dict(g=None), INVALID, "cross_epilogue_bwd: null g/x0"), (_bwd, dict(x0=None), INVALID, "cross_epilogue_bwd: null g/x0"),
    (_bwd, dict(u=None, dx0=None, act=1), INVALID, "cross_epilogue_bwd: an activation needs the saved u"),
    (_bwd, dict(u=None), INVALID, "cross_epilogue_bwd: dx0 needs u and x"), (_bwd, dict(x=None), INVALID, "cross_epilogue_bwd: dx0 needs u and x"),
    (_bwd, dict(m=-1), INVALID, "cross_epilogue_bwd: bad sizes"), (_bwd, dict(n=-2), INVALID, "cross_epilogue_bwd: bad sizes"),
    (_bwd, dict(ld=7), INVALID, "cross_epilogue_bwd: bad sizes"), (_bwd, dict(dtype=-1), INVALID, "cross_epilogue_bwd: dtype must be f32 or bf16"),
    (_bwd, dict(m=2 ** 31), UNSUPPORTED, "cross_epilogue_bwd: m <= 2^31 - 1"),
    (_bwd, dict(dbias=16, ws=16, ws_bytes=4 * 8 * 4 - 1), INVALID, "cross_epilogue_bwd: workspace too small"),
    (_dense, dict(g=None), INVALID, "dense_act_bwd: null operand"), (_dense, dict(dz=None), INVALID, "dense_act_bwd: null operand"),
    (_dense, dict(y=None), INVALID, "dense_act_bwd: an activation needs the saved output y"),
    (_dense, dict(m=-1), INVALID, "dense_act_bwd: bad sizes"), (_dense, dict(ldg=7), INVALID, "dense_act_bwd: bad sizes"),
    (_dense, dict(ldy=7), INVALID, "dense_act_bwd: bad sizes"), (_dense, dict(lddz=0), INVALID, "dense_act_bwd: bad sizes"),
    (_dense, dict(dtype=2), INVALID, "dense_act_bwd: dtype must be f32 or bf16"),
    (_dense, dict(m=2 ** 31), UNSUPPORTED, "dense_act_bwd: m <= 2^31 - 1"),
    (_dense, dict(dbias=16, ws=16, ws_bytes=0), INVALID, "dense_act_bwd: workspace too small"),
    (_colsum, dict(a=None), INVALID, "colsum: null operand"), (_colsum, dict(out=None), INVALID, "colsum: null operand"),
    (_colsum, dict(m=-1), INVALID, "colsum: bad sizes"), (_colsum, dict(n=-1), INVALID, "colsum: bad sizes"),
    (_colsum, dict(dtype=7), INVALID, "colsum: dtype must be f32 or bf16"), (_colsum, dict(m=2 ** 31), UNSUPPORTED, "colsum: m <= 2^31 - 1"),
    (_colsum, dict(ws=16, ws_bytes=127), INVALID, "colsum: workspace too small"),
    (_bce, dict(pred=None), INVALID, "bce: null argument"), (_bce, dict(labels=None), INVALID, "bce: null argument"),
    (_bce, dict(loss=None), INVALID, "bce: null argument"), (_bce, dict(n=0), INVALID, "bce: empty batch"),
    (_bce, dict(dtype=2), INVALID, "bce: bad dtype"), (_bce, dict(eps=0.0), INVALID, "bce: epsilon must be in (0, 0.5)"),
    (_bce, dict(eps=0.5), INVALID, "bce: epsilon must be in (0, 0.5)"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=[f"{f.__name__[1:]}-{'-'.join(map(str, kw))}-{i}" for i, (f, kw, _, _) in enumerate(REFUSALS)])
def test_refusals_come_before_the_first_launch_and_leave_no_route(k):
    call, kw, code, message = REFUSALS[k]
    rc = call(**kw)
    assert rc == code and L.lib().krs_last_error().decode() == message, (rc, L.lib().krs_last_error())
    assert last_route() == (0,) * 8 and L.lib().krs_dense_walk_last_route(None) == 0


def test_empty_calls_are_no_ops_and_the_plan_entry_refuses_what_the_entries_do():
    # (no column sums asked for: nothing to clear, so no call reaches the device)
    assert _fwd(m=0) == 0 and _fwd(n=0, ld=0) == 0 and _bwd(m=0) == 0 and _bwd(n=0) == 0 and _dense(m=0) == 0 and _dense(n=0) == 0
    assert _colsum(n=0) == 0 and last_route() == (0,) * 8
    rt = L.DenseWalkRoute()
    lds, ptrs = (C.c_int64 * 1)(8), (C.c_void_p * 1)(4096)
    plan = lambda entry=1, m=4, n=8, dtype=0, ld=lds, n_ld=1: L.lib().krs_dense_walk_plan_route(entry, m, n, dtype, ld, n_ld, ptrs, 1, 1, 1, 1, C.byref(rt))
    assert plan() == 0 and route_tuple(rt) == (T.VEC, 4, 1, 1, 1, 1, 4, 1)
    assert L.lib().krs_dense_walk_plan_route(1, 4, 8, 0, lds, 1, ptrs, 1, 1, 1, 1, None) == 0 and last_route() == (0,) * 8
    for kw, code, message in ((dict(entry=4), INVALID, "unknown entry"), (dict(entry=-1), INVALID, "unknown entry"),
                              (dict(m=-1), INVALID, "bad sizes"), (dict(n=9), INVALID, "bad sizes"), (dict(ld=None), INVALID, "bad sizes"),
                              (dict(dtype=2), INVALID, "dtype must be f32 or bf16"), (dict(m=2 ** 31), UNSUPPORTED, "m <= 2^31 - 1")):
        assert plan(**kw) == code and route_tuple(rt) == (0,) * 8, kw
        assert L.lib().krs_last_error().decode() == "dense_walk_plan_route: " + message
    assert plan(m=0) == 0 and route_tuple(rt) == (0,) * 8


# ---- (e) the bounds have teeth --------------------------------------------------------------------------------------
def _patched(fn, case, t):
    old = R.act_grad
    R.act_grad = fn
    try:
        return T.run(case, t)[0]
    finally:
        R.act_grad = old


def _faults(case, t, ref):
    """name -> what the restatement gives with that mistake made, for the mistakes this case can show."""
    kernel, v, acc, two_stage, rows, strips, chunks, grid_y = T.claim(case)
    sums = [k for k in ("dbias", "colsum") if k in ref]
    bad = {}
    if case.entry in ("cross_bwd", "dense_act_bwd", "colsum"):
        gk = "a" if case.entry == "colsum" else "g"
        if rows >= 2:
            i = np.arange(case.m)
            stale = i[((i % rows == rows - 1) | (i == case.m - 1)) & (i % rows != 0)]
            g = t[gk].copy()
            g[stale] = t[gk][stale - 1]
            bad["the last row of a chunk from the row before's g"] = T.run(case, {**t, gk: g})[0]
        if sums and chunks >= 2:
            cut = (chunks - 1) * rows
            part = lambda sl: T.run(case, {k: v[sl] for k, v in t.items()})[0][sums[0]]
            bad["the last chunk left out of the column sums"] = {**ref, sums[0]: part(slice(0, cut))}
            if kernel == T.VEC and chunks % 4:
                bad["an idle wave's slot added twice"] = {**ref, sums[0]: ref[sums[0]] + part(slice(cut, case.m))}
        if case.act == R.RELU:
            bad["relu'(0) = 1"] = _patched(lambda act, u: (u >= 0).astype(np.float64), case, t)
        if case.act == R.SIGMOID:
            bad["sigmoid' = 1 - u^2"] = _patched(lambda act, u: 1.0 - u * u, case, t)
        if case.fold:
            bad["the folded direct term dropped"] = T.run(dataclasses.replace(case, fold=False, outs=tuple(o for o in case.outs if o != "dxd")), t)[0]
        if case.acc and "dx0" in case.outs:
            bad["dx0's initial value ignored"] = T.run(case, {k: v for k, v in t.items() if k != "init"})[0]
    if case.entry == "bce":
        lo, hi = R.bce_bounds(T.BCE_EPS)
        p = np.clip(t["pred"], lo, hi)
        bad["BCE's gradient kept outside the clip"] = {**ref, "dpred": T.BCE_SCALE / case.n * ((1 - t["labels"]) / (1 - p) - t["labels"] / p)}
    return bad


def test_the_bounds_would_not_hide_a_mistake():
    applied = {}
    for index, case in enumerate(T.CASES):
        t, ref, mag, bound = T.reference_of(index)
        assert T.worst_ratio(ref, ref, bound)[0] == 0.0
        # the restatement rounded once to the output's dtype is inside its own bound
        once = {k: T.round_to(v, "fp32" if k in ("dbias", "colsum", "loss") else case.dtype) for k, v in ref.items()}
        assert T.worst_ratio(once, ref, bound)[0] <= 1.0, case.name
        for what, got in _faults(case, t, ref).items():
            if all(np.array_equal(got[k], ref[k]) for k in ref):
                continue                    # (these inputs cannot show it: a left-out row of zeros, no u == 0 with g x0 != 0)
            ratio, where = T.worst_ratio(got, ref, bound)
            assert ratio > 1.0, f"{what} stays inside the bound of {case.name} (worst ratio {ratio:.3f} at {where})"
            applied[what] = applied.get(what, 0) + 1
    assert len(applied) == 8 and min(applied.values()) >= 8, applied
