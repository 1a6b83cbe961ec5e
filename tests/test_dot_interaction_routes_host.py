"""The DotInteraction (K4) route table (tests/dot_interaction_cases.py), checked without a GPU.  Every expected
krs_dot_route record is asserted against the planner (keras_rs_amd/csrc/dot_plan.h through
krs_dot_interaction_plan_route, which launches nothing); the table names every one of the 40 kernel builds of
keras_rs_amd/csrc/dot_interaction.hip -- enumerated here, so a case dropped from it fails, not silently; refusals return
their status and an all-zero record; the float64 restatement's own fp32 evaluation stays inside the bound the GPU test
holds the kernels to; and the planner's invariants are walked by a stand-alone program built with the sanitizers
(tests/host/dot_plan_check.cpp).  tests/test_dot_interaction_matrix_gpu.py asserts the same records against what ran."""

import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dot_interaction_restatement as RS
from tests.dot_interaction_cases import ALT, BLOCK_MASK, CASES, ES, FIELDS, FULL, MODES, ONE, R, feature_layout, inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def _have(pred=lambda c: True, **want):
    """the cases whose fields / route fields equal `want` and that satisfy `pred`"""
    def ok(c):
        return all((getattr(c, k) if hasattr(c, k) else c.route[k]) == v for k, v in want.items()) and pred(c)
    return [c for c in CASES if ok(c)]


def test_the_table_is_well_formed():
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        assert set(c.route) == set(FIELDS), c.name
        assert c.B * c.F * c.D * 4 <= 80 << 20 and c.B * max(c.cols, 1) * ES[c.dtype] <= 40 << 20, c.name
        assert c.off in (0, 2, 4, 8) and (c.mask == 0 or c.direction == "bwd"), c.name
        assert not c.odd_ld or c.route["kernel"].endswith(("generic", "block")), c.name


def test_every_kernel_build_is_expected_somewhere():
    # dot_fwd_mfma_kernel<ES, KS>: 4
    assert [(dt, ks) for dt, ks in (("bf16", 8), ("bf16", 4), ("bf16", 0), ("f32", 0))
            if not _have(kernel="fwd_mfma", dtype=dt, ks=ks)] == []
    # dot_bwd_mfma_kernel<SELF, ACC, NG, 4>: 8
    assert [k for k in itertools.product((0, 1), (0, 1), (9, 16))
            if not _have(kernel="bwd_mfma", self=k[0], acc=k[1], ng=k[2])] == []
    # dot_bwd_valu_kernel<ES, FR, SELF, MULTI, ACC>: 2 x {28 one sample, 32 one sample, 32 MULTI} x 2 x 2 = 24
    missing = [k for k in itertools.product(("f32", "bf16"), ((28, 0), (32, 0), (32, 1)), (0, 1), (0, 1))
               if not _have(kernel="bwd_valu", dtype=k[0], fr=k[1][0], multi=k[1][1], self=k[2], acc=k[3])]
    assert missing == []
    # the plain and the block kernels: 4, in both dtypes
    for k, dt in itertools.product(("fwd_generic", "bwd_generic", "fwd_block", "bwd_block"), ("f32", "bf16")):
        assert _have(kernel=k, dtype=dt), (k, dt)
    assert {c.route["kernel"] for c in CASES} == {"fwd_mfma", "fwd_generic", "fwd_block", "bwd_mfma", "bwd_valu",
                                                  "bwd_generic", "bwd_block"}
    # every build that reads skip_gather at run time, in both layouts of the output / incoming gradient
    for dt, ks in (("bf16", 8), ("bf16", 4), ("bf16", 0), ("f32", 0)):
        assert {c.skip for c in _have(kernel="fwd_mfma", dtype=dt, ks=ks)} == {False, True}
    for k in itertools.product(("f32", "bf16"), (0, 1), (0, 1)):      # (FR 28 is never the [F, F] layout)
        for fr, multi in ((32, 0), (32, 1)):
            assert {c.skip for c in _have(kernel="bwd_valu", dtype=k[0], fr=fr, multi=multi, self=k[1], acc=k[2])} == {False, True}, k
    for k in ("fwd_generic", "bwd_generic", "fwd_block", "bwd_block"):
        assert {(c.self_i, c.skip) for c in _have(kernel=k)} == set(MODES), k


def test_the_shapes_of_the_issue_are_in_the_table():
    fm = _have(kernel="fwd_mfma")
    assert {c.F for c in fm} >= {1, 2, 27, 32} and {(c.dtype, c.D) for c in fm} == {
        ("bf16", 128), ("bf16", 64), ("bf16", 8), ("bf16", 72), ("f32", 4), ("f32", 12)}
    for dt, ks in (("bf16", 8), ("bf16", 4), ("bf16", 0), ("f32", 0)):          # the prefetched second sample
        assert _have(kernel="fwd_mfma", dtype=dt, ks=ks, F=2, B=2048 * 4 + 3)
    bm = _have(kernel="bwd_mfma")
    assert {c.D for c in bm} == {32, 64, 96, 128} and {c.F for c in bm} == {2, 5, 27, 32}
    assert {c.route["acc"] for c in _have(kernel="bwd_mfma", F=2, D=32, B=2048 * 2 + 3)} == {0, 1}
    bv = _have(kernel="bwd_valu")
    assert {c.D for c in bv} >= {2, 4, 6, 16, 72, 130, 160, 256} and {c.F for c in bv} >= {22, 23, 24, 25, 28, 29, 32}
    assert {c.D for c in bv if c.dtype == "bf16"} >= {72, 130, 160, 256}
    assert {(c.self_i, c.skip) for c in bv} == set(MODES)
    for F in (23, 24):       # hole 1: the [F, F] layout of 529 / 576 columns without SELF takes the MULTI build
        assert _have(kernel="bwd_valu", F=F, self_i=False, skip=True, multi=1, spw=1, dtype="f32")
        assert _have(kernel="bwd_valu", F=F, self_i=False, skip=True, multi=1, spw=1, dtype="bf16")
    assert _have(kernel="bwd_valu", F=24, self_i=True, skip=True, multi=0, ng=9)
    # hole 2: D in {6, 8} with SELF, D = 4, D = 2 -- never more than 64 KiB of LDS
    assert _have(kernel="bwd_valu", D=6, self_i=True, spw=15) and _have(kernel="bwd_valu", D=8, self_i=True, spw=15)
    assert {c.route["spw"] for c in _have(kernel="bwd_valu", D=4)} >= {15, 16}
    assert {c.route["spw"] for c in _have(kernel="bwd_valu", D=2)} >= {15, 16}
    assert max(c.route["lds_bytes"] for c in CASES) == 1024 + 2 * 16 * 497 * 4 <= 65536
    for multi in (0, 1):     # a workgroup's second group of samples
        assert _have(lambda c: c.B == 16384 * c.route["spw"] + 5, kernel="bwd_valu", F=2, multi=multi)
    for k in ("fwd_generic", "bwd_generic"):
        got = _have(kernel=k)
        assert [c for c in got if c.D % 2] and [c for c in got if c.off == 4] and {33, 64} <= {c.F for c in got}
        assert [c for c in got if c.odd_ld]
        assert [c for c in got if c.B * c.F * (c.D if k == "bwd_generic" else c.F) > 65536 * 256]
    for k in ("fwd_block", "bwd_block"):
        assert {c.F for c in _have(kernel=k)} == {65, 129, 130}
    assert [c for c in _have(kernel="fwd_block") if c.B * 32 * 64 > 65536 * 256]
    masked = _have(lambda c: c.mask & BLOCK_MASK == BLOCK_MASK, kernel="bwd_block")
    assert {(c.self_i, c.skip) for c in masked} >= {(False, False), (True, True), (False, True), (True, False)}
    for k in ("bwd_mfma", "bwd_valu"):       # empty, full, one bit, alternating under all four modes
        for mode in MODES:
            got = {c.mask for c in _have(kernel=k, self_i=mode[0], skip=mode[1])}
            assert 0 in got and {FULL & 31, ONE, ALT & 31} <= got, (k, mode)


# ---- the table against the planner -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    from keras_rs_amd import dense_ops as D
    from keras_rs_amd.build import build

    build()
    return D


def _planned(D, c):
    """the plan of the call tests/test_dot_interaction_matrix_gpu.py makes for case c, on fake addresses"""
    from keras_rs_amd import _lib as L

    lead, cols, widths = feature_layout(c)
    es = ES[c.dtype]
    step = 1 << 32
    if c.layout == "concat":
        ptrs = [0x7F0000100000 + col * es for col in cols]
        gptrs = [0x7E0000100000 + col * es for col in cols]
    else:
        ptrs = [0x7F0000100000 + f * step + lead * es for f in range(c.F)]
        gptrs = [0x7E0000100000 + f * step + lead * es for f in range(c.F)]
    return D.dot_plan_route(c.direction == "bwd", ptrs, widths, c.B, c.D, L.BF16 if c.dtype == "bf16" else L.F32, c.self_i,
                            c.skip, 0x7D0000100000, c.cols + 5, gptrs if c.direction == "bwd" else None,
                            widths if c.direction == "bwd" else None, c.mask)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_planner_gives_every_case_its_expected_route(ops, case):
    assert _planned(ops, case) == (0, case.route)


def test_the_environment_switch_keeps_the_matrix_cores_out(ops, monkeypatch):
    c = _have(kernel="bwd_mfma", F=27, D=96)[0]
    monkeypatch.setenv("KRS_DOT_BWD_VALU", "1")
    status, rt = _planned(ops, c)
    assert status == 0 and rt["kernel"] == "bwd_valu" and rt["fr"] == (32 if c.skip else 28) and rt["lps_log2"] == 6
    monkeypatch.delenv("KRS_DOT_BWD_VALU")
    assert _planned(ops, c) == (0, c.route)


def test_refusals_return_their_status_and_no_record(ops):
    import ctypes as C

    from keras_rs_amd import _lib as L

    lib = L.lib()
    ptrs = (C.c_void_p * 2)(0x7F0000100000, 0x7F0000200000)
    nulls = (C.c_void_p * 2)(0x7F0000100000, None)
    lds = (C.c_int64 * 2)(128, 128)
    ok = [1, ptrs, lds, 2, 100, 128, L.BF16, 0, 0, 0x7D0000100000, 8, ptrs, lds, 0]
    rt = L.DotRoute()
    before = ops.dot_last_route()
    assert lib.krs_dot_interaction_plan_route(*ok, C.byref(rt)) == 0 and rt.kernel == 4
    assert ops.dot_last_route() == before        # (the query does not touch the record of the last call)
    assert C.sizeof(rt) == 56
    for what, pos, value in (("null feats", 1, None), ("null ld", 2, None), ("no features", 3, 0), ("negative batch", 4, -1),
                             ("dim 0", 5, 0), ("bad dtype", 6, L.I8), ("null grad_out", 9, None), ("null grad_feats", 11, None),
                             ("null grad_feat_ld", 12, None), ("a null feature", 1, nulls), ("a null gradient", 11, nulls)):
        args = list(ok)
        args[pos] = value
        rt = L.DotRoute(kernel=9, blocks=9)
        assert lib.krs_dot_interaction_plan_route(*args, C.byref(rt)) == INVALID, what
        assert ops._dot_route_dict(rt) == R(), what
        assert lib.krs_last_error(), what
        # the entries themselves refuse before any launch and leave an all-zero record
        assert lib.krs_dot_interaction_bwd_accumulate(*args[1:], None) == INVALID, what
        assert ops.dot_last_route() == R() and lib.krs_dot_interaction_last_route(None) == 0, what
    for what, pos, value in (("null feats", 1, None), ("null out", 9, None), ("dim 0", 5, 0)):
        args = list(ok)
        args[pos] = value
        assert lib.krs_dot_interaction_fwd(*args[1:11], None) == INVALID, what
        assert ops.dot_last_route() == R(), what
    # an empty call succeeds, launches nothing and leaves no record either
    args = list(ok)
    args[4] = 0
    assert lib.krs_dot_interaction_plan_route(*args, C.byref(rt)) == 0 and ops._dot_route_dict(rt) == R()
    assert lib.krs_dot_interaction_bwd_accumulate(*args[1:], None) == 0 and ops.dot_last_route() == R()
    assert lib.krs_dot_interaction_fwd(*args[1:11], None) == 0 and ops.dot_last_route() == R()


# ---- the restatement's own fp32 evaluation stays inside the bound the kernels are held to ------------------------------

SMALL = [c for c in CASES if c.B * c.F * c.D <= 1 << 16 and c.B * max(c.cols, 1) <= 1 << 16]


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_the_restatement_evaluated_in_fp32_stays_inside_the_bound(case):
    c, h = case, inputs(case.name)
    bf16 = c.dtype == "bf16"
    X = h["X"].astype(np.float64)
    if c.direction == "fwd":
        ref, S = RS.forward(X, c.self_i, c.skip)
        got = RS.forward_fp32(h["X"], c.self_i, c.skip, bf16)
        tol = RS.bound(ref, S, c.D, bf16)
    else:
        chunked = c.route["kernel"] == "bwd_block"
        ex = None if h["existing"] is None else h["existing"].astype(np.float64)
        ref, S, partial = RS.backward(X, h["G"].astype(np.float64), c.self_i, c.skip, ex, c.mask, chunked)
        got = RS.backward_fp32(h["X"], h["G"], c.self_i, c.skip, bf16, h["existing"], c.mask, chunked)
        tol = RS.bound(ref, S, c.F + (1 if c.mask else 0), bf16, partial if bf16 else None)
    assert got.shape == ref.shape and np.isfinite(ref).all()
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    if c.skip and c.direction == "fwd":      # the masked part of the [F, F] layout is zero, with a zero bound
        i, j = np.triu_indices(c.F, 0 if not c.self_i else 1)
        assert (ref.reshape(c.B, c.F, c.F)[:, i, j] == 0).all() and (tol.reshape(c.B, c.F, c.F)[:, i, j] == 0).all()


# ---- the planner's invariants, walked by a stand-alone program under the sanitizers ------------------------------------

def test_the_planner_header_compiles_without_hip_and_keeps_its_invariants_under_the_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dot_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "dot_plan_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "0 failed checks" in run.stdout
