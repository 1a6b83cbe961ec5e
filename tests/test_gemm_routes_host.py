"""The krs_gemm route table (tests/gemm_route_cases.py), checked without a GPU.  Every expected route record is asserted
against the planner (keras_rs_amd/csrc/gemm_plan.h through krs_gemm_plan_route, which launches nothing); the planner's
invariants are walked by a stand-alone program built with the sanitizers (tests/host/gemm_plan_check.cpp); and the table
names every kernel family, build, width, reduce kernel and pipeline of keras_rs_amd/csrc/gemm.hip, so a case dropped
from it fails here, not silently.  tests/test_gemm_routes_gpu.py asserts the same records against what ran."""

import ctypes as C
import os
import shutil
import subprocess

import pytest

from tests.gemm_route_cases import ACT_FORMS, CASES, FORMS, R, leading_dims, split_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILE_KERNELS = ("mfma", "glds", "pp256", "pp64")


def _have(**want):
    """the cases whose fields / route fields equal `want`"""
    def ok(c):
        return all((getattr(c, k) if hasattr(c, k) else c.route[k]) == v for k, v in want.items())
    return [c for c in CASES if ok(c)]


def test_the_table_is_well_formed():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert set(c.route) == {"kernel", "splits", "reduce", "epilogue", "ep_vec", "thin_width", "thin_is_a"}, c.name
        assert (c.route["splits"] > 1) == (c.route["reduce"] is not None), c.name
        assert all(ld >= ext for ld, ext in zip(leading_dims(c)[2:], (c.n,) * 4)), c.name
        assert set(c.pad) <= set("abcxur") and set(c.off) <= {"a", "b", "c", "bias", "x0", "x", "u", "r"}, c.name
        if "u" in FORMS[c.ep]:       # (a kernel that confused ldu and ldx must read inside x0's allocation)
            assert leading_dims(c)[4] <= leading_dims(c)[3], c.name


def test_every_kernel_family_dtype_and_layout_is_expected_somewhere():
    built = {   # family -> (input dtypes, layouts) it is built for / reachable with
        "generic": (("bf16", "f32"), ("nn", "nt", "tn")),
        "mfma": (("bf16", "f32"), ("nn", "nt", "tn")),
        "glds": (("bf16", "f32"), ("nt",)),
        "tn_glds": (("bf16",), ("tn",)),
        "pp256": (("bf16",), ("nt",)),
        "pp256_kstrided": (("bf16",), ("tn",)),
        "pp64": (("bf16",), ("nt",)),
        "thin": (("bf16", "f32"), ("tn",)),
        "rowdot": (("bf16", "f32"), ("nn", "nt")),
        "smallk": (("bf16", "f32"), ("nn", "nt")),
    }
    missing = [(k, dt, lay) for k, (dts, lays) in built.items() for dt in dts for lay in lays
               if not _have(kernel=k, idt=dt, layout=lay)]
    assert missing == []
    assert {c.route["kernel"] for c in CASES} == set(built) | {None}
    # every bf16 product also with fp32 output (the ABI allows it on every route)
    assert [k for k in built if not _have(kernel=k, idt="bf16", odt="f32")] == []
    # fp32 output from bf16 input with a cross and with a residual epilogue
    assert [c for c in CASES if c.idt == "bf16" and c.odt == "f32" and "x0" in FORMS[c.ep]]
    assert [c for c in CASES if c.idt == "bf16" and c.odt == "f32" and "r" in FORMS[c.ep]]


def test_every_epilogue_build_and_store_path_of_the_tile_kernels():
    missing = [(k, e) for k in TILE_KERNELS for e in (0, 1, 2) if not _have(kernel=k, epilogue=e, splits=1)]
    missing += [(k, "ep_vec", v) for k in TILE_KERNELS for v in (True, False) if not _have(kernel=k, ep_vec=v, splits=1)]
    assert missing == []
    # partial tiles on both edges and an n that is not a multiple of 8, once per tile kernel that accepts such an n
    for k in TILE_KERNELS:
        assert [c for c in _have(kernel=k) if c.n % 8 and c.m % 256 and c.n % 256 and c.m % 128 and c.n % 128], k
    for k in ("tn_glds", "pp256_kstrided"):      # (these need m and n in whole vectors)
        assert [c for c in _have(kernel=k) if c.m % 128 and c.n % 128 and c.m % 256 and c.n % 256], k


def test_every_thin_width_on_both_sides_split_and_unsplit():
    missing = [(w, a, split) for w in (1, 4, 8, 16) for a in (True, False) for split in (True, False)
               if not [c for c in _have(kernel="thin", thin_width=w, thin_is_a=a) if (c.route["splits"] > 1) == split]]
    assert missing == []
    assert all(not c.ws for c in _have(kernel="thin", splits=1))      # the unsplit form: no workspace passed


def test_split_k_reaches_every_reduce_kernel_and_every_split_tile_kernel_with_a_short_last_split():
    def short_last(cases):
        return [c for c in cases if 0 < split_geometry(c)[1] < split_geometry(c)[0]]

    assert [r for r in ("scalar", "vec4", "vec8") if not short_last(_have(reduce=r))] == []
    split = [c for c in CASES if c.route["splits"] > 1]
    for k in ("tn_glds", "pp256_kstrided", "pp256", "pp64", "thin", "mfma"):
        assert short_last([c for c in split if c.route["kernel"] == k]), k
    # the split ring: 32-k blocks (K = 32 mod 64) on gemm_pp256_kernel, 64-k blocks on gemm_pp64_kernel
    assert [c for c in short_last(split) if c.route["kernel"] == "pp256" and c.layout == "nt" and c.k % 64 == 32]
    assert [c for c in short_last(split) if c.route["kernel"] == "pp64" and c.k % 64 == 0]
    # a NULL epilogue on a split product (what gemm_slab_reduce_vec4_kernel requires), and on an unsplit one
    assert all(c.ep == "null" for c in _have(reduce="vec4"))
    assert [c for c in CASES if c.ep == "null" and c.route["splits"] == 1 and c.route["kernel"]]


def test_pipelines_small_eligible_shapes_and_the_empty_products():
    ring = [c for c in CASES if c.layout == "nt" and c.idt == "bf16" and -(-c.m // 256) * -(-c.n // 256) >= 192]
    assert {c.pipe for c in ring} == {0, 4, 5}
    assert {c.route["kernel"] for c in ring if c.pipe == 4} == {"pp64"}
    assert {c.route["kernel"] for c in ring if c.pipe == 5} == {"pp256"}
    assert {c.route["kernel"] for c in ring if c.pipe == 0} <= {"mfma", "glds"}
    assert [c for c in _have(kernel="mfma", idt="f32") if max(c.m, c.n, c.k) <= 4]
    assert [c for c in _have(kernel="mfma", idt="bf16") if max(c.m, c.n, c.k) <= 8]
    assert [c for c in CASES if c.k == 0 and c.m and c.n and c.ep == "bias"]        # C = relu(bias)
    assert [c for c in CASES if c.m == 0 and c.route["kernel"] is None]


def test_the_argument_classes_the_layers_use_are_present():
    for key in "abcxur":                             # every leading dimension padded somewhere ...
        assert [c for c in CASES if c.pad.get(key)], key
    for key in ("a", "b", "c", "x0", "x", "r"):      # ... and every base pointer off 16 bytes somewhere
        assert [c for c in CASES if c.off.get(key)], key
    assert {c.ep for c in CASES} == set(FORMS)
    for v in (0.0, 0.5, 1.0, 2.0, -2.0):
        assert [c for c in CASES if c.diag == v and "x0" in FORMS[c.ep]], ("diag_scale", v)
        assert [c for c in CASES if c.beta == v and "r" in FORMS[c.ep]], ("beta", v)
    assert set(ACT_FORMS) <= set(FORMS)


# ---- the table against the planner -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from keras_rs_amd import _lib as L
    from keras_rs_amd.build import build

    build()
    yield L
    L.lib().krs_gemm_set_option(0, 4)


def _planned(L, c, ws=None):
    """(status, route) of the call tests/test_gemm_routes_gpu.py makes for case c: its leading dimensions, a fake base
    address 0x100000 + offset per operand (only alignment is read), its epilogue struct, the workspace of the query."""
    from keras_rs_amd import dense_ops as D

    es_in, es_out = (2 if c.idt == "bf16" else 4), (2 if c.odt == "bf16" else 4)
    lda, ldb, ldc, ldx, ldu, ldr = leading_dims(c)

    def addr(key, es):
        return 0x100000 + c.off.get(key, 0) * es

    form, ep = FORMS[c.ep], None
    if c.ep != "null":
        ep = L.GemmEpilogue()
        ep.act, ep.diag_scale, ep.beta = 0, c.diag, c.beta
        if "bias" in form:
            ep.bias = addr("bias", 4)
        if "x0" in form:
            ep.x0, ep.x, ep.ldx = addr("x0", es_out), addr("x", es_out), ldx
        if "u" in form:
            ep.u_out, ep.ldu = addr("u", es_out), ldu
        if "r" in form:
            ep.r, ep.ldr = addr("r", es_out), ldr
    a_km, b_nk = c.layout == "tn", c.layout == "nt"
    if ws is None:
        ws = int(L.lib().krs_gemm_workspace_bytes(c.m, c.n, c.k, int(a_km))) if c.ws else 0
    L.check(L.lib().krs_gemm_set_option(0, c.pipe), "krs_gemm_set_option")
    try:
        return D.plan_gemm_route(addr("a", es_in), lda, a_km, addr("b", es_in), ldb, b_nk, addr("c", es_out), ldc, c.m, c.n,
                                 c.k, L.F32 if c.idt == "f32" else L.BF16, L.F32 if c.odt == "f32" else L.BF16, ep, ws)
    finally:
        L.lib().krs_gemm_set_option(0, 4)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_planner_gives_every_case_its_expected_route(lib, case):
    assert _planned(lib, case) == (0, case.route)


def test_the_planner_refuses_a_split_product_without_its_workspace_and_leaves_no_record(lib):
    from keras_rs_amd import dense_ops as D

    case = next(c for c in CASES if c.name == "ring-split-64k-vec8")
    assert (case.layout, case.idt, case.m, case.n, case.k) == ("nt", "bf16", 1032, 520, 2112)
    before = D.last_gemm_route()
    status, route = _planned(lib, case, ws=0)
    assert status != 0 and route == R(None)
    assert b"workspace" in lib.lib().krs_last_error()
    assert D.last_gemm_route() == before          # (the query does not touch the record of the last call)
    # the two findings of the planner's first reading, at their shapes: the short last split and the undersized query
    assert _planned(lib, next(c for c in CASES if c.name == "pp256k-split-short-last"))[1]["splits"] == 8
    assert lib.lib().krs_gemm_workspace_bytes(2056, 1032, 6144, 0) == 6 * 2056 * 1032 * 4


def _cross_bwd_planned(L, m, n, k, pipe, lda_pad=0, ldb_pad=0, misalign=False, dense=True, store_g=True):
    """(route, epilogue) krs_gemm_cross_bwd_plan_route gives the bf16 call tests/test_dense_bwd_fusion_gpu.py makes"""
    from keras_rs_amd import dense_ops as D

    base, ep = 0x100000, C.c_int(-1)
    L.check(L.lib().krs_gemm_set_option(0, pipe), "krs_gemm_set_option")
    try:
        route = L.lib().krs_gemm_cross_bwd_plan_route(
            base + (2 if misalign else 0), k + lda_pad, base, k + ldb_pad, None if dense else base, n, 1.0,
            base if store_g else None, n, None if dense else base, base, base, None if dense else base, n, 0, None, m, n, k,
            L.BF16, C.byref(ep))
    finally:
        L.lib().krs_gemm_set_option(0, 4)
    return D.CROSS_BWD_ROUTES[route], ep.value


def test_the_cross_backward_planner_fuses_exactly_the_shapes_the_gpu_test_expects(lib):
    from tests.test_dense_bwd_fusion_gpu import SHAPES, _aligned, _expected_route

    for name, (m, n, k, lda_pad, ldb_pad, mis) in SHAPES.items():
        for pipe in (0, 4, 5):
            want = _expected_route(m, n, k, pipe, _aligned(m, n, k, lda_pad, ldb_pad, mis))
            for store_g in (True, False):
                got = _cross_bwd_planned(lib, m, n, k, pipe, lda_pad, ldb_pad, mis, store_g=store_g)
                assert got == (want, (10 if store_g else 9) if want != "two_call" else 0), (name, pipe, store_g)
    # the cross form (x0, R): epilogue 3 on the C3 shape, two-call below 192 tiles
    assert _cross_bwd_planned(lib, 16384, 768, 256, 4, dense=False) == ("pp64", 3)
    assert _cross_bwd_planned(lib, 16384, 768, 256, 5, dense=False) == ("pp256", 3)
    assert _cross_bwd_planned(lib, 191 * 256, 256, 256, 4, dense=False) == ("two_call", 0)
    assert _cross_bwd_planned(lib, 0, 256, 256, 4) == (None, 0)


# ---- the planner's invariants, walked by a stand-alone program under the sanitizers ------------------------------------

def test_the_planner_keeps_its_invariants_over_the_lattice_under_the_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gemm_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "gemm_plan_check.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "0 failed checks" in run.stdout
