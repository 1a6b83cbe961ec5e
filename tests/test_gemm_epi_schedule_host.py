"""The epilogue schedules of gemm_pp64_kernel (krs_gemm_set_option(KRS_GEMM_OPT_EPI_SCHEDULE, v)), checked without a GPU:
what krs_gemm_plan_route reports for the calls tests/test_gemm_epi_schedule_gpu.py makes, that the option never moves a
product to another kernel, and the planner's promises about the schedules walked by a stand-alone program under the
sanitizers (tests/host/gemm_epi_schedule_check.cpp)."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 0x100000

# (M, N, K) of the GPU test's ring cases: the smallest M that puts the cross build on the unsplit ring at N = 3456 is 14 x 14
# tiles, the smallest K is 256 (gplan::kRingMinK; K = 192, three 64-k blocks, stays on the 128 x 128 kernels)
SHAPES = [(3584, 3456, 256), (3500, 3456, 512), (3584, 3464, 512), (3500, 3464, 256)]


@pytest.fixture(scope="module")
def lib():
    from keras_rs_amd import _lib as L
    from keras_rs_amd.build import build

    build()
    yield L
    L.lib().krs_gemm_set_option(L.GEMM_OPT_EPI_SCHEDULE, -1)
    L.lib().krs_gemm_set_option(L.GEMM_OPT_PIPELINE, 4)


def _epilogue(L, n, form, x_is_x0=False):
    ep = L.GemmEpilogue()
    if form == "cross":
        ep.x0, ep.x, ep.ldx = BASE, BASE if x_is_x0 else BASE + 0x1000, n
        ep.bias, ep.u_out, ep.ldu = BASE, BASE, n
    elif form == "res":
        ep.r, ep.ldr, ep.beta = BASE, n, 1.0
    return ep


def _plan(L, m, n, k, form, sched, x_is_x0=False, pipe=4):
    from keras_rs_amd import dense_ops as D

    L.check(L.lib().krs_gemm_set_option(L.GEMM_OPT_PIPELINE, pipe), "krs_gemm_set_option")
    L.check(L.lib().krs_gemm_set_option(L.GEMM_OPT_EPI_SCHEDULE, sched), "krs_gemm_set_option")
    try:
        args = (BASE, k, False, BASE, k, True, BASE, n, m, n, k, L.BF16, L.BF16,
                _epilogue(L, n, form, x_is_x0) if form != "plain" else None, 0)
        status, route = D.plan_gemm_route(*args)
        return status, route, D.plan_gemm_schedule(*args)
    finally:
        L.lib().krs_gemm_set_option(L.GEMM_OPT_EPI_SCHEDULE, -1)
        L.lib().krs_gemm_set_option(L.GEMM_OPT_PIPELINE, 4)


def test_the_smallest_ring_shape_is_fourteen_by_fourteen_tiles(lib):
    assert _plan(lib, 3584, 3456, 256, "cross", 0)[1]["kernel"] == "pp64"
    assert _plan(lib, 3584 - 256, 3456, 256, "cross", 0)[1]["kernel"] != "pp64"
    # K = 192 is three 64-k blocks, which the ring's loop can run, but the planner keeps K < 256 on the 128 x 128 kernels:
    # the GPU test's K = 192 cases run there, under every schedule option, and name no schedule
    for sched in (0, 1, 2, 3):
        status, route, schedule = _plan(lib, 3584, 3456, 192, "cross", sched)
        assert (status, route["kernel"], route["epilogue"], schedule) == (0, "mfma", 1, set())


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_each_option_value_names_its_schedule_and_moves_no_product(lib, m, n, k):
    want = {
        ("cross", False): {0: set(), 1: {"lds_landing"}, 2: {"stagger"}, 3: {"lds_landing", "stagger"}},
        ("cross", True): {0: set(), 1: {"x_is_x0"}, 2: {"stagger"}, 3: {"x_is_x0", "stagger"}},
        ("res", False): {0: set(), 1: set(), 2: {"stagger"}, 3: {"stagger"}},
        ("plain", False): {0: set(), 1: set(), 2: set(), 3: set()},
    }
    for (form, same), by_option in want.items():
        status0, route0, _ = _plan(lib, m, n, k, form, 0, same)
        assert status0 == 0 and route0["kernel"] == "pp64" and route0["splits"] == 1
        assert route0["epilogue"] == {"cross": 1, "res": 2, "plain": 0}[form]
        for sched, names in by_option.items():
            status, route, schedule = _plan(lib, m, n, k, form, sched, same)
            assert (status, route) == (0, route0), (form, same, sched)
            assert schedule == names, (form, same, sched)


def test_off_the_64k_ring_the_option_names_nothing(lib):
    for pipe, kernel in ((5, "pp256"), (0, "mfma")):
        for sched in (0, 1, 2, 3):
            for same in (False, True):
                status, route, schedule = _plan(lib, 3584, 3456, 512, "cross", sched, same, pipe=pipe)
                assert status == 0 and route["kernel"] == kernel and route["epilogue"] == 1 and schedule == set()
    # fewer than 192 tiles: the 128 x 128 kernels
    assert _plan(lib, 2048, 3456, 512, "cross", 3)[2] == set()


def test_the_option_refuses_values_it_does_not_know(lib):
    assert lib.lib().krs_gemm_set_option(lib.GEMM_OPT_EPI_SCHEDULE, 4) != 0
    assert lib.lib().krs_gemm_set_option(lib.GEMM_OPT_EPI_SCHEDULE, -2) != 0
    assert lib.lib().krs_gemm_set_option(2, 0) != 0
    assert lib.lib().krs_gemm_set_option(lib.GEMM_OPT_EPI_SCHEDULE, -1) == 0      # (-1: back to the default)


def test_the_planner_keeps_its_schedule_invariants_under_the_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gemm_epi_schedule_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "gemm_epi_schedule_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "0 failed checks" in run.stdout
