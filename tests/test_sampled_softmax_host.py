"""K30 without a GPU: the host planner (csrc/sampled_softmax_plan.h) through tests/host/sampled_softmax_plan_check.cpp
under the sanitizers, and krs_sampled_softmax_plan_route's answers: the route, DPAD and VEC of the GPU test's case table
and every refusal include/krs.h (K30) lists."""

import ctypes as C
import os
import shutil
import subprocess

import pytest

from keras_rs_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1 << 20        # an address on 16 bytes; A + 4 is not


def test_the_planner_keeps_its_invariants_over_the_grid_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tests/host/sampled_softmax_plan_check.cpp")
    exe = str(tmp_path / "sampled_softmax_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "sampled_softmax_plan_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "0 failed checks", run.stdout[-4000:] + run.stderr[-4000:]
    one = subprocess.run([exe, "387", "3", "100", "64", "1", "0", "1"], capture_output=True, text=True)
    assert one.stdout.splitlines()[0].split()[:9] == ["0", "1", "64", "1", "6", "15", "5", "1", "4"]


def plan(d=64, edt=L.BF16, tdt=L.F32, t=387, g=3, n=100, emb=A, table=A, lde=None, ldt=None, ldd=None, weight=None,
         pq=None, nq=None, itype=L.I32, neg=A, dneg=A):
    route = L.SampledSoftmaxRoute()
    rc = L.lib().krs_sampled_softmax_plan_route(emb, d if lde is None else lde, edt, table, d if ldt is None else ldt, tdt,
                                                1000, A, neg, itype, weight, pq, nq, t, g, n, d, 1, A, A, A,
                                                d if ldd is None else ldd, dneg, C.byref(route))
    return rc, route


# d, emb dtype, table dtype, overrides -> kernel, dpad, vec (the builds tests/test_sampled_softmax_gpu.py claims)
CASES = [
    (8, L.BF16, L.BF16, {}, (L.SSM_FAST, 32, 1)),
    (50, L.BF16, L.F32, {}, (L.SSM_FAST, 64, 0)),
    (64, L.BF16, L.F32, {}, (L.SSM_FAST, 64, 1)),
    (64, L.BF16, L.F32, {"table": A + 8}, (L.SSM_FAST, 64, 0)),
    (64, L.BF16, L.BF16, {"lde": 68}, (L.SSM_FAST, 64, 0)),
    (64, L.BF16, L.F32, {"ldt": 68}, (L.SSM_FAST, 64, 1)),           # 272-byte fp32 rows
    (100, L.BF16, L.F32, {}, (L.SSM_FAST, 128, 0)),
    (128, L.BF16, L.BF16, {"weight": A}, (L.SSM_FAST, 128, 1)),
    (129, L.BF16, L.BF16, {}, (L.SSM_GENERIC, 0, 0)),
    (50, L.F32, L.F32, {}, (L.SSM_GENERIC, 0, 0)),
    (200, L.F32, L.BF16, {}, (L.SSM_GENERIC, 0, 0)),
    (512, L.BF16, L.F32, {}, (L.SSM_GENERIC, 0, 0)),
]


@pytest.mark.parametrize("d,edt,tdt,over,want", CASES)
def test_plan_route_answers_the_claimed_build(d, edt, tdt, over, want):
    rc, r = plan(d, edt, tdt, **over)
    fast = want[0] == L.SSM_FAST
    assert rc == 0 and (r.kernel, r.dpad, r.vec) == want
    assert (r.grid_tokens, r.splits, r.split_tiles) == ((6, 5, 1) if fast else (387, 1, 5))
    assert r.grid_negs == (15 if fast else 300) and r.launches == int("weight" in over) + 3 + int(fast)
    size = L.lib().krs_sampled_softmax_workspace_bytes(387, 3, 100, d, edt)
    assert size == 4 * ((64 + 387 + r.grid_tokens + 63) // 64 * 64 + (5 * 300 * d if fast else 0))


@pytest.mark.parametrize("over,names", [({"n": 0}, "1 <= n <= 4096"), ({"n": 4097}, "1 <= n <= 4096"), ({"d": 0}, "1 <= d <= 512"),
                                        ({"d": 513}, "1 <= d <= 512"), ({"t": 388}, "t % g == 0"), ({"g": 0}, "g >= 1"),
                                        ({"t": 2 ** 31, "g": 1}, "t <= 2^31 - 1"),
                                        ({"t": 2 ** 20, "g": 2 ** 20, "n": 4096}, "g * n <= 2^31 - 1"),
                                        ({"pq": A}, "both or neither"), ({"nq": A}, "both or neither"), ({"edt": 2}, "emb dtype"),
                                        ({"tdt": 2}, "table dtype"), ({"itype": 7}, "id type"), ({"lde": 63}, "ld_emb >= d"),
                                        ({"ldt": 63}, "ld_table >= d"), ({"ldd": 63}, "ld_demb >= d"), ({"neg": None}, "non-null"),
                                        ({"dneg": None}, "non-null")])
def test_plan_refusals_name_the_limit(over, names):
    rc, r = plan(**over)
    assert rc == -1 and not any(getattr(r, f) for f, _ in r._fields_)
    assert names.encode() in L.lib().krs_last_error()
