"""The K8 route table (tests/retrieval_cases.py), checked without a GPU.  Every expected krs_retrieval_route record is
asserted against the planner (keras_rs_amd/csrc/retrieval_plan.h through krs_retrieval_plan_route, which launches
nothing); the table names every (ES, VEC) build of retr_stage1_kernel, every selection route that a source of pairs can
reach and a multi-chunk slab run -- enumerated here, so a case dropped from it fails, not silently; refusals return their
status and an all-zero record; and the planner's invariants are walked by a stand-alone program built with the sanitizers
(tests/host/retrieval_plan_check.cpp).  tests/test_retrieval_matrix_gpu.py asserts the same records against what ran."""

import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest
import torch

from tests.retrieval_cases import CASES, DTYPES, ELEM_D, FIELDS, R, VEC_D, inputs
from tests.retrieval_restatement import TORCH_DTYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
BASE = 0x7F0000100000          # a 16-byte aligned stand-in for a device address


def _have(pred=lambda c: True, **want):
    """the cases whose fields / route fields equal `want` and that satisfy `pred`"""
    def ok(c):
        return all((getattr(c, k) if hasattr(c, k) else c.route[k]) == v for k, v in want.items()) and pred(c)
    return [c for c in CASES if ok(c)]


def test_the_table_is_well_formed():
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        assert set(c.route) == set(FIELDS), c.name
        assert c.b * c.n * 8 <= 40 << 20 and c.n * max(c.d, 1) * 4 <= 4 << 20, c.name        # a fraction of a second each
        assert (c.entry == "rows") == (c.route["kernel"] == "rows") and 1 <= c.k <= c.n, c.name
        assert c.layout == "plain" or c.route["vec"] == 0, c.name
    for name in (CASES[0].name, _have(group="special")[0].name, _have(group="rows", data="bucket")[0].name):
        again = inputs.__wrapped__(name)
        for key, value in inputs(name).items():
            assert value is None or (value.tobytes() == again[key].tobytes()), (name, key)       # seeded by the name


def test_every_build_route_and_chunking_is_expected_somewhere():
    # retr_stage1_kernel<ES, VEC>: 4 builds, every width of the plan, with random normal data too
    for dt in DTYPES:
        assert {c.d for c in _have(group="build", dtype=dt, vec=1)} == set(VEC_D[dt])
        assert {c.d for c in _have(group="build", dtype=dt, vec=0, layout="plain")} == set(ELEM_D[dt])
        # element loads by layout at a VEC width: a misaligned base with an odd stride, an aligned base with an odd stride
        for lay in ("col_slice", "odd_stride"):
            lost = _have(group="build", dtype=dt, vec=0, layout=lay)
            assert lost and all(_have(group="build", dtype=dt, vec=1, d=c.d, layout="plain") for c in lost)
        for vec in (0, 1):
            assert _have(group="normal", dtype=dt, vec=vec, kernel="fused")
    assert _have(group="build", ids="signed")
    # the selection routes: stage 1's lists (PairSrc) carry k <= 128 pairs per slice, so their merge never sorts more than
    # 128 slots per row and the global merge is a route of matrix rows (MatSrc) alone
    assert {c.route["select"] for c in _have(kernel="fused")} == {"lds", "radix"}
    assert {c.route["select"] for c in _have(kernel="slab")} == {"lds", "radix"}
    assert {c.route["select"] for c in _have(kernel="rows")} == {"lds", "radix", "radix_merge"}
    assert {c.route["select_p"] for c in _have(select="radix_merge")} == {4096, 8192}
    # both sides of 2048 pairs, from both sources
    assert {c.route["select_len"] for c in _have(kernel="fused", group="merge")} >= {2040, 2048, 2064, 80}
    assert {c.n for c in _have(kernel="rows")} >= {2048, 2049}
    # stage-1 order: every residue of (k - 1) & 3, a full queue at k = 128, every pattern in both dtypes
    for dt, data in itertools.product(DTYPES, ("ramp", "saw", "late")):
        ks = {c.k for c in _have(group="order", dtype=dt, data=data, S=8)}
        assert ks == {1, 2, 3, 5, 64, 127, 128} and {(k - 1) & 3 for k in ks} == {0, 1, 2, 3}
    # NaN and infinities through the four routes, fewer and more NaN candidates than k
    for dt in DTYPES:
        sp = _have(group="special", dtype=dt)
        assert {(c.route["kernel"], c.route["select"], c.d > 512) for c in sp} == {
            ("fused", "lds", False), ("fused", "radix", False), ("slab", "lds", False), ("slab", "lds", True)}
        for c in sp:
            assert [o for o in sp if (o.n, o.d, o.k) == (c.n, c.d, c.k) and (o.nan < o.k) != (c.nan < c.k)], c.name
    # the chunk loop: once, three times with a short tail, once per row
    for dt in DTYPES:
        assert {(c.route["chunks"], c.route["chunk_rows"]) for c in _have(group="chunks", dtype=dt)} == {(1, 70), (3, 32), (70, 1)}
    # the row selection: all keys equal with k across the bucket edges, and a bucket taken whole at the first digit
    assert {c.k for c in _have(group="rows", data="equal")} == {1, 255, 256, 257, 2048, 4999, 5000}
    assert _have(group="rows", data="bucket", select="radix")


# ---- the table against the planner -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    from keras_rs_amd import retrieval_ops
    from keras_rs_amd.build import build

    build()
    return retrieval_ops


def _planned(ops, c):
    """the plan of the call tests/test_retrieval_matrix_gpu.py makes for case c, on stand-in addresses"""
    dtype = TORCH_DTYPES[c.dtype]
    if c.entry == "rows":
        return ops.plan_route("rows", c.b, c.n, 0, c.k, dtype, c=BASE)
    return ops.plan_route("topk", c.b, c.n, c.d, c.k, dtype, ldq=c.ld, ldc=c.ld, q=BASE + (1 << 32) + c.base_offset,
                          c=BASE + c.base_offset)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_planner_gives_every_case_its_expected_route(ops, case, monkeypatch):
    monkeypatch.delenv("KRS_RETRIEVAL_SLAB_BYTES", raising=False)
    if case.budget:
        monkeypatch.setenv("KRS_RETRIEVAL_SLAB_BYTES", str(case.budget))
    assert _planned(ops, case) == (0, case.route)


def test_the_slab_budget_is_read_on_each_call_and_sizes_the_workspace(ops, monkeypatch):
    b, n, d, k = 70, 3000, 16, 200
    monkeypatch.delenv("KRS_RETRIEVAL_SLAB_BYTES", raising=False)
    whole = ops.retrieval_topk_workspace_bytes(b, n, d, k, torch.float32)
    assert whole >= b * n * 4 + b * 256 * 8
    monkeypatch.setenv("KRS_RETRIEVAL_SLAB_BYTES", "450000")
    small = ops.retrieval_topk_workspace_bytes(b, n, d, k, torch.float32)
    assert 32 * n * 4 + 32 * 256 * 8 <= small <= 450000 + 512 < whole
    assert ops.plan_route("topk", b, n, d, k, torch.float32)[1]["chunks"] == 3
    # the budget is the two-step path's: the fused path and the row selection do not read it
    assert ops.plan_route("topk", b, n, d, 100, torch.float32)[1]["chunks"] == 0
    for junk in ("0", "-5", "12x", ""):                # not a positive integer: the default of 1 GiB stands
        monkeypatch.setenv("KRS_RETRIEVAL_SLAB_BYTES", junk)
        assert ops.retrieval_topk_workspace_bytes(b, n, d, k, torch.float32) == whole
    monkeypatch.delenv("KRS_RETRIEVAL_SLAB_BYTES")
    assert ops.retrieval_topk_workspace_bytes(b, n, d, k, torch.float32) == whole


def test_variants_and_the_workspace_queries_answer_from_one_plan(ops):
    from keras_rs_amd import _lib as L

    lists = 33 * 8 * 10 * 8
    st, rt = ops.plan_route("q8", 33, 255, 100, 10, torch.float32)
    assert st == 0 and (rt["kernel"], rt["variant"], rt["es"], rt["vec"], rt["row_bytes"]) == ("fused", "q8", 1, 0, 128)
    assert rt["lds_bytes"] == 32 * (128 + 16) + 65536 + 256 + 128                      # + the query steps
    assert ops.retrieval_topk_q8_workspace_bytes(33, 255, 100, 10) == -(-lists // 256) * 256 + -(-33 * 128 // 256) * 256 + 256
    assert ops.plan_route("q8", 33, 255, 128, 10, torch.bfloat16)[1]["vec"] == 1
    assert ops.plan_route("q8", 33, 255, 128, 10, torch.bfloat16, c=BASE + 1)[1]["vec"] == 0
    st, rt = ops.plan_route("mine", 33, 255, 64, 10, torch.bfloat16)
    assert st == 0 and (rt["kernel"], rt["variant"], rt["es"], rt["vec"], rt["row_bytes"]) == ("fused", "mine", 2, 1, 128)
    assert rt["lds_bytes"] == 32 * (128 + 16) + 65536 + 256 + 256 + 128                # + the positives' ids, the positives
    assert ops.retrieval_mine_workspace_bytes(33, 255, 64, 10, torch.bfloat16) == -(-lists // 256) * 256
    assert ops.retrieval_topk_workspace_bytes(33, 255, 64, 10, torch.bfloat16) == -(-lists // 256) * 256
    assert L.lib().krs_retrieval_last_route(None) in (0, 1, 2, 3)


def test_refusals_return_their_status_and_no_record(ops):
    from keras_rs_amd import _lib as L

    lib = L.lib()
    ok = dict(variant=1, q=BASE, ldq=64, c=BASE + (1 << 32), ldc=64, dtype=L.F32, b=33, n=255, d=64, k=10)

    def plan(**change):
        rt = L.RetrievalRoute(kernel=9, blocks=9)
        rc = lib.krs_retrieval_plan_route(*{**ok, **change}.values(), C.byref(rt))
        return rc, ops._route_dict(rt)

    before = ops.last_route()
    rc, rt = plan()
    assert rc == 0 and rt["kernel"] == "fused" and C.sizeof(L.RetrievalRoute) == 88
    assert ops.last_route() == before                     # (the query does not touch the record of the last call)
    assert lib.krs_retrieval_plan_route(*ok.values(), None) == 0          # (the record is optional)
    for what, change in (("null q", dict(q=None)), ("null c", dict(c=None)), ("negative b", dict(b=-1)), ("n 0", dict(n=0)),
                         ("d 0", dict(d=0)), ("k 0", dict(k=0)), ("k above n", dict(k=256)), ("ldc below d", dict(ldc=63)),
                         ("ldq below d", dict(ldq=63)), ("bad dtype", dict(dtype=L.I8)), ("bad variant", dict(variant=7)),
                         ("no variant", dict(variant=0)), ("mine: k = n", dict(variant=3, k=255)),
                         ("mine: no slab path", dict(variant=3, k=129)), ("rows: ld below cols", dict(variant=4, ldc=254))):
        assert plan(**change) == (INVALID, R()), what
        assert lib.krs_last_error(), what
    for what, change in (("q8: k above 128", dict(variant=2, k=129)), ("q8: d above 512", dict(variant=2, d=513, ldq=513, ldc=513))):
        assert plan(**change) == (UNSUPPORTED, R()), what
    # a grid past 32 bits is refused, not truncated: 2^31 - 1 rows of 8192 list slots are 2^33 sort blocks
    big = (1 << 31) - 1
    assert plan(variant=4, b=big, n=big, ldc=big, k=4097) == (UNSUPPORTED, R())
    # no query rows: a success that launches nothing, whatever the pointers
    assert plan(b=0) == (0, R()) and plan(b=0, q=None, c=None) == (0, R())
    # the entries themselves refuse before any launch and leave an all-zero record
    assert lib.krs_retrieval_topk(None, 64, None, 64, None, L.F32, 33, 255, 64, 10, None, None, None, 0, None) == INVALID
    assert ops.last_route() == R() and lib.krs_retrieval_last_route(None) == 0
    assert lib.krs_retrieval_topk(BASE, 64, BASE, 64, None, L.F32, 33, 255, 64, 10, None, BASE, None, 0, None) == WORKSPACE
    assert ops.last_route() == R()
    assert lib.krs_retrieval_topk(None, 64, None, 64, None, L.F32, 0, 255, 64, 10, None, None, None, 0, None) == 0
    assert lib.krs_topk_rows(None, None, 0.0, 100, L.F32, 0, 100, 5, None, None, None, 0, None) == 0
    assert lib.krs_topk_rows(None, None, 0.0, 100, L.F32, 3, 100, 5, None, None, None, 0, None) == INVALID
    assert lib.krs_retrieval_topk_q8(BASE, 64, L.F32, BASE, 64, BASE, None, 33, 255, 64, 129, None, L.F32, BASE, None, None, 0,
                                     None) == UNSUPPORTED
    assert lib.krs_retrieval_mine(BASE, 64, BASE, 64, L.F32, 33, 255, 64, 255, None, None, None, L.I32, 0.0, BASE, BASE, BASE,
                                  None, 0, None) == INVALID
    assert ops.last_route() == R()


# ---- the planner's invariants, walked by a stand-alone program under the sanitizers ------------------------------------

def test_the_planner_header_compiles_without_hip_and_keeps_its_invariants_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tests/host/retrieval_plan_check.cpp")
    exe = str(tmp_path / "retrieval_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "retrieval_plan_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last.endswith(" 0 failed checks") and int(last.split()[0]) > 10000, last
