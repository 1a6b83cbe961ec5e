"""The krs_embed_bag_fwd route table (tests/embed_fwd_cases.py), checked without a GPU.  Every expected route record is
asserted against the planner (keras_rs_amd/csrc/embed_fwd_plan.h through krs_embed_bag_fwd_plan_route, which launches
nothing); the table names every kernel instantiation of keras_rs_amd/csrc/embed_bag_fwd.hip -- enumerated here, so a case
dropped from it fails, not silently; the planner's refusals return their status and no record; the float64 reference's
own fp32 evaluation stays inside the bound the GPU test holds the kernels to; and the planner's invariants are walked by
a stand-alone program built with the sanitizers (tests/host/embed_fwd_plan_check.cpp).
tests/test_embed_fwd_matrix_gpu.py asserts the same records against what ran."""

import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import embed_fwd_restatement as RS
from tests.embed_fwd_cases import BAD32, BAD64, CASES, DIMS, ES, GENERIC_DIMS, LPRS, PAIRS, R, inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1


def _have(pred=lambda c: True, **want):
    """the cases whose fields / route fields equal `want` and that satisfy `pred`"""
    def ok(c):
        return all((getattr(c, k) if hasattr(c, k) and k != "route" else c.route[k]) == v for k, v in want.items()) and pred(c)
    return [c for c in CASES if ok(c)]


def _n_vec(dt):
    return 16 // ES[dt]


def _slot_offsets(c):
    """byte offset of every feature slot of a case's output rows from a 16-byte boundary"""
    return {((c.base_off + col) * ES[c.odt]) % 16 for col in c.out_cols}


def test_the_table_is_well_formed():
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        assert set(c.route) == set(R(None)), c.name
        assert c.batch <= 200 and max(c.vocabs) <= 300 and (c.n_feats <= 4 or "features" in c.name), c.name
        assert c.lead >= 1 and c.tail >= 1 and (c.gap >= 1 or "features" in c.name), c.name      # sentinel columns
        assert c.width * c.batch * 4 <= 4 << 20, c.name                                          # a few MB at the most
        if c.bad:
            assert set(c.bad) in (set(BAD32), set(BAD64)) and (c.id64 or set(c.bad) == set(BAD32)), c.name
    assert sorted(c.n_feats for c in CASES if c.n_feats > 4) == [128, 128, 129]


def test_every_instantiation_of_the_pooled_kernel_is_expected_somewhere():
    # embed_bag_fwd_vec<TT, OT, LPR, HAS_W, STREAM>: 4 x 4 x 2 x 2 = 64, each in the dense or the CSR form
    missing = [(p, lpr, w, s) for p, lpr, w, s in itertools.product(PAIRS, LPRS, (False, True), (False, True))
               if not _have(kernel="vec", tdt=p[0], odt=p[1], lpr=lpr, has_w=w, stream=s, hot_rows=0, hot_opt=0)]
    assert missing == []
    # ... and the four HR builds (bf16 / bf16, LPR 16, unweighted), dense and CSR, with all three combiners
    for hr, s, csr in itertools.product((64, 128), (False, True), (False, True)):
        got = _have(lambda c: c.csr == csr, kernel="vec", hot_rows=hr, stream=s, tdt="bf16", odt="bf16", lpr=16, has_w=False)
        assert got and all({k for _, k in c.feats} == {RS.SUM, RS.MEAN, RS.SQRTN} for c in got), (hr, s, csr)
    assert {c.hot_opt for c in CASES} == {0, 64, 128}                      # every value of the option
    assert len(_have(lambda c: c.hot_opt and not c.route["hot_rows"])) >= 3     # ... also where the gate refuses it
    assert [c for c in _have(kernel="vec") if min(c.vocabs[t] for t, _ in c.feats) < 64 and c.route["hot_rows"]]
    # both forms, the three combiners within one call, per dtype pair; the dense (1, 1, 1) stream with weights
    for p in PAIRS:
        for csr in (False, True):
            assert _have(lambda c: c.csr == csr and {k for _, k in c.feats} == {RS.SUM, RS.MEAN, RS.SQRTN}, kernel="vec",
                         tdt=p[0], odt=p[1]), (p, csr)
    assert _have(lambda c: c.hots == (1, 1, 1) and c.weights, kernel="vec", stream=True)
    for c in _have(lambda c: c.csr, kernel="vec", stream=True, hot_opt=0):
        assert set(c.lens) <= {0, 1, 2} and c.nnz < 2 * len(c.lens), c.name
    # one dim with idle lanes and one that fills the group, per table dtype and LPR
    for tdt, lpr in itertools.product(("f32", "bf16"), LPRS):
        idle, full = DIMS[tdt][lpr]
        assert idle * ES[tdt] % 16 == 0 and (lpr // 2 if lpr > 8 else 0) < idle * ES[tdt] // 16 < lpr, (tdt, lpr)
        assert full * ES[tdt] == 16 * lpr and _have(kernel="vec", tdt=tdt, dim=idle) and _have(kernel="vec", tdt=tdt, dim=full)
    assert _have(kernel="vec", tdt="f32", dim=12) and _have(kernel="vec", tdt="f32", dim=20)
    # store_row_piece's element-store branch per output type and piece width: slots, and the output base, off their vector
    for p in PAIRS:
        got = _have(kernel="vec", tdt=p[0], odt=p[1])
        assert [c for c in got if c.base_off == 0 and _slot_offsets(c) - {0}] and [c for c in got if c.base_off == 1], p
        assert [c for c in got if _slot_offsets(c) == {0}], p


def test_every_instantiation_of_the_gather_and_generic_kernels_is_expected_somewhere():
    # embed_gather_hot1<TT, OT, LPR, 16>: 16; reached by the dtype pair, by 129 features, by an unaligned output
    assert [(p, lpr) for p, lpr in itertools.product(PAIRS, LPRS)
            if not _have(kernel="hot1", tdt=p[0], odt=p[1], lpr=lpr)] == []
    assert _have(lambda c: c.n_feats == 129, kernel="hot1", tdt="f32", odt="f32", dim=4)
    for dt in ("f32", "bf16"):
        assert _have(lambda c: c.base_off == 1, kernel="hot1", tdt=dt, odt=dt)
        assert _have(lambda c: c.base_off == 0 and c.width * ES[dt] % 16, kernel="hot1", tdt=dt, odt=dt)
    for p in PAIRS:      # aligned and unaligned stores per pair, the three batch sizes, the slow loop
        assert {bool(_slot_offsets(c) - {0}) for c in _have(kernel="hot1", tdt=p[0], odt=p[1])} >= (
            {True, False} if p[0] != p[1] else {True}), p
        assert {c.batch for c in _have(kernel="hot1", tdt=p[0], odt=p[1])} >= {1, 64, 70}, p
        assert _have(lambda c: any(h != 1 for h in c.hots), kernel="hot1", tdt=p[0], odt=p[1]), p
    # embed_gather_hot1_rows<TT, LPR, 16>: 8; aligned slots, slots off by 1 and by N - 1 elements
    for dt, lpr in itertools.product(("f32", "bf16"), LPRS):
        got = _have(kernel="hot1_rows", tdt=dt, odt=dt, lpr=lpr)
        assert [c for c in got if _slot_offsets(c) == {0}], (dt, lpr)
        assert [c for c in got if {ES[dt], (_n_vec(dt) - 1) * ES[dt]} <= _slot_offsets(c)], (dt, lpr)
    for dt in ("f32", "bf16"):
        got = _have(kernel="hot1_rows", tdt=dt)
        assert [c for c in got if c.id64] and [c for c in got if not c.id64]
        assert [c for c in got if sorted(c.hots) == [0, 1, 2] and {k for _, k in c.feats} >= {RS.MEAN, RS.SQRTN}]
        assert [c for c in got if c.batch * c.n_feats % 64] and [c for c in got if c.n_feats == 128]
    # embed_bag_fwd_generic: the dims of the issue, four pairs, dense and CSR
    for p, csr in itertools.product(PAIRS, (False, True)):
        assert {c.dim for c in _have(lambda c: c.csr == csr, kernel="generic", tdt=p[0], odt=p[1])} >= set(GENERIC_DIMS[p[0]])
    assert {c.route["kernel"] for c in CASES} == {"vec", "hot1", "hot1_rows", "generic"}
    # the dtype pair and the LPR of the gather kernels that the earlier tests never ran
    assert {c.route["lpr"] for c in _have(kernel="hot1")} == {c.route["lpr"] for c in _have(kernel="hot1_rows")} == set(LPRS)
    # fp32 -> bf16 and bf16 -> fp32 gathers carry the special values (inf, subnormals, ties, NaN)
    assert _have(kernel="hot1", tdt="f32", odt="bf16", specials=True) and _have(kernel="hot1", tdt="bf16", odt="f32", specials=True)


def test_ids_offsets_bags_per_group_and_windows_are_pinned():
    for k in ("vec", "hot1", "hot1_rows", "generic"):      # per kernel family: both id types, each with its invalid ids
        assert _have(kernel=k, id64=False, bad=BAD32) and _have(kernel=k, id64=True, bad=BAD64), k
    for k in ("vec", "generic"):                            # ... and both offset types; half of the CSR cases use int64
        assert _have(lambda c: c.csr, kernel=k, off64=True) and _have(lambda c: c.csr, kernel=k, off64=False), k
    csr = [c for c in CASES if c.csr]
    assert 0.35 <= sum(c.off64 for c in csr) / len(csr) <= 0.65
    assert _have(kernel="vec", stream=True, id64=True, bad=BAD64) and _have(kernel="vec", stream=False, id64=True, bad=BAD64)
    # every case with an invalid id sits on poisoned tables; a few cases look row 0 up for real
    assert all(c.poison for c in CASES if c.bad) and {c.route["kernel"] for c in CASES if not c.poison} == {
        "vec", "hot1", "hot1_rows"}
    # bags per group at mean lengths 1, 2, 3, 5, 9, 40: batch 1, one whole wave of groups, one bag more
    for mean, bpg in ((1, 16), (2, 16), (3, 10), (5, 6), (9, 3), (40, 1)):
        got = _have(lambda c: c.name.startswith(f"bpg{bpg}-mean{mean}-"), kernel="vec", bpg=bpg)
        assert all(c.nnz // (c.n_feats * c.batch) == mean for c in got)
        wave = {(64 // c.route["lpr"]) * bpg for c in got}
        assert len(wave) == 1 and {c.batch for c in got} == {1, min(wave), min(wave) + 1}, (mean, bpg)
    # a group's stream of WIN - 1, WIN, WIN + 1 lookups at LPR 8 and LPR 64, mean with weights
    for lpr in (8, 64):
        got = _have(lambda c: c.name.startswith("window-lpr"), kernel="vec", lpr=lpr, bpg=1, batch=3)
        assert {c.hots[0] for c in got} == {8 * lpr - 1, 8 * lpr, 8 * lpr + 1}
        assert all(c.weights == "uniform" and (0, RS.MEAN) in c.feats for c in got)
    for c in _have(lambda c: c.name.startswith("window-csr-edges")):
        win, bpg, off = 8 * c.route["lpr"], c.route["bpg"], np.concatenate([[0], np.cumsum(c.lens[:c.route["bpg"]])])
        assert bpg == 6 and c.weights and (0, RS.MEAN) in c.feats
        ends_on_last = [b for b in range(bpg) if c.lens[b] and off[b + 1] % win == 0]
        assert ends_on_last and c.lens[ends_on_last[0] + 1] == 0                       # ... followed by an empty bag
        assert off[ends_on_last[0] + 2] % win == 0 and c.lens[ends_on_last[0] + 2] > 0  # ... then one from slot 0
        assert any(c.lens[b] and (off[b + 1] - 1) // win - off[b] // win == 2 for b in range(bpg))   # three windows
        assert c.lens[bpg - 1] == 0                                                    # an empty last bag of the group
    assert len(_have(lambda c: c.name.startswith("window-csr-edges"))) >= 1
    assert _have(weights="pm_half", kernel="vec") and _have(weights="pm_half", kernel="generic")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_inputs_of_every_case_are_what_the_case_says(case):
    c, h = case, inputs(case.name)
    ids = h["ids"].astype(np.int64)
    assert h["ids"].dtype == (np.int64 if c.id64 else np.int32) and ids.shape[0] == c.nnz
    assert (h["offsets"] is None) == (not c.csr) and (h["weights"] is None) == (c.weights is None)
    if c.csr:
        assert h["offsets"].dtype == (np.int64 if c.off64 else np.int32) and h["offsets"][-1] == c.nnz
    start, end = RS.bag_bounds(c.n_feats, c.batch, c.hots, h["offsets"])
    vocab = np.repeat(np.array([c.vocabs[t] for t, _ in c.feats]).repeat(c.batch), end - start)
    valid = (ids >= 0) & (ids < vocab)
    planted = {"vocab" if v == vocab[i] else int(v) for i, v in enumerate(ids) if not valid[i]}
    assert planted == set(c.bad) and valid.any()
    for t, tab in enumerate(h["tables"]):
        assert tab.shape == (c.vocabs[t], c.dim) and tab.dtype == np.float32
        assert np.isnan(tab[0]).all() == c.poison and (c.specials or np.isfinite(tab[1:]).all())
    assert not c.poison or (ids[valid] != 0).all()
    if c.weights == "uniform":
        assert h["weights"].min() >= 0.25 and h["weights"].max() <= 1.0


# ---- the table against the planner -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from keras_rs_amd import _lib as L
    from keras_rs_amd.build import build

    build()
    yield L
    L.lib().krs_embed_set_option(3, 0)


def _dt(L, name):
    return L.F32 if name == "f32" else L.BF16


def _planned(L, c):
    """the plan of the call tests/test_embed_fwd_matrix_gpu.py makes for case c: a fake address per pointer (0x100000 for
    the output buffer plus the case's base offset; only nullness and alignment are read)"""
    from keras_rs_amd import embedding_ops as E

    L.check(L.lib().krs_embed_set_option(3, c.hot_opt), "krs_embed_set_option")
    try:
        return E.embed_fwd_plan_route(c.n_feats, 0x200000 if c.csr else None, 0x300000 if c.weights else None, c.nnz,
                                      c.batch, c.dim, _dt(L, c.tdt), 0x100000 + c.base_off * ES[c.odt], _dt(L, c.odt),
                                      c.width)
    finally:
        L.lib().krs_embed_set_option(3, 0)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_planner_gives_every_case_its_expected_route(lib, case):
    assert _planned(lib, case) == dict(case.route, status=0)


def test_block_counts_and_option_values_at_known_shapes(lib):
    from keras_rs_amd import embedding_ops as E

    def plan(n_feats, batch, dim, nnz, tdt=lib.BF16, odt=lib.BF16, offsets=None, weights=None, out=0x100000, ld=None):
        return E.embed_fwd_plan_route(n_feats, offsets, weights, nnz, batch, dim, tdt, out, odt, ld or n_feats * dim)

    # the one-hot headline shape: 26 features, batch 16384, bf16 dim 128 -> 6656 waves of 64 (sample, feature) units
    assert plan(26, 16384, 128, 26 * 16384) == dict(R("hot1_rows", "bf16", "bf16", 16, blocks=1664), status=0)
    assert plan(26, 16384, 128, 26 * 16384, out=0x100002)["kernel"] == "hot1"
    assert plan(26, 16384, 128, 26 * 16384, odt=lib.F32) == dict(R("hot1", "bf16", "f32", 16, blocks=1664), status=0)
    assert plan(129, 64, 128, 129 * 64)["kernel"] == "hot1" and plan(128, 64, 128, 128 * 64)["kernel"] == "hot1_rows"
    # pooled: mean 3 -> 10 bags per group, 4 groups per wave: ceil(100 / 40) = 3 waves x 2 features = 6 -> 2 workgroups
    assert plan(2, 100, 128, 600) == dict(R("vec", "bf16", "bf16", 16, bpg=10, blocks=2), status=0)
    assert plan(2, 100, 128, 600, weights=0x10)["has_w"] and plan(2, 100, 128, 399, offsets=0x10)["stream"]
    assert not plan(2, 100, 128, 400, offsets=0x10)["stream"]
    assert plan(2, 100, 6, 600, tdt=lib.F32, odt=lib.F32) == dict(R("generic", "f32", "f32", 8, blocks=7), status=0)
    assert plan(0, 100, 128, 0) == dict(R(None), status=0) and plan(2, 0, 128, 0) == dict(R(None), status=0)
    for value, want in ((0, 0), (64, 64), (128, 128)):
        lib.check(lib.lib().krs_embed_set_option(3, value), "krs_embed_set_option")
        try:
            assert plan(2, 100, 128, 600)["hot_rows"] == want
        finally:
            lib.lib().krs_embed_set_option(3, 0)
    assert lib.lib().krs_embed_set_option(3, 32) != 0


def test_refusals_return_their_status_and_no_record(lib):
    import ctypes as C

    from keras_rs_amd import embedding_ops as E

    ok = dict(n_feats=2, offsets=None, weights=None, nnz=600, batch=100, dim=128, table_dtype=lib.BF16, out=0x100000,
              out_dtype=lib.BF16, out_ld=256)
    assert E.embed_fwd_plan_route(**ok)["status"] == 0
    INVALID, UNSUPPORTED = -1, -2
    refused = [
        ("bad table dtype", dict(table_dtype=2), INVALID), ("bad output dtype", dict(out_dtype=-1), INVALID),
        ("negative batch", dict(batch=-1), INVALID), ("negative features", dict(n_feats=-1), INVALID),
        ("negative nnz", dict(nnz=-1), INVALID), ("dim 0", dict(dim=0), INVALID), ("negative dim", dict(dim=-8), INVALID),
        ("null out", dict(out=None), INVALID),
        # the kernels form (batch + bags_per_wave - 1) / bags_per_wave, bags_per_wave <= 128, and (batch + 63) / 64 in int
        ("batch beyond INT_MAX - 128", dict(batch=INT_MAX - 127, nnz=0), UNSUPPORTED),
        ("batch INT_MAX, one-hot", dict(batch=INT_MAX, n_feats=1, nnz=INT_MAX), UNSUPPORTED),
        # generic kernel at lpr 64: four bags per workgroup, 5 x (2^31 - 200) bags need more than 2^31 - 1 workgroups
        ("grid too large", dict(n_feats=5, batch=INT_MAX - 199, dim=260, table_dtype=lib.F32, out_dtype=lib.F32, nnz=0),
         UNSUPPORTED),
    ]
    before = E.embed_fwd_last_route()
    for what, change, status in refused:
        assert E.embed_fwd_plan_route(**dict(ok, **change)) == dict(R(None), status=status), what
        assert lib.lib().krs_last_error(), what
    # the largest batch the planner accepts, and a grid of exactly 2^31 - 1 workgroups
    assert E.embed_fwd_plan_route(**dict(ok, batch=INT_MAX - 128, nnz=0))["status"] == 0
    edge = E.embed_fwd_plan_route(**dict(ok, n_feats=4, batch=INT_MAX - 128, dim=260, table_dtype=lib.F32, nnz=0))
    assert edge["status"] == 0 and edge["blocks"] == INT_MAX - 128
    assert E.embed_fwd_last_route() == before            # (the query does not touch the record of the last call)
    # the entry's own refusals come before any launch, so they can be made here: a bad index type, null ids, and what
    # the planner refuses; each leaves an all-zero record
    fake = 0x100000
    call = [fake, fake, 2, fake, lib.I32, None, lib.I32, None, 600, 100, 128, lib.BF16, fake, lib.BF16, 256, None, None, None]
    for what, pos, value, status in (("bad id type", 4, 2, INVALID), ("bad offset type", 6, -1, INVALID),
                                     ("null ids", 3, None, INVALID), ("null tables", 0, None, INVALID),
                                     ("bad dtype", 11, 7, INVALID), ("dim 0", 10, 0, INVALID),
                                     ("batch beyond INT_MAX - 128", 9, INT_MAX - 100, UNSUPPORTED)):
        args = list(call)
        args[pos] = value
        assert lib.lib().krs_embed_bag_fwd(*args) == status, what
        assert E.embed_fwd_last_route() == R(None), what
        assert lib.lib().krs_embed_bag_fwd_last_route(None) == 0          # (the pointer is optional)
    # an empty call succeeds and leaves no record either
    args = list(call)
    args[9] = 0
    assert lib.lib().krs_embed_bag_fwd(*args) == 0 and E.embed_fwd_last_route() == R(None)
    rt = lib.EmbedFwdRoute()
    assert C.sizeof(rt) == 40


# ---- the reference's own fp32 evaluation stays inside the bound the kernels are held to --------------------------------

POOLED = [c for c in CASES if c.route["kernel"] in ("vec", "generic") or any(h != 1 for h in (c.hots or ()))]


@pytest.mark.parametrize("case", POOLED, ids=[c.name for c in POOLED])
def test_the_reference_evaluated_in_fp32_stays_inside_the_bound(case):
    import torch

    h = inputs(case.name)
    args = (h["tables"], case.feats, case.batch, case.dim, h["ids"])
    kw = dict(hots=case.hots, offsets=h["offsets"], weights=h["weights"])
    ref = RS.restate(*args, **kw)
    out32, scale32 = RS.evaluate_fp32(*args, **kw)
    assert ref["bad"] == bool(case.bad)
    assert np.isfinite(ref["out"]).all() and np.isfinite(out32).all()          # the poisoned row 0 is never a valid id
    if case.odt == "bf16":
        out32 = torch.from_numpy(out32).to(torch.bfloat16).float().numpy()
    zero = ref["den"] == 0
    assert (ref["out"][zero] == 0).all() and (out32[zero] == 0).all() and (scale32[zero] == 0).all()
    if case.weights == "pm_half":          # the weights of every mean bag cancel exactly
        assert zero[[f for f, (_, k) in enumerate(case.feats) if k == RS.MEAN]].all() and (ref["n"] == 2).all()
    err, tol = np.abs(out32 - ref["out"]), RS.bound(ref, case.odt == "bf16")
    assert (err[~zero] <= tol[~zero]).all(), float((err[~zero] / np.maximum(tol[~zero], 1e-300)).max())
    assert (np.abs(scale32 - ref["scale"]) <= RS.scale_bound(ref)).all()
    assert (scale32[ref["comb"] == RS.SUM] == 1.0).all()
    assert case.weights != "uniform" or (np.abs(ref["den"][ref["n"] > 0]) >= 0.25).all()      # never small


# ---- the planner's invariants, walked by a stand-alone program under the sanitizers ------------------------------------

def test_the_planner_header_compiles_without_hip_and_keeps_its_invariants_under_the_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "embed_fwd_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "embed_fwd_plan_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "0 failed checks" in run.stdout
