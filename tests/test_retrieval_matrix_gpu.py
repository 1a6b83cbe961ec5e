"""K8 on the GPU, case by case (tests/retrieval_cases.py): every case calls retrieval_ops.retrieval_topk or topk_rows,
asserts last_route() field by field against the record the case must have -- so the table proves which stage-1 build,
which selection route and how many slab chunks ran -- and compares ids and scores with the numpy restatement of the
contract (tests/retrieval_restatement.py) on float64 scores of the dtype-rounded inputs.

All data but the "normal" group's is chosen so that fp32 arithmetic is exact in any order (small integers, powers of two,
infinities), so those comparisons are bit for bit.  The "normal" group's bound is derived: a returned score is an fp32 sum
of d products in an order that is not known, so |got - exact| <= (d + 1) * 2^-24 * (|q| . |c|^T) whatever the order (bf16
products are exact in fp32; an fp32 product adds one rounding, covered by the + 1), plus 2^-8 * |exact| where the output
is rounded to bf16."""

import os

import numpy as np
import pytest
import torch

from keras_rs_amd import retrieval_ops
from tests import retrieval_restatement as RS
from tests.retrieval_cases import CASES, FIELDS, inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENV = "KRS_RETRIEVAL_SLAB_BYTES"


def _group(name):
    return [c for c in CASES if c.group == name]


def _ids(cases):
    return [c.name for c in cases]


def _device(a: np.ndarray, c):
    """a [rows, d] on the GPU in the case's dtype and layout; the filling around a slice is NaN and must reach no result"""
    dtype = RS.TORCH_DTYPES[c.dtype]
    t = torch.from_numpy(a).to(DEV, dtype)
    rows, d = a.shape
    if c.layout == "plain":
        return t
    lead = 1 if c.layout == "col_slice" else 0
    parent = torch.full((rows, c.ld), float("nan"), dtype=dtype, device=DEV)
    parent[:, lead:lead + d] = t
    view = parent[:, lead:lead + d]
    assert view.stride(0) == c.ld and view.data_ptr() % 16 == c.base_offset and parent.data_ptr() % 16 == 0
    return view


def _assert_route(c):
    got = retrieval_ops.last_route()
    for field in FIELDS:
        assert got[field] == c.route[field], (field, got, c.route)
    assert set(got) == set(FIELDS)


def _topk(c, h):
    """(scores, ids) of the case's retrieval_topk call as numpy (scores as fp32), its route asserted"""
    q, cand = _device(h["q"], c), _device(h["c"], c)
    ids = None if h["ids"] is None else torch.from_numpy(h["ids"]).to(DEV)
    s, i = retrieval_ops.retrieval_topk(q, cand, c.k, ids=ids)
    _assert_route(c)
    torch.cuda.synchronize()
    assert s.shape == (c.b, c.k) and i.shape == (c.b, c.k) and s.dtype == RS.TORCH_DTYPES[c.dtype] and i.dtype == torch.int32
    return s, i


_ORDER = {}


def _expected(c, h):
    """(indices [b, k], float64 scores [b, n]) of the contract; the ramp and sawtooth cases share one full ranking"""
    scores = RS.scores64(h["q"], h["c"], c.dtype)
    if c.group == "order" and c.data != "late":
        key = (c.data, c.dtype)
        if key not in _ORDER:
            _ORDER[key] = RS.expected_topk(scores, 128)
        return _ORDER[key][:, :c.k], scores
    return RS.expected_topk(scores, c.k), scores


def _assert_exact(c, h, s, i):
    idx, scores = _expected(c, h)
    want_ids = idx if h["ids"] is None else h["ids"][idx]
    np.testing.assert_array_equal(i.cpu().numpy(), want_ids)
    want = torch.from_numpy(np.take_along_axis(scores, idx, 1).astype(np.float32)).to(RS.TORCH_DTYPES[c.dtype])
    assert torch.equal(s.cpu(), want)
    return idx


# ---- a. every stage-1 build ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _group("build"), ids=_ids(_group("build")))
def test_every_stage1_build_is_tie_exact(case):
    h = inputs(case.name)
    s, i = _topk(case, h)
    _assert_exact(case, h, s, i)
    assert not torch.isnan(s.float()).any()


# ---- b. score order in stage 1 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _group("order"), ids=_ids(_group("order")))
def test_stage1_keeps_the_best_k_whatever_order_the_scores_come_in(case):
    h = inputs(case.name)
    s, i = _topk(case, h)
    idx = _assert_exact(case, h, s, i)
    zero_rows = np.nonzero(h["q"][:, 0] == 0)[0]
    assert zero_rows.size >= 6
    np.testing.assert_array_equal(idx[zero_rows], np.tile(np.arange(case.k), (zero_rows.size, 1)))   # all tied: index order
    up = np.nonzero(h["q"][:, 0] > 0)[0]
    if case.data == "ramp":
        np.testing.assert_array_equal(idx[up], np.tile(case.n - 1 - np.arange(case.k), (up.size, 1)))
    if case.data == "late":          # candidates 0 .. k - 2, then the late arrival in place of candidate k - 1
        np.testing.assert_array_equal(idx[up], np.tile(np.append(np.arange(case.k - 1), 300), (up.size, 1)))


# ---- c. NaN and infinite scores ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _group("special"), ids=_ids(_group("special")))
def test_nan_ranks_above_inf_through_every_route(case):
    h = inputs(case.name)
    s, i = _topk(case, h)
    idx, scores = _expected(case, h)
    # the restatement itself: the zero row scores NaN against the non-finite candidates and +0.0 elsewhere
    finite = np.isfinite(h["c"][:, 0])
    assert np.isnan(scores[-1, ~finite]).all() and (scores[-1, finite] == 0).all() and (~finite).sum() > 10
    assert np.isnan(scores[0, case.n - case.nan:]).all() and (idx[0, :min(case.nan, case.k)] >= case.n - case.nan).all()
    np.testing.assert_array_equal(i.cpu().numpy(), idx)
    want = np.take_along_axis(scores, idx, 1).astype(np.float32) + np.float32(0.0)          # (-0.0 comes back as +0.0)
    want = torch.from_numpy(want).to(RS.TORCH_DTYPES[case.dtype]).float().numpy()
    got = s.float().cpu().numpy()
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert nan.any() and (case.nan >= case.k or np.isinf(want).any())     # (more NaN than k: nothing else is returned)


# ---- d. the merge of the slice lists -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _group("merge"), ids=_ids(_group("merge")))
def test_the_slice_merge_on_both_sides_of_2048_pairs(case):
    h = inputs(case.name)
    s, i = _topk(case, h)
    _assert_exact(case, h, s, i)


# ---- e. the two-step path in chunks --------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _group("chunks"), ids=_ids(_group("chunks")))
def test_the_slab_chunks_give_the_bits_of_one_chunk(case, monkeypatch):
    h = inputs(case.name)
    monkeypatch.delenv(ENV, raising=False)
    if case.budget:
        monkeypatch.setenv(ENV, str(case.budget))
    s, i = _topk(case, h)
    _assert_exact(case, h, s, i)
    if case.budget:
        monkeypatch.delenv(ENV)
        assert ENV not in os.environ
        q, cand = _device(h["q"], case), _device(h["c"], case)
        s1, i1 = retrieval_ops.retrieval_topk(q, cand, case.k, ids=None)
        one = retrieval_ops.last_route()
        assert (one["kernel"], one["chunks"], one["chunk_rows"]) == ("slab", 1, case.b)
        torch.cuda.synchronize()
        assert torch.equal(s, s1) and torch.equal(i, i1)


# ---- f. the row selection ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _group("rows"), ids=_ids(_group("rows")))
def test_topk_rows_on_every_selection_route(case):
    x = inputs(case.name)["x"]
    xt = torch.from_numpy(x).to(DEV, RS.TORCH_DTYPES[case.dtype])
    idx, keys = retrieval_ops.topk_rows(xt, case.k, want_keys=True)
    _assert_route(case)
    torch.cuda.synchronize()
    exp = RS.expected_topk(x.astype(np.float64), case.k)
    np.testing.assert_array_equal(idx.cpu().numpy(), exp)
    np.testing.assert_array_equal(keys.cpu().numpy(), np.take_along_axis(x, exp, 1))
    if case.data == "equal":
        np.testing.assert_array_equal(exp, np.tile(np.arange(case.k), (case.b, 1)))
    if case.data == "bucket":
        assert (np.sort(exp, 1) == np.sort(np.argwhere(x >= 2.0)[:, 1].reshape(case.b, case.k), 1)).all()


# ---- g. random normal data, one case per build ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", _group("normal"), ids=_ids(_group("normal")))
def test_random_normal_scores_stay_inside_the_derived_bound(case):
    h = inputs(case.name)
    s, i = _topk(case, h)
    exact = RS.scores64(h["q"], h["c"], case.dtype)
    bound = (case.d + 1) * 2.0 ** -24 * RS.abs_scores64(h["q"], h["c"], case.dtype)       # of an fp32 score, any order
    ids = i.cpu().numpy().astype(np.int64)
    got = s.float().cpu().numpy().astype(np.float64)
    mine = np.take_along_axis(exact, ids, 1)
    tol = np.take_along_axis(bound, ids, 1) + (np.abs(mine) * 2.0 ** -8 if case.dtype == "bf16" else 0.0)
    err = np.abs(got - mine)
    print(f"{case.name}: max |got - exact| / bound = {float((err / tol).max()):.4f}")
    assert (err <= tol).all()
    assert (np.diff(got, axis=1) <= 0).all()                       # sorted
    for r in range(case.b):
        kth_at = np.argsort(-exact[r], kind="stable")[case.k - 1]
        kth, tol_s = exact[r, kth_at], 2.0 * bound[r, kth_at]
        want = set(np.nonzero(exact[r] > kth + tol_s)[0])
        allowed = set(np.nonzero(exact[r] >= kth - tol_s)[0])
        got_set = set(ids[r])
        assert want <= got_set <= allowed and len(got_set) == case.k, r
