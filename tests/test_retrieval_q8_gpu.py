"""K17 on the GPU: krs_retrieval_topk_q8 and the quantized BruteForceRetrieval against the numpy restatement
(tests/retrieval_q8_restatement.py).  Integer dot products are exact, so ids AND score bits must be equal to the
restatement: there is no tolerance anywhere in this file."""

import functools

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import embedding_ops, retrieval_ops
from keras_rs_amd.layers import BruteForceRetrieval
from tests import retrieval_q8_restatement as RQ

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _call(q, cq, cstep, k, ids=None, out="f32", want_scores=True, err=None):
    """krs_retrieval_topk_q8 through the C ABI on device tensors (q, cq may be column slices of wider tensors):
    (scores as float32 numpy or None, ids numpy)."""
    b, d = q.shape
    n = cq.shape[0]
    assert q.stride(1) == 1 and cq.stride(1) == 1 and cq.dtype == torch.int8 and cstep.dtype == torch.float32
    scores = torch.full((b, k), float("nan"), dtype=TORCH_DT[out], device=DEV) if want_scores else None
    out_ids = torch.full((b, k), -7, dtype=torch.int32, device=DEV)
    size = retrieval_ops.retrieval_topk_q8_workspace_bytes(b, n, d, k)
    assert size > 0
    ws = torch.empty(size, dtype=torch.uint8, device=DEV)
    rc = L.lib().krs_retrieval_topk_q8(L.ptr(q), q.stride(0), L.fdtype(q), L.ptr(cq), cq.stride(0), L.ptr(cstep),
                                       L.ptr(ids), b, n, d, k, L.ptr(scores), L.BF16 if out == "bf16" else L.F32,
                                       L.ptr(out_ids), L.ptr(err), L.ptr(ws), size, L.stream_ptr())
    L.check(rc, "krs_retrieval_topk_q8")
    torch.cuda.synchronize()
    return (None if scores is None else scores.float().cpu().numpy()), out_ids.cpu().numpy()


def _assert_equal(got_scores, got_ids, ref, what=""):
    np.testing.assert_array_equal(got_ids, ref["ids"], err_msg=f"{what}: ids")
    if got_scores is not None:
        np.testing.assert_array_equal(_bits(got_scores), _bits(ref["scores"]), err_msg=f"{what}: score bits")


# ---- integer data: every score an exact integer, ties everywhere ---------------------------------------------------------
def _integer_rows(rng, rows, d, patterns=None):
    """integer-valued float32 rows in [-127, 127] whose abs-max is exactly 127 (so step = 1.0f and q = x); with
    `patterns`, every row is one of that many byte-identical patterns"""
    src = rng.integers(-127, 128, size=(patterns or rows, d)).astype(np.float32)
    src[np.arange(src.shape[0]), rng.integers(0, d, size=src.shape[0])] = rng.choice([-127.0, 127.0], size=src.shape[0])
    return src[rng.integers(0, patterns, size=rows)] if patterns else src


# (d, k, n, b): one partial step; d = 1; the unaligned path; k at its limit with k = n - 1 and two query tiles, the last
# one ragged; several slices of several steps on the byte-load path; the widest rows
TIE_SHAPES = [(16, 5, 40, 3), (1, 3, 10, 1), (17, 1, 200, 1), (128, 128, 129, 33), (100, 10, 3000, 40),
              (512, 100, 1500, 32)]


@pytest.mark.parametrize("d,k,n,b", TIE_SHAPES)
def test_integer_ties_equal_the_restatement(d, k, n, b):
    rng = np.random.default_rng(d * 7919 + k * 31 + n + b)
    query = _integer_rows(rng, b, d)
    cand = _integer_rows(rng, n, d, patterns=7)
    cq, cstep, _ = RQ.quantize(cand)
    qq, qstep, _ = RQ.quantize(query)
    assert (cstep == np.float32(1.0)).all() and (cq == cand).all()          # checked on the CPU: the scores are integers
    assert (qstep == np.float32(1.0)).all() and (qq == query).all()
    ref = RQ.restate(query, cq, cstep, k)
    assert (ref["s"] == np.rint(ref["s"])).all()
    assert len(np.unique(ref["s"][0])) < n or n <= 10                      # ties are everywhere
    got = _call(_dev(query), _dev(cq), _dev(cstep), k)
    _assert_equal(*got, ref, f"d={d} k={k} n={n} b={b}")


@pytest.mark.parametrize("rising", [True, False], ids=["rising", "falling"])
def test_every_queue_cut_runs_on_monotone_scores(rising):
    """n = 4000 is 8 slices of 512 candidates = four 128-candidate steps each.  Candidate j = (127, h, h, l, 0 ...) with
    h = j div 254 - 8, l = j mod 254 - 127 and query (x, 127, 127, 1, 0 ...): score = 127 x + 254 h + l rises strictly with
    j, so every candidate beats the threshold and every queue is cut; the answer is the last k indices.  The mirrored
    query gives falling scores: after the first cut nothing enters a queue and the first k of slice 0 survive."""
    n, d, k = 4000, 16, 100
    j = np.arange(n)
    cq = np.zeros((n, d), np.int8)
    cq[:, 0], cq[:, 1], cq[:, 2], cq[:, 3] = 127, j // 254 - 8, j // 254 - 8, j % 254 - 127
    cstep = np.ones((n,), np.float32)
    sign = 1.0 if rising else -1.0
    query = np.zeros((3, d), np.float32)
    query[:, 0], query[:, 1], query[:, 2], query[:, 3] = [0.0, 5.0, -7.0], 127 * sign, 127 * sign, sign
    ref = RQ.restate(query, cq, cstep, k)
    assert (ref["qstep"] == np.float32(1.0)).all()
    s = ref["s"][0]
    assert (np.diff(s) > 0).all() if rising else (np.diff(s) < 0).all()
    want = np.arange(n - 1, n - 1 - k, -1) if rising else np.arange(k)
    assert (ref["ids"] == want[None, :]).all()
    got = _call(_dev(query), _dev(cq), _dev(cstep), k)
    _assert_equal(*got, ref, "monotone")


# ---- random normal data ---------------------------------------------------------------------------------------------------
RANDOM_SHAPES = [(64, 20000, 128, 100), (40, 3000, 100, 10), (33, 5000, 64, 128), (1, 129, 512, 7)]


@functools.lru_cache(maxsize=None)
def _random_case(b, n, d, k, qdt):
    """host inputs and the restatement of one random case, computed once and shared (never modified)"""
    rng = np.random.default_rng(b + n + d + k)
    query = torch.from_numpy(rng.standard_normal((b, d)).astype(np.float32)).to(TORCH_DT[qdt])
    cand = rng.standard_normal((n, d)).astype(np.float32) * rng.choice([0.01, 1.0, 30.0], size=(n, 1)).astype(np.float32)
    cq, cstep, _ = RQ.quantize(cand)
    ids = (rng.permutation(n) * 3 - 11).astype(np.int32)
    q32 = query.float().numpy()
    ref = {False: RQ.restate(q32, cq, cstep, k), True: RQ.restate(q32, cq, cstep, k, out_bf16=True)}
    return query, cand, cq, cstep, ids, ref


@pytest.mark.parametrize("out", ["f32", "bf16"])
@pytest.mark.parametrize("qdt", ["f32", "bf16"])
@pytest.mark.parametrize("b,n,d,k", RANDOM_SHAPES)
def test_random_normal_equals_the_restatement(b, n, d, k, qdt, out):
    query, cand, cq, cstep, ids, refs = _random_case(b, n, d, k, qdt)
    ref = refs[out == "bf16"]
    # the candidates are quantized on the device by krs_quantize_rows_q8, whose output is the restatement's too
    dq, dstep = embedding_ops.quantize_rows(_dev(cand))
    np.testing.assert_array_equal(dq.cpu().numpy(), cq)
    np.testing.assert_array_equal(_bits(dstep.cpu().numpy()), _bits(cstep))
    q = query.to(DEV)
    _assert_equal(*_call(q, dq, dstep, k, out=out), ref, "no ids")
    got_s, got_i = _call(q, dq, dstep, k, ids=_dev(ids), out=out)
    np.testing.assert_array_equal(got_i, ids[ref["index"]])
    np.testing.assert_array_equal(_bits(got_s), _bits(ref["scores"]))
    none_s, got_i = _call(q, dq, dstep, k, out=out, want_scores=False)           # out_scores = NULL
    assert none_s is None
    np.testing.assert_array_equal(got_i, ref["ids"])


def test_strided_operands_and_forced_byte_loads():
    b, n, d, k = 64, 20000, 128, 100
    query, _, cq, cstep, _, refs = _random_case(b, n, d, k, "f32")
    wide_q = torch.full((b, d + 5), float("nan"), device=DEV)
    wide_q[:, :d] = query.to(DEV)
    wide_c = torch.full((n, d + 9), -128, dtype=torch.int8, device=DEV)          # ldc = 137: no 16-byte loads
    wide_c[:, :d] = _dev(cq)
    assert wide_c.stride(0) % 16 != 0 and wide_q.stride(0) > d
    _assert_equal(*_call(wide_q[:, :d], wide_c[:, :d], _dev(cstep), k), refs[False], "ldq > d, ldc % 16 != 0")
    # the wrapper passes the same strides on
    s, i = retrieval_ops.retrieval_topk_q8(wide_q[:, :d], wide_c[:, :d], _dev(cstep), k)
    assert [retrieval_ops.last_route()[f] for f in ("kernel", "variant", "es", "vec", "row_bytes")] == ["fused", "q8", 1, 0, d]
    torch.cuda.synchronize()
    _assert_equal(s.cpu().numpy(), i.cpu().numpy(), refs[False], "wrapper")


def test_candidate_rows_holding_minus_128():
    rng = np.random.default_rng(128)
    b, n, d, k = 33, 700, 48, 20
    cq = rng.integers(-128, 128, size=(n, d)).astype(np.int8)
    cq[::3, 0] = -128
    cq[5] = -128                                                  # a whole row of -128
    cstep = rng.uniform(1e-3, 2.0, size=(n,)).astype(np.float32)
    query = rng.standard_normal((b, d)).astype(np.float32)
    query[0] = -1.0                                               # qq = -127 everywhere: the largest |idot| against row 5
    ref = RQ.restate(query, cq, cstep, k)
    assert int(RQ.idot(ref["qq"], cq)[0, 5]) == 127 * 128 * d
    _assert_equal(*_call(_dev(query), _dev(cq), _dev(cstep), k), ref, "-128")


def test_nonfinite_query_rows_score_zero_and_raise_the_flag():
    b, n, d, k = 40, 3000, 100, 10
    query, _, cq, cstep, _, refs = _random_case(b, n, d, k, "f32")
    dq, dstep = _dev(cq), _dev(cstep)
    clean = torch.zeros(1, dtype=torch.int32, device=DEV)
    _assert_equal(*_call(query.to(DEV), dq, dstep, k, err=clean), refs[False], "clean")
    assert int(clean.item()) == 0                                              # no flag on clean input
    bad = query.numpy().copy()
    bad[3, 7], bad[33, 99] = np.nan, -np.inf                                   # one row in each query tile
    ref = RQ.restate(bad, cq, cstep, k)
    assert ref["bad"].sum() == 2 and ref["flag"] == RQ.FLAG_NONFINITE_ROW
    assert (ref["ids"][[3, 33]] == np.arange(k)[None, :]).all() and (_bits(ref["scores"][[3, 33]]) == 0).all()
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = _call(_dev(bad), dq, dstep, k, err=err)
    _assert_equal(*got, ref, "non-finite rows")
    assert int(err.item()) == L.FLAG_NONFINITE_ROW
    _assert_equal(*_call(_dev(bad), dq, dstep, k, err=None), ref, "err_flag = NULL")


def test_two_calls_are_bitwise_equal():
    b, n, d, k = 64, 20000, 128, 100
    query, _, cq, cstep, _, _ = _random_case(b, n, d, k, "bf16")
    q, dq, dstep = query.to(DEV), _dev(cq), _dev(cstep)
    first, second = _call(q, dq, dstep, k, out="bf16"), _call(q, dq, dstep, k, out="bf16")
    np.testing.assert_array_equal(_bits(first[0]), _bits(second[0]))
    np.testing.assert_array_equal(first[1], second[1])


# ---- the layer --------------------------------------------------------------------------------------------------------------
def _layer_case():
    b, n, d, k = 40, 3000, 100, 10
    query, cand, cq, cstep, ids, refs = _random_case(b, n, d, k, "f32")
    ref = RQ.restate(query.numpy(), cq, cstep, k, ids=ids)
    return query, cand, cq, cstep, ids, ref, k


def test_quantized_layer_agrees_with_the_restatement_and_holds_the_int8_state():
    query, cand, cq, cstep, ids, ref, k = _layer_case()
    layer = BruteForceRetrieval(cand, ids, k=k)
    config = layer.get_config()
    layer.quantize("int8")
    assert layer.quantization_mode == "int8" and layer.candidate_embeddings is None and not layer._converted
    assert [w is layer.candidate_ids for w in layer.weights] == [True]
    assert set(layer.state_dict()) == {"candidate_ids", "candidate_embeddings_q", "candidate_embeddings_step"}
    assert layer.candidate_embeddings_q.dtype == torch.int8 and layer.candidate_embeddings_step.dtype == torch.float32
    assert layer.get_config() == config
    np.testing.assert_array_equal(layer.candidate_embeddings_q.cpu().numpy(), cq)
    with pytest.raises(ValueError, match="already quantized"):
        layer.quantize("int8")
    s, i = layer(query.to(DEV))
    torch.cuda.synchronize()
    assert s.dtype == torch.float32 and i.dtype == torch.int32
    _assert_equal(s.cpu().numpy(), i.cpu().numpy(), ref, "layer")
    # .bfloat16() keeps the steps fp32 (and the rows int8); bf16 queries give bf16 scores
    layer.bfloat16()
    assert layer.candidate_embeddings_step.dtype == torch.float32 and layer.candidate_embeddings_q.dtype == torch.int8
    np.testing.assert_array_equal(_bits(layer.candidate_embeddings_step.cpu().numpy()), _bits(cstep))
    qb = query.to(DEV).bfloat16()
    sb, ib = layer(qb)
    refb = RQ.restate(qb.float().cpu().numpy(), cq, cstep, k, ids=ids, out_bf16=True)
    assert sb.dtype == torch.bfloat16
    _assert_equal(sb.float().cpu().numpy(), ib.cpu().numpy(), refb, "bf16 queries")
    # a bf16 index that has served fp32 queries holds a converted fp32 copy: quantize() drops it with the float weight
    cand16 = torch.from_numpy(cand).to(DEV, torch.bfloat16)
    from16 = BruteForceRetrieval(cand16, ids, k=k)
    from16(query.to(DEV))
    assert list(from16._converted) == [torch.float32]
    from16.quantize("int8")
    assert not from16._converted and from16.candidate_embeddings is None
    q16, step16, _ = RQ.quantize(cand16.float().cpu().numpy())
    s16, i16 = from16(query.to(DEV))
    _assert_equal(s16.cpu().numpy(), i16.cpu().numpy(), RQ.restate(query.numpy(), q16, step16, k, ids=ids), "bf16 index")
    # ids alone
    only_ids = BruteForceRetrieval(cand, k=k, return_scores=False)
    only_ids.quantize()
    assert only_ids.weights == [] and set(only_ids.state_dict()) == {"candidate_embeddings_q", "candidate_embeddings_step"}
    np.testing.assert_array_equal(only_ids(query.to(DEV)).cpu().numpy(), ref["index"])
    # load_state_dict into a second layer quantized the same way reproduces the outputs
    rng = np.random.default_rng(9)
    other = BruteForceRetrieval(rng.standard_normal(cand.shape).astype(np.float32), np.zeros(len(ids), np.int32), k=k)
    other.quantize("int8")
    assert not torch.equal(other(query.to(DEV))[1], i)
    other.load_state_dict(layer.state_dict())
    s2, i2 = other(query.to(DEV))
    assert torch.equal(s2, s) and torch.equal(i2, i)


def test_update_candidates_on_a_quantized_layer():
    query, cand, cq, cstep, ids, ref, k = _layer_case()
    layer = BruteForceRetrieval(np.zeros_like(cand) + 1.0, ids, k=k)
    layer.quantize("int8")
    q_ptr, step_ptr = layer.candidate_embeddings_q.data_ptr(), layer.candidate_embeddings_step.data_ptr()
    layer.update_candidates(cand)
    assert (layer.candidate_embeddings_q.data_ptr(), layer.candidate_embeddings_step.data_ptr()) == (q_ptr, step_ptr)
    s, i = layer(query.to(DEV))
    _assert_equal(s.cpu().numpy(), i.cpu().numpy(), ref, "after update_candidates")
    poisoned = cand.copy()
    poisoned[17, 3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        layer.update_candidates(poisoned)
    with pytest.raises(ValueError, match="shape"):
        layer.update_candidates(cand[:-1])
    s2, i2 = layer(query.to(DEV))
    assert torch.equal(s2, s) and torch.equal(i2, i)                         # the index is untouched
    # a candidate row that cannot be quantized leaves an unquantized layer as it was
    plain = BruteForceRetrieval(poisoned, ids, k=k)
    with pytest.raises(ValueError, match="NaN"):
        plain.quantize("int8")
    assert plain.quantization_mode is None and plain.candidate_embeddings is not None
    assert set(plain.state_dict()) == {"candidate_embeddings", "candidate_ids"}


def test_graph_capture_then_update_candidates_replays_the_new_answer():
    query, cand, cq, cstep, ids, ref, k = _layer_case()
    rng = np.random.default_rng(5)
    layer = BruteForceRetrieval(rng.standard_normal(cand.shape).astype(np.float32), ids, k=k)
    layer.quantize("int8")
    q = query.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = layer(q)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = layer(q)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    layer.update_candidates(cand)
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out[1], eager[1])
    _assert_equal(out[0].cpu().numpy(), out[1].cpu().numpy(), ref, "replay after update_candidates")


def test_unquantized_layer_returns_what_retrieval_topk_returns():
    query, cand, _, _, ids, _, k = _layer_case()
    layer = BruteForceRetrieval(cand, ids, k=k)
    q = query.to(DEV)
    s, i = layer(q)
    es, ei = retrieval_ops.retrieval_topk(q, _dev(cand), k, ids=_dev(ids))
    assert layer.quantization_mode is None and torch.equal(s, es) and torch.equal(i, ei)


def test_example_reports_an_overlap(capsys):
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("two_tower_retrieval",
                                                  os.path.join(root, "examples", "two_tower_retrieval.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    served = example.main(steps=2, quantize=True)
    with capsys.disabled():
        print(f"\nint8 index against the exact one: overlap {served['overlap']:.4f}, bytes {served['index_bytes']} -> "
              f"{served['quantized_index_bytes']}")
    assert 0.0 <= served["overlap"] <= 1.0
    assert served["quantized_index_bytes"] < served["index_bytes"]
    assert tuple(served["ids"].shape) == (256, 5)
