"""K21 on the GPU: krs_retrieval_ivf and PartitionedRetrieval against the numpy restatement
(tests/retrieval_ivf_restatement.py) on the integer data of tests/retrieval_ivf_cases.py, and against K8 itself on
seeded normal data.  Every comparison is exact -- ids, order and score bits: there is no tolerance in this file."""

import functools

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import retrieval_ops
from keras_rs_amd.layers import BruteForceRetrieval, PartitionedRetrieval
from tests import retrieval_ivf_cases as CASES
from tests import retrieval_ivf_restatement as RI

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a, dtype=None, pad=0):
    """a on the device; with pad, as the first columns of a wider tensor whose other columns hold a value no test uses"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = t if dtype is None else t.to(dtype)
    if pad:
        wide = torch.full((t.shape[0], t.shape[1] + pad), 100.0, dtype=t.dtype, device=DEV)
        wide[:, :t.shape[1]] = t
        t = wide[:, :t.shape[1]]
    return t


def _call(q, centroids, rows, offsets, row_index, probes, k, ids=None):
    """krs_retrieval_ivf through the C ABI on device tensors (column slices of wider tensors allowed), the outputs
    preset to values the call never writes: (scores as float32 numpy, ids numpy, leaves numpy)."""
    b, d = q.shape
    n, leaves = rows.shape[0], centroids.shape[0]
    scores = torch.full((b, k), float("nan"), dtype=q.dtype, device=DEV)
    out_ids = torch.full((b, k), -7, dtype=torch.int32, device=DEV)
    out_leaves = torch.full((b, probes), -7, dtype=torch.int32, device=DEV)
    size = retrieval_ops.retrieval_ivf_workspace_bytes(b, n, d, leaves, probes, k, q.dtype)
    assert size > 0
    ws = torch.empty(size, dtype=torch.uint8, device=DEV)
    rc = L.lib().krs_retrieval_ivf(L.ptr(q), q.stride(0), L.ptr(centroids), centroids.stride(0), L.ptr(rows),
                                   rows.stride(0), L.ptr(offsets), L.ptr(row_index), L.ptr(ids), L.fdtype(q), b, n, d,
                                   leaves, probes, k, L.ptr(scores), L.ptr(out_ids), L.ptr(out_leaves), L.ptr(ws), size,
                                   L.stream_ptr())
    L.check(rc, "krs_retrieval_ivf")
    torch.cuda.synchronize()
    return scores.float().cpu().numpy(), out_ids.cpu().numpy(), out_leaves.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(name):
    c = CASES.make(name)
    ref = RI.restate(c["query"], c["centroids"], c["cand"], c["assignments"], c["probes"], c["k"], ids=c["ids"],
                     out_bf16=c["dtype"] == "bf16")
    return c, ref


# ---- the case table, exact --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES.NAMES)
def test_case_equals_the_restatement(name):
    c, ref = _case(name)
    dt, pad = TORCH_DT[c["dtype"]], c["pad"]
    row_index, offsets = RI.layout(c["assignments"], len(c["sizes"]))
    got = _call(_dev(c["query"], dt, pad), _dev(c["centroids"], dt, pad), _dev(c["cand"][row_index], dt, pad),
                _dev(offsets), _dev(row_index), c["probes"], c["k"], ids=None if c["ids"] is None else _dev(c["ids"]))
    np.testing.assert_array_equal(got[2], ref["leaves"], err_msg=f"{name}: probed leaves")
    np.testing.assert_array_equal(got[1], ref["ids"], err_msg=f"{name}: ids")
    np.testing.assert_array_equal(_bits(got[0]), _bits(ref["scores"]), err_msg=f"{name}: score bits")


# ---- seeded normal data: K8 is the reference ----------------------------------------------------------------------------
N, D, LEAVES, K = 3000, 64, 12, 20


@functools.lru_cache(maxsize=None)
def _normal(dtype):
    """(candidates, centroids, assignments, queries) on the device: normal rows, any partition (the contract does not
    ask for a good one)"""
    rng = np.random.default_rng(77)
    dt = TORCH_DT[dtype]
    cand = _dev(rng.standard_normal((N, D)).astype(np.float32), dt)
    centroids = _dev(rng.standard_normal((LEAVES, D)).astype(np.float32), dt)
    assign = rng.integers(0, LEAVES, size=N)
    query = _dev(rng.standard_normal((40, D)).astype(np.float32), dt)
    return cand, centroids, assign, query


def _layer(dtype, probes, with_ids=False, k=K):
    cand, centroids, assign, _ = _normal(dtype)
    ids = torch.arange(N, dtype=torch.int32, device=DEV) * 2 + 5 if with_ids else None
    return PartitionedRetrieval.from_partition(cand, centroids, assign, candidate_ids=ids, k=k,
                                               num_leaves_to_search=probes)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_full_probe_equals_brute_force_bit_for_bit(dtype):
    cand, _, _, query = _normal(dtype)
    ids = torch.arange(N, dtype=torch.int32, device=DEV) * 2 + 5
    want_scores, want_ids = BruteForceRetrieval(cand, candidate_ids=ids, k=K)(query)
    got_scores, got_ids = _layer(dtype, LEAVES, with_ids=True)(query)
    assert got_scores.dtype == want_scores.dtype and got_ids.dtype == torch.int32
    assert torch.equal(got_ids, want_ids)
    assert torch.equal(got_scores.view(torch.int16 if dtype == "bf16" else torch.int32),
                       want_scores.view(torch.int16 if dtype == "bf16" else torch.int32))
    # an fp32 query against a bf16 index is promoted to fp32, as in BruteForceRetrieval
    if dtype == "bf16":
        q32 = query.float()
        want = BruteForceRetrieval(cand, k=K)(q32)
        got = _layer(dtype, LEAVES)(q32)
        assert got[0].dtype == torch.float32 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_partial_probe_equals_k8_on_the_gathered_rows(dtype):
    cand, _, assign, query = _normal(dtype)
    query = query[:8]
    scores, ids, leaves = _layer(dtype, 3).call(query, return_leaves=True)
    assert tuple(leaves.shape) == (8, 3)
    for i in range(8):
        pool = np.flatnonzero(np.isin(assign, leaves[i].cpu().numpy()))           # ascending original index
        pool_t = torch.from_numpy(pool.astype(np.int32)).to(DEV)
        want_scores, want_ids = retrieval_ops.retrieval_topk(query[i:i + 1], cand[pool_t.long()].contiguous(), K,
                                                             ids=pool_t)
        assert torch.equal(ids[i:i + 1], want_ids), i
        assert torch.equal(scores[i:i + 1].float(), want_scores.float()), i


def test_two_calls_give_identical_bytes():
    layer = _layer("bf16", 5)
    _, _, _, query = _normal("bf16")
    first = layer(query)
    second = layer(query)
    assert torch.equal(first[1], second[1]) and torch.equal(first[0].view(torch.int16), second[0].view(torch.int16))
    ids_only = PartitionedRetrieval.from_partition(*_normal("bf16")[:3], k=K, num_leaves_to_search=5,
                                                   return_scores=False)(query)
    assert torch.equal(ids_only, first[1])


def test_a_captured_call_replays_on_new_queries():
    layer = _layer("bf16", 4, with_ids=True)
    _, _, _, query = _normal("bf16")
    buf = query[:33].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer(buf)                                                      # (first use: kernel attributes, allocator)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = layer(buf)
    fresh = torch.flip(query, dims=(0,))[:33].contiguous()
    buf.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    want = layer(fresh)
    assert not torch.equal(want[1], layer(query[:33])[1])               # (the new queries do ask for other candidates)
    assert torch.equal(captured[1], want[1])
    assert torch.equal(captured[0].view(torch.int16), want[0].view(torch.int16))


# ---- the index build ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixture():
    """16 well-separated Gaussians in 16 dimensions: (candidates [1600, 16], queries [64, 16]) on the device"""
    rng = np.random.default_rng(9)
    centers = 10.0 * np.eye(16, dtype=np.float32) + 3.0
    cand = centers[np.arange(1600) % 16] + 0.5 * rng.standard_normal((1600, 16)).astype(np.float32)
    query = centers[np.arange(64) % 16] + 0.5 * rng.standard_normal((64, 16)).astype(np.float32)
    return _dev(cand.astype(np.float32)), _dev(query.astype(np.float32))


@functools.lru_cache(maxsize=None)
def _trained():
    cand, _ = _mixture()
    return PartitionedRetrieval(cand, k=10, num_leaves=16, num_leaves_to_search=2, training_iterations=4, seed=3)


def test_the_build_is_deterministic():
    cand, _ = _mixture()
    layer = _trained()
    first = layer.assignments.clone()
    centroids = layer.centroids.clone()
    assert first.dtype == torch.int32 and tuple(first.shape) == (1600,) and int(first.min()) >= 0 and int(first.max()) < 16
    layer.update_candidates(cand)
    assert torch.equal(layer.assignments, first) and torch.equal(layer.centroids, centroids)
    again = PartitionedRetrieval(cand, k=10, num_leaves=16, num_leaves_to_search=2, training_iterations=4, seed=3)
    assert torch.equal(again.assignments, first)
    # the layout the kernel is given: a stable sort by leaf
    row_index, offsets = RI.layout(first.cpu().numpy(), 16)
    assert (layer.row_index.cpu().numpy() == row_index).all() and (layer.leaf_offsets.cpu().numpy() == offsets).all()
    # centroids are unit vectors (an empty leaf keeps its own, a unit vector too)
    norms = layer.centroids.float().norm(dim=1)
    assert torch.allclose(norms, torch.ones_like(norms), atol=1e-5)


def test_state_dict_round_trip_serves_identical_results():
    _, query = _mixture()
    layer = _trained()
    want = layer(query)
    state = {name: t.clone() for name, t in layer.state_dict().items()}
    assert set(state) == {"candidate_rows", "leaf_offsets", "row_index", "centroids"}
    fresh = PartitionedRetrieval(k=10, num_leaves_to_search=2, training_iterations=10 ** 6)     # (would never finish)
    fresh.load_state_dict(state)
    got = fresh(query)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
    assert torch.equal(fresh.assignments, layer.assignments)


def test_more_probes_never_lose_the_exact_top1():
    """Monotonicity, not a tuned number: the probed leaves contain the exact top-1 for at least as many queries with 8
    probes as with 1, and for every query when all 16 leaves are probed.  (Measured recalls: DESIGN.md section 4, K21.)"""
    cand, query = _mixture()
    layer = _trained()
    top1 = BruteForceRetrieval(cand, k=1, return_scores=False)(query)[:, 0].long()
    home = layer.assignments[top1]                                      # the leaf that holds each query's exact top-1
    hits = {}
    for probes in (1, 8, 16):
        layer.num_leaves_to_search = probes
        _, ids, leaves = layer.call(query, return_leaves=True)
        hits[probes] = int((leaves == home[:, None]).any(dim=1).sum())
        print(f"probes={probes}: the exact top-1 is in the probed leaves for {hits[probes]} of {query.shape[0]} queries")
        if probes == 16:
            assert torch.equal(ids[:, 0].long(), top1)
    layer.num_leaves_to_search = 2
    assert hits[8] >= hits[1] and hits[16] == query.shape[0]


def test_example_serves_both_indexes_and_reports_a_recall(capsys):
    from examples import approximate_retrieval

    served = approximate_retrieval.main(steps=2, batch=64, users=100, items=300, dim=16, copies=3)
    assert 0.0 <= served["recall"] <= 1.0 and tuple(served["ids"].shape) == (64, 10)
    out = capsys.readouterr().out
    assert "Time taken by brute force layer" in out and "Time taken by partitioned layer" in out and "recall" in out
