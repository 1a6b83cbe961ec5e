"""K23 on the GPU: krs_ah_encode, krs_retrieval_ivf_ah, krs_retrieval_rescore and AsymmetricHashingRetrieval against the
numpy restatement (tests/retrieval_ah_restatement.py) on the integer data of tests/retrieval_ah_cases.py, against K8
itself (BruteForceRetrieval) for the rescored bits, and against float64 for the AH scores of normal data.  Except for that
last bound, which is derived in its test, every comparison is exact -- codes, ids, order and score bits."""

import functools

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import retrieval_ops
from keras_rs_amd.layers import AsymmetricHashingRetrieval, BruteForceRetrieval
from tests import retrieval_ah_cases as CASES
from tests import retrieval_ah_restatement as RA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _raw(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _dev(a, dtype=None, pad=0):
    """a on the device; with pad, as the first columns of a wider tensor whose other columns hold a value no test uses"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = t if dtype is None else t.to(dtype)
    if pad:
        wide = torch.full((t.shape[0], t.shape[1] + pad), 100, dtype=t.dtype, device=DEV)
        wide[:, :t.shape[1]] = t
        t = wide[:, :t.shape[1]]
    return t


# ---- the encoder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype,m,pad", [(100, "bf16", 8, 0), (100, "f32", 2, 0), (100, "bf16", 4, 3), (32, "bf16", 2, 0),
                                           (32, "f32", 4, 0), (32, "f32", 8, 4)])
def test_encoder_codes_equal_the_restatement_bit_for_bit(d, dtype, m, pad):
    """Random normal rows, N = 300: D = 100 takes element loads in bf16 (200-byte rows) and has a padded last block with
    m = 8, D = 32 takes 16-byte loads; the rows are gathered through row_index as the layer does."""
    rng = np.random.default_rng(41)
    n, leaves = 300, 5
    dt = TORCH_DT[dtype]
    x = _dev(rng.standard_normal((n, d)).astype(np.float32), dt, pad)
    cen = _dev(rng.standard_normal((leaves, d)).astype(np.float32), dt, pad)
    blocks = RA.blocks_of(d, m)
    cb = 0.7 * rng.standard_normal((blocks, 16, m)).astype(np.float32)
    cb[:, 3] = cb[:, 9]                                                  # two equal centres: real ties
    cb = cb.reshape(-1)
    cb[(np.arange(blocks)[:, None, None] * m + np.arange(m)[None, None, :] + np.zeros((1, 16, 1), int)).reshape(-1) >= d] = 0
    cb = _dev(cb.reshape(blocks, 16, m), torch.bfloat16)
    row_index = rng.permutation(n).astype(np.int32)
    leaf = rng.integers(0, leaves, size=n).astype(np.int32)              # of the STORED rows
    got = retrieval_ops.ah_encode(x, _dev(leaf), cen, cb, row_index=_dev(row_index))
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, RA.code_bytes(d, m))
    want = RA.encode(x.float().cpu().numpy()[row_index], leaf, cen.float().cpu().numpy(), cb.float().cpu().numpy())
    np.testing.assert_array_equal(got.cpu().numpy(), RA.pack(want, d, m))
    assert 9 not in np.unique(want) and len(np.unique(want)) > 2         # centre 9 equals centre 3: the lower code wins
    plain = retrieval_ops.ah_encode(x, _dev(leaf[np.argsort(row_index)]), cen, cb)     # the same rows without the gather
    assert torch.equal(plain[_dev(row_index).long()], got)


# ---- the case table, exact --------------------------------------------------------------------------------------------
def _call(q, centroids, codebooks, codes, offsets, row_index, probes, k, r, rows=None, ids=None):
    """krs_retrieval_ivf_ah through the C ABI on device tensors (column slices of wider tensors allowed), the outputs
    preset to values the call never writes: (scores as float32 numpy, ids numpy, leaves numpy)."""
    b, d = q.shape
    n, leaves, m = codes.shape[0], centroids.shape[0], codebooks.shape[2]
    scores = torch.full((b, k), float("nan"), dtype=q.dtype, device=DEV)
    out_ids = torch.full((b, k), -7, dtype=torch.int32, device=DEV)
    out_leaves = torch.full((b, probes), -7, dtype=torch.int32, device=DEV)
    size = retrieval_ops.retrieval_ivf_ah_workspace_bytes(b, n, d, leaves, probes, k, r, m, rows is not None, q.dtype)
    assert size > 0
    ws = torch.empty(size, dtype=torch.uint8, device=DEV)
    rc = L.lib().krs_retrieval_ivf_ah(L.ptr(q), q.stride(0), L.ptr(centroids), centroids.stride(0), L.ptr(codebooks), m,
                                      L.ptr(codes), codes.stride(0), L.ptr(offsets), L.ptr(row_index), L.ptr(rows),
                                      0 if rows is None else rows.stride(0), L.ptr(ids), L.fdtype(q), b, n, d, leaves,
                                      probes, k, r, L.ptr(scores), L.ptr(out_ids), L.ptr(out_leaves), L.ptr(ws), size,
                                      L.stream_ptr())
    L.check(rc, "krs_retrieval_ivf_ah")
    torch.cuda.synchronize()
    return scores.float().cpu().numpy(), out_ids.cpu().numpy(), out_leaves.cpu().numpy()


@pytest.mark.parametrize("name", CASES.NAMES)
def test_case_equals_the_restatement(name):
    c = CASES.make(name)
    k, r, d, m = c["k"], c["r"], c["cand"].shape[1], c["m"]
    ref = RA.restate(c["query"], c["centroids"], c["codebooks"], c["nibbles"], c["assignments"], c["probes"], k, r=r,
                     rows=None if r is None else c["cand"], ids=c["ids"], out_bf16=c["dtype"] == "bf16")
    dt, pad = TORCH_DT[c["dtype"]], c["pad"]
    row_index, offsets = RA.layout(c["assignments"], len(c["sizes"]))
    rows, centroids = _dev(c["cand"], dt, pad), _dev(c["centroids"], dt, pad)
    codebooks = _dev(c["codebooks"], torch.bfloat16)
    # the encoder first: the stored codes are the restatement's, in leaf order
    codes = retrieval_ops.ah_encode(rows, _dev(c["assignments"][row_index].astype(np.int32)), centroids, codebooks,
                                    row_index=_dev(row_index))
    np.testing.assert_array_equal(codes.cpu().numpy(), RA.pack(c["nibbles"][row_index], d, m), err_msg=f"{name}: codes")
    if pad:                                                             # a code row stride beyond the row's bytes
        wide = torch.full((codes.shape[0], codes.shape[1] + 4), 0xFF, dtype=torch.uint8, device=DEV)
        wide[:, :codes.shape[1]] = codes
        codes = wide[:, :codes.shape[1]]
    got = _call(_dev(c["query"], dt, pad), centroids, codebooks, codes, _dev(offsets), _dev(row_index), c["probes"], k,
                k if r is None else r, rows=None if r is None else rows,
                ids=None if c["ids"] is None else _dev(c["ids"]))
    np.testing.assert_array_equal(got[2], ref["leaves"], err_msg=f"{name}: probed leaves")
    np.testing.assert_array_equal(got[1], ref["ids"], err_msg=f"{name}: ids")
    np.testing.assert_array_equal(_bits(got[0]), _bits(ref["scores"]), err_msg=f"{name}: score bits")


# ---- the rescore: K8's bits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("d", [100, 128])
def test_rescored_scores_are_k8_bits(dtype, d):
    """krs_retrieval_rescore over all 128 indices, listed in a different order for every query, against
    BruteForceRetrieval(k = 128): the score of every id is bit-equal, and so is the order."""
    rng = np.random.default_rng(43)
    n, b = 128, 37
    dt = TORCH_DT[dtype]
    cand = _dev(rng.standard_normal((n, d)).astype(np.float32), dt)
    query = _dev(rng.standard_normal((b, d)).astype(np.float32), dt)
    ids = torch.arange(n, dtype=torch.int32, device=DEV) * 3 + 11
    want_scores, want_ids = BruteForceRetrieval(cand, candidate_ids=ids, k=n)(query)
    idx = _dev(np.stack([rng.permutation(n) for _ in range(b)]).astype(np.int32))
    got_scores, got_ids = retrieval_ops.retrieval_rescore(query, cand, idx, n, ids=ids)
    assert torch.equal(got_ids, want_ids)
    assert torch.equal(_raw(got_scores), _raw(want_scores))
    # a shorter list with padding: the k best of the listed ones, then -1 / -inf
    idx[:, 40:] = -1
    part_scores, part_ids = retrieval_ops.retrieval_rescore(query, cand, idx[:, :64], 50)
    ref = RA.rescore_select(query.float().cpu().numpy(), cand.float().cpu().numpy(), idx[:, :64].cpu().numpy(), 50)
    assert (part_ids.cpu().numpy()[:, 40:] == -1).all() and torch.isinf(part_scores[:, 40:].float()).all()
    want_raw, want_index = _raw(want_scores).cpu().numpy(), ((want_ids - 11) // 3).cpu().numpy()
    part_raw, part_index, listed = _raw(part_scores).cpu().numpy(), part_ids.cpu().numpy(), idx.cpu().numpy()
    for i in range(b):
        full = dict(zip(want_index[i].tolist(), want_raw[i].tolist()))
        assert sorted(part_index[i, :40].tolist()) == sorted(listed[i, :40].tolist())
        # K8's bits for every listed id
        assert part_raw[i, :40].tolist() == [full[j] for j in part_index[i, :40].tolist()]
        if dtype == "f32":                                               # and K8's order (fp32 scores come back whole)
            assert part_index[i].tolist() == ref["ids"][i].tolist()


# ---- the layer on a Gaussian mixture --------------------------------------------------------------------------------------
N, D, LEAVES, PROBES, K, R = 8192, 32, 32, 8, 10, 100


@functools.lru_cache(maxsize=None)
def _mixture():
    """(candidates [8192, 32], queries [48, 32]) fp32 on the device: 32 Gaussians around random centres"""
    rng = np.random.default_rng(45)
    centers = 3.0 * rng.standard_normal((LEAVES, D)).astype(np.float32)
    cand = centers[rng.integers(0, LEAVES, size=N)] + rng.standard_normal((N, D)).astype(np.float32)
    query = centers[rng.integers(0, LEAVES, size=48)] + rng.standard_normal((48, D)).astype(np.float32)
    return _dev(cand), _dev(query)


def _build(reorder):
    cand, _ = _mixture()
    return AsymmetricHashingRetrieval(cand, k=K, num_leaves=LEAVES, num_leaves_to_search=PROBES, training_iterations=3,
                                      seed=5, training_sample_size=2048, num_reordering_candidates=reorder)


@functools.lru_cache(maxsize=None)
def _trained(reorder):
    """The index with reordering, and the SAME index (partition, codebooks, codes) without it."""
    if reorder:
        return _build(R)
    on = _trained(True)
    cand, _ = _mixture()
    off = AsymmetricHashingRetrieval.from_codebooks(cand, on.centroids, on.assignments, on.codebooks, k=K,
                                                    num_leaves_to_search=PROBES)
    assert torch.equal(off.codes, on.codes) and torch.equal(off.row_index, on.row_index)
    return off


def test_the_build_is_deterministic():
    first = _trained(True)
    again = _build(R)
    assert first.codebooks.dtype == torch.bfloat16 and tuple(first.codebooks.shape) == (D // 2, 16, 2)
    assert first.codes.dtype == torch.uint8 and tuple(first.codes.shape) == (N, RA.code_bytes(D, 2))
    assert torch.equal(_raw(again.codebooks), _raw(first.codebooks)) and torch.equal(again.codes, first.codes)
    assert torch.equal(again.centroids, first.centroids) and torch.equal(again.row_index, first.row_index)
    # the stored codes are the restatement's for the stored codebooks
    cand, _ = _mixture()
    want = RA.encode(cand.cpu().numpy(), first.assignments.cpu().numpy(), first.centroids.cpu().numpy(),
                     first.codebooks.float().cpu().numpy())
    np.testing.assert_array_equal(first.codes.cpu().numpy(), RA.pack(want[first.row_index.cpu().numpy()], D, 2))


def test_reorder_never_loses():
    """Derivable: the AH top-R contains the AH top-k, so for every query and every j <= k the j-th rescored score is at
    least the j-th largest exact score among the ids the same index returns with reordering off."""
    cand, query = _mixture()
    on_scores, on_ids = _trained(True)(query)
    _, off_ids = _trained(False)(query)
    off_exact, _ = retrieval_ops.retrieval_rescore(query, cand, off_ids, K)     # their exact scores, K8's bits, sorted
    assert (on_scores >= off_exact).all()
    print(f"reordering changes {int((on_ids != off_ids).any(dim=1).sum())} of {query.shape[0]} result lists")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_reordering_every_candidate_equals_brute_force_bit_for_bit(dtype):
    """N = 100, 4 leaves, all probed, R = 128: the reorder sees every candidate, so the codes cannot matter -- trained
    ones (fp32) or random ones over a random partition (bf16)."""
    rng = np.random.default_rng(47)
    dt = TORCH_DT[dtype]
    cand = _dev(rng.standard_normal((100, 32)).astype(np.float32), dt)
    query = _dev(rng.standard_normal((33, 32)).astype(np.float32), dt)
    ids = torch.arange(100, dtype=torch.int32, device=DEV) * 2 + 5
    want_scores, want_ids = BruteForceRetrieval(cand, candidate_ids=ids, k=10)(query)
    if dtype == "f32":
        layer = AsymmetricHashingRetrieval(cand, candidate_ids=ids, k=10, num_leaves=4, num_leaves_to_search=4,
                                           training_iterations=2, num_reordering_candidates=128, dimensions_per_block=4)
    else:
        layer = AsymmetricHashingRetrieval.from_codebooks(
            cand, rng.standard_normal((4, 32)).astype(np.float32), rng.integers(0, 4, size=100),
            rng.standard_normal((8, 16, 4)).astype(np.float32), candidate_ids=ids, k=10, num_leaves_to_search=4,
            num_reordering_candidates=128)
    got_scores, got_ids = layer(query)
    assert got_scores.dtype == want_scores.dtype and torch.equal(got_ids, want_ids)
    assert torch.equal(_raw(got_scores), _raw(want_scores))
    if dtype == "bf16":                     # an fp32 query against a bf16 index is promoted, as in BruteForceRetrieval
        want = BruteForceRetrieval(cand, candidate_ids=ids, k=10)(query.float())
        got = layer(query.float())
        assert got[0].dtype == torch.float32 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_ah_scores_against_float64():
    """fp32 queries and centroids holding bf16-exact values, so every operand of the chain is bf16-exact and the
    accumulation is fp32: |chain - exact| <= (D + 1) u S with S = sum |q_i| |r_i| and u = 2^-24, the probe score is
    within K8's own bound (D + 1) u P with P = sum |q_i| |centroid_i|, and the final addition adds one rounding of a
    value of at most (S + |probe|)(1 + ...): |AH - q . (centroid + decode)| <= (D + 2) u (S + |probe|) + (D + 1) u P."""
    rng = np.random.default_rng(49)
    n, d, leaves, m, b, k = 600, 100, 6, 4, 20, 50
    bf = lambda a: torch.from_numpy(a).to(torch.bfloat16).float().numpy()           # noqa: E731
    cand = bf(rng.standard_normal((n, d)).astype(np.float32))
    centroids = bf(0.5 * rng.standard_normal((leaves, d)).astype(np.float32))
    query = bf(rng.standard_normal((b, d)).astype(np.float32))
    blocks = RA.blocks_of(d, m)
    codebooks = bf(0.8 * rng.standard_normal((blocks, 16, m)).astype(np.float32))
    assign = rng.integers(0, leaves, size=n)
    layer = AsymmetricHashingRetrieval.from_codebooks(_dev(cand), _dev(centroids), assign, _dev(codebooks), k=k,
                                                      num_leaves_to_search=3)
    scores, ids = layer(_dev(query))
    scores, ids = scores.cpu().numpy().astype(np.float64), ids.cpu().numpy()
    assert (ids >= 0).all()
    nib = RA.unpack(layer.codes.cpu().numpy(), d, m)
    stored = np.empty(n, np.int64)
    stored[layer.row_index.cpu().numpy()] = np.arange(n)
    recon = RA.decode(nib[stored], codebooks, d).astype(np.float64)                   # original order
    q64, cen64 = query.astype(np.float64), centroids.astype(np.float64)[assign]
    u = 2.0 ** -24
    worst = 0.0
    for i in range(b):
        r, c = recon[ids[i]], cen64[ids[i]]
        exact = r @ q64[i] + c @ q64[i]
        s_abs, p_abs = np.abs(r) @ np.abs(q64[i]), np.abs(c) @ np.abs(q64[i])
        bound = (d + 2) * u * (s_abs + np.abs(c @ q64[i])) + (d + 1) * u * p_abs
        err = np.abs(scores[i] - exact)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (i, float((err / bound).max()))
    print(f"largest error / bound: {worst:.3f}")


def test_two_calls_give_identical_bytes():
    _, query = _mixture()
    for reorder in (True, False):
        layer = _trained(reorder)
        first, second = layer(query), layer(query)
        assert torch.equal(first[1], second[1]) and torch.equal(first[0], second[0])
    # the probed leaves do not depend on the reorder stage
    assert torch.equal(_trained(True).call(query, return_leaves=True)[2],
                       _trained(False).call(query, return_leaves=True)[2])


@pytest.mark.parametrize("reorder", [True, False])
def test_a_captured_call_replays_on_overwritten_queries(reorder):
    layer = _trained(reorder)
    _, query = _mixture()
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
    assert torch.equal(captured[1], want[1]) and torch.equal(captured[0], want[0])


def test_state_dict_round_trip_serves_identical_results():
    _, query = _mixture()
    names = {"leaf_offsets", "row_index", "centroids", "codebooks", "codes"}
    for reorder in (True, False):
        layer = _trained(reorder)
        want = layer(query)
        state = {name: t.clone() for name, t in layer.state_dict().items()}
        # the float rows are kept only for reordering, in ORIGINAL order
        assert set(state) == (names | {"float_rows"} if reorder else names)
        assert (layer.float_rows is not None) == reorder and layer._converted == {}
        fresh = AsymmetricHashingRetrieval(k=K, num_leaves_to_search=PROBES, training_iterations=10 ** 6,
                                           num_reordering_candidates=R if reorder else None)
        fresh.load_state_dict(state)
        got = fresh(query)
        assert fresh.built and torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
        assert torch.equal(fresh.assignments, layer.assignments)
        assert fresh.index_bytes() == sum(t.numel() * t.element_size() for t in state.values())
    assert torch.equal(_trained(True).float_rows, _mixture()[0])
    # an index saved without float rows cannot reorder, and says so
    bare = AsymmetricHashingRetrieval(k=K, num_leaves_to_search=PROBES, num_reordering_candidates=R)
    bare.load_state_dict({name: t.clone() for name, t in _trained(False).state_dict().items()})
    with pytest.raises(ValueError, match="no float rows"):
        bare(query)
    # a bf16 query dtype below the index dtype is promoted; the converted copies follow the reorder switch
    half = _trained(False)(query.to(torch.bfloat16))
    assert half[0].dtype == torch.float32 and _trained(False)._converted == {}


def test_example_serves_the_ah_index_and_reports_bytes_and_recall(capsys):
    from examples import approximate_retrieval

    served = approximate_retrieval.main(steps=2, batch=64, users=100, items=300, dim=16, copies=3, ah=True, reorder=40)
    ah = served["ah"]
    assert 0.0 <= ah["recall"] <= 1.0 and tuple(ah["ids"].shape) == (64, 10)
    assert ah["index_bytes"] > ah["float_bytes"] > 0                    # (reordering keeps the float rows as well)
    out = capsys.readouterr().out
    assert "Time taken by asymmetric hashing layer" in out and "index bytes" in out and "reordering 40 candidates" in out
