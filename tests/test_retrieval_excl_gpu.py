"""K27 on the GPU: krs_retrieval_topk_excl / krs_retrieval_topk_q8_excl and BruteForceRetrieval.call(exclusions=...)
against an exact numpy reference.

Embeddings are small integers (every dot product is exact in bf16 -> fp32, in fp32 and, with one +-127 per row so that
K16's step is 1.0, in int8), so ids and score bits must be EQUAL to: mask the excluded entries, sort by (-score, index),
pad with -1 / -inf.  Ties are plentiful.  Every row excludes its own unexcluded best first, so a kernel that ignores
the lists fails every row."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
B = 33                         # two query tiles, the second partial


def _ops():
    from keras_rs_amd import retrieval_ops
    return retrieval_ops


def _inputs(n, d, q8=False, seed=0):
    rng = np.random.default_rng(seed)
    q = rng.integers(-3, 4, (B, d)).astype(np.int64)
    c = rng.integers(-3, 4, (n, d)).astype(np.int64)
    if q8:                     # abs-max 127 in every row: quantization step 1.0, the int8 rows are these integers
        q[np.arange(B), rng.integers(0, d, B)] = 127 * rng.choice([-1, 1], B)
        c[np.arange(n), rng.integers(0, d, n)] = 127 * rng.choice([-1, 1], n)
    c = c[np.argsort(c @ q[6], kind="stable")]     # row 6 meets its scores in ascending order: every step passes the threshold
    return q, c


def _reference(q, c, excl, k):
    n = c.shape[0]
    scores = (q @ c.T).astype(np.float64)
    ids = np.full((B, k), -1, np.int32)
    out = np.full((B, k), -np.inf, np.float32)
    for r in range(B):
        keep = np.ones(n, bool)
        keep[[v for v in excl[r] if 0 <= v < n]] = False
        idx = np.flatnonzero(keep)
        idx = idx[np.lexsort((idx, -scores[r, idx]))][:k]
        ids[r, :len(idx)] = idx
        out[r, :len(idx)] = scores[r, idx]
    return out, ids


def _lists(q, c, e, k, slice_):
    """[B, e] int32: each row's own top candidates, then what bites where the kernel can go wrong."""
    n = c.shape[0]
    _, top = _reference(q, c, [[]] * B, min(40, n))
    rows = [list(top[r][: 5 + r]) for r in range(B)]
    rows[1] += [0, n - 1, slice_ - 1, slice_, 2 * slice_ - 1, 2 * slice_]   # the ends of the index and of the slices
    rows[2] = list(range(128, 258)) + rows[2]                               # a whole 128-candidate step and two more
    rows[3] = rows[3] * 3                                                   # duplicates
    rows[4] = rows[4][:3] + [-1, -1] + rows[4][3:] + [n, n + 5, -7, 2**31 - 1]   # padding inside, values out of range
    rows[5] = list(range(n - 1, -1, -1))                                    # all the list can hold, from the far end
    rows[6] += list(range(100, 140)) + list(range(300, 420))                # inside the steps whose queue is cut back
    x = np.full((B, e), -1, np.int64)
    for r, row in enumerate(rows):
        x[r, : min(e, len(row))] = row[:e]
    return x.astype(np.int32)


def _check(scores, ids, ref_scores, ref_ids, dtype):
    assert torch.equal(ids.cpu(), torch.from_numpy(ref_ids))
    assert torch.equal(scores.cpu(), torch.from_numpy(ref_scores).to(dtype))   # exact integers: equal values are equal bits


def _n_for(k):
    return 2045 + k            # with e = 2048, row 5 keeps k - 3 candidates: a short result


FLOAT_CASES = [(dt, d, k, e) for dt in (torch.float32, torch.bfloat16) for d in (8, 50) for k in (1, 10, 128)
               for e in (130, 2048)] + [(torch.float32, 8, 129, 2048)]          # the last: the slab path


@pytest.mark.parametrize("dtype,d,k,e", FLOAT_CASES)
def test_topk_excl_matches_exact_reference(dtype, d, k, e):
    ops, n = _ops(), _n_for(k)
    q, c = _inputs(n, d)
    plan = ops.plan_route("topk_excl", B, n, d, k, dtype)[1]
    x = _lists(q, c, e, k, plan["slice"] or 384)
    qt = torch.tensor(q, dtype=dtype, device="cuda")
    ct = torch.tensor(c, dtype=dtype, device="cuda")
    scores, ids = ops.retrieval_topk(qt, ct, k, exclusions=torch.from_numpy(x).cuda())
    route = ops.last_route()
    assert route["variant"] == "topk_excl" and route["kernel"] == ("slab" if k == 129 else "fused")
    if k != 129:
        assert route["S"] >= 2 and route["slice"] < n and route["vec"] == (d == 8)
    _check(scores, ids, *_reference(q, c, x, k), dtype)


@pytest.mark.parametrize("e", [130, 2048])
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("d", [8, 16, 50])
def test_topk_q8_excl_matches_exact_reference(d, k, e):
    from keras_rs_amd import embedding_ops
    ops, n = _ops(), _n_for(k)
    q, c = _inputs(n, d, q8=True)
    x = _lists(q, c, e, k, ops.plan_route("q8_excl", B, n, d, k, torch.float32)[1]["slice"])
    cq, step = embedding_ops.quantize_rows(torch.tensor(c, dtype=torch.float32, device="cuda"))
    assert torch.all(step == 1.0)
    qt = torch.tensor(q, dtype=torch.float32, device="cuda")
    scores, ids = ops.retrieval_topk_q8(qt, cq, step, k, exclusions=torch.from_numpy(x).cuda())
    route = ops.last_route()
    assert route["variant"] == "q8_excl" and route["S"] >= 2 and route["vec"] == (d == 16)
    _check(scores, ids, *_reference(q, c, x, k), torch.float32)


@pytest.mark.parametrize("q8", [False, True])
def test_no_exclusions_is_the_parent_call_bit_for_bit(q8):
    from keras_rs_amd import embedding_ops
    ops, n, d, k = _ops(), 2100, 16, 10
    q, c = _inputs(n, d, q8=q8)
    qt = torch.tensor(q, dtype=torch.float32, device="cuda")
    ct = torch.tensor(c, dtype=torch.float32, device="cuda")
    if q8:
        cq, step = embedding_ops.quantize_rows(ct)
        call = lambda **kw: ops.retrieval_topk_q8(qt, cq, step, k, **kw)
    else:
        call = lambda **kw: ops.retrieval_topk(qt, ct, k, **kw)
    parent = call()
    for x in (torch.empty((B, 0), dtype=torch.int32), torch.full((B, 5), -1, dtype=torch.int32),
              torch.full((B, 3), n, dtype=torch.int64)):
        got = call(exclusions=x.cuda())
        assert torch.equal(got[0].view(torch.int32), parent[0].view(torch.int32)) and torch.equal(got[1], parent[1])


@pytest.mark.parametrize("quantized", [False, True])
def test_layer_excludes_candidate_ids_and_ignores_unknown_ones(quantized):
    import keras_rs_amd.layers as kl
    n, d, k = 2100, 16, 10
    q, c = _inputs(n, d, q8=quantized)
    rng = np.random.default_rng(1)
    cand_ids = (rng.permutation(n) * 7 + 3).astype(np.int32)         # shuffled, not contiguous
    _, top = _reference(q, c, [[]] * B, 12)
    rows = np.concatenate([top, np.full((B, 2), -1, np.int32)], axis=1)
    x_ids = np.where(rows >= 0, cand_ids[rows], -1)
    x_ids[:, 3] = 1                                                  # no candidate has id 1: ignored
    rows[:, 3] = -1
    layer = kl.BruteForceRetrieval(torch.tensor(c, dtype=torch.float32, device="cuda"),
                                   torch.from_numpy(cand_ids).cuda(), k=k)
    if quantized:
        layer.quantize("int8")
    scores, ids = layer(torch.tensor(q, dtype=torch.float32, device="cuda"), exclusions=torch.from_numpy(x_ids).cuda())
    ref_scores, ref_rows = _reference(q, c, rows, k)
    _check(scores, ids, ref_scores, cand_ids[ref_rows], torch.float32)
    with pytest.raises(NotImplementedError, match="exclusions"):
        kl.PartitionedRetrieval.call(None, None, exclusions=x_ids)


def test_graph_replay_reads_the_current_exclusions():
    ops, n, d, k = _ops(), 2100, 8, 10
    q, c = _inputs(n, d)
    qt = torch.tensor(q, dtype=torch.bfloat16, device="cuda")
    ct = torch.tensor(c, dtype=torch.bfloat16, device="cuda")
    lists = [_lists(q, c, 64, k, 384), np.roll(_lists(q, c, 64, k, 384), 7, axis=0)]
    x = torch.from_numpy(lists[0]).cuda()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.retrieval_topk(qt, ct, k, exclusions=x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scores, ids = ops.retrieval_topk(qt, ct, k, exclusions=x)
    for step in (1, 0, 1):
        x.copy_(torch.from_numpy(lists[step]))
        graph.replay()
        _check(scores, ids, *_reference(q, c, lists[step], k), torch.bfloat16)


@pytest.mark.parametrize("example", ["sas_rec", "sequential_retrieval"])
def test_examples_serve_without_the_history(example):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", example + ".py")
    spec = importlib.util.spec_from_file_location(example + "_excl_example", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.main(steps=1, batch=64, vocabulary_size=200, quiet=True, exclude_history=True)
    history = out["inputs"]["item_ids"] if example == "sas_rec" else out["context"]
    history = torch.where(history > 0, history, -1)                        # (0 pads a sequence)
    pred = out["outputs"]["predictions"]
    assert pred.shape == (64, 10) and bool((pred >= 0).all())
    assert not bool((pred[:, :, None] == history[:, None, :]).any())
    plain = ex.main(steps=1, batch=64, vocabulary_size=200, quiet=True)["outputs"]["predictions"]
    assert bool((plain[:, :, None] == history[:, None, :]).any())          # without the flag the history does come back
