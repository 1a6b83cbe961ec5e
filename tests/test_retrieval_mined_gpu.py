"""Hard-negative mining inside the fused in-batch softmax loss on the GPU (K14), against the float64 restatement of
tests/retrieval_mined_restatement.py.

Exact cases: embeddings are multiples of 1/4 in [-1, 1] with D <= 64, biases multiples of 1/8 and hit_value = -64, so
every corrected score is an exact fp32 number whatever the summation order: float64 and the kernel must select the
same candidates (ties are frequent: the tie rule is tested), the mined scores are bit-equal, and loss, dq and dc are
held to the restatement's bounds.  Random cases compare the loss on the rows whose k-th and (k+1)-th negative scores
are further apart than twice the score bound.  Then the slab path as a second implementation, the C ABI's contract,
and peak memory.  Tolerances are the stated bounds of the restatement, never tuned; `_close` prints the worst
error / bound ratio before it asserts."""

import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers, retrieval_ops
from tests import retrieval_loss_restatement as R
from tests import retrieval_mined_restatement as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIB = 1 << 20
HIT = -64.0
DTYPES = [torch.bfloat16, torch.float32]
REDUCTIONS = ["none", None, "sum", "sum_over_batch_size", "mean", "mean_with_sample_weight"]
# (B, N, num_hard_negatives, D): 32 query rows per workgroup (B = 31, 33, 70), 128 candidates per step (N = 129), a queue
# compaction (N = 3000: three steps per slice, the second holds more than 128 pairs), always 8 slices; k = N - 1 by the
# clamp (129 / 500 and 2 / 5); D = 20: bf16 rows that are not whole 16-byte chunks
SHAPES = [(1, 2, 1, 1), (1, 2, 5, 8), (31, 129, 5, 8), (33, 129, 128, 20), (31, 129, 500, 64), (70, 1000, 32, 20),
          (33, 3000, 128, 64), (70, 3000, 1, 8), (31, 1000, 5, 1), (1, 3000, 32, 20)]
ARRANGEMENTS = ["ascending", "descending", "last_block", "other_slice", "shared_positive", "popular", "high_word_ids"]


def _exact(b, n, d, seed, dtype):
    """q, c in multiples of 1/4, bias in multiples of 1/8, positives, int32 ids and row weights (CPU tensors)."""
    gen = torch.Generator().manual_seed(seed)
    q = (torch.randint(-4, 5, (b, d), generator=gen) / 4.0).to(dtype)
    c = (torch.randint(-4, 5, (n, d), generator=gen) / 4.0).to(dtype)
    bias = torch.randint(-8, 9, (n,), generator=gen) / 8.0
    pos = torch.randint(0, n, (b,), generator=gen)
    ids = torch.randint(0, max(2, n // 2), (n,), generator=gen, dtype=torch.int32)
    w = torch.rand(b, generator=gen) * 2.0 - 0.5
    return q, c, bias, pos, ids, w


def _dev(t):
    return None if t is None else t.to(DEV)


def _mine(q, c, k, pos, bias, ids, hit, fn=None, **kw):
    """retrieval_mine (or `fn`) on device copies: CPU (int64 indices, fp32 scores, fp32 positive scores)."""
    ops = retrieval_ops._xent_operands(_dev(q), _dev(c), _dev(pos), _dev(bias), _dev(ids))
    idx, val, ps = (fn or retrieval_ops.retrieval_mine)(ops[0], ops[1], k, ops[2], ops[3], ops[4], hit, **kw)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and ps.dtype == torch.float32
    return idx.cpu().to(torch.int64), val.cpu(), ps.cpu()


def _run(q, c, nhn, pos=None, bias=None, ids=None, hit=HIT, ls=0.0, g=None, path="fused", **kw):
    """The op on device copies with reduction "none" and upstream g: CPU (loss [B], dq, dc)."""
    qd = q.clone().to(DEV).requires_grad_(True)
    cd = c.clone().to(DEV).requires_grad_(True)
    loss = retrieval_ops.retrieval_xent(qd, cd, positive_index=_dev(pos), cand_bias=_dev(bias), cand_ids=_dev(ids),
                                        hit_value=hit, label_smoothing=ls, path=path, num_hard_negatives=nhn, **kw)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (q.shape[0],)
    ok = ~torch.isnan(loss.detach())
    (loss if g is None else loss * g.to(DEV))[ok].sum().backward()
    assert qd.grad.dtype == q.dtype and cd.grad.dtype == c.dtype
    return loss.detach().cpu(), qd.grad.cpu(), cd.grad.cpu()


def _close(what, got, ref):
    """loss, dq and dc within the restatement's bounds on the rows that have a positive; NaN exactly where stated."""
    ok, nan_dc = ref["ok"], ref["nan_dc"]
    assert bool(torch.isnan(got[0][~ok]).all()) and bool(torch.isnan(got[1][~ok]).all()), f"{what}: NaN rows"
    assert bool(torch.isnan(got[2][nan_dc]).all()), f"{what}: dc rows mined by a row without a positive"
    for name, value, key, keep in (("loss", got[0], "loss", ok), ("dq", got[1], "dq", ok), ("dc", got[2], "dc", ~nan_dc)):
        err = (value.double() - ref[key]).abs()[keep]
        tol = ref[key + "_tol"][keep]
        ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
        print(f"{what} {name}: worst error / bound = {ratio:.3f}")
        assert bool((err <= tol).all()), f"{what} {name}: worst error / bound = {ratio}"


def _check_exact(what, q, c, nhn, pos, bias, ids, ls, g, path="fused", mine=None, **kw):
    """Selection and mined scores exactly, then loss and gradients within the bounds.  Returns the reference."""
    n = c.shape[0]
    k = min(nhn, n - 1)
    ref = M.reference(q, c, k, pos, bias, ids, HIT, ls, g, out_bf16=q.dtype == torch.bfloat16)
    idx, val, ps = _mine(q, c, k, pos, bias, ids, HIT, fn=mine)
    assert torch.equal(idx, ref["idx"]), f"{what}: the selection differs from the total order's"
    assert torch.equal(val, ref["scores"].to(torch.float32)), f"{what}: the mined scores are not bit-equal"
    assert torch.equal(ps[ref["ok"]], ref["pos_score"][ref["ok"]].to(torch.float32)), f"{what}: the positives' scores"
    assert bool(torch.isnan(ps[~ref["ok"]]).all())
    _close(what, _run(q, c, nhn, pos, bias, ids, HIT, ls, g, path=path, **kw), ref)
    return ref


# ---- 1. exact cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_shapes(shape, dtype):
    b, n, nhn, d = shape
    q, c, bias, pos, ids, w = _exact(b, n, d, seed=b + 7 * n + nhn + d, dtype=dtype)
    odd = (b + nhn) % 2 == 1           # half the shapes: given positives and label smoothing
    _check_exact(f"{shape}", q, c, nhn, pos if odd else None, bias, ids, 0.1 if odd else 0.0, w)


def _arrangement(name, dtype):
    """(q, c, k, pos, bias, ids) of an input arrangement."""
    b, n, d, k = 70, 3000, 8, 32
    if name in ("ascending", "descending"):
        d = 1
    if name == "last_block":
        n, d = 1000, 20
    q, c, bias, pos, ids, _ = _exact(b, n, d, seed=len(name), dtype=dtype)
    j, i = torch.arange(n), torch.arange(b)
    if name == "ascending":            # every candidate beats the row's threshold: every step compacts the queue
        bias = 2.5 * j
    elif name == "descending":         # after the first k none does
        bias = -2.5 * j
    elif name == "last_block":         # N = 1000: slice 7 is the partial block [896, 1000)
        pos = n - 1 - i % 50
    elif name == "other_slice":        # slices of 384: the positives in slice 7, every mined negative in slice 0
        pos, bias = 2688 + i, bias + 32.0 * (j < 384)
    elif name == "shared_positive":
        pos = i % 3
    elif name == "popular":            # candidate 77 is mined by every query: one long dc segment
        pos, k = 100 + i, 5
        bias = bias + 40.0 * (j == 77)
    elif name == "high_word_ids":      # equal low words: only the high word of the int64 tells the ids apart
        ids = (j % 5) + ((j % 3) << 32)
    return q, c, k, pos, bias.to(torch.float32), ids


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", ARRANGEMENTS)
def test_exact_arrangements(name, dtype):
    q, c, k, pos, bias, ids = _arrangement(name, dtype)
    ref = _check_exact(name, q, c, k, pos, bias, ids, 0.0, None)
    if name == "popular":
        assert bool((ref["idx"] == 77).any(-1).all())
    if name == "other_slice":
        assert bool((ref["idx"] < 384).all())
    if name == "high_word_ids":
        # a candidate that shares only the low word of the positive's id is no accidental hit
        plain = M.reference(q, c, k, pos, bias, (ids & 0xffffffff), HIT)
        assert not torch.equal(plain["idx"], ref["idx"])


@pytest.mark.parametrize("reduction", REDUCTIONS, ids=str)
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "sample_weight"])
def test_label_smoothing_with_every_reduction(reduction, weighted):
    b, n, d, k, ls = 33, 129, 8, 5, 0.2
    q, c, bias, pos, ids, w = _exact(b, n, d, seed=11, dtype=torch.bfloat16)
    w = w if weighted else None
    if reduction in ("none", None, "sum"):
        g = torch.ones(b) if w is None else w
    elif reduction == "mean_with_sample_weight" and w is not None:
        g = w / w.sum()
    else:
        g = (torch.ones(b) if w is None else w) / b
    ref = M.reference(q, c, k, pos, bias, ids, HIT, ls, g)
    qd, cd = q.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
    value = retrieval_ops.retrieval_xent(qd, cd, positive_index=_dev(pos), cand_bias=_dev(bias), cand_ids=_dev(ids),
                                         hit_value=HIT, label_smoothing=ls, sample_weight=_dev(w), reduction=reduction,
                                         num_hard_negatives=k)
    value.sum().backward()
    want = R.reduce(ref["loss"], None if w is None else w.double(), reduction)
    # the row bounds weighted as the reduction weights the rows, plus the fp32 sum over B terms
    scale = g.double().abs()
    if reduction in ("none", None):
        tol = ref["loss_tol"] * scale + 2 * M.U32 * want.abs()
        assert tuple(value.shape) == (b,)
    else:
        tol = (ref["loss_tol"] * scale).sum() + 4 * (b + 16) * M.U32 * (scale * ref["loss"].abs()).sum()
        assert value.dim() == 0
    err = (value.detach().cpu().double() - want).abs()
    print(f"{reduction} weighted={weighted}: worst error / bound = {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())
    # the gradients of the reduced value are those of sum_i g_i loss_i (the row losses were checked above)
    _close(f"{reduction}", (ref["loss"].float(), qd.grad.cpu(), cd.grad.cpu()), ref)


def test_layer_passes_the_argument_on():
    b, n, d, k = 33, 129, 8, 5
    q, c, _, pos, ids, w = _exact(b, n, d, seed=11, dtype=torch.bfloat16)
    prob = torch.rand(n, generator=torch.Generator().manual_seed(1)) * 0.5 + 1e-3
    bias = -torch.log(torch.clamp(prob.to(torch.float32), 1e-6, 1.0))
    outs = []
    for mined in (True, False):
        qd, cd = q.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
        if mined:
            value = layers.InBatchSoftmaxLoss(label_smoothing=0.1, reduction="sum", accidental_hit_value=HIT,
                                              num_hard_negatives=k)(
                qd, cd, positive_index=_dev(pos), candidate_ids=_dev(ids), candidate_sampling_probability=_dev(prob),
                sample_weight=_dev(w))
        else:
            value = retrieval_ops.retrieval_xent(qd, cd, positive_index=_dev(pos), cand_bias=_dev(bias),
                                                 cand_ids=_dev(ids), hit_value=HIT, label_smoothing=0.1,
                                                 sample_weight=_dev(w), reduction="sum", num_hard_negatives=k)
        value.backward()
        outs.append((value.detach(), qd.grad, cd.grad))
    for a, z in zip(*outs):
        assert torch.equal(a, z)


# ---- 2. random cases: the loss ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(70, 1000, 20, 32), (33, 300, 16, 5), (70, 1000, 20, 1), (64, 3000, 64, 128)],
                         ids=lambda s: "x".join(map(str, s)))
def test_random_loss_where_the_selection_is_determined(shape):
    b, n, d, k = shape
    gen = torch.Generator().manual_seed(0)
    q = torch.randn(b, d, generator=gen).bfloat16()
    c = torch.randn(n, d, generator=gen).bfloat16()
    prob = torch.rand(n, generator=gen)
    bias = -torch.log(torch.clamp(prob.to(torch.float32), 1e-6, 1.0))
    ref = M.reference(q, c, k, None, bias)
    qd, cd = q.to(DEV), c.to(DEV)
    loss = retrieval_ops.retrieval_xent(qd, cd, cand_bias=_dev(bias), path="fused", num_hard_negatives=k).cpu().double()
    # below a gap of 2 delta fp32 may legitimately rank the (k+1)-th negative above the k-th
    keep = ref["gap"] > 2 * ref["delta"]
    skipped = 1.0 - float(keep.double().mean())
    err, tol = (loss - ref["loss"]).abs()[keep], ref["loss_tol"][keep]
    print(f"{shape}: {100 * skipped:.2f} % of the rows skipped, worst error / bound = {float((err / tol).max()):.3f}")
    assert skipped <= 0.10
    assert bool((err <= tol).all())


# ---- 3. the paths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_fused_and_slab_paths_agree(dtype):
    b, n, d, k = 70, 1000, 20, 32
    q, c, bias, pos, ids, w = _exact(b, n, d, seed=3, dtype=dtype)
    pos[5] = n          # one row without a positive on both paths
    ref = _check_exact("fused", q, c, k, pos, bias, ids, 0.1, w, path="fused")
    slab_bytes = 4 * n * 32            # 32 query rows per slab: three slabs
    again = _check_exact("slab", q, c, k, pos, bias, ids, 0.1, w, path="slab", slab_bytes=slab_bytes,
                         mine=lambda *a: retrieval_ops.retrieval_mine_slab(*a, slab_bytes=slab_bytes))
    assert torch.equal(ref["idx"], again["idx"])


def test_one_candidate_is_the_unmined_loss():
    q, c, bias, _, ids, w = _exact(33, 1, 8, seed=2, dtype=torch.bfloat16)
    pos = torch.zeros(33, dtype=torch.int64)
    outs = []
    for nhn in (4, None):
        qd, cd = q.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
        loss = retrieval_ops.retrieval_xent(qd, cd, positive_index=_dev(pos), cand_bias=_dev(bias), hit_value=HIT,
                                            label_smoothing=0.1, num_hard_negatives=nhn)
        (loss * w.to(DEV)).sum().backward()
        outs.append((loss.detach(), qd.grad, cd.grad))
    for a, z in zip(*outs):
        assert torch.equal(a, z)


@pytest.mark.parametrize("shape", [(33, 300, 200, 8), (5, 40, 3, 520)], ids=["k200", "d520"])
def test_large_k_and_wide_rows_take_the_slab_path(shape, monkeypatch):
    b, n, nhn, d = shape

    def refuse(*a, **kw):
        raise AssertionError("the fused kernel was called for a shape it does not cover")

    q, c, bias, pos, ids, w = _exact(b, n, d, seed=d, dtype=torch.float32)
    ref = M.reference(q, c, nhn, pos, bias, ids, HIT, 0.0, w, out_bf16=False)
    idx, val, _ = _mine(q, c, nhn, pos, bias, ids, HIT, fn=retrieval_ops.retrieval_mine_slab)
    assert torch.equal(idx, ref["idx"]) and torch.equal(val, ref["scores"].float())
    monkeypatch.setattr(retrieval_ops, "retrieval_mine", refuse)
    _close(f"{shape}", _run(q, c, nhn, pos, bias, ids, HIT, 0.0, w, path="auto"), ref)
    monkeypatch.undo()
    with pytest.raises(L.KrsError, match="krs_retrieval_mine"):
        _run(q, c, nhn, pos, bias, ids, HIT, 0.0, w, path="fused")


# ---- 4. the C ABI ------------------------------------------------------------------------------------------------------
def _abi(q, c, k, ws, ws_bytes, idx, val, ps, ldq=None, ldc=None):
    b, d = q.shape
    return L.lib().krs_retrieval_mine(L.ptr(q), ldq or d, L.ptr(c), ldc or d, L.fdtype(q), b, c.shape[0], d, k, None, None,
                                      None, L.I32, 0.0, L.ptr(idx), L.ptr(val), L.ptr(ps), L.ptr(ws), ws_bytes,
                                      L.stream_ptr())


def test_abi_refusals_and_workspace_contents():
    b, n, d, k = 33, 1000, 20, 32
    q, c, *_ = _exact(b, n, d, seed=1, dtype=torch.bfloat16)
    qd, cd = q.to(DEV), c.to(DEV)
    need = retrieval_ops.retrieval_mine_workspace_bytes(b, n, d, k, q.dtype)
    assert need >= b * 8 * k * 8
    out = lambda: (torch.empty((b, k), dtype=torch.int32, device=DEV),   # noqa: E731
                   torch.empty((b, k), dtype=torch.float32, device=DEV), torch.empty((b,), dtype=torch.float32, device=DEV))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    idx, val, ps = out()
    assert _abi(qd, cd, 0, ws, need, idx, val, ps) == -1                     # KRS_ERR_INVALID
    assert _abi(qd, cd, n, ws, need, idx, val, ps) == -1
    assert _abi(qd, cd, k, ws, need, None, val, ps) == -1
    assert _abi(qd, cd, k, ws, need, idx, None, ps) == -1
    assert _abi(qd, cd, k, ws, need, idx, val, None) == -1
    assert _abi(qd, cd, k, ws, need - 1, idx, val, ps) == -4                 # KRS_ERR_WORKSPACE
    assert _abi(qd, cd, k, None, need, idx, val, ps) == -4
    assert _abi(qd, cd, k, ws, need, idx, val, ps) == 0
    nan_ws = torch.full((need // 4 + 1,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)
    idx2, val2, ps2 = out()
    assert _abi(qd, cd, k, nan_ws, need, idx2, val2, ps2) == 0
    assert torch.equal(idx, idx2) and torch.equal(val, val2) and torch.equal(ps, ps2)
    ref = M.reference(q, c, k)
    assert torch.equal(idx.cpu().to(torch.int64), ref["idx"]) and torch.equal(val.cpu(), ref["scores"].float())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_row_strides_larger_than_d(dtype):
    b, n, d, k = 33, 300, 20, 5
    q, c, bias, pos, ids, _ = _exact(b, n, d, seed=4, dtype=dtype)
    wide_q = torch.cat((q, torch.ones(b, 3, dtype=dtype)), 1).to(DEV)[:, :d]
    wide_c = torch.cat((c, torch.ones(n, 12, dtype=dtype)), 1).to(DEV)[:, :d]
    assert wide_q.stride(0) == d + 3 and wide_c.stride(0) == d + 12
    ref = M.reference(q, c, k, pos, bias, ids, HIT, out_bf16=dtype == torch.bfloat16)
    ops = retrieval_ops._xent_operands(wide_q, wide_c, _dev(pos), _dev(bias), _dev(ids))
    assert ops[0].stride(0) == d + 3 and ops[1].stride(0) == d + 12          # (no copy was made)
    idx, val, ps = retrieval_ops.retrieval_mine(ops[0], ops[1], k, ops[2], ops[3], ops[4], HIT)
    # (40 bytes of bf16 per row: element loads; 80 bytes of fp32 on a stride of 128: 16-byte loads)
    assert [retrieval_ops.last_route()[f] for f in ("kernel", "variant", "vec")] == ["fused", "mine", int(dtype == torch.float32)]
    assert torch.equal(idx.cpu().to(torch.int64), ref["idx"]) and torch.equal(val.cpu(), ref["scores"].float())
    assert torch.equal(ps.cpu(), ref["pos_score"].float())
    qd, cd = wide_q.detach().requires_grad_(True), wide_c.detach().requires_grad_(True)
    loss = retrieval_ops.retrieval_xent(qd, cd, positive_index=_dev(pos), cand_bias=_dev(bias), cand_ids=_dev(ids),
                                        hit_value=HIT, num_hard_negatives=k)
    loss.sum().backward()
    _close("strided", (loss.detach().cpu(), qd.grad.cpu(), cd.grad.cpu()), ref)


def test_a_positive_outside_the_candidates():
    b, n, d, k = 33, 129, 8, 5
    q, c, bias, pos, ids, w = _exact(b, n, d, seed=6, dtype=torch.bfloat16)
    pos[3], pos[17], pos[32] = n, -1, 2**40
    ref = _check_exact("bad positives", q, c, k, pos, bias, ids, 0.1, w)
    assert ref["ok"].sum() == b - 3 and 0 < int(ref["nan_dc"].sum()) <= 3 * k
    loss, dq, dc = _run(q, c, k, pos, bias, ids, HIT, 0.1, w)
    assert bool(torch.isfinite(loss[ref["ok"]]).all() and torch.isfinite(dq[ref["ok"]]).all())
    assert bool(torch.isfinite(dc[~ref["nan_dc"]]).all())
    # the default positives with more queries than candidates: the rows beyond N have none
    ref = _check_exact("b > n", q, c[:20], k, None, bias[:20], ids[:20], 0.0, w)
    assert ref["ok"].tolist() == [True] * 20 + [False] * 13


def test_two_calls_are_bit_identical():
    q, c, k, pos, bias, ids = _arrangement("popular", torch.bfloat16)
    first = _run(q, c, k, pos, bias, ids)
    second = _run(q, c, k, pos, bias, ids)
    for a, z in zip(first, second):
        assert torch.equal(a, z)
    assert _mine(q, c, k, pos, bias, ids, HIT)[0].tolist() == _mine(q, c, k, pos, bias, ids, HIT)[0].tolist()


# ---- 5. memory ---------------------------------------------------------------------------------------------------------
def test_peak_memory_stays_far_below_the_score_matrix():
    b = n = 4096
    d, k = 32, 8
    gen = torch.Generator().manual_seed(0)
    q = (torch.randn(b, d, generator=gen) * 0.5).bfloat16().to(DEV).requires_grad_(True)
    c = (torch.randn(n, d, generator=gen) * 0.5).bfloat16().to(DEV).requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = retrieval_ops.retrieval_xent(q, c, reduction="sum_over_batch_size", path="fused", num_hard_negatives=k)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / MIB:.2f} MiB against a {b * n * 4 / MIB:.0f} MiB score matrix")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(q.grad.float()).all())
    assert rise < b * n * 4 // 4
