"""K13 (csrc/retrieval_xent.hip) on every instantiation of xent_kernel<DPAD, MODE, VEC>, under score orders that stress
the online statistics, with its options at their edges, through its C ABI directly, and on the slab path's edges.

The cases come from tests/retrieval_xent_cases.py; tests/test_retrieval_xent_cases_host.py shows without a GPU that the
table reaches every instantiation on a sliced and an unsliced sweep and that its float64 references are ones the bounds
can tell from a wrong result.  Every value comparison uses the stated bounds of tests/retrieval_xent_restatement.py
through `_close` of tests/test_retrieval_xent_gpu.py, unchanged; every "same result" comparison is torch.equal.
`_close` prints the worst error / bound ratio of each quantity before it asserts."""

import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers, retrieval_ops
from tests import retrieval_xent_cases as T
from tests import retrieval_xent_restatement as X
from tests.test_retrieval_xent_gpu import REDUCTIONS, _close, _run, _tols

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KRS_ERR_WORKSPACE = -4
NAN = float("nan")


def _same(a, z):
    return all(torch.equal(x, y) for x, y in zip(a, z))


# ---- 1. every instantiation against float64 ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.CASES, ids=[c.name for c in T.CASES])
def test_every_instantiation_against_float64(case):
    q, c, pos, bias, w = T.matrix_inputs(case)
    got = _run(q, c, pos, bias, ls=T.LS, g=w)
    ref = X.reference(q, c, pos, bias, ls=T.LS, g=w)
    _close(f"matrix {case.name} DPAD {case.dpad} VEC {case.vec}", got, ref, _tols(ref))


@pytest.mark.parametrize("shape", list(T.PLANS), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("d", [48, 200])
def test_a_misaligned_base_takes_the_element_loads_and_leaks_nothing(d, shape):
    # a column slice at element 1 of rows of d + 3: d % 8 == 0, yet no row starts on 16 bytes; NaN around the slice
    b, n = shape
    off, pad = 1, 3
    q, c, pos, prob, w = T.inputs(b, n, d, seed=300 + d + b)
    bias = T.bias_of(prob)
    wide_q = torch.full((b, d + pad), NAN, dtype=torch.bfloat16)
    wide_c = torch.full((n, d + pad), NAN, dtype=torch.bfloat16)
    wide_q[:, off:off + d], wide_c[:, off:off + d] = q, c
    wide_q, wide_c = wide_q.to(DEV).requires_grad_(True), wide_c.to(DEV).requires_grad_(True)
    vq, vc = wide_q[:, off:off + d], wide_c[:, off:off + d]
    assert vq.stride(0) == d + pad and vq.data_ptr() % 16 != 0 and vc.data_ptr() % 16 != 0
    loss = retrieval_ops.retrieval_xent(vq, vc, positive_index=pos.to(DEV), cand_bias=bias.to(DEV),
                                        label_smoothing=T.LS, path="fused")
    (loss * w.to(DEV)).sum().backward()
    plain = _run(q, c, pos, bias, ls=T.LS, g=w)
    assert torch.equal(loss.detach(), plain[0])
    assert torch.equal(wide_q.grad[:, off:off + d], plain[1]) and torch.equal(wide_c.grad[:, off:off + d], plain[2])
    ref = X.reference(q, c, pos, bias, ls=T.LS, g=w)
    _close(f"matrix misaligned {shape} d {d}", plain, ref, _tols(ref))


# ---- 2. score orders that stress the online statistics -----------------------------------------------------------------
@pytest.mark.parametrize("case", T.ORDERS, ids=[c.name for c in T.ORDERS])
def test_structured_score_orders_against_float64(case):
    q, c, pos, bias, w = T.order_inputs(case)
    got = _run(q, c, pos, bias, ls=T.LS, g=w)
    ref = X.reference(q, c, pos, bias, ls=T.LS, g=w)
    _close(f"orders {case.name}", got, ref, _tols(ref))


# ---- 3. options at their edges -----------------------------------------------------------------------------------------
def test_ids_that_differ_in_the_high_word_only_are_no_hits():
    b, n, d = 40, 161, 40
    q, c, pos, prob, w = T.inputs(b, n, d, seed=41)
    bias = T.bias_of(prob)
    j = torch.arange(n, dtype=torch.int64)
    ids = (j % 20) | ((j // 20) << 32)
    assert len(set(ids.tolist())) == n and len(set((ids & 0xffffffff).tolist())) == 20
    with_ids = _run(q, c, pos, bias, ids, hit_value=-1e30, ls=T.LS, g=w)
    without = _run(q, c, pos, bias, None, ls=T.LS, g=w)
    assert _same(with_ids, without)


def test_negative_ids_as_int64_and_int32_against_float64():
    b, n, d = 40, 161, 40
    q, c, pos, prob, w = T.inputs(b, n, d, seed=42)
    bias = T.bias_of(prob)
    j = torch.arange(n, dtype=torch.int64)
    ids = torch.where((j // 20) % 2 == 1, -1 - j % 20, j % 20)          # 40 distinct values, half of them negative
    assert int((ids < 0).sum()) > 0 and len(set(ids.tolist())) == 40
    ref = X.reference(q, c, pos, bias, ids, hit_value=-1e30, ls=T.LS, g=w)
    runs = []
    for id_dtype in (torch.int64, torch.int32):
        runs.append(_run(q, c, pos, bias, ids.to(id_dtype), hit_value=-1e30, ls=T.LS, g=w))
        _close(f"options negative ids {id_dtype}", runs[-1], ref, _tols(ref))
    assert _same(runs[0], runs[1])


def test_an_int64_positive_beyond_int32_marks_its_row_and_wraps_nowhere():
    b, n, d = 40, 161, 40
    q, c, pos, prob, w = T.inputs(b, n, d, seed=43)
    bias = T.bias_of(prob)
    bad = pos.to(torch.int64).clone()
    bad[3], bad[b - 2] = 2 ** 40, -2 ** 40                          # (both are 0 in their low 32 bits)
    good_loss, good_dq, _ = _run(q, c, pos.to(torch.int64), bias, ls=T.LS, g=w)
    loss, dq, dc = _run(q, c, bad, bias, ls=T.LS, g=w)
    rows = torch.zeros(b, dtype=torch.bool)
    rows[3] = rows[b - 2] = True
    assert bool(torch.isnan(loss.cpu()[rows]).all()) and torch.equal(loss.cpu()[~rows], good_loss.cpu()[~rows])
    assert bool(torch.isnan(dq.cpu()[rows]).all()) and torch.equal(dq.cpu()[~rows], good_dq.cpu()[~rows])
    assert bool(torch.isnan(dc).all())


def test_removed_hits_with_label_smoothing_against_float64():
    b, n, d = 33, 65, 16
    q, c, pos, prob, w = T.inputs(b, n, d, seed=44)
    bias = T.bias_of(prob)
    ids = torch.arange(n) % 20
    got = _run(q, c, pos, bias, ids, hit_value=-1e30, ls=T.LS, g=w)
    ref = X.reference(q, c, pos, bias, ids, hit_value=-1e30, ls=T.LS, g=w)
    # every removed hit keeps its smoothed label: the loss is about ls / n * 1e30 per hit, finite in fp32
    assert bool(torch.isfinite(got[0]).all()) and float(got[0].min()) > 1e26
    _close("options removed hits with smoothing", got, ref, _tols(ref))


@pytest.mark.parametrize("shape", [(5, 1, 8), (1, 70, 200)], ids=["5x1x8", "1x70x200"])
def test_one_candidate_and_one_query(shape):
    b, n, d = shape
    q, c, pos, prob, w = T.inputs(b, n, d, seed=45 + n)
    bias = T.bias_of(prob)
    got = _run(q, c, pos, bias, ls=T.LS, g=w)
    ref = X.reference(q, c, pos, bias, ls=T.LS, g=w)
    _close(f"options {shape}", got, ref, _tols(ref))


def test_an_empty_batch():
    n, d = 70, 24
    _, c, _, prob, _ = T.inputs(1, n, d, seed=46)
    q = torch.zeros((0, d), dtype=torch.bfloat16)
    loss, dq, dc = _run(q, c, torch.zeros(0, dtype=torch.int64), T.bias_of(prob), ls=T.LS)
    assert tuple(loss.shape) == (0,) and tuple(dq.shape) == (0, d)
    assert tuple(dc.shape) == (n, d) and bool((dc == 0).all())
    for reduction in REDUCTIONS:
        for weight in (None, torch.zeros(0)):
            qd, cd = q.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
            out = layers.InBatchSoftmaxLoss(label_smoothing=T.LS, reduction=reduction)(
                qd, cd, candidate_sampling_probability=prob.to(DEV), sample_weight=weight)
            assert tuple(out.shape) == ((0,) if reduction in ("none", None) else ())
            assert bool((out == 0).all())
            out.sum().backward()
            assert tuple(qd.grad.shape) == (0, d) and bool((cd.grad == 0).all())


# ---- 4. the C ABI, called directly -------------------------------------------------------------------------------------
class _Abi:
    """The operands of one shape on the device, and krs_retrieval_xent_fwd / _bwd on them with every argument the
    wrapper fixes left to the caller."""

    def __init__(self, b, n, d, seed):
        self.b, self.n, self.d = b, n, d
        self.cpu = T.inputs(b, n, d, seed=seed)
        q, c, pos, prob, w = self.cpu
        self.bias_cpu = T.bias_of(prob)
        self.q, self.c, self.w = q.to(DEV), c.to(DEV), w.to(DEV)
        self.pos, self.bias = pos.to(torch.int32).to(DEV), self.bias_cpu.to(DEV)
        self.size = retrieval_ops.retrieval_xent_workspace_bytes(b, n, d)

    def wrapper(self, g=None):
        q, c, pos, _, w = self.cpu
        return _run(q, c, pos, self.bias_cpu, ls=T.LS, g=w if g is None else g)

    def workspace(self, extra=4096):
        """size + extra bytes of 0xFF: a float read from it is NaN"""
        return torch.full((self.size + extra,), 0xFF, dtype=torch.uint8, device=DEV)

    def fwd(self, ws, ws_bytes, loss=None, lse=None):
        loss = torch.empty(self.b, dtype=torch.float32, device=DEV) if loss is None else loss
        lse = torch.empty(self.b, dtype=torch.float32, device=DEV) if lse is None else lse
        rc = L.lib().krs_retrieval_xent_fwd(L.ptr(self.q), self.d, L.ptr(self.c), self.d, L.BF16, self.b, self.n, self.d,
                                            L.ptr(self.pos), L.ptr(self.bias), None, L.I32, 0.0, T.LS, L.ptr(loss),
                                            L.ptr(lse), L.ptr(ws), ws_bytes, L.stream_ptr())
        return rc, loss, lse

    def bwd(self, lse, ws, ws_bytes, dq, dc, g="w", g_scale=1.0):
        g = self.w if isinstance(g, str) else g
        return L.lib().krs_retrieval_xent_bwd(L.ptr(self.q), self.d, L.ptr(self.c), self.d, L.BF16, self.b, self.n,
                                              self.d, L.ptr(self.pos), L.ptr(self.bias), None, L.I32, 0.0, T.LS,
                                              L.ptr(lse), L.ptr(g), g_scale, L.ptr(dq), 0 if dq is None else dq.stride(0),
                                              L.ptr(dc), 0 if dc is None else dc.stride(0), L.ptr(ws), ws_bytes,
                                              L.stream_ptr())

    def grads(self, dq_pad=0, dc_pad=0, fill=7.0):
        dq = torch.full((self.b, self.d + dq_pad), fill, dtype=torch.bfloat16, device=DEV)
        dc = torch.full((self.n, self.d + dc_pad), fill, dtype=torch.bfloat16, device=DEV)
        return dq, dc


# (40, 161, 40): forward and dq sliced (their partials go through the combine kernels), dc unsliced; its swap: dc sliced
ABI_SHAPES = [(40, 161, 40), (161, 40, 40)]
_abi_ids = ["40x161x40", "161x40x40"]


@pytest.fixture(scope="module", params=ABI_SHAPES, ids=_abi_ids)
def abi(request):
    b, n, d = request.param
    a = _Abi(b, n, d, seed=50 + b)
    assert a.size > 0
    a.joint = a.wrapper()                                   # (loss, dq, dc) of the wrapper, computed once
    return a


def test_abi_stays_inside_the_advertised_workspace_and_reads_no_partial_it_did_not_write(abi):
    ws = abi.workspace()
    rc, loss, lse = abi.fwd(ws, abi.size)
    assert rc == 0
    dq, dc = abi.grads()
    assert abi.bwd(lse, ws, abi.size, dq, dc) == 0
    assert torch.equal(loss, abi.joint[0]) and torch.equal(dq, abi.joint[1]) and torch.equal(dc, abi.joint[2])
    assert bool((ws[abi.size:] == 0xFF).all()) and ws.numel() - abi.size == 4096


def test_abi_refuses_a_short_or_missing_workspace_before_any_launch(abi):
    ws = abi.workspace(extra=0)
    rc, _, lse = abi.fwd(ws, abi.size)
    assert rc == 0
    # backward with both gradients needs exactly the advertised size on these shapes (one of its sweeps is sliced)
    for args in ((ws, abi.size - 1), (None, abi.size), (None, 0)):
        dq, dc = abi.grads()
        assert abi.bwd(lse, *args, dq, dc) == KRS_ERR_WORKSPACE
        assert b"workspace" in L.lib().krs_last_error()
        assert bool((dq == 7.0).all()) and bool((dc == 7.0).all())
    # forward: its partials are (m, Z, S, A) per slice and query, 16 S b bytes in whole 256-byte blocks
    slices = T.PLANS[(abi.b, abi.n)][0][1]
    need = -(-16 * slices * abi.b // 256) * 256 if slices > 1 else 0
    loss = torch.full((abi.b,), 7.0, dtype=torch.float32, device=DEV)
    out_lse = torch.full((abi.b,), 7.0, dtype=torch.float32, device=DEV)
    if need:
        assert need <= abi.size
        for args in ((ws, need - 1), (None, abi.size)):
            assert abi.fwd(*args, loss=loss, lse=out_lse)[0] == KRS_ERR_WORKSPACE
            assert bool((loss == 7.0).all()) and bool((out_lse == 7.0).all())
        assert abi.fwd(ws, need, loss=loss, lse=out_lse)[0] == 0
    else:
        assert abi.fwd(None, 0, loss=loss, lse=out_lse)[0] == 0      # an unsliced forward needs no workspace
    assert torch.equal(loss, abi.joint[0]) and torch.equal(out_lse, lse)


def test_abi_gradient_row_strides_leave_the_padding_alone(abi):
    ws = abi.workspace()
    _, _, lse = abi.fwd(ws, abi.size)
    dq, dc = abi.grads(dq_pad=5, dc_pad=3)
    assert dq.stride(0) == abi.d + 5 and dc.stride(0) == abi.d + 3
    assert abi.bwd(lse, ws, abi.size, dq, dc) == 0
    assert torch.equal(dq[:, :abi.d], abi.joint[1]) and torch.equal(dc[:, :abi.d], abi.joint[2])
    assert bool((dq[:, abi.d:] == 7.0).all()) and bool((dc[:, abi.d:] == 7.0).all())


def test_abi_one_gradient_alone_equals_its_half_of_the_joint_call(abi):
    ws = abi.workspace()
    _, _, lse = abi.fwd(ws, abi.size)
    dq, dc = abi.grads()
    ws.fill_(0xFF)
    assert abi.bwd(lse, ws, abi.size, dq, None) == 0
    assert torch.equal(dq, abi.joint[1])
    ws.fill_(0xFF)                                           # dc's partials now start at offset 0 of the workspace
    assert abi.bwd(lse, ws, abi.size, None, dc) == 0
    assert torch.equal(dc, abi.joint[2])
    assert bool((ws[abi.size:] == 0xFF).all())
    # the same through autograd: one leaf only
    q, c, pos, _, w = abi.cpu
    for which in (0, 1):
        qd, cd = q.to(DEV).requires_grad_(which == 0), c.to(DEV).requires_grad_(which == 1)
        loss = retrieval_ops.retrieval_xent(qd, cd, positive_index=abi.pos, cand_bias=abi.bias, label_smoothing=T.LS,
                                            path="fused")
        (loss * abi.w).sum().backward()
        assert torch.equal((qd, cd)[which].grad, abi.joint[1 + which]) and (qd, cd)[1 - which].grad is None


def test_abi_g_and_g_scale(abi):
    ws = abi.workspace()
    _, _, lse = abi.fwd(ws, abi.size)

    def grads(g, g_scale):
        dq, dc = abi.grads()
        assert abi.bwd(lse, ws, abi.size, dq, dc, g=g, g_scale=g_scale) == 0
        return dq, dc

    quarter = torch.full((abi.b,), 0.25, dtype=torch.float32, device=DEV)
    assert _same(grads(None, 0.25), grads(quarter, 1.0))
    assert _same(grads(abi.w, 0.5), grads(abi.w * 0.5, 1.0))       # (a power of two: the product is exact)
    assert _same(grads(abi.w, 1.0), abi.joint[1:])


# ---- 5. the slab path's edges ------------------------------------------------------------------------------------------
def test_slab_of_one_row_in_fp32():
    b, n, d = 5, 70, 24
    q, c, pos, prob, w = T.inputs(b, n, d, seed=61, dtype=torch.float32)
    bias = T.bias_of(prob)
    assert retrieval_ops._slabs(b, n, 1) == [(r, r + 1) for r in range(b)]        # a budget below one score row
    got = _run(q, c, pos, bias, ls=T.LS, g=w, path="slab", slab_bytes=1)
    ref = X.reference(q, c, pos, bias, ls=T.LS, g=w, p_bf16=False, out_bf16=False)
    _close("slab (5, 70, 24) fp32, one row per slab", got, ref, _tols(ref))


def test_slab_remainder_in_bf16():
    b, n, d = 129, 300, 100
    q, c, pos, prob, w = T.inputs(b, n, d, seed=62)
    bias = T.bias_of(prob)
    budget = n * 4 * 50
    assert retrieval_ops._slabs(b, n, budget) == [(0, 50), (50, 100), (100, 129)]
    got = _run(q, c, pos, bias, ls=T.LS, g=w, path="slab", slab_bytes=budget)
    ref = X.reference(q, c, pos, bias, ls=T.LS, g=w, p_bf16=False, out_bf16=True)
    _close("slab (129, 300, 100) bf16, 29-row remainder", got, ref, _tols(ref))


@pytest.mark.parametrize("with_ids", [False, True], ids=["no-ids", "ids"])
def test_slab_path_marks_a_bad_positive_like_the_fused_path(with_ids):
    b, n, d = 33, 65, 16
    q, c, pos, prob, w = T.inputs(b, n, d, seed=63)
    bias = T.bias_of(prob)
    ids = torch.arange(n) % 20 if with_ids else None
    bad = pos.clone()
    bad[2], bad[b - 1] = n + 5, -1
    rows = torch.zeros(b, dtype=torch.bool)
    rows[2] = rows[b - 1] = True
    budget = n * 4 * 10                                                          # slabs of 10 rows: the last has 3
    fused = _run(q, c, bad, bias, ids, hit_value=-1e30, g=w, path="fused")
    slab = _run(q, c, bad, bias, ids, hit_value=-1e30, g=w, path="slab", slab_bytes=budget)
    for name, (loss, dq, dc) in (("fused", fused), ("slab", slab)):
        assert torch.equal(torch.isnan(loss).cpu(), rows), name
        assert torch.equal(torch.isnan(dq).cpu(), rows[:, None].expand(b, d)), name
        assert bool(torch.isnan(dc).all()), name
    # the good rows: loss and dq of a row depend on no other row
    ref = X.reference(q, c, pos, bias, ids, hit_value=-1e30, g=w, p_bf16=False, out_bf16=True)
    good = ~rows
    part = {k: (v[good] if v.dim() and v.shape[0] == b else v) for k, v in ref.items()}
    for name, value, key in (("loss", slab[0], "loss"), ("dq", slab[1], "dq")):
        err = (value.cpu().double()[good] - part[key]).abs()
        ratio = float((err / part[key + "_tol"].clamp_min(1e-300)).max())
        print(f"slab bad positive ids={with_ids} {name}: worst error / bound = {ratio:.3f}")
        assert bool((err <= part[key + "_tol"]).all()), (name, ratio)
