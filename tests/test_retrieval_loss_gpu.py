"""The retrieval training head on the GPU (K11): the softmax cross-entropy against float64 autograd of
tests/retrieval_loss_restatement.py over every path of the kernel (packed rows, LDS-staged rows up to 9216 columns,
streamed rows beyond; vector and scalar accesses; leading dimensions), every reduction and weight form, the two logit
corrections, determinism, graph capture, out-of-range sparse labels, and the assembled head of
examples/two_tower_retrieval.py.

Tolerances (stated, not tuned), u = 2^-24, N the row length, y' the smoothed labels, p = softmax(x), S = sum y':
    per-row loss      |loss - ref| <= 4 (N + 16) u sum_j |y'_j| (|m - x_j| + |log Z| + 1)
    gradient          |grad - ref| <= 4 (N + 16) u |g| (S p_j (1 + |m - x_j|) + |y'_j|) + 1e-37
                      (1e-37: fp32 underflow of p_j; a bf16 gradient adds one rounding, 2^-8 |ref|)
A reduced loss is an fp32 sum of R weighted row losses: the row bounds add up with the weights |g_r| = |w_r| / divisor,
plus 4 (R + 16) u sum_r |g_r v_r| for that sum."""

import importlib.util
import os

import numpy as np
import pytest
import torch

from keras_rs_amd import layers, retrieval_ops
from tests import retrieval_loss_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCTIONS = ["none", None, "sum", "sum_over_batch_size", "mean", "mean_with_sample_weight"]
U = R.U32


def _logits(shape, scale, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _one_hot(shape, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    idx = torch.randint(0, shape[-1], shape[:-1], generator=g)
    return idx, R.one_hot(idx, shape[-1], torch.float32)


def _soft(shape, seed):
    g = torch.Generator().manual_seed(seed + 2000)
    return torch.rand(shape, generator=g) * (torch.rand(shape, generator=g) < 0.3)     # sparse-ish, not normalised


def _check(x, y, ls=0.0, reduction="sum_over_batch_size", weight=None, upstream=None, loss=None, y_arg=None,
           bf16_roundings=1):
    """Runs `loss` (default CategoricalCrossentropy(ls, reduction)) on device copies of x [..., N] and y (y_arg: what
    the loss is handed instead of y, e.g. class indices) and compares value and gradient with float64 autograd.
    bf16_roundings: how many times a bf16 gradient is rounded on its way out (2^-8 |ref| each)."""
    loss = loss or layers.CategoricalCrossentropy(label_smoothing=ls, reduction=reduction)
    n = x.shape[-1]
    xd = x.clone().to(DEV).requires_grad_(True)
    out = loss((y if y_arg is None else y_arg).to(DEV), xd, sample_weight=None if weight is None else weight.to(DEV))
    assert out.dtype == torch.float32
    (out if upstream is None else out * upstream.to(DEV)).sum().backward()
    assert xd.grad.dtype == x.dtype and xd.grad.shape == x.shape
    x64 = x.double().requires_grad_(True)
    v64 = R.row_loss(x64, y.double(), ls)
    w64 = None if weight is None else weight.double()
    ref = R.reduce(v64, w64, reduction)
    assert tuple(out.shape) == tuple(ref.shape)
    (gv,) = torch.autograd.grad(ref.sum(), v64, retain_graph=True)       # g_r = w_r / divisor
    (ref if upstream is None else ref * upstream.double()).sum().backward()
    lm, gm = R.magnitudes(x, y, ls)
    bound = 4 * (n + 16) * U
    v64, ref = v64.detach(), ref.detach()
    err = (out.detach().cpu().double() - ref).abs()
    if reduction in ("none", None):
        ltol = bound * gv.abs() * lm
    else:
        ltol = (bound * gv.abs() * lm).sum() + 4 * (v64.numel() + 16) * U * (gv * v64).abs().sum()
    worst = int((err - ltol).argmax())
    print(f"loss err {float(err.flatten()[worst]):.3e} bound {float(ltol.flatten()[worst]):.3e}")
    assert bool((err <= ltol).all()), f"loss err {float(err.flatten()[worst])} > {float(ltol.flatten()[worst])}"
    g_total = gv if upstream is None else gv * upstream.double()
    gtol = bound * g_total.abs()[..., None] * gm + 1e-37
    if x.dtype == torch.bfloat16:
        gtol = gtol + bf16_roundings * 2.0 ** -8 * (1.0 + 2.0 ** -8) * x64.grad.abs() if bf16_roundings > 1 else \
            gtol + 2.0 ** -8 * x64.grad.abs()
    gerr = (xd.grad.cpu().double() - x64.grad).abs()
    worst = int((gerr - gtol).argmax())
    print(f"grad err {float(gerr.flatten()[worst]):.3e} bound {float(gtol.flatten()[worst]):.3e}")
    assert bool((gerr <= gtol).all()), f"grad err {float(gerr.flatten()[worst])} > {float(gtol.flatten()[worst])}"
    return out.detach(), xd.grad


# 9216 is the last LDS-staged row length, 9217 and 20000 stream; 1024 is the last packed one
COLS = [1, 2, 5, 63, 64, 65, 1000, 1024, 1025, 4097, 9216, 9217, 20000]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", [1, 3, 130])
@pytest.mark.parametrize("cols", COLS)
def test_loss_and_gradient_against_float64(cols, rows, dtype):
    seed = cols * 7 + rows
    idx, hot = _one_hot((rows, cols), seed)
    scales = (1.0, 30.0, 100.0) if rows <= 3 or cols <= 1025 else (30.0,)
    for scale in scales:
        x = _logits((rows, cols), scale, dtype, seed)
        _check(x, _soft((rows, cols), seed), ls=0.1 if scale == 1.0 else 0.0)
        dense = _check(x, hot, ls=0.1 if scale == 100.0 else 0.0)
        if scale == 30.0:
            sparse = _check(x, hot, loss=layers.SparseCategoricalCrossentropy(), y_arg=idx)
            assert torch.equal(dense[0], sparse[0]) and torch.equal(dense[1], sparse[1])


@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cols", [5, 65, 1025, 4100, 20000])
def test_dense_and_sparse_label_forms_agree(cols, dtype, ls):
    x = _logits((3, cols), 30.0, dtype, cols).to(DEV)
    idx, hot = _one_hot((3, cols), cols)
    g = torch.tensor([0.5, -1.25, 2.0], device=DEV)
    a = retrieval_ops.softmax_xent(x, labels=hot.to(DEV), label_smoothing=ls, g=g, g_scale=0.5)
    b = retrieval_ops.softmax_xent(x, label_index=idx.to(DEV), label_smoothing=ls, g=g, g_scale=0.5)
    c = retrieval_ops.softmax_xent(x, label_index=idx.to(DEV).to(torch.int32), label_smoothing=ls, g=g, g_scale=0.5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(b[0], c[0]) and torch.equal(b[1], c[1])
    ref = R.row_loss(x.cpu().double(), hot.double(), ls)
    lm, gm = R.magnitudes(x.cpu(), hot, ls)
    assert bool(((a[0].cpu().double() - ref).abs() <= 4 * (cols + 16) * U * lm).all())
    gref = R.row_grad(x.cpu().double(), hot.double(), ls, 0.5 * g.cpu().double())
    gtol = 4 * (cols + 16) * U * (0.5 * g.cpu().double().abs())[:, None] * gm + 1e-37
    if dtype == torch.bfloat16:
        gtol = gtol + 2.0 ** -8 * gref.abs()
    assert bool(((a[1].cpu().double() - gref).abs() <= gtol).all())


# (cols, storage width, first column): leading dimensions above cols that keep the 16-byte accesses (4104 and 9304),
# ones that do not (odd widths), and an aligned width behind a misaligned first column
STRIDED = [(65, 70, 0), (1030, 1031, 0), (4104, 4112, 0), (4104, 4112, 3), (9304, 9312, 0), (20000, 20001, 1)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cols,width,first", STRIDED)
def test_leading_dimensions_of_logits_and_labels(cols, width, first, dtype):
    rows = 3
    wide_x = _logits((rows, width + first), 30.0, dtype, cols).to(DEV)
    wide_y = _soft((rows, width + first), cols).to(DEV)
    x, y = wide_x[:, first:first + cols], wide_y[:, first:first + cols]
    assert not x.is_contiguous() and not y.is_contiguous()
    loss, dx = retrieval_ops.softmax_xent(x, labels=y, label_smoothing=0.1)
    packed = retrieval_ops.softmax_xent(x.contiguous(), labels=y.contiguous(), label_smoothing=0.1)
    ref = R.row_loss(x.cpu().double(), y.cpu().double(), 0.1)
    lm, gm = R.magnitudes(x.cpu(), y.cpu(), 0.1)
    bound = 4 * (cols + 16) * U
    gref = R.row_grad(x.cpu().double(), y.cpu().double(), 0.1)
    gtol = bound * gm + 1e-37 + (2.0 ** -8 * gref.abs() if dtype == torch.bfloat16 else 0.0)
    for got_loss, got_dx in ((loss, dx), packed):
        assert bool(((got_loss.cpu().double() - ref).abs() <= bound * lm).all())
        assert bool(((got_dx.cpu().double() - gref).abs() <= gtol).all())


@pytest.mark.parametrize("reduction", REDUCTIONS, ids=str)
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_reductions_and_weights(reduction, sparse):
    b, n = 37, 24
    x = _logits((b, n), 3.0, torch.float32, 5)
    idx, hot = _one_hot((b, n), 5)
    y = hot if sparse else _soft((b, n), 5)
    g = torch.Generator().manual_seed(9)
    ls = 0.0 if sparse else 0.1
    for w in (None, torch.rand(b, generator=g), torch.rand((b, 1), generator=g), torch.tensor(2.5), torch.zeros(b)):
        loss = layers.SparseCategoricalCrossentropy(reduction=reduction) if sparse else None
        if w is not None and w.dim() == 2:
            out, _ = _check_weight_alias(x, y, reduction, w, w.reshape(b), loss, idx if sparse else None, ls)
        else:
            out, _ = _check(x, y, ls, reduction, weight=w, loss=loss, y_arg=idx if sparse else None)
        assert tuple(out.shape) == ((b,) if reduction in ("none", None) else ())


def _check_weight_alias(x, y, reduction, w, w_ref, loss, y_arg, ls):
    """A [B, 1] weight gives what the [B] weight gives, bit for bit; the latter is checked against float64."""
    loss = loss or layers.CategoricalCrossentropy(label_smoothing=ls, reduction=reduction)
    ref = _check(x, y, ls, reduction, weight=w_ref, loss=loss, y_arg=y_arg)
    xd = x.clone().to(DEV).requires_grad_(True)
    out = loss((y if y_arg is None else y_arg).to(DEV), xd, sample_weight=w.to(DEV))
    out.sum().backward()
    assert torch.equal(out.detach(), ref[0]) and torch.equal(xd.grad, ref[1])
    return ref


@pytest.mark.parametrize("shape", [(24,), (5, 7, 24)], ids=["rank1", "rank3"])
@pytest.mark.parametrize("reduction", ["none", "sum_over_batch_size", "mean_with_sample_weight"])
def test_logits_of_rank_one_and_three(shape, reduction):
    x = _logits(shape, 3.0, torch.float32, 11)
    y = _soft(shape, 11)
    g = torch.Generator().manual_seed(3)
    weights = [None, torch.tensor(0.5)] + ([torch.rand(shape[:-1], generator=g), torch.rand(5, generator=g)]
                                           if len(shape) > 1 else [])
    for w in weights:
        if w is not None and w.dim() == 1 and len(shape) == 3:
            w = w.reshape(5, 1)                    # one weight per leading row
        out, _ = _check(x, y, 0.1, reduction, weight=w)
        assert tuple(out.shape) == (shape[:-1] if reduction == "none" else ())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("reduction", ["sum", "sum_over_batch_size", "mean_with_sample_weight"])
def test_non_unit_upstream_gradient(reduction, dtype):
    """A scalar reduction's backward multiplies the gradient the forward launch stored by the incoming scalar.  In
    fp32 that product's rounding is far inside the bound.  A bf16 gradient was rounded once when it was stored; the
    product rounds it again unless the scalar is a power of two, so -2.0 is held to the one-rounding bound and -2.5
    to two roundings, each 2^-8 of a value that may already be 2^-8 off."""
    x = _logits((33, 300), 5.0, dtype, 21)
    w = torch.rand(33, generator=torch.Generator().manual_seed(2))
    _check(x, _soft((33, 300), 21), 0.1, reduction, weight=w, upstream=torch.tensor(-2.0))
    _check(x, _soft((33, 300), 21), 0.1, reduction, weight=w, upstream=torch.tensor(-2.5), bf16_roundings=2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cols", [40, 1500, 9300])
def test_none_with_per_row_upstream(cols, dtype):
    g = torch.Generator().manual_seed(cols)
    x = _logits((9, cols), 5.0, dtype, cols)
    up = torch.randn(9, generator=g)
    for w in (None, torch.rand(9, generator=g)):
        _check(x, _soft((9, cols), cols), 0.1, "none", weight=w, upstream=up)


# ---- SamplingProbabilityCorrection -----------------------------------------------------------------------------------------
def _probs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(shape, generator=g) * 0.9
    r = torch.rand(shape, generator=g)
    p = torch.where(r < 0.1, torch.zeros_like(p), p)             # exact zeros: the lower side of the clip
    return torch.where(r > 0.9, torch.full_like(p, 1.5), p)      # above 1: the upper side


SPC_SHAPES = [((10,), (10,)), ((20, 10), (10,)), ((20, 10), (20, 10)), ((15, 20, 10), (10,)), ((15, 20, 10), (20, 10)),
              ((15, 20, 10), (15, 20, 10)), ((3, 1030), (1030,)), ((130, 1032), (1032,)), ((130, 1032), (130, 1032))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,pshape", SPC_SHAPES, ids=str)
def test_sampling_probability_correction(shape, pshape, dtype):
    eps = 1e-6
    x = _logits(shape, 2.0, dtype, len(shape) * 100 + len(pshape))
    p = _probs(pshape, 7)
    assert bool((p == 0).any()) and bool((p > 1).any())
    xd = x.clone().to(DEV).requires_grad_(True)
    out = layers.SamplingProbabilityCorrection(epsilon=eps)(xd, p.to(DEV))
    assert out.dtype == dtype and out.shape == x.shape
    p64 = torch.clamp(p.double(), float(np.float32(eps)), 1.0)
    ref = R.sampling_correction(x.double(), p.double(), float(np.float32(eps)))
    tol = 8 * U * (x.double().abs() + torch.log(p64).abs() + 1.0)
    if dtype == torch.bfloat16:
        tol = tol + 2.0 ** -8 * ref.abs()            # the output's one rounding to bf16
    err = (out.detach().cpu().double() - ref).abs()
    assert bool((err <= tol).all()), float((err - tol).max())
    below_one = torch.broadcast_to(p64 < 1.0, x.shape)
    if dtype == torch.float32:
        assert bool((out.detach().cpu()[below_one] > x[below_one]).all())
    else:
        assert bool((out.detach().cpu()[below_one] >= x[below_one]).all())
    assert torch.equal(out.detach().cpu()[~below_one], x[~below_one])          # log(1) = 0
    up = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)
    out.backward(up)
    assert torch.equal(xd.grad, up)


# ---- RemoveAccidentalHits ----------------------------------------------------------------------------------------------------
RAH_SHAPES = [((10,), (10,)), ((20, 10), (10,)), ((20, 10), (20, 10)), ((15, 20, 10), (10,)), ((15, 20, 10), (20, 10)),
              ((15, 20, 10), (15, 20, 10)), ((7, 200), (200,)), ((3, 1500), (3, 1500))]


def _rah_inputs(shape, ishape, itype, seed, id_range=4):
    g = torch.Generator().manual_seed(seed)
    logits = torch.rand(shape, generator=g)
    _, labels = _one_hot(shape, seed)
    ids = torch.randint(0, id_range, ishape, generator=g).to(itype)        # a small range: every row has duplicates
    return logits, labels, ids


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("itype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("shape,ishape", RAH_SHAPES, ids=str)
def test_remove_accidental_hits_ops_bit_exact(shape, ishape, itype):
    logits, labels, ids = _rah_inputs(shape, ishape, itype, 42)
    for value in (-1e9, 0.5):
        out = retrieval_ops.remove_accidental_hits(logits.to(DEV), labels.to(DEV), ids.to(DEV), value).cpu()
        exp = torch.from_numpy(R.remove_accidental_hits_f32(logits.numpy(), labels.numpy(), ids.numpy(), value))
        assert torch.equal(_bits(out), _bits(exp))
        assert torch.equal(out[labels == 1], logits[labels == 1])             # positives are unchanged


def test_remove_accidental_hits_bf16_logits():
    logits, labels, ids = _rah_inputs((7, 200), (200,), torch.int32, 3)
    logits = logits.to(torch.bfloat16)
    out = retrieval_ops.remove_accidental_hits(logits.to(DEV), labels.to(DEV), ids.to(DEV), 0.5).cpu()
    exp = torch.from_numpy(R.remove_accidental_hits_f32(logits.float().numpy(), labels.numpy(), ids.numpy(), 0.5))
    assert out.dtype == torch.bfloat16 and torch.equal(out, exp.to(torch.bfloat16))


@pytest.mark.parametrize("itype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("shape,ishape", RAH_SHAPES[:6], ids=str)
def test_remove_accidental_hits_layer_property(shape, ishape, itype):
    """The reference's own test (remove_accidental_hits_test.py:test_call) at atol = 1e-6: the positive's logit is
    unchanged, a duplicate of the positive's id moves by SMALLEST_FLOAT, every other logit is unchanged."""
    logits, labels, ids = _rah_inputs(shape, ishape, itype, 42, id_range=shape[-1])
    xd = logits.clone().to(DEV).requires_grad_(True)
    out = layers.RemoveAccidentalHits()(xd, labels.to(DEV), ids.to(DEV))
    got = out.detach().cpu()
    torch.testing.assert_close((got * labels).sum(-1), (logits * labels).sum(-1), atol=1e-6, rtol=1e-6)
    full_ids = torch.broadcast_to(ids, shape)
    pos = labels.argmax(-1, keepdim=True)
    dup = (torch.gather(full_ids, -1, pos) == full_ids) & (labels == 0)
    exp = torch.where(dup, logits + retrieval_ops.SMALLEST_FLOAT, logits)
    torch.testing.assert_close(got, exp, atol=1e-6, rtol=1e-6)
    up = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    out.backward(up)
    assert torch.equal(xd.grad, up)


def test_remove_accidental_hits_keeps_the_subnormal_on_zero_logits():
    _, labels, ids = _rah_inputs((20, 10), (10,), torch.int32, 8)
    logits = torch.zeros((20, 10))
    out = layers.RemoveAccidentalHits()(logits.to(DEV), labels.to(DEV), ids.to(DEV)).cpu()
    exp = torch.from_numpy(R.remove_accidental_hits_f32(logits.numpy(), labels.numpy(), ids.numpy(),
                                                        retrieval_ops.SMALLEST_FLOAT))
    assert torch.equal(_bits(out), _bits(exp))
    moved = out != 0
    assert bool(moved.any()) and bool((out[moved] == np.float32(retrieval_ops.SMALLEST_FLOAT)).all())
    assert 0.0 < float(out[moved][0]) < float(np.finfo(np.float32).tiny)


def test_remove_accidental_hits_label_ties_and_zero_rows():
    labels = torch.tensor([[0.5, 1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 2.0, 2.0],
                           [-0.0, 0.0, -0.0, 0.0, 0.0]])
    ids = torch.tensor([3, 5, 9, 5, 3], dtype=torch.int32)
    logits = torch.arange(20, dtype=torch.float32).reshape(4, 5)
    out = retrieval_ops.remove_accidental_hits(logits.to(DEV), labels.to(DEV), ids.to(DEV), 0.5).cpu()
    # positives: 1 (first of the tied maxima), 0 (all-zero row), 3, 0 (-0 == +0)
    dup = torch.tensor([[0, 1, 0, 1, 0], [1, 0, 0, 0, 1], [0, 1, 0, 1, 0], [1, 0, 0, 0, 1]], dtype=torch.float32)
    assert torch.equal(out, logits + (dup - labels) * 0.5)
    exp = torch.from_numpy(R.remove_accidental_hits_f32(logits.numpy(), labels.numpy(), ids.numpy(), 0.5))
    assert torch.equal(_bits(out), _bits(exp))
    wide = torch.zeros((2, 1500))
    wide[0, 700], wide[0, 1400] = 1.0, 1.0          # a tie across the waves of a one-row workgroup: the first wins
    wide_ids = (torch.arange(1500) % 700).to(torch.int32)
    out = retrieval_ops.remove_accidental_hits(torch.zeros((2, 1500), device=DEV), wide.to(DEV), wide_ids.to(DEV),
                                               0.5).cpu()
    exp = torch.from_numpy(R.remove_accidental_hits_f32(np.zeros((2, 1500), np.float32), wide.numpy(),
                                                        wide_ids.numpy(), 0.5))
    assert torch.equal(_bits(out), _bits(exp)) and float(out[0, 0]) == 0.5 and float(out[1, 700]) == 0.5


# ---- calls and capture -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [40, 1500, 20000])
def test_repeated_calls_are_bit_identical(cols):
    x = _logits((9, cols), 30.0, torch.float32, cols).to(DEV)
    y = _soft((9, cols), cols).to(DEV)
    a = retrieval_ops.softmax_xent(x, labels=y, label_smoothing=0.1)
    b = retrieval_ops.softmax_xent(x, labels=y, label_smoothing=0.1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("reduction", ["sum_over_batch_size", "mean_with_sample_weight", "none"])
def test_graph_capture_replays_bit_identically(reduction):
    b, n = 64, 1500
    loss = layers.CategoricalCrossentropy(label_smoothing=0.1, reduction=reduction)
    y = _soft((b, n), 17).to(DEV)
    w = torch.rand(b, generator=torch.Generator().manual_seed(4)).to(DEV)
    x = _logits((b, n), 5.0, torch.float32, 17).clone().to(DEV).requires_grad_(True)
    fresh = _logits((b, n), 5.0, torch.float32, 18).to(DEV)

    def step(inp):
        inp.grad = None
        out = loss(y, inp, sample_weight=w)
        out.sum().backward()
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    x.grad = None
    with torch.cuda.graph(graph):
        out = loss(y, x, sample_weight=w)
        out.sum().backward()
    with torch.no_grad():
        x.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    eager_in = fresh.clone().requires_grad_(True)
    eager = step(eager_in)
    assert torch.equal(out.detach(), eager.detach()) and torch.equal(x.grad, eager_in.grad)


@pytest.mark.parametrize("cols", [7, 1500, 20000])
def test_out_of_range_sparse_label_marks_its_row_nan(cols):
    x = _logits((5, cols), 3.0, torch.float32, cols).to(DEV)
    idx = torch.tensor([1, -1, 0, cols, cols - 1], device=DEV)
    good = torch.tensor([0, 2, 4], device=DEV)
    loss, dx = retrieval_ops.softmax_xent(x, label_index=idx)
    ref_loss, ref_dx = retrieval_ops.softmax_xent(x[good].contiguous(), label_index=idx[good])
    assert bool(loss[[1, 3]].isnan().all()) and bool(dx[[1, 3]].isnan().all())
    assert torch.equal(loss[good], ref_loss) and torch.equal(dx[good], ref_dx)
    out = layers.SparseCategoricalCrossentropy(reduction="none")(idx, x)
    assert out.isnan().tolist() == [False, True, False, True, False]


# ---- the assembled head --------------------------------------------------------------------------------------------------------
def _example():
    spec = importlib.util.spec_from_file_location("two_tower_retrieval",
                                                  os.path.join(ROOT, "examples", "two_tower_retrieval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


HEAD_CASES = {"plain": {}, "cand_prob": {"prob": True}, "duplicate_ids": {"ids": True},
              "hard_negatives": {"num_hard_negatives": 4},
              "all": {"prob": True, "ids": True, "num_hard_negatives": 4}}


@pytest.mark.parametrize("case", list(HEAD_CASES))
def test_assembled_retrieval_head(case):
    """retrieval_task_loss at B = N = 16, D = 8 against the float64 composition of the same stages
    (retrieval_loss_restatement.retrieval_head).  The bounds above, propagated through the fp32 stages before them:
        scores      ds_ij = (D + 2) u sum_k |q_ik c_jk|                          (an fp32 dot product of D terms)
        correction  ds_ij += 8 u (|s_ij| + |log p^_j| + 1)
        hits        ds_ij += 1e-37                                               (the subnormal and its rounding)
        loss        |loss - ref| <= mean_r [sum_j (p_rj + y_rj) ds_rj + 4 (n + 16) u sum_j |y_rj| (|m - x_rj| + |log Z|
                    + 1)] + 4 (B + 16) u mean_r |v_r|          (|dv_r / ds_rj| = |p_rj - y_rj| <= p_rj + y_rj)
        dlogits     dG_rj = g p_rj (ds_rj + sum_k p_rk ds_rk) + 4 (n + 16) u g (p_rj (1 + |m - x_rj|) + y_rj) + 1e-37,
                    g = 1 / B                                   (|dp_j / ds_k| <= p_j (delta_jk + p_k))
        d loss / dq |.| <= dG |c| + (N + 2) u |G| |c|;   d loss / dc: |.| <= dG^T |q| + (B + 2) u |G|^T |q|
    with n the row length after mining, and G scattered back to [B, N] where mining gathered."""
    cfg = HEAD_CASES[case]
    b = n_c = 16
    d = 8
    g = torch.Generator().manual_seed(31)
    q, c = torch.randn((b, d), generator=g), torch.randn((n_c, d), generator=g)
    ids = torch.randint(0, 5, (n_c,), generator=g).to(torch.int32) if cfg.get("ids") else None
    prob = (torch.rand(n_c, generator=g) * 0.5 + 0.01) if cfg.get("prob") else None
    nhn = cfg.get("num_hard_negatives")
    qd, cd = q.clone().to(DEV).requires_grad_(True), c.clone().to(DEV).requires_grad_(True)
    out = _example().retrieval_task_loss(qd, cd, cand_ids=None if ids is None else ids.to(DEV),
                                         cand_prob=None if prob is None else prob.to(DEV), num_hard_negatives=nhn)
    out.backward()
    q64, c64 = q.double().requires_grad_(True), c.double().requires_grad_(True)
    ref, s64, y64 = R.retrieval_head(q64, c64, ids, prob, nhn, value=retrieval_ops.SMALLEST_FLOAT)
    s64.retain_grad()
    ref.backward()
    n = s64.shape[1]
    qa, ca = q.double().abs(), c.double().abs()
    raw = (q.double() @ c.double().T)
    ds = (d + 2) * U * (qa @ ca.T)
    if prob is not None:
        ds = ds + 8 * U * (raw.abs() + torch.log(torch.clamp(prob.double(), 1e-6, 1.0)).abs()[None, :] + 1.0)
    if ids is not None:
        ds = ds + 1e-37
    where = None
    if nhn is not None:      # the columns mining kept, in its order: match them by value (continuous scores: no ties)
        full = raw if prob is None else R.sampling_correction(raw, prob.double())
        where = (s64.detach()[:, :, None] - full[:, None, :]).abs().argmin(-1)
        ds = torch.gather(ds, 1, where)
    s, y = s64.detach(), y64
    lm, gm = R.magnitudes(s, y)
    p = torch.softmax(s, -1)
    v = R.row_loss(s, y)
    kb = 4 * (n + 16) * U
    ltol = float((((p + y) * ds).sum(-1) + kb * lm).mean() + 4 * (b + 16) * U * v.abs().mean())
    assert abs(float(out) - float(ref)) <= ltol, (float(out), float(ref), ltol)
    gs = 1.0 / b
    dG = gs * p * (ds + (p * ds).sum(-1, keepdim=True)) + kb * gs * gm + 1e-37
    G = s64.grad.abs()
    if where is not None:
        dG = torch.zeros((b, n_c), dtype=torch.float64).scatter_(1, where, dG)
        G = torch.zeros((b, n_c), dtype=torch.float64).scatter_(1, where, G)
    qtol = dG @ ca + (n_c + 2) * U * (G @ ca)
    ctol = dG.T @ qa + (b + 2) * U * (G.T @ qa)
    qerr, cerr = (qd.grad.cpu().double() - q64.grad).abs(), (cd.grad.cpu().double() - c64.grad).abs()
    print(f"loss err {abs(float(out) - float(ref)):.3e} bound {ltol:.3e}; dq err {float(qerr.max()):.3e} bound "
          f"{float(qtol.min()):.3e}; dc err {float(cerr.max()):.3e} bound {float(ctol.min()):.3e}")
    assert bool((qerr <= qtol).all()) and bool((cerr <= ctol).all())
