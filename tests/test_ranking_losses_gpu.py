"""The ranking losses on the GPU (K9): every value of the reference's tests through the HIP path, random fp32 / bf16
lists against float64 autograd of tests/ranking_restatement.py, masks, invalid labels, ties, the exact gradients at
the non-smooth points, the two-launch "none" backward, determinism, graph capture and the list-length limit.

Tolerance of the random cases (stated, not tuned): an output element of the kernel is an fp32 sum of at most L + 16
terms, each rounded a few times, so |got - ref| <= 4 (L + 16) u M with u = 2^-24 and M the float64 sum of the
absolute values of those terms (ranking_restatement.magnitudes); a bf16 gradient adds one rounding, 2^-8 |ref|."""

import json
import os

import pytest
import torch

from keras_rs_amd import KrsError, losses
from tests import ranking_restatement as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ranking_losses.json")))
KINDS = {"PairwiseHingeLoss": "hinge", "PairwiseLogisticLoss": "logistic", "PairwiseSoftZeroOneLoss": "soft_zero_one",
         "PairwiseMeanSquaredError": "mse", "ListMLELoss": "listmle"}
CLASS = {k: getattr(losses, n) for n, k in KINDS.items()}
REDUCTIONS = ["none", "sum", "sum_over_batch_size", "mean", "mean_with_sample_weight"]


@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: f"{c['loss']}-{c['case']}")
def test_reference_values(c):
    loss = getattr(losses, c["loss"])(temperature=c["temperature"], reduction=c["reduction"])
    y = torch.tensor(GOLD["labels"], device=DEV)
    s = torch.tensor(GOLD["scores"], device=DEV)
    if c["rank"] == 1:
        y, s = y[0], s[0]
    y_true = y if c["mask"] is None else {"labels": y, "mask": torch.tensor(c["mask"], device=DEV)}
    w = None if c["sample_weight"] is None else torch.tensor(c["sample_weight"], device=DEV)
    got = loss(y_true, s, sample_weight=w)
    exp = torch.tensor(c["expected"], dtype=torch.float32)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(exp.shape)
    # the reference's assertAllClose(..., atol=1e-5) keeps keras' rtol=1e-6 (143.8 * 5 is not within 1e-5 in fp32)
    torch.testing.assert_close(got.cpu(), exp, atol=1e-5, rtol=1e-6)


def _inputs(b, n, dtype, seed, ties=False, neg=0.0, masked=0.0):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn((b, n), generator=g) * 2.0
    if ties:
        s = torch.round(s)           # many exact score ties
    y = torch.randint(0, 4, (b, n), generator=g).float()
    if neg:
        y = torch.where(torch.rand((b, n), generator=g) < neg, torch.full_like(y, -1.0), y)
    mask = torch.rand((b, n), generator=g) >= masked if masked else None
    return s.to(dtype).to(DEV), y.to(DEV), None if mask is None else mask.to(DEV)


def _check(kind, s, y, mask, temperature, reduction, weight=None, upstream=None):
    loss = CLASS[kind](temperature=temperature, reduction=reduction)
    x = s.clone().requires_grad_(True)
    out = loss(y if mask is None else {"labels": y, "mask": mask}, x, sample_weight=weight)
    (out if upstream is None else out * upstream).sum().backward()
    s64 = s.double().requires_grad_(True)
    w64 = None if weight is None else weight.double()
    v64 = RR.unreduced(kind, s64, y.double(), mask, temperature)
    if w64 is not None and w64.dim() > v64.dim():
        w64 = w64.reshape(v64.shape)         # one weight per list, [B, 1], against ListMLE's [B] (keras squeezes it)
    ref = RR.reduce(v64, w64, reduction)
    (ref if upstream is None else ref * upstream.double()).sum().backward()
    n = s.shape[1]
    # the per-element weight the gradient carries (for the magnitudes): upstream * w / divisor
    gw = torch.ones_like(v64)
    if w64 is not None:
        gw = gw * torch.broadcast_to(w64, v64.shape)
    if upstream is not None:
        gw = gw * upstream.double()
    lm, gm = RR.magnitudes(kind, s, y.double(), mask, temperature, gw)
    bound = 4 * (n + 16) * RR.U32
    if reduction == "none":
        ltol = bound * lm * (1.0 if w64 is None else torch.broadcast_to(w64, lm.shape).abs())
        err = (out.double() - ref.detach()).abs()
        assert bool((err <= ltol + 1e-30).all()), f"loss err {float(err.max())} > {float((ltol).max())}"
        scale = 1.0
    else:
        div = {"sum": 1.0}.get(reduction, float(v64.numel()))
        if reduction == "mean_with_sample_weight" and w64 is not None:
            div = float(torch.broadcast_to(w64, v64.shape).sum())
        scale = 1.0 / div if div else 0.0
        ltol = bound * float((lm * (gw.abs() if gw.shape == lm.shape else 1.0)).sum()) * scale * 2 + 1e-6
        assert abs(float(out.detach()) - float(ref.detach())) <= ltol, (float(out.detach()), float(ref.detach()), ltol)
    gtol = bound * gm * scale + 1e-30
    if s.dtype == torch.bfloat16:
        gtol = gtol + 2.0 ** -8 * s64.grad.abs()
    err = (x.grad.double() - s64.grad).abs()
    assert x.grad.dtype == s.dtype
    assert bool((err <= gtol).all()), f"grad err {float(err.max())} at tol {float(gtol.flatten()[err.argmax()])}"


LENGTHS = [1, 2, 5, 63, 64, 65, 256, 2048, 4096]


@pytest.mark.parametrize("kind", list(CLASS))
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_random_against_float64(kind, n, dtype):
    b = {1: 300, 2: 257, 5: 300, 63: 40, 64: 33, 65: 17, 256: 9, 2048: 2, 4096: 1}[n]
    s, y, mask = _inputs(b, n, dtype, seed=n, neg=0.1, masked=0.1)
    _check(kind, s, y, mask, 0.7, "sum_over_batch_size")


@pytest.mark.parametrize("kind", list(CLASS))
@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_reductions_and_weights(kind, reduction):
    s, y, mask = _inputs(37, 24, torch.float32, seed=3, neg=0.1)
    shape = (37,) if kind == "listmle" else (37, 24)
    g = torch.Generator().manual_seed(5)
    for w in (None, torch.tensor(2.5), torch.rand(shape, generator=g), torch.rand((37, 1), generator=g)):
        _check(kind, s, y, mask, 1.0, reduction, None if w is None else w.to(DEV))


@pytest.mark.parametrize("kind", list(CLASS))
def test_none_with_nonuniform_upstream(kind):
    s, y, mask = _inputs(19, 40, torch.float32, seed=11, neg=0.2, masked=0.1)
    shape = (19,) if kind == "listmle" else (19, 40)
    up = (torch.rand(shape, generator=torch.Generator().manual_seed(2)) - 0.3).to(DEV)
    w = torch.rand(shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    _check(kind, s, y, mask, 0.5, "none", w, upstream=up)


@pytest.mark.parametrize("kind", list(CLASS))
def test_invalid_items_ties_and_empty_lists(kind):
    s, y, mask = _inputs(64, 33, torch.float32, seed=7, ties=True, neg=0.3, masked=0.2)
    y[3] = -1.0                      # a list with no valid item
    mask[5] = False                  # another
    _check(kind, s, y, mask, 1.0, "sum")
    x = s.clone().requires_grad_(True)
    out = CLASS[kind](reduction="none")({"labels": y, "mask": mask}, x)
    out.sum().backward()
    invalid = (y < 0) | ~mask
    assert bool((x.grad[invalid] == 0).all())
    assert bool((out[3] == 0).all() and (out[5] == 0).all())


def test_listmle_label_ties_take_index_order():
    # labels tie: the order is index ascending, so the loss is that of the list in its given order
    s = torch.tensor([[0.3, 2.0, -1.0, 0.5]], device=DEV)
    y = torch.tensor([[1.0, 1.0, 1.0, 1.0]], device=DEV)
    got = float(losses.ListMLELoss(reduction="sum")(y, s))
    z = s[0].double().cpu() - 2.0
    exp = sum(float(torch.log(torch.exp(z[r:]).sum() + 1e-10) - z[r]) for r in range(4))
    assert abs(got - exp) < 1e-5
    y2 = torch.tensor([[1.0, 1.0, 2.0, 1.0]], device=DEV)   # item 2 first, then 0, 1, 3
    got2 = float(losses.ListMLELoss(reduction="sum")(y2, s))
    z2 = z[[2, 0, 1, 3]]
    exp2 = sum(float(torch.log(torch.exp(z2[r:]).sum() + 1e-10) - z2[r]) for r in range(4))
    assert abs(got2 - exp2) < 1e-5


def test_exact_gradients_at_non_smooth_points():
    # logistic at a score tie x == 0: gradient 0 (relu'(0) = abs'(0) = 0), not the smooth -0.5
    x = torch.tensor([[1.5, 1.5]], device=DEV, requires_grad=True)
    losses.PairwiseLogisticLoss(reduction="sum")(torch.tensor([[1.0, 0.0]], device=DEV), x).backward()
    assert x.grad.tolist() == [[0.0, 0.0]]
    # hinge at x == 1: gradient 0; just inside (x < 1) it is -1 / +1
    x = torch.tensor([[2.0, 1.0]], device=DEV, requires_grad=True)
    losses.PairwiseHingeLoss(reduction="sum")(torch.tensor([[1.0, 0.0]], device=DEV), x).backward()
    assert x.grad.tolist() == [[0.0, 0.0]]
    x = torch.tensor([[1.5, 1.0]], device=DEV, requires_grad=True)
    losses.PairwiseHingeLoss(reduction="sum")(torch.tensor([[1.0, 0.0]], device=DEV), x).backward()
    assert x.grad.tolist() == [[-1.0, 1.0]]


@pytest.mark.parametrize("kind", list(CLASS))
def test_strided_column_slice(kind):
    s, y, _ = _inputs(12, 80, torch.float32, seed=9)
    wide = torch.randn((12, 200), device=DEV)
    wide[:, 50:130] = s
    view = wide[:, 50:130]
    assert view.stride(0) == 200
    a = CLASS[kind](reduction="none")(y, view)
    b = CLASS[kind](reduction="none")(y, s.contiguous())
    assert torch.equal(a, b)


@pytest.mark.parametrize("kind", list(CLASS))
def test_bit_identical_repeats(kind):
    s, y, mask = _inputs(128, 300, torch.float32, seed=13, neg=0.1)
    res = []
    for _ in range(3):
        x = s.clone().requires_grad_(True)
        out = CLASS[kind]()({"labels": y, "mask": mask} if mask is not None else y, x)
        out.backward()
        res.append((out.detach().clone(), x.grad.clone()))
    for o, g in res[1:]:
        assert torch.equal(o, res[0][0]) and torch.equal(g, res[0][1])


@pytest.mark.parametrize("kind", list(CLASS))
@pytest.mark.parametrize("reduction", ["sum_over_batch_size", "none"])
def test_graph_capture_replays_bit_identically(kind, reduction):
    s, y, _ = _inputs(64, 40, torch.float32, seed=17, neg=0.1)
    loss = CLASS[kind](reduction=reduction)
    x = s.clone().requires_grad_(True)

    def step():
        x.grad = None
        out = loss(y, x)
        out.sum().backward()
        return out

    eager = step().detach().clone()
    eager_g = x.grad.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    x.grad = None
    with torch.cuda.graph(graph):
        out = loss(y, x)
        out.sum().backward()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(x.grad, eager_g)


@pytest.mark.parametrize("kind", list(CLASS))
def test_list_of_4097_raises(kind):
    s = torch.zeros((2, 4097), device=DEV)
    with pytest.raises(KrsError, match="4096"):
        CLASS[kind]()(torch.ones_like(s), s)


def test_no_grad_pass_when_not_needed():
    s, y, _ = _inputs(4, 10, torch.float32, seed=1)
    out = losses.PairwiseLogisticLoss()(y, s)
    assert not out.requires_grad
