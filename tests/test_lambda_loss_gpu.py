"""K28 on the GPU: the pairwise losses with LambdaRank pair weights against a float64 restatement of include/krs.h's K28
formulas (the [B, L, L] tensors, autograd for the gradient, ranks by (-s, index) on the same stored scores, so the
ranks agree exactly), the options, the degenerate lists, the unchanged default, repeatability and the refusals.

Tolerance (derived, not tuned): K9's bound 4 (n + 16) u on the pair sums (tests/test_ranking_losses_gpu.py, u = 2^-24)
plus the weight's own relative error (min(topn, n) + 32) u from the ideal-DCG sum and the gain / discount roundings,
times the float64 sum of the absolute values of the terms (lambda inside, each term counted with its argument's size
as in ranking_restatement.magnitudes); a bf16 gradient adds one rounding, 2^-8 |ref|."""

import pytest
import torch

from keras_rs_amd import KrsError, losses, ranking_ops
from tests import ranking_restatement as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLASS = {"hinge": losses.PairwiseHingeLoss, "logistic": losses.PairwiseLogisticLoss,
         "soft_zero_one": losses.PairwiseSoftZeroOneLoss}
KINDS = list(CLASS)


def _inputs(b, n, dtype, seed, ties=False, neg=0.1, masked=0.1):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn((b, n), generator=g) * 2.0
    if ties:
        s = torch.round(s)
    y = torch.randint(0, 4, (b, n), generator=g).float()
    y = torch.where(torch.rand((b, n), generator=g) < neg, torch.full_like(y, -1.0), y)
    mask = torch.rand((b, n), generator=g) >= masked
    return s.to(dtype).to(DEV), y.to(DEV), mask.to(DEV)


def _reference(kind, s, y, mask, temperature, lw, g=None):
    """float64 (per-item losses [B, L] autodiff-able in s, loss magnitudes, gradient magnitudes for the item weights g)."""
    b, n = s.shape
    valid = RR._valid(y, mask)
    vp = valid[:, :, None] & valid[:, None, :]
    nv = valid.sum(1, keepdim=True)
    op = lw.operands(y)
    topn = op.topn or n
    r1 = torch.arange(1, n + 2, device=s.device, dtype=torch.float64)
    disc = 1.0 / torch.log2(1.0 + r1) if op.discount is None else op.discount.double()
    gain = torch.pow(2.0, y.double()) - 1.0 if op.gain is None else op.gain.double()
    order = torch.sort(torch.where(valid, s.detach(), torch.full_like(s, -float("inf"))), dim=1, descending=True,
                       stable=True).indices
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(1, n + 1, device=s.device).expand(b, n))
    if op.normalized:
        top = torch.sort(torch.where(valid, gain, torch.full_like(gain, -float("inf"))), dim=1, descending=True).values
        keep = r1[:n] <= torch.clamp(nv, max=topn)
        z = (torch.where(keep, top, torch.zeros_like(top)) * disc[:n]).sum(1, keepdim=True)
        gain = torch.where(z > 0, gain / torch.where(z > 0, z, torch.ones_like(z)), torch.zeros_like(gain))
    dcut = torch.where(r1 <= topn, disc, torch.zeros_like(disc))[rank - 1]
    dist = (rank[:, :, None] - rank[:, None, :]).abs()
    rd = torch.where(dist > 0, (disc[(dist - 1).clamp(min=0)] - disc[dist]).abs(), torch.zeros_like(dcut[:, :, None]))
    sig = op.smooth_fraction
    lam = (gain[:, :, None] - gain[:, None, :]).abs() * ((1 - sig) * (dcut[:, :, None] - dcut[:, None, :]).abs() + sig * rd)
    lam = lam * (torch.minimum(rank[:, :, None], rank[:, None, :]) <= topn)
    w = lam * ((y[:, :, None] > y[:, None, :]) & vp)
    x = (s[:, :, None] - s[:, None, :]) / temperature
    phi = {"hinge": lambda: torch.relu(1.0 - x),
           "logistic": lambda: torch.relu(-x) + torch.log(1.0 + torch.exp(-torch.abs(x))),
           "soft_zero_one": lambda: torch.where(x > 0, 1.0 - torch.sigmoid(x), torch.sigmoid(-x))}[kind]()
    sd = s.detach()
    ax = 1.0 + x.detach().abs() + (sd.abs()[:, :, None] + sd.abs()[:, None, :]) / temperature   # |phi| <= 1 + |x|, |phi'| <= 1
    gi = torch.ones_like(sd) if g is None else torch.broadcast_to(g, s.shape).double().abs()
    gm = ((gi[:, :, None] * w + gi[:, None, :] * w.transpose(1, 2)) * ax).sum(-1) / temperature
    return (phi * w).sum(-1), (w * ax).sum(-1), gm, (4 * (n + 16) + min(topn, n) + 32) * RR.U32


def _check(kind, s, y, mask, lw, temperature=1.0, reduction="sum_over_batch_size", weight=None, upstream=None):
    x = s.clone().requires_grad_(True)
    out = CLASS[kind](temperature=temperature, reduction=reduction, lambda_weights=lw)({"labels": y, "mask": mask}, x,
                                                                                     sample_weight=weight)
    (out if upstream is None else out * upstream).sum().backward()
    s64 = s.double().requires_grad_(True)
    gw = torch.ones(s.shape, dtype=torch.float64, device=s.device)
    if weight is not None:
        gw = gw * weight.double()
    ref_w = None if weight is None else weight.double()
    if upstream is not None:
        gw = gw * upstream.double()
    v64, lm, gm, bound = _reference(kind, s64, y, mask, temperature, lw, gw)
    ref = RR.reduce(v64, ref_w, reduction)
    (ref if upstream is None else ref * upstream.double()).sum().backward()
    scale = 1.0 if reduction in ("none", "sum") else 1.0 / v64.numel()
    err = (out.detach().double() - ref.detach()).abs()
    if reduction == "none":
        tol = bound * lm * (1.0 if ref_w is None else ref_w.abs()) + 1e-30
    else:
        tol = bound * (lm * gw.abs()).sum() * scale * 2 + 1e-6
    gtol = bound * gm * scale + 1e-30
    if s.dtype == torch.bfloat16:
        gtol = gtol + 2.0 ** -8 * s64.grad.abs()
    gerr = (x.grad.double() - s64.grad).abs()
    print(f"{kind} n={s.shape[1]} {s.dtype}: loss {float((err / tol).max()):.3f} grad {float((gerr / gtol).max()):.3f} of the bound")
    assert x.grad.dtype == s.dtype and bool(torch.isfinite(out).all())
    assert bool((err <= tol).all()), f"loss err {float(err.max())}"
    assert bool((gerr <= gtol).all()), f"grad err {float(gerr.max())} at tol {float(gtol.flatten()[gerr.argmax()])}"
    return out.detach(), x.grad


BATCH = {1: 300, 2: 257, 5: 300, 63: 40, 64: 33, 65: 17, 1024: 3, 1025: 2, 4096: 1}   # pack, wave, tpl and maximum boundaries


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", list(BATCH))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ndcg_weights_against_float64(kind, n, dtype):
    s, y, mask = _inputs(BATCH[n], n, dtype, seed=n)
    _check(kind, s, y, mask, losses.NDCGLambdaWeight(), temperature=0.7)


@pytest.mark.parametrize("n", [37, 300])
@pytest.mark.parametrize("topn", [1, 3, 0, 5], ids=["top1", "top3", "topn", "topn+5"])   # 0 / 5: n, n + 5
@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("smooth", [0.0, 0.25])
def test_options(n, topn, normalized, smooth):
    topn = topn if topn in (1, 3) else n + topn
    kind = KINDS[(topn + normalized + int(smooth > 0)) % 3]
    s, y, mask = _inputs(9, n, torch.float32, seed=n + topn)
    _check(kind, s, y, mask, losses.DCGLambdaWeight(topn=topn, normalized=normalized, smooth_fraction=smooth))


@pytest.mark.parametrize("n", [37, 300])
def test_precision_weight_and_callables(n):
    s, y, mask = _inputs(9, n, torch.float32, seed=n)
    _check("logistic", s, y, mask, losses.PrecisionLambdaWeight(3))
    _check("hinge", s, y, mask, losses.NDCGLambdaWeight(topn=7, gain_fn=lambda t: t * t + 0.5, smooth_fraction=0.5,
                                                        rank_discount_fn=lambda r: 1.0 / r))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [20, 70])   # (20: several lists to a wave, with cut rows)
def test_ties_degenerate_lists_none_reduction_and_a_column_slice(kind, n):
    s, y, mask = _inputs(16, n, torch.float32, seed=7, ties=True, neg=0.3, masked=0.2)   # ties: the rank is by index
    y[3] = -1.0          # no valid item
    y[5] = 2.0           # all labels equal
    y[7] = 0.0           # ideal DCG 0
    g = torch.Generator().manual_seed(2)
    up, w = (torch.rand((16, n), generator=g) - 0.3).to(DEV), torch.rand((16, n), generator=g).to(DEV)
    lw = losses.NDCGLambdaWeight(topn=10)
    out, grad = _check(kind, s, y, mask, lw, 0.5, "none", w, up)
    assert not bool(out[[3, 5, 7]].any()) and not bool(grad[[3, 5, 7]].any())
    assert not bool(grad[(y < 0) | ~mask].any())
    wide = torch.randn((16, 200), device=DEV)
    wide[:, 50:50 + n] = s
    both = [CLASS[kind](reduction="none", lambda_weights=lw)({"labels": y, "mask": mask}, v) for v in (wide[:, 50:50 + n], s)]
    assert torch.equal(*both)


@pytest.mark.parametrize("kind", KINDS)
def test_without_lambda_weights_nothing_changes(kind):
    s, y, mask = _inputs(33, 65, torch.bfloat16, seed=3)
    x = s.clone().requires_grad_(True)
    out = CLASS[kind](temperature=0.7, reduction="sum", lambda_weights=None)({"labels": y, "mask": mask}, x)
    out.backward()
    v, dx = ranking_ops.pairwise_loss(kind, s, y, mask, inv_temperature=1.0 / 0.7)   # K9's entry point, as before
    assert torch.equal(out.detach(), v.sum()) and torch.equal(x.grad, dx)


@pytest.mark.parametrize("kind", KINDS)
def test_repeats_and_graph_replays_are_bit_identical(kind):
    s, y, mask = _inputs(40, 300, torch.float32, seed=13)
    loss = CLASS[kind](lambda_weights=losses.NDCGLambdaWeight(topn=10, smooth_fraction=0.25))
    x = s.clone().requires_grad_(True)

    def step():
        x.grad = None
        out = loss({"labels": y, "mask": mask}, x)
        out.backward()
        return out

    eager, eager_g = step().detach().clone(), x.grad.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            assert torch.equal(step().detach(), eager) and torch.equal(x.grad, eager_g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    x.grad = None
    with torch.cuda.graph(graph):
        out = loss({"labels": y, "mask": mask}, x)
        out.backward()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(x.grad, eager_g)


def test_refusals():
    lw = losses.NDCGLambdaWeight()
    for cls in (losses.PairwiseMeanSquaredError, losses.ListMLELoss):
        with pytest.raises(NotImplementedError, match="lambda_weights"):
            cls(lambda_weights=lw)
    s = torch.zeros((2, 4097), device=DEV)
    with pytest.raises(KrsError, match="4096"):
        losses.PairwiseLogisticLoss(lambda_weights=lw)(torch.ones_like(s), s)
    with pytest.raises(ValueError, match="serialized"):
        losses.PairwiseHingeLoss(lambda_weights=losses.DCGLambdaWeight(gain_fn=lambda t: t)).get_config()
    cfg = losses.PairwiseHingeLoss(lambda_weights=losses.NDCGLambdaWeight(topn=5, smooth_fraction=0.5)).get_config()
    assert losses.PairwiseHingeLoss.from_config(cfg).get_config() == cfg
