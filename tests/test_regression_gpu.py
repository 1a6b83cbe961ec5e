"""K24 on the GPU, over the case table of tests/regression_cases.py: dpred bit for bit against the numpy fp32
restatement of the op order include/krs.h pins (bf16 rounding included); the loss and the batch sums within the bound
the summation order gives (depth x fp32 unit round-off x sum |terms|, tests/regression_restatement.py); the route; the
same bits from call to call, fused and apart, in a group and alone, in a HIP graph and eagerly; autograd through every
reduction; the C ABI called directly; no rows.

Every case prints the fraction of its bounds it used (`-s`); the largest observed over the table, 0.351 (a per-row loss
under reduction "none"; the batch sums reach 0.046), is recorded in DESIGN.md section 4, K24."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import regression_ops
from keras_rs_amd.layers import losses as KL
from keras_rs_amd.layers import metrics as KM
from tests import regression_cases as T
from tests import regression_restatement as R

pytestmark = pytest.mark.gpu
F32 = np.float32
G_SCALE = 0.75        # the upstream gradient of the scalar reductions in the table run: not 1


@functools.lru_cache(maxsize=None)
def _host(name):
    """(tensors, float64 reference, fp32 gradient) of a case: computed once, shared, never written."""
    case = T.BY_NAME[name]
    t = T.tensors(case)
    ref = R.reference64(t["pred"], t["target"], t["weight"], case.kind, T.DELTA, case.reduction)
    g = t["g"] if case.reduction == "none" else G_SCALE
    grad = R.gradient32(t["pred"], t["target"], t["weight"], case.kind, T.DELTA, case.reduction, g=g, dtype=case.dtype)
    for a in list(t.values()) + [grad]:
        if a is not None:
            a.setflags(write=False)
    return t, ref, grad


def _strided(values, dtype, ld, offset):
    """values [b, c] as the first c columns of rows of ld elements, `offset` elements after a 16-byte boundary"""
    b, c = values.shape
    buf = torch.zeros(offset + b * ld + 64, dtype=dtype, device="cuda")
    view = buf[offset:offset + b * ld].as_strided((b, c), (ld, 1)) if b else buf[:0].reshape(0, c)
    view.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(dtype))
    return view


def _device(case):
    t, _, _ = _host(case.name)
    dt = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    ld = case.c + case.pad
    pred = _strided(t["pred"], dt, ld, case.offset)
    target = _strided(t["target"], torch.float32, ld, 0)
    w = None if t["weight"] is None else torch.from_numpy(t["weight"]).cuda()
    g = torch.from_numpy(t["g"]).cuda() if case.reduction == "none" else None
    return pred, target, w, g


def _run(case, want_loss=True, want_grad=True, want_sums=True):
    pred, target, w, g = _device(case)
    sums = torch.full((3,), float("nan"), device="cuda") if want_sums else None
    loss, dp = regression_ops.regression(pred, target, w, case.kind, T.DELTA, case.reduction, g=g,
                                         g_scale=1.0 if g is not None else G_SCALE, want_loss=want_loss,
                                         want_grad=want_grad, sums=sums)
    return loss, dp, sums


def _same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _within(got, want, bound):
    """|got - want| <= bound where want is finite; the same NaN / infinity where it is not"""
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound)
    finite = np.isfinite(want)
    ok = np.array_equal(got[~finite], want[~finite], equal_nan=True) if (~finite).any() else True
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)[finite] if finite.any() else np.zeros(0)
    b = np.broadcast_to(bound, want.shape)[finite]
    frac = float(np.max(err[b > 0] / b[b > 0])) if (b > 0).any() else 0.0
    return ok and bool(np.all(err <= b)), frac


FRACTIONS = {}


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_case(name):
    case = T.BY_NAME[name]
    t, ref, grad = _host(name)
    loss, dp, sums = _run(case)
    route = regression_ops.last_route()
    assert route.kernel == case.route, (route.kernel, route.v, route.blocks)
    if case.b == 0:
        assert tuple(dp.shape) == (0, case.c) and not sums.cpu().numpy().any()
        assert loss.numel() == 0 if case.reduction == "none" else float(loss) == 0.0
        return
    assert route.blocks == R.blocks_for(case.b // route.v)
    got = dp.to(torch.float32).cpu().numpy()
    assert dp.dtype == (torch.bfloat16 if case.dtype == "bf16" else torch.float32)
    assert _same_bits(got, grad), f"dpred differs at {np.argwhere(got != grad)[:4].tolist()}"
    bound, sums_bound = R.bounds(ref, case.b, case.c, case.dtype, case.route == T.VEC, case.reduction, bool(case.weights))
    ok, frac = _within(loss.cpu().numpy(), ref["loss"], bound)
    ok_s, frac_s = _within(sums.cpu().numpy(), ref["sums"], sums_bound)
    FRACTIONS[name] = max(frac, frac_s)
    print(f"{name}: loss {frac:.3f} sums {frac_s:.3f} of the bound; largest so far {max(FRACTIONS.values()):.3f}")
    assert ok, (loss.cpu().numpy(), ref["loss"], bound)
    assert ok_s, (sums.cpu().numpy(), ref["sums"], sums_bound)
    if not case.weights:
        assert float(sums[2]) == float(case.b * case.c)


SAMPLE = ["grid-vec-huber-mean_with_sample_weight-mixed-bf16", "grid-elem-mse-none-mixed-fp32", "two-stage-vec",
          "two-stage-elem-weighted", "c5", "fill-vec-bf16-8193", "nan-mae-elem"]


@pytest.mark.parametrize("name", SAMPLE)
def test_two_calls_give_the_same_bits_and_a_fused_call_equals_its_parts(name):
    case = T.BY_NAME[name]
    loss, dp, sums = _run(case)
    loss2, dp2, sums2 = _run(case)
    for a, b in ((loss, loss2), (dp, dp2), (sums, sums2)):
        assert _same_bits(a.float().cpu().numpy(), b.float().cpu().numpy())
    only_loss, none_a, none_b = _run(case, want_grad=False, want_sums=False)
    none_c, only_dp, none_d = _run(case, want_loss=False, want_sums=False)
    none_e, none_f, only_sums = _run(case, want_loss=False, want_grad=False)
    assert none_a is none_b is none_c is none_d is none_e is none_f is None
    for a, b in ((loss, only_loss), (dp, only_dp), (sums, only_sums)):
        assert _same_bits(a.float().cpu().numpy(), b.float().cpu().numpy())


def _members():
    return [KM.RootMeanSquaredError(), KM.MeanSquaredError(), KM.MeanAbsoluteError()]


def _rating_batch(b=5000, seed=3, dtype=torch.bfloat16):
    gen = torch.Generator().manual_seed(seed)
    y = (torch.randint(1, 11, (b,), generator=gen) * 0.5).cuda()
    p = (y.cpu() + torch.randn(b, generator=gen)).to(dtype).reshape(b, 1).cuda()
    w = torch.rand(b, generator=gen).cuda()
    return y, p, w


def test_a_group_member_has_the_state_it_has_alone_and_the_loss_call_updates_it_too():
    y, p, w = _rating_batch()
    group = KM.RegressionMetricGroup(_members())
    alone = _members()
    through_loss = KM.RegressionMetricGroup(_members())
    loss = KL.MeanSquaredError(metrics=through_loss)
    for weight in (None, w, w):
        group.update_state(y, p, sample_weight=weight)
        for m in alone:
            m.update_state(y, p, sample_weight=weight)
        loss(y, p, sample_weight=weight)
    for a, b, c in zip(group.metrics, alone, through_loss.metrics):
        assert torch.equal(torch.stack(a.variables), torch.stack(b.variables)), a.name
        assert torch.equal(torch.stack(a.variables), torch.stack(c.variables)), a.name
    # and the values are the restatement's
    ref = R.reference64(p.float().cpu().numpy(), y.cpu().numpy().reshape(-1, 1), None, "mse", 1.0, "sum")["sums"]
    refw = R.reference64(p.float().cpu().numpy(), y.cpu().numpy().reshape(-1, 1), w.cpu().numpy(), "mse", 1.0, "sum")["sums"]
    tot = ref + 2 * refw
    got = group.result()
    np.testing.assert_allclose(float(got["mean_squared_error"]), tot[0] / tot[2], rtol=1e-5)
    np.testing.assert_allclose(float(got["root_mean_squared_error"]), np.sqrt(tot[0] / tot[2]), rtol=1e-5)
    np.testing.assert_allclose(float(got["mean_absolute_error"]), tot[1] / tot[2], rtol=1e-5)


def test_a_fused_loss_call_equals_loss_gradient_and_metrics_done_apart():
    y, p, w = _rating_batch(b=70001)
    for cls, kwargs in ((KL.MeanSquaredError, {}), (KL.MeanAbsoluteError, {"reduction": "mean_with_sample_weight"}),
                        (KL.Huber, {"delta": 0.5, "reduction": "sum"})):
        fused_group, apart_group = KM.RegressionMetricGroup(_members()), KM.RegressionMetricGroup(_members())
        pf = p.clone().requires_grad_(True)
        fused = cls(metrics=fused_group, **kwargs)(y, pf, sample_weight=w)
        (gf,) = torch.autograd.grad(fused, pf)
        pa = p.clone().requires_grad_(True)
        apart = cls(**kwargs)(y, pa, sample_weight=w)
        (ga,) = torch.autograd.grad(apart, pa)
        apart_group.update_state(y, p, sample_weight=w)
        assert torch.equal(fused, apart) and torch.equal(gf, ga) and gf.dtype == p.dtype
        for a, b in zip(fused_group.metrics, apart_group.metrics):
            assert torch.equal(torch.stack(a.variables), torch.stack(b.variables)), a.name


def test_graph_replays_equal_eager_updates():
    y, p, w = _rating_batch(b=3 * 1024 + 17)

    def fresh():
        # one warm-up update on a side stream (it allocates the states), then empty states
        group = KM.RegressionMetricGroup(_members())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            group.update_state(y, p, sample_weight=w)
        torch.cuda.current_stream().wait_stream(side)
        group.reset_state()
        return group

    eager = fresh()
    for _ in range(3):
        eager.update_state(y, p, sample_weight=w)
    captured = fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):              # (a host wait anywhere in the update would fail the capture)
        captured.update_state(y, p, sample_weight=w)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager.metrics, captured.metrics):
        assert torch.equal(torch.stack(a.variables), torch.stack(b.variables)), a.name
        assert float(a.variables[1]) != 0.0


@pytest.mark.parametrize("reduction", ["none", None, "sum", "sum_over_batch_size", "mean", "mean_with_sample_weight"])
@pytest.mark.parametrize("cls,kind", [(KL.MeanSquaredError, "mse"), (KL.MeanAbsoluteError, "mae"), (KL.Huber, "huber")])
def test_autograd_grad_through_each_reduction_with_a_non_unit_upstream(cls, kind, reduction):
    b, c = 37, 5
    gen = torch.Generator().manual_seed(11)
    y = torch.randint(-3, 4, (b, c), generator=gen).float()
    p = (y + torch.randn(b, c, generator=gen)).to(torch.float32)
    w = torch.rand(b, generator=gen) + 0.25
    up = torch.rand(b, generator=gen) - 0.5
    pd = p.cuda().requires_grad_(True)
    loss = cls(reduction=reduction)(y.cuda(), pd, sample_weight=w.cuda())
    red = "none" if reduction in (None, "none") else "sum_over_batch_size" if reduction == "mean" else reduction
    if red == "none":
        assert tuple(loss.shape) == (b,)
        (got,) = torch.autograd.grad(loss, pd, grad_outputs=up.cuda())
        want = R.gradient32(p.numpy(), y.numpy(), w.numpy(), kind, 1.0, red, g=up.numpy())
        assert _same_bits(got.cpu().numpy(), want)
    else:
        assert loss.dim() == 0
        (got,) = torch.autograd.grad(loss * 3.0, pd)
        # the forward's gradient at unit upstream, times the incoming scalar: two roundings, as the Function does it
        want = R.gradient32(p.numpy(), y.numpy(), w.numpy(), kind, 1.0, red, g=1.0) * F32(3.0)
        assert _same_bits(got.cpu().numpy(), want)
    # against float64 autograd of the textbook expression
    p64 = p.double().requires_grad_(True)
    e = p64 - y.double()
    f = {"mse": e * e, "mae": e.abs(), "huber": torch.where(e.abs() <= 1.0, 0.5 * e * e, e.abs() - 0.5)}[kind]
    t = w.double() * f.mean(dim=1)
    scalar = {"none": (t * up.double()).sum(), "sum": 3 * t.sum(), "sum_over_batch_size": 3 * t.sum() / b,
              "mean_with_sample_weight": 3 * t.sum() / w.double().sum()}[red]
    (want64,) = torch.autograd.grad(scalar, p64)
    np.testing.assert_allclose(got.cpu().numpy(), want64.numpy(), rtol=1e-5, atol=1e-7)
    ref = R.reference64(p.numpy(), y.numpy(), w.numpy(), kind, 1.0, red)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), ref["loss"], rtol=1e-5)


def test_y_true_gets_no_gradient_and_rank_one_inputs_are_one_row():
    y = torch.tensor([1.0, 2.0, 4.0], device="cuda", requires_grad=True)
    p = torch.tensor([1.5, 2.0, 2.0], device="cuda", requires_grad=True)
    loss = KL.MeanSquaredError(reduction="none")(y, p, sample_weight=2.0)
    assert loss.dim() == 0 and float(loss.detach()) == pytest.approx(2.0 * (0.25 + 4.0) / 3)
    loss.backward()
    assert y.grad is None and torch.equal(p.grad.cpu(), torch.tensor([2.0 * 1.0 / 3, 0.0, 2.0 * -4.0 / 3]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_c_abi_called_directly_with_a_nan_filled_workspace_and_its_own_gradient_stride(dtype):
    b, c, ldp, ldt, ldd = 3000, 3, 5, 4, 7
    gen = torch.Generator().manual_seed(5)
    y = torch.randint(-2, 3, (b, c), generator=gen).float()
    p = (y + torch.randn(b, c, generator=gen)).to(dtype)
    w = torch.rand(b, generator=gen) + 0.5
    pred = torch.zeros(b, ldp, dtype=dtype, device="cuda")
    pred[:, :c] = p.cuda()
    target = torch.full((b, ldt), float("nan"), device="cuda")
    target[:, :c] = y.cuda()
    dpred = torch.full((b, ldd), 7.0, dtype=dtype, device="cuda")
    wd = w.cuda()
    loss = torch.full((), float("nan"), device="cuda")
    sums = torch.full((3,), float("nan"), device="cuda")
    size = regression_ops.workspace_bytes(b, c)
    ws = torch.full((size // 4,), float("nan"), device="cuda")
    rc = L.lib().krs_regression_fwd_bwd(L.REG_HUBER, 0.5, L.REG_MEAN_WITH_SAMPLE_WEIGHT, pred.data_ptr(), ldp,
                                        L.fdtype(pred), target.data_ptr(), ldt, wd.data_ptr(), b, c, None, 2.0,
                                        loss.data_ptr(), dpred.data_ptr(), ldd, sums.data_ptr(), ws.data_ptr(), size,
                                        L.stream_ptr())
    L.check(rc, "krs_regression_fwd_bwd")
    route = L.RegressionRoute()
    assert L.lib().krs_regression_last_route(C.byref(route)) == L.REG_ELEM
    assert (route.v, route.blocks, route.launches) == (1, 3, 3)
    name = "bf16" if dtype == torch.bfloat16 else "fp32"
    want = R.gradient32(p.float().numpy(), y.numpy(), w.numpy(), "huber", 0.5, "mean_with_sample_weight", g=2.0, dtype=name)
    assert _same_bits(dpred[:, :c].float().cpu().numpy(), want)
    assert bool((dpred[:, c:] == 7.0).all())                       # nothing beyond a row's c columns is written
    ref = R.reference64(p.float().numpy(), y.numpy(), w.numpy(), "huber", 0.5, "mean_with_sample_weight")
    bound, sums_bound = R.bounds(ref, b, c, name, False, "mean_with_sample_weight", True)
    assert _within(loss.cpu().numpy(), ref["loss"], bound)[0]
    assert _within(sums.cpu().numpy(), ref["sums"], sums_bound)[0]


def test_no_rows():
    y, p = torch.zeros(0, 1, device="cuda"), torch.zeros(0, 1, device="cuda", requires_grad=True)
    group = KM.RegressionMetricGroup(_members())
    for reduction in ("sum", "sum_over_batch_size", "mean_with_sample_weight"):
        loss = KL.MeanSquaredError(reduction=reduction, metrics=group)(y, p, sample_weight=torch.zeros(0, device="cuda"))
        assert loss.dim() == 0 and float(loss) == 0.0
        (g,) = torch.autograd.grad(loss, p)
        assert tuple(g.shape) == (0, 1)
    assert tuple(KL.Huber(reduction="none")(y, p).shape) == (0,)
    assert all(float(v) == 0.0 for v in group.result().values())


KERAS_Y = [[0.0, 1.0], [0.0, 0.0]]


@pytest.mark.parametrize("cls,pred,kwargs,weight,want", [
    (KL.MeanSquaredError, [[1.0, 1.0], [1.0, 0.0]], {}, None, 0.5),
    (KL.MeanSquaredError, [[1.0, 1.0], [1.0, 0.0]], {}, [0.7, 0.3], 0.25),
    (KL.MeanSquaredError, [[1.0, 1.0], [1.0, 0.0]], {"reduction": "sum"}, None, 1.0),
    (KL.MeanSquaredError, [[1.0, 1.0], [1.0, 0.0]], {"reduction": "none"}, None, [0.5, 0.5]),
    (KL.MeanAbsoluteError, [[1.0, 1.0], [1.0, 0.0]], {}, None, 0.5),
    (KL.Huber, [[0.6, 0.4], [0.4, 0.6]], {}, None, 0.155),
    (KL.Huber, [[0.6, 0.4], [0.4, 0.6]], {}, [1.0, 0.0], 0.09),
    (KL.Huber, [[0.6, 0.4], [0.4, 0.6]], {"reduction": "sum"}, None, 0.31),
    (KL.Huber, [[0.6, 0.4], [0.4, 0.6]], {"reduction": None}, None, [0.18, 0.13]),
])
def test_keras_published_losses(cls, pred, kwargs, weight, want):
    w = None if weight is None else torch.tensor(weight, device="cuda")
    got = cls(**kwargs)(torch.tensor(KERAS_Y, device="cuda"), torch.tensor(pred, device="cuda"), sample_weight=w)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-6)


@pytest.mark.parametrize("cls,weight,want", [(KM.RootMeanSquaredError, None, 0.5), (KM.RootMeanSquaredError, [1.0, 0.0], 0.70710677),
                                             (KM.MeanSquaredError, None, 0.25), (KM.MeanSquaredError, [1.0, 0.0], 0.5)])
def test_keras_published_metrics(cls, weight, want):
    m = cls()
    m.update_state(torch.tensor(KERAS_Y, device="cuda"), torch.tensor([[1.0, 1.0], [0.0, 0.0]], device="cuda"),
                   sample_weight=None if weight is None else torch.tensor(weight, device="cuda"))
    np.testing.assert_allclose(float(m.result()), want, rtol=1e-6)
    m.reset_state()
    assert float(m.result()) == 0.0
