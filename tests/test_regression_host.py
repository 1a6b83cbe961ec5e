"""K24 without a GPU: the restatement against Keras' published examples and hand-computed gradients; the case table's
coverage; the host planner under the sanitizers and the routes the table claims; every refusal of the entry (they come
before the first launch, so NULL and made-up pointers do); the workspace formula; the classes' argument checks, shape
rule and config round trips; and the bounds' teeth."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers, regression_ops
from keras_rs_amd.layers import losses as KL
from keras_rs_amd.layers import metrics as KM
from tests import regression_cases as T
from tests import regression_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
Y = np.array([[0, 1], [0, 0]], dtype=F32)
P1 = np.array([[1, 1], [1, 0]], dtype=F32)
P2 = np.array([[0.6, 0.4], [0.4, 0.6]], dtype=F32)
P3 = np.array([[1, 1], [0, 0]], dtype=F32)


def _loss(p, y, w, kind, reduction, delta=1.0):
    return R.reference64(p, y, None if w is None else np.asarray(w, dtype=F32), kind, delta, reduction)["loss"]


# ---- (a) Keras' published examples ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,p,w,reduction,want", [
    ("mse", P1, None, "sum_over_batch_size", 0.5),
    ("mse", P1, [0.7, 0.3], "sum_over_batch_size", 0.25),
    ("mse", P1, None, "sum", 1.0),
    ("mse", P1, None, "none", [0.5, 0.5]),
    ("mae", P1, None, "sum_over_batch_size", 0.5),
    ("huber", P2, None, "sum_over_batch_size", 0.155),
    ("huber", P2, [1, 0], "sum_over_batch_size", 0.09),
    ("huber", P2, None, "sum", 0.31),
    ("huber", P2, None, "none", [0.18, 0.13]),
])
def test_the_restatement_gives_keras_published_losses(kind, p, w, reduction, want):
    np.testing.assert_allclose(_loss(p, Y, w, kind, reduction), want, rtol=1e-6)


@pytest.mark.parametrize("w,rmse,mse", [(None, 0.5, 0.25), ([1, 0], 0.70710677, 0.5)])
def test_the_restatement_gives_keras_published_metrics(w, rmse, mse):
    s = R.reference64(P3, Y, None if w is None else np.asarray(w, dtype=F32), "mse", 1.0, "sum")["sums"]
    np.testing.assert_allclose(s[0] / s[2], mse, rtol=1e-6)
    np.testing.assert_allclose(np.sqrt(s[0] / s[2]), rmse, rtol=1e-6)


def test_mean_with_sample_weight_divides_by_the_weights_and_is_zero_for_none():
    assert _loss(P1, Y, [0.7, 0.3], "mse", "mean_with_sample_weight") == pytest.approx(0.5)
    assert _loss(P1, Y, [0.0, 0.0], "mse", "mean_with_sample_weight") == 0.0
    assert _loss(P1, Y, None, "mse", "mean_with_sample_weight") == pytest.approx(0.5)


# ---- (b) hand-computed gradients --------------------------------------------------------------------------------------
def test_hand_computed_gradients_and_the_tie_and_zero_cases():
    y = np.zeros((2, 2), dtype=F32)
    p = np.array([[1.0, -3.0], [0.0, 0.5]], dtype=F32)
    # mse, sum_over_batch_size: 2 e / (C B) = e / 2
    np.testing.assert_array_equal(R.gradient32(p, y, None, "mse", 1.0, "sum_over_batch_size"), p / 2)
    # mae, sum: sign(e) / C, and sign(0) = 0 exactly (not a NaN, not +-1)
    np.testing.assert_array_equal(R.gradient32(p, y, None, "mae", 1.0, "sum"), [[0.5, -0.5], [0.0, 0.5]])
    # huber(delta = 0.5), sum, weights (2, 4): inside e, outside delta sign(e); both give 0.5 at |e| == delta
    got = R.gradient32(p, y, np.array([2, 4], dtype=F32), "huber", 0.5, "sum")
    np.testing.assert_array_equal(got, [[0.5, -0.5], [0.0, 1.0]])
    tie = np.array([[0.5, -0.5]], dtype=F32)
    np.testing.assert_array_equal(R.derivative32(tie, "huber", 0.5), tie)
    np.testing.assert_array_equal(R.derivative32(tie, "huber", 0.5), F32(0.5) * R.sign32(tie))
    # "none" with an upstream vector, mean_with_sample_weight with weights (1, 3): s = w / 4
    np.testing.assert_array_equal(R.gradient32(p, y, None, "mse", 1.0, "none", g=np.array([2, -1], dtype=F32)),
                                  [[2.0, -6.0], [0.0, -0.5]])
    np.testing.assert_array_equal(R.gradient32(p, y, np.array([1, 3], dtype=F32), "mse", 1.0,
                                               "mean_with_sample_weight"), [[0.25, -0.75], [0.0, 0.375]])
    np.testing.assert_array_equal(R.gradient32(p, y, np.zeros(2, dtype=F32), "mse", 1.0, "mean_with_sample_weight"),
                                  np.zeros((2, 2)))


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_nan_error_gives_a_nan_gradient_and_an_infinite_one_keeps_its_sign(kind):
    p = np.array([[np.nan, np.inf, -np.inf]], dtype=F32)
    d = R.gradient32(p, np.zeros((1, 3), dtype=F32), None, kind, 0.5, "sum")
    assert np.isnan(d[0, 0]) and d[0, 1] > 0 and d[0, 2] < 0


def test_bf16_rounding_is_nearest_even_and_keeps_the_specials():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, np.inf, -np.inf, 3.0e38], dtype=F32)
    np.testing.assert_array_equal(R.round_bf16(x)[:6], [1.0, 1.0, 1.015625, -1.0, np.inf, -np.inf])
    assert np.isnan(R.round_bf16(np.array([np.nan], dtype=F32))[0])
    got = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    np.testing.assert_array_equal(R.round_bf16(x), got)


def test_the_ordered_sum_is_the_stated_order():
    # 2049 values: three workgroups, one round
    x = np.zeros(2049, dtype=F32)
    x[0], x[512], x[1024], x[2048] = 1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24
    # tree of workgroup 0: x[0] + x[512] = 1 (the half ulp is lost); partials 1, 2^-24, 2^-24 in order: each is lost
    assert R.ordered_sum32(x) == F32(1.0)
    assert R.ordered_sum32(x[::-1].copy()) > F32(1.0)                       # the small ones first add up
    assert R.blocks_for(0) == 1 and R.blocks_for(1024) == 1 and R.blocks_for(1025) == 2 and R.blocks_for(10 ** 9) == 256


# ---- (c) the table's coverage -----------------------------------------------------------------------------------------
def test_the_case_table_reaches_what_it_claims():
    grid = {(c.kind, c.reduction, bool(c.weights), c.dtype, c.route) for c in T.CASES}
    assert grid == {(k, r, w, d, route) for k in R.KINDS for r in R.REDUCTIONS for w in (False, True)
                    for d in ("fp32", "bf16") for route in (T.VEC, T.ELEM)} | {(c.kind, c.reduction, bool(c.weights),
                                                                               c.dtype, 0) for c in T.CASES if c.b == 0}
    for route in (T.VEC, T.ELEM):
        assert {0, 1, 63, 64, 65} <= {c.b for c in T.CASES if c.route in (route, 0)}
    rows = {(c.b, c.dtype, c.route) for c in T.CASES}
    assert {(1024, "fp32", T.ELEM), (1025, "fp32", T.ELEM), (4096, "fp32", T.VEC), (4097, "fp32", T.VEC),
            (8192, "bf16", T.VEC), (8193, "bf16", T.VEC)} <= rows
    full = L.REG_MAX_BLOCKS * L.REG_THREADS + 1
    assert any(c.b == full and c.route == T.ELEM for c in T.CASES)
    assert any(c.b // 4 == full and c.b % 4 and c.route == T.VEC and c.dtype == "fp32" for c in T.CASES)
    assert any(c.b >= full and c.weights and c.reduction == "mean_with_sample_weight" for c in T.CASES)
    assert {1, 3, 5, 300} <= {c.c for c in T.CASES}
    assert any(c.pad for c in T.CASES) and any(c.offset for c in T.CASES)
    assert any(c.weights == "zero" and c.reduction == "mean_with_sample_weight" for c in T.CASES)
    assert {"nan", "inf"} <= {c.special for c in T.CASES}
    for case in T.CASES:
        t = T.tensors(case)
        assert t["pred"].shape == (case.b, case.c) and t["target"].dtype == F32 and t["pred"].dtype == F32
        if case.dtype == "bf16":
            np.testing.assert_array_equal(R.round_bf16(t["pred"]), t["pred"])       # already rounded
        if case.b * case.c >= 6:
            e = (t["pred"] - t["target"]).reshape(-1)
            assert e[0] == T.DELTA and e[1] == -T.DELTA and e[2] == 0 and e[3] > T.DELTA and 0 < -e[4] < T.DELTA
            assert case.special != "nan" or np.isnan(e[5])
            assert case.special != "inf" or np.isposinf(e[5])
        if case.weights == "mixed" and case.b >= 3:
            assert (t["weight"] == 0).any() and (t["weight"] < 0).any() and t["weight"].sum() > 0.1 * case.b
        if case.weights == "zero":
            assert not t["weight"].any()


# ---- (d) the planner --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tests/host/regression_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("regression_plan") / "regression_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "regression_plan_check.cpp"),
                    "-o", exe], check=True)

    def ask(*args):
        run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
        lines = run.stdout.strip().splitlines()
        assert " 0 failed checks" in lines[-1]
        return [list(map(int, line.split())) for line in lines[:-1]]

    return ask


def test_the_planner_keeps_its_invariants_under_the_sanitizers_and_knows_the_stated_geometry(planner):
    assert planner() == []
    ws = 5 * L.REG_MAX_BLOCKS * 4
    # RED DTYPE B C LDP LDT LDD MISALIGN HAS_W HAS_DPRED -> status kernel v blocks launches workspace
    assert planner(2, 0, 4096, 1, 1, 1, 1, 0, 0, 1) == [[0, L.REG_VEC, 4, 1, 1, ws]]
    assert planner(2, 1, 65536, 1, 1, 1, 1, 0, 0, 1) == [[0, L.REG_VEC, 8, 8, 2, ws]]
    assert planner(3, 0, 1 << 22, 1, 1, 1, 1, 0, 1, 1) == [[0, L.REG_VEC, 4, 256, 3, ws]]
    assert planner(3, 0, 1 << 22, 1, 1, 1, 1, 0, 0, 1) == [[0, L.REG_VEC, 4, 256, 2, ws]]       # no weights: no W pass
    assert planner(2, 0, 4096, 1, 1, 1, 1, 1, 0, 1) == [[0, L.REG_ELEM, 1, 4, 2, ws]]           # pred off 16 bytes
    assert planner(2, 0, 4096, 1, 1, 1, 1, 8, 0, 0) == [[0, L.REG_VEC, 4, 1, 1, ws]]            # (no dpred: not asked)
    assert planner(2, 0, 4096, 1, 2, 1, 1, 0, 0, 1) == [[0, L.REG_ELEM, 1, 4, 2, ws]]           # a row stride of 2
    assert planner(2, 0, 65536, 5, 5, 5, 5, 0, 0, 1) == [[0, L.REG_ELEM, 1, 64, 2, ws]]
    assert planner(2, 0, 3, 1, 1, 1, 1, 0, 0, 1) == [[0, L.REG_VEC, 4, 1, 1, ws]]               # tail rows only
    assert planner(2, 0, 0, 1, 1, 1, 1, 0, 0, 1) == [[0, 0, 0, 0, 0, 0]]
    assert planner(2, 0, 8, 5, 4, 5, 5, 0, 0, 1)[0][0] == -1                                     # KRS_ERR_INVALID


def _fake(n, off=0):
    return 0x7f0000001000 + 0x100000 * n + off


def _plan_route(case, dpred=True):
    """krs_regression_plan_route for a table case with made-up addresses laid out as the GPU test lays them out."""
    from keras_rs_amd.build import build

    build()
    route = L.RegressionRoute()
    esize = 2 if case.dtype == "bf16" else 4
    ld = case.c + case.pad
    rc = L.lib().krs_regression_plan_route(
        regression_ops.REDUCTION_CODES[case.reduction], _fake(0, case.offset * esize), ld,
        L.BF16 if case.dtype == "bf16" else L.F32, _fake(1), ld, _fake(2) if case.weights else None, case.b, case.c,
        None, _fake(3), _fake(4) if dpred else None, case.c, C.byref(route))
    return rc, route


def test_the_routes_the_table_claims_are_the_planners():
    for case in T.CASES:
        rc, route = _plan_route(case)
        assert rc == 0 and route.kernel == case.route, case.name
        assert route.v == (0 if case.b == 0 else 1 if case.route == T.ELEM else R.vec_rows(case.dtype))
        if case.b:
            assert route.blocks == R.blocks_for(case.b // route.v)


# ---- (e) refusals, (f) workspace --------------------------------------------------------------------------------------
def _entry(kind=0, delta=1.0, reduction=2, pred=_fake(0), ldp=1, dtype=0, target=_fake(1), ldt=1, w=None, b=8, c=1, g=None,
           g_scale=1.0, loss=_fake(3), dpred=_fake(4), ldd=1, sums=None, ws=_fake(5), ws_bytes=1 << 20):
    from keras_rs_amd.build import build

    build()
    rc = L.lib().krs_regression_fwd_bwd(kind, delta, reduction, pred, ldp, dtype, target, ldt, w, b, c, g, g_scale, loss,
                                        dpred, ldd, sums, ws, ws_bytes, None)
    return rc, L.lib().krs_last_error().decode()


@pytest.mark.parametrize("kwargs,word", [
    (dict(kind=3), "kind 3"), (dict(kind=-1), "kind -1"),
    (dict(reduction=4), "reduction"), (dict(reduction=-1), "reduction"),
    (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"),
    (dict(kind=2, delta=0.0), "delta 0"), (dict(kind=2, delta=-1.0), "delta -1"), (dict(kind=2, delta=float("nan")), "delta"),
    (dict(b=-1), "b -1"), (dict(c=0), "c 0"), (dict(b=1 << 31), "b 2147483648"), (dict(c=1 << 31, ldp=1 << 31, ldt=1 << 31,
                                                                                    ldd=1 << 31), "c 2147483648"),
    (dict(c=5, ldp=4, ldt=5, ldd=5), "ld_pred 4"), (dict(c=5, ldp=5, ldt=4, ldd=5), "ld_target 4"),
    (dict(c=5, ldp=5, ldt=5, ldd=4), "ld_dpred 4"),
    (dict(pred=None), "null"), (dict(target=None), "null"), (dict(loss=None, dpred=None), "null outputs"),
])
def test_the_entry_refuses_with_the_value_named(kwargs, word):
    rc, text = _entry(**kwargs)
    assert rc == -1 and "krs_regression_fwd_bwd" in text and word in text, text      # KRS_ERR_INVALID


def test_the_entry_refuses_a_small_or_missing_workspace_and_accepts_no_rows():
    need = regression_ops.workspace_bytes(8, 1)
    assert need == 5 * L.REG_MAX_BLOCKS * 4 == regression_ops.workspace_bytes(1 << 22, 5)
    assert regression_ops.workspace_bytes(0, 1) == 0 == regression_ops.workspace_bytes(-3, 1)
    for kwargs in (dict(ws_bytes=need - 1), dict(ws=None)):
        rc, text = _entry(**kwargs)
        assert rc == -4 and "workspace" in text and str(need) in text        # KRS_ERR_WORKSPACE
    # b == 0 is a successful no-op that needs nothing: not a pointer, not a workspace
    assert _entry(b=0, pred=None, target=None, loss=None, dpred=None, ws=None, ws_bytes=0)[0] == 0
    assert L.lib().krs_regression_last_route(None) == 0
    # a delta that Huber would refuse is not read by the other kinds
    assert _entry(kind=0, delta=-1.0, b=0)[0] == 0


# ---- (g) the classes --------------------------------------------------------------------------------------------------
LOSSES = (KL.MeanSquaredError, KL.MeanAbsoluteError, KL.Huber)
METRICS = (KM.RootMeanSquaredError, KM.MeanSquaredError, KM.MeanAbsoluteError)


def test_the_classes_are_exported():
    assert layers.MeanSquaredError is KL.MeanSquaredError and layers.Huber is KL.Huber
    assert layers.MeanAbsoluteError is KL.MeanAbsoluteError and layers.RootMeanSquaredError is KM.RootMeanSquaredError
    assert layers.MeanSquaredErrorMetric is KM.MeanSquaredError and layers.MeanAbsoluteErrorMetric is KM.MeanAbsoluteError
    assert layers.RegressionMetricGroup is KM.RegressionMetricGroup


@pytest.mark.parametrize("cls", LOSSES)
def test_loss_arguments_and_config_round_trip(cls):
    with pytest.raises(ValueError, match="reduction"):
        cls(reduction="average")
    with pytest.raises(ValueError, match="float32"):
        cls(dtype="float64")
    with pytest.raises(ValueError, match="metrics"):
        cls(metrics=KM.BinaryAccuracy())
    loss = cls(reduction="sum", name="mine")
    again = cls.from_config(loss.get_config())
    assert again.get_config() == loss.get_config() and again.name == "mine" and again.reduction == "sum"
    assert cls().reduction == "sum_over_batch_size"
    assert cls().name == {"MeanSquaredError": "mean_squared_error", "MeanAbsoluteError": "mean_absolute_error",
                          "Huber": "huber_loss"}[cls.__name__]
    for reduction in (None, "none", "mean", "mean_with_sample_weight"):
        assert cls(reduction=reduction).reduction == reduction


def test_huber_delta():
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="delta"):
            KL.Huber(delta=bad)
    assert KL.Huber().delta == 1.0
    assert KL.Huber.from_config(KL.Huber(delta=0.25).get_config()).delta == 0.25


@pytest.mark.parametrize("cls", LOSSES)
def test_the_shape_rule_and_the_cpu_refusal(cls):
    loss = cls()
    b = 4
    for yt, yp in (((b,), (b, 2)), ((b, 2), (b, 3)), ((b,), (b + 1,)), ((b, 1, 1), (b,)), ((b, 2), (b, 2, 2))):
        with pytest.raises(ValueError, match="same shape"):
            loss(torch.zeros(yt), torch.zeros(yp))
    with pytest.raises(ValueError, match="sample_weight"):
        loss(torch.zeros(b, 1), torch.zeros(b, 1), sample_weight=torch.ones(b + 1))
    with pytest.raises(ValueError, match="scalar"):
        loss(torch.zeros(b), torch.zeros(b), sample_weight=torch.ones(b))        # rank 1 is ONE row
    # the shapes the rule accepts get as far as the device check: there is no CPU fallback
    for yt, yp in (((b,), (b, 1)), ((b, 1), (b,)), ((b, 1), (b, 1)), ((b, 5), (b, 5)), ((b,), (b,)), ((2, b, 3), (2, b, 3))):
        with pytest.raises(L.KrsError, match="no CPU fallback"):
            loss(torch.zeros(yt), torch.zeros(yp))


def test_standardize_keeps_rows_and_never_broadcasts_a_vector_against_a_column():
    y, p, w, shape = regression_ops.standardize(torch.arange(4.0), torch.zeros(4, 1), torch.ones(4), "t")
    assert tuple(y.shape) == tuple(p.shape) == (4, 1) and tuple(w.shape) == (4,) and shape == (4,)
    y, p, w, shape = regression_ops.standardize(torch.zeros(5), torch.zeros(5), 2.0, "t")
    assert tuple(p.shape) == (1, 5) and shape == () and tuple(w.shape) == (1,) and float(w[0]) == 2.0
    y, p, w, shape = regression_ops.standardize(torch.zeros(2, 3, 5), torch.zeros(2, 3, 5), torch.ones(2), "t")
    assert tuple(p.shape) == (6, 5) and shape == (2, 3) and tuple(w.shape) == (6,)
    y, p, _, _ = regression_ops.standardize(torch.zeros(3, 1, dtype=torch.int64), torch.zeros(3, dtype=torch.float64), None, "t")
    assert y.dtype == torch.float32 and p.dtype == torch.float32 and tuple(p.shape) == (3, 1)
    assert regression_ops.standardize([1.0, 2.0], torch.zeros(2, dtype=torch.bfloat16), None, "t")[1].dtype == torch.bfloat16


@pytest.mark.parametrize("cls", METRICS)
def test_metric_arguments_state_and_config(cls):
    with pytest.raises(ValueError, match="float32"):
        cls(dtype="float16")
    m = cls()
    assert m.name == {"RootMeanSquaredError": "root_mean_squared_error", "MeanSquaredError": "mean_squared_error",
                      "MeanAbsoluteError": "mean_absolute_error"}[cls.__name__]
    assert float(m.result()) == 0.0 and len(m.variables) == 2
    again = cls.from_config(cls(name="other").get_config())
    assert again.name == "other" and again.get_config() == {"name": "other", "dtype": "float32"}
    m.reset_state()
    with pytest.raises(ValueError, match="same shape"):
        m.update_state(torch.zeros(4), torch.zeros(4, 2))
    with pytest.raises(L.KrsError, match="no CPU fallback"):
        m.update_state(torch.zeros(4), torch.zeros(4, 1))
    # result() from a state: RMSE takes the root
    m._state = torch.tensor([8.0, 2.0])
    assert float(m.result()) == (2.0 if cls is KM.RootMeanSquaredError else 4.0)
    m._state = torch.tensor([8.0, 0.0])
    assert float(m.result()) == 0.0


def test_group_arguments_and_the_sums_each_member_adds():
    with pytest.raises(ValueError, match="RegressionMetricGroup takes"):
        KM.RegressionMetricGroup([KM.BinaryAccuracy()])
    with pytest.raises(ValueError, match="at least one"):
        KM.RegressionMetricGroup([])
    with pytest.raises(ValueError, match="distinct names"):
        KM.RegressionMetricGroup([KM.MeanSquaredError(), KM.MeanSquaredError()])
    members = [KM.RootMeanSquaredError(), KM.MeanSquaredError(), KM.MeanAbsoluteError()]
    group = KM.RegressionMetricGroup(members)
    group._add(torch.tensor([4.0, 6.0, 2.0]))
    group._add(torch.tensor([4.0, 6.0, 2.0]))
    got = group.result()
    assert sorted(got) == ["mean_absolute_error", "mean_squared_error", "root_mean_squared_error"]
    assert float(got["root_mean_squared_error"]) == pytest.approx(2.0 ** 0.5)
    assert float(got["mean_squared_error"]) == 2.0 and float(got["mean_absolute_error"]) == 3.0
    assert [float(v) for v in members[2].variables] == [12.0, 4.0]
    group.reset_state()
    assert all(float(v) == 0.0 for m in members for v in m.variables)


def test_the_ops_refuse_a_bad_kind_and_cpu_tensors():
    with pytest.raises(ValueError, match="kind"):
        regression_ops.regression(torch.zeros(2, 1), torch.zeros(2, 1), None, "logcosh")
    with pytest.raises(L.KrsError, match="no CPU fallback"):
        regression_ops.regression(torch.zeros(2, 1), torch.zeros(2, 1), None, "mse")


# ---- (h) the bounds have teeth ----------------------------------------------------------------------------------------
def test_the_bounds_tell_mae_from_huber_and_a_dropped_weight_from_the_reference():
    told_kind = told_weight = told_c = 0
    for case in T.CASES:
        if case.b == 0 or case.special or case.b > 10000:
            continue
        t = T.tensors(case)
        vec = case.route == T.VEC
        ref = R.reference64(t["pred"], t["target"], t["weight"], case.kind, T.DELTA, case.reduction)
        bound, sums_bound = R.bounds(ref, case.b, case.c, case.dtype, vec, case.reduction, bool(case.weights))
        assert np.all(np.asarray(bound) < 1e-3 * (1 + np.abs(ref["loss"]))), case.name      # a bound, not a shrug
        if case.kind in ("mae", "huber"):
            other = R.reference64(t["pred"], t["target"], t["weight"], "huber" if case.kind == "mae" else "mae", T.DELTA,
                                  case.reduction)
            told_kind += bool(np.any(np.abs(other["loss"] - ref["loss"]) > bound))
        if case.weights == "mixed":
            other = R.reference64(t["pred"], t["target"], None, case.kind, T.DELTA, case.reduction)
            told_weight += bool(np.any(np.abs(other["loss"] - ref["loss"]) > bound))
            assert np.any(np.abs(other["sums"] - ref["sums"]) > sums_bound), case.name
        if case.c > 1:      # the mean over the last axis forgotten
            told_c += bool(np.any(np.abs(ref["loss"] * case.c - ref["loss"]) > bound))
    assert told_kind >= 30 and told_weight >= 30 and told_c >= 20
