"""K12 on the device (csrc/binary_metric.hip through keras_rs_amd.layers.BinaryAccuracy / AUC / BinaryMetricGroup)
against the numpy restatement (tests/binary_metric_restatement.py) and keras' published answers
(tests/golden/binary_metrics.json).

Where the weights are absent or multiples of 1/8 in [0, 4] and n < 2^18, every partial sum is a multiple of 1/8 below
2^21 and so exact in fp32: states must then be BIT-equal to the restatement's float64 sums, whatever the summation
order.  With other weights the order matters, and the tests ask for the same bits from run to run, in and out of a
group, in and out of a HIP graph."""

import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import keras_rs_amd.layers as kl
from keras_rs_amd import metric_ops
from tests import binary_metric_restatement as BR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "binary_metrics.json")))
C = metric_ops.BINARY_CHUNK
GROUPS = 256                                   # KRS_BINARY_METRIC_GROUPS
SIZES = [1, 4, C - 1, C, C + 1, 3 * C + 17]
EXPLICIT = [0.6, 0.2, 0.9, 0.2, 0.45]          # unsorted, one duplicate: T = 7 with the end points
STATE_KEYS = ("tp", "fp", "tn", "fn")


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _states(m):
    return [v.cpu().numpy() for v in m.variables]


def _thresholds32(m, even):
    return None if even else np.asarray(m.thresholds, np.float32)


def _edge_predictions(thresholds64):
    """0, 1, the clamp cases, and every threshold rounded to fp32 with its two fp32 neighbours."""
    t = np.asarray(thresholds64, np.float64).astype(np.float32)
    edges = np.concatenate([t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))])
    return np.concatenate([np.array([0.0, 1.0, -0.25, 1.5, np.nan], np.float32), edges.astype(np.float32)])


def _inputs(edges, n, seed, weighted):
    """n predictions (the edge cases first, in a shuffled order, then uniform ones), labels with 30 % positives and a
    few that are neither 0 nor 1, and weights that are multiples of 1/8 in [0, 4] (or None)."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([rng.permutation(edges), rng.uniform(-0.05, 1.05, max(n - len(edges), 0)).astype(np.float32)])
    p = pool[:n].astype(np.float32)
    y = (rng.uniform(size=n) < 0.3).astype(np.float32)
    odd = rng.uniform(size=n) < 0.05
    y[odd] = rng.choice(np.array([2.0, 0.5, -1.0], np.float32), size=int(odd.sum()))
    w = (rng.integers(0, 33, n) / 8.0).astype(np.float32) if weighted else None
    return p, y, w


def _check_exact(metric, acc, p32, y, w, even, from_logits=False):
    """metric (an AUC) and acc (a BinaryAccuracy) hold one update of (y, p32, w): bit-equal to the restatement."""
    exp = BR.confusion(y, p32, w, metric.num_thresholds, _thresholds32(metric, even), from_logits)
    for got, e, key in zip(_states(metric), exp, STATE_KEYS):
        assert np.array_equal(e.astype(np.float32).astype(np.float64), e), "the expected sums are exact in fp32"
        assert np.array_equal(got, e.astype(np.float32)), (key, metric.num_thresholds, len(p32))
    if acc is not None:
        total, count = BR.accuracy(y, p32, w, acc.threshold)
        assert [float(v) for v in acc.variables] == [total, count], len(p32)


# ---- keras' published answers -------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", GOLD["auc"]["cases"], ids=lambda c: str(c["weights"]))
def test_golden_auc_rows(c):
    a = GOLD["auc"]
    y, p = _dev(np.asarray(a["y_true"], np.float32)), _dev(np.asarray(a["y_pred"], np.float32))
    w = None if c["weights"] is None else _dev(np.asarray(c["weights"], np.float32))
    for key, expected in c["results"].items():
        curve, method = key.split("/")
        m = kl.AUC(num_thresholds=a["num_thresholds"], curve=curve, summation_method=method)
        m.update_state(y, p, sample_weight=w)
        if c["state"] is not None:
            for got, k in zip(_states(m), STATE_KEYS):
                assert got.tolist() == c["state"][k], (key, k)
        r = m.result()
        assert r.dtype == torch.float32 and r.dim() == 0 and r.is_cuda
        assert abs(float(r) - expected) <= GOLD["atol"] + GOLD["rtol"] * abs(expected), (key, float(r))


@pytest.mark.parametrize("c", GOLD["binary_accuracy"]["cases"], ids=lambda c: str(c["weights"]))
def test_golden_binary_accuracy_rows(c):
    b = GOLD["binary_accuracy"]
    y, p = _dev(np.asarray(b["y_true"], np.float32)), _dev(np.asarray(b["y_pred"], np.float32))
    w = None if c["weights"] is None else _dev(np.asarray(c["weights"], np.float32))
    m = kl.BinaryAccuracy(threshold=b["threshold"])
    r = m(y, p, sample_weight=w)
    assert r.dtype == torch.float32 and r.dim() == 0 and r.is_cuda
    assert abs(float(r) - c["result"]) <= GOLD["atol"]
    total, count = BR.accuracy(b["y_true"], b["y_pred"], c["weights"], b["threshold"])
    assert [float(v) for v in m.variables] == [total, count]


# ---- exact states -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "eighths"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T", [2, 3, 200, 201, 2048])
def test_even_threshold_states_are_exact(T, dtype, weighted):
    edges = _edge_predictions(BR.default_thresholds(T))
    sizes = list(SIZES)
    if len(edges) > SIZES[-1]:
        sizes.append(len(edges))               # (every edge of the longest list in one update)
    if T == 200:
        sizes.append((GROUPS + 3) * C + 17)    # more chunks than workgroups: a workgroup adds several chunks
    for n in sizes:
        p, y, w = _inputs(edges, n, 1000 * T + n, weighted)
        pd = _dev(p, dtype)
        auc, acc = kl.AUC(num_thresholds=T), kl.BinaryAccuracy()
        kl.BinaryMetricGroup([acc, auc]).update_state(_dev(y), pd, sample_weight=None if w is None else _dev(w))
        _check_exact(auc, acc, pd.float().cpu().numpy(), y, w, even=T >= 3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_explicit_threshold_states_are_exact(dtype):
    wrapped = [0.0 - 1e-7] + sorted(EXPLICIT) + [1.0 + 1e-7]
    edges = _edge_predictions(wrapped)
    for n in SIZES:
        for weighted in (False, True):
            p, y, w = _inputs(edges, n, 7000 + n, weighted)
            pd = _dev(p, dtype)
            auc, acc = kl.AUC(thresholds=EXPLICIT), kl.BinaryAccuracy(threshold=0.45)
            assert auc.num_thresholds == 7
            kl.BinaryMetricGroup([acc, auc]).update_state(_dev(y), pd, sample_weight=None if w is None else _dev(w))
            _check_exact(auc, acc, pd.float().cpu().numpy(), y, w, even=False)


def test_from_logits_states_are_exact():
    """Logits in [-12, 12].  fp32 sigmoids of two correct implementations differ by a few ulp (relative 1e-6 at the
    most), that is by at most 2e-4 in p * (T - 1) <= 199: logits whose exact sigmoid lies within 1e-3 of a bucket
    edge are left out (0.2 % of them), and every other one has one bucket whatever the last bits of expf are."""
    T, n = 200, 3 * C + 17
    rng = np.random.default_rng(23)
    x = rng.uniform(-12, 12, 2 * n).astype(np.float32)
    x = np.concatenate([np.array([-12.0, 12.0, 0.0], np.float32), x])
    frac = (1.0 / (1.0 + np.exp(-x.astype(np.float64)))) * (T - 1)
    x = x[np.abs(frac - np.round(frac)) > 1e-3][:n]
    assert len(x) == n
    y = (rng.uniform(size=n) < 0.3).astype(np.float32)
    for w in (None, (rng.integers(0, 33, n) / 8.0).astype(np.float32)):
        auc, acc = kl.AUC(num_thresholds=T, from_logits=True), kl.BinaryAccuracy(threshold=0.0)
        kl.BinaryMetricGroup([acc, auc]).update_state(_dev(y), _dev(x), sample_weight=None if w is None else _dev(w))
        _check_exact(auc, acc, x, y, w, even=True, from_logits=True)


# ---- results ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scored():
    """5000 predictions with 30 % positives, their exact state (float64 restatement) and the device state."""
    rng = np.random.default_rng(5)
    n = 5000
    y = (rng.uniform(size=n) < 0.3).astype(np.float32)
    p = np.clip(rng.normal(0.35 + 0.25 * y, 0.2), 0, 1).astype(np.float32)
    m = kl.AUC()
    m.update_state(_dev(y), _dev(p))
    return BR.confusion(y, p, None, 200), torch.stack(m.variables).clone()


@pytest.mark.parametrize("method", ["interpolation", "minoring", "majoring"])
@pytest.mark.parametrize("curve", ["ROC", "PR"])
def test_results_match_float64(scored, curve, method):
    exact, state = scored
    m = kl.AUC(curve=curve, summation_method=method)
    m._device_state(torch.device(DEV)).copy_(state)
    expected = BR.auc_from_confusion(*exact, curve, method)
    got = float(m.result())
    print(f"{curve}/{method}: device {got!r} float64 {expected!r} error {abs(got - expected):.3e}")
    assert 0.5 < expected < 0.9
    assert abs(got - expected) <= 1e-5 + 1e-5 * abs(expected)


# ---- determinism --------------------------------------------------------------------------------------------------

def _members():
    return [kl.BinaryAccuracy(), kl.AUC(), kl.AUC(num_thresholds=1000, curve="PR", name="pr_1000"),
            kl.AUC(thresholds=EXPLICIT, name="explicit"), kl.AUC(num_thresholds=2048, from_logits=True, name="logits")]


def _random_inputs(n, seed):
    rng = np.random.default_rng(seed)
    y = (rng.uniform(size=n) < 0.3).astype(np.float32)
    p = rng.uniform(-0.05, 1.05, n).astype(np.float32)
    w = rng.uniform(0.05, 3.0, n).astype(np.float32)      # not dyadic: the order of a sum shows in its last bits
    return _dev(y), _dev(p), _dev(w), (y, p, w)


@pytest.mark.parametrize("n", [3 * C + 17, (GROUPS + 3) * C + 17])
def test_runs_and_group_members_are_bit_identical(n):
    y, p, w, _ = _random_inputs(n, 31)
    runs = []
    for _ in range(2):
        group = kl.BinaryMetricGroup(_members())
        group.update_state(y, p, sample_weight=w)
        runs.append([torch.stack(m.variables).clone() for m in group.metrics])
    alone = []
    for m in _members():
        m.update_state(y, p, sample_weight=w)
        alone.append(torch.stack(m.variables).clone())
    for a, b, c, m in zip(runs[0], runs[1], alone, _members()):
        assert torch.equal(a, b), f"{m.name}: two runs differ"
        assert torch.equal(a, c), f"{m.name}: in a group and alone differ"
        assert float(a.sum()) > 0


def test_three_accumulated_updates_match_the_restatement():
    n = C + 1
    group = kl.BinaryMetricGroup(_members()[:2])
    acc, auc = group.metrics
    exp_state, exp_acc = np.zeros((4, 200)), np.zeros(2)
    for step in range(3):
        y, p, w, (yn, pn, wn) = _random_inputs(n, 40 + step)
        group.update_state(y, p, sample_weight=w)
        exp_state += np.stack(BR.confusion(yn, pn, wn, 200))
        exp_acc += np.asarray(BR.accuracy(yn, pn, wn, 0.5))
    np.testing.assert_allclose(np.stack(_states(auc)), exp_state, rtol=1e-5, atol=0)
    np.testing.assert_allclose([float(v) for v in acc.variables], exp_acc, rtol=1e-5, atol=0)
    results = group.result()
    assert sorted(results) == ["auc", "binary_accuracy"]
    np.testing.assert_allclose(float(results["auc"]), BR.auc_from_confusion(*exp_state), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(float(results["binary_accuracy"]), exp_acc[0] / exp_acc[1], rtol=1e-5)
    group.reset_state()
    assert not torch.stack(auc.variables).any() and float(acc.result()) == 0.0


# ---- HIP graph ----------------------------------------------------------------------------------------------------

def test_graph_replays_equal_eager_updates():
    y, p, w, _ = _random_inputs(3 * C + 17, 53)

    def fresh():
        # one warm-up update on a side stream (it allocates the states and uploads the thresholds), then empty states
        group = kl.BinaryMetricGroup(_members())
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
        assert torch.equal(a.result(), b.result()), a.name
        assert float(torch.stack(a.variables).sum()) > 0


# ---- input forms --------------------------------------------------------------------------------------------------

def test_input_forms():
    n = C + 1
    y, p, w, _ = _random_inputs(n, 61)

    def state(y_, p_, sw):
        group = kl.BinaryMetricGroup(_members()[:2])
        group.update_state(y_, p_, sample_weight=sw)
        return torch.cat([torch.stack(m.variables).reshape(-1) for m in group.metrics])

    base = state(y, p, None)
    assert torch.equal(state(y[:, None], p[:, None], None), base)
    assert torch.equal(state(y[:, None], p, None), base) and torch.equal(state(y, p[:, None], None), base)
    assert torch.equal(state(y, p, 1.0), base)
    assert torch.equal(state(y.cpu().numpy(), p, None), base)
    weighted = state(y, p, w)
    assert not torch.equal(weighted, base)
    assert torch.equal(state(y[:, None], p[:, None], w), weighted)
    assert torch.equal(state(y[:, None], p[:, None], w[:, None]), weighted)
    assert torch.equal(state(y, p, w[:, None]), weighted)
    twos = state(y, p, torch.full((n,), 2.0, device=DEV))
    assert torch.equal(state(y, p, 2.0), twos) and torch.equal(state(y, p, torch.tensor(2.0, device=DEV)), twos)
    assert torch.equal(twos, 2.0 * base)       # (doubling is exact)
    assert torch.equal(state(y.double(), p.double(), None), base)
    for m in (kl.AUC(), kl.BinaryAccuracy(), kl.BinaryMetricGroup(_members())):
        with pytest.raises(ValueError, match="same number of elements"):
            m.update_state(y[:-1], p)
        with pytest.raises(ValueError, match="sample_weight"):
            m.update_state(y, p, sample_weight=w[:-1])
    with pytest.raises(ValueError, match="2048"):
        kl.AUC(num_thresholds=2049)
    with pytest.raises(ValueError, match="2048"):
        kl.AUC(thresholds=list(np.linspace(0, 1, 2047)))
    empty = kl.AUC()
    empty.update_state(y[:0], p[:0])
    assert not torch.stack(empty.variables).any()


# ---- the example --------------------------------------------------------------------------------------------------

def test_train_step_updates_the_metrics():
    spec = importlib.util.spec_from_file_location("dlrm_dcn_v2", os.path.join(ROOT, "examples", "dlrm_dcn_v2.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    B, E = 64, 16
    hots = [3, 1, 2, 5, 1, 2]
    vocabs = [500, 7, 300, 900, 3, 40]
    model = ex.build_model(B, vocabs, hots, embedding_dim=E, projection=8, cross_layers=2, bottom=(32, E),
                           top=(32, 16, 1), table_optimizer=kl.SGD(0.1), embedding_threshold=50, dtype="float32",
                           embedding_dtype="float32")
    rng = np.random.default_rng(3)
    group = kl.BinaryMetricGroup([kl.BinaryAccuracy(), kl.AUC()])
    by_hand = kl.BinaryMetricGroup([kl.BinaryAccuracy(), kl.AUC()])
    box = [None]
    for _ in range(2):
        ids = {t: torch.from_numpy(rng.integers(0, vocabs[t], (B, hots[t])).astype(np.int32)).to(DEV) for t in range(6)}
        inputs = {"dense_input": _dev(rng.uniform(0, 0.9, (B, 13)).astype(np.float32)),
                  "large_emb_inputs": {f"cat_{t:02d}_id": ids[t] for t in (0, 2, 3)},
                  "small_emb_inputs": {f"cat_{t:02d}_id": ids[t] for t in (1, 4, 5)}}
        labels = _dev((rng.uniform(0, 1, (B, 1)) < 0.3).astype(np.float32))
        pred = model(inputs).detach().clone()          # the step's predictions: the same weights, the same kernels
        loss = ex.train_step(model, box, inputs, labels, metrics=group)
        assert torch.isfinite(loss)
        by_hand.update_state(labels, pred)
    for a, b in zip(group.metrics, by_hand.metrics):
        assert torch.equal(torch.stack(a.variables), torch.stack(b.variables)), a.name
    acc, auc = group.metrics
    assert float(acc.variables[1]) == 2 * B
    tp, fp, tn, fn = auc.variables
    assert float(tp[0] + fn[0] + fp[0] + tn[0]) == 2 * B
    assert 0.0 <= float(group.result()["auc"]) <= 1.0
