"""Host-side checks of the binary metrics (K12): keras' published answers for AUC and BinaryAccuracy through
auc_from_confusion on CPU tensors and through the float64 restatement the GPU tests compare against, the constructors'
ValueErrors and NotImplementedErrors, the threshold lists, config round trips and the C ABI's limits -- none of it
needs a GPU."""

import json
import os
import re

import numpy as np
import pytest
import torch

import keras_rs_amd.layers as kl
from keras_rs_amd import _lib as L
from keras_rs_amd import metric_ops
from tests import binary_metric_restatement as BR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "binary_metrics.json")))
ATOL, RTOL = GOLD["atol"], GOLD["rtol"]
AUC_ROWS = [(c, key) for c in GOLD["auc"]["cases"] for key in c["results"]]
STATE_KEYS = ("tp", "fp", "tn", "fn")


def _close(got, expected):
    return abs(got - expected) <= ATOL + RTOL * abs(expected)


def _restated_state(c):
    a = GOLD["auc"]
    return BR.confusion(a["y_true"], a["y_pred"], c["weights"], a["num_thresholds"])


def test_golden_file_is_the_published_set():
    assert ATOL == 1e-6 and RTOL == 1e-6
    assert len(AUC_ROWS) == 8 and len(GOLD["binary_accuracy"]["cases"]) == 2
    weighted = GOLD["auc"]["cases"][2]
    assert sorted(weighted["results"]) == sorted(f"{c}/{m}" for c in ("ROC", "PR")
                                                 for m in ("interpolation", "minoring", "majoring"))


@pytest.mark.parametrize("c", GOLD["auc"]["cases"], ids=lambda c: str(c["weights"]))
def test_restatement_reproduces_golden_states(c):
    state = _restated_state(c)
    if c["state"] is not None:
        for got, key in zip(state, STATE_KEYS):
            assert np.array_equal(got, np.asarray(c["state"][key], np.float64)), key
    tp, fp, tn, fn = state
    assert np.array_equal(tp + fn, np.full(3, tp[0] + fn[0])) and np.array_equal(fp + tn, np.full(3, fp[0] + tn[0]))


@pytest.mark.parametrize("c,key", AUC_ROWS, ids=lambda v: v if isinstance(v, str) else str(v["weights"]))
def test_auc_from_confusion_reproduces_golden_results(c, key):
    curve, method = key.split("/")
    state = _restated_state(c)
    assert _close(BR.auc_from_confusion(*state, curve, method), c["results"][key])
    tensors = [torch.from_numpy(v.astype(np.float32)) for v in state]
    got = kl.auc_from_confusion(*tensors, curve=curve, summation_method=method)
    assert got.dtype == torch.float32 and got.dim() == 0
    assert _close(float(got), c["results"][key])


@pytest.mark.parametrize("c", GOLD["binary_accuracy"]["cases"], ids=lambda c: str(c["weights"]))
def test_restatement_reproduces_golden_accuracy(c):
    b = GOLD["binary_accuracy"]
    total, count = BR.accuracy(b["y_true"], b["y_pred"], c["weights"], b["threshold"])
    assert _close(total / count, c["result"])


def test_auc_of_an_empty_state_is_zero():
    z = torch.zeros(5)
    for curve in ("ROC", "PR"):
        for method in ("interpolation", "minoring", "majoring"):
            assert float(kl.auc_from_confusion(z, z, z, z, curve, method)) == 0.0
    assert float(kl.AUC().result()) == 0.0 and float(kl.BinaryAccuracy().result()) == 0.0


def test_bucket_and_comparison_forms_differ_so_the_bucket_form_is_the_contract():
    """On the predictions k/199 in fp32 the bucket of ceil(p * 199) - 1 and the count of thresholds i/199 below p
    disagree: the restatement (and the kernel) follow keras' bucket form."""
    p = (np.arange(200) / 199.0).astype(np.float32)
    bucket = BR.buckets(p, 200)
    compared = BR.buckets(p, 200, BR.default_thresholds(200).astype(np.float32))
    assert bucket.min() == 0 and bucket.max() == 198 and compared.max() <= 198
    assert 0 < np.count_nonzero(bucket != compared) < 200


def test_restatement_clamp_nan_and_labels():
    p = BR.probability(np.array([-0.25, 1.5, np.nan, 0.25], np.float32))
    assert p.tolist() == [0.0, 1.0, 0.0, 0.25]
    tp, fp, tn, fn = BR.confusion([1, 2, 0, -1], [0.9, 0.9, 0.9, 0.9], None, 3)   # positive iff label != 0
    assert tp.tolist() == [3, 3, 0] and fp.tolist() == [1, 1, 0]
    total, count = BR.accuracy([1, 2, 0, 0.5], [0.9, 0.9, 0.1, 0.9], None, 0.5)  # 2 and 0.5 match nothing
    assert (total, count) == (2.0, 4.0)


def test_constructor_errors():
    for bad in (1, 0, -3, 2.5, "7", None, True):
        with pytest.raises(ValueError, match="num_thresholds"):
            kl.AUC(num_thresholds=bad)
    for bad in ([-0.1, 0.5], [0.5, 1.1]):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            kl.AUC(thresholds=bad)
    with pytest.raises(ValueError, match="curve"):
        kl.AUC(curve="roc")
    with pytest.raises(ValueError, match="summation method"):
        kl.AUC(summation_method="trapezoid")
    with pytest.raises(ValueError, match="float32"):
        kl.AUC(dtype="float64")
    with pytest.raises(ValueError, match="float32"):
        kl.BinaryAccuracy(dtype="bfloat16")
    for kwargs in ({"multi_label": True}, {"num_labels": 3}, {"label_weights": [1.0, 2.0]}):
        with pytest.raises(NotImplementedError, match="one label"):
            kl.AUC(**kwargs)
    with pytest.raises(ValueError, match=str(metric_ops.MAX_THRESHOLDS)):
        kl.AUC(num_thresholds=metric_ops.MAX_THRESHOLDS + 1)
    kl.AUC(num_thresholds=metric_ops.MAX_THRESHOLDS)
    kl.AUC(dtype="float32"), kl.AUC(dtype=torch.float32), kl.BinaryAccuracy(dtype=None)


def test_threshold_generation():
    assert kl.AUC(num_thresholds=3).thresholds == [0.0 - 1e-7, 0.5, 1.0 + 1e-7]
    assert kl.AUC(num_thresholds=2).thresholds == [0.0 - 1e-7, 1.0 + 1e-7]
    m = kl.AUC()
    assert m.num_thresholds == 200 and len(m.thresholds) == 200 and m.name == "auc"
    assert np.array_equal(np.asarray(m.thresholds), BR.default_thresholds(200))
    g = kl.AUC(thresholds=[0.7, 0.2, 0.2, 1.0])                  # sorted, wrapped, duplicates kept
    assert g.num_thresholds == 6 and g.thresholds == [0.0 - 1e-7, 0.2, 0.2, 0.7, 1.0, 1.0 + 1e-7]
    # keras' route choice: the bucket route for an even list of three or more, the comparison route otherwise
    assert m._even and kl.AUC(thresholds=[0.5])._even and kl.AUC(thresholds=[0.25, 0.5, 0.75])._even
    assert not g._even and not kl.AUC(num_thresholds=2)._even and not kl.AUC(thresholds=[0.4])._even


def test_variables_are_the_four_vectors_in_keras_order():
    m = kl.AUC(num_thresholds=5)
    assert [tuple(v.shape) for v in m.variables] == [(5,)] * 4
    assert all(v.dtype == torch.float32 and not v.any() for v in m.variables)
    assert [tuple(v.shape) for v in kl.BinaryAccuracy().variables] == [(), ()]


def test_config_round_trips():
    a = kl.AUC(num_thresholds=17, curve="PR", summation_method="minoring", name="pr", from_logits=True)
    cfg = a.get_config()
    assert cfg == {"name": "pr", "dtype": "float32", "num_thresholds": 17, "curve": "PR",
                   "summation_method": "minoring", "multi_label": False, "num_labels": None, "label_weights": None,
                   "from_logits": True}
    b = kl.AUC.from_config(cfg)
    assert b.get_config() == cfg and b.thresholds == a.thresholds
    t = kl.AUC(thresholds=[0.9, 0.1])
    cfg = t.get_config()
    assert cfg["thresholds"] == [0.1, 0.9] and cfg["num_thresholds"] == 4
    assert kl.AUC.from_config(cfg).thresholds == t.thresholds and kl.AUC.from_config(cfg).get_config() == cfg
    acc = kl.BinaryAccuracy(threshold=0.3, name="acc")
    assert acc.get_config() == {"name": "acc", "dtype": "float32", "threshold": 0.3}
    assert kl.BinaryAccuracy.from_config(acc.get_config()).get_config() == acc.get_config()
    assert kl.BinaryAccuracy().name == "binary_accuracy" and kl.BinaryAccuracy().threshold == 0.5


def test_group_membership_rules():
    kl.BinaryMetricGroup([kl.BinaryAccuracy(), kl.AUC()])
    kl.BinaryMetricGroup([kl.AUC(name=f"a{i}") for i in range(metric_ops.MAX_AUCS)])
    with pytest.raises(ValueError, match="at most one BinaryAccuracy"):
        kl.BinaryMetricGroup([kl.BinaryAccuracy(), kl.BinaryAccuracy(name="b"), kl.AUC()])
    with pytest.raises(ValueError, match="1 to 4"):
        kl.BinaryMetricGroup([kl.BinaryAccuracy()])
    with pytest.raises(ValueError, match="1 to 4"):
        kl.BinaryMetricGroup([kl.AUC(name=f"a{i}") for i in range(metric_ops.MAX_AUCS + 1)])
    with pytest.raises(ValueError, match="distinct names"):
        kl.BinaryMetricGroup([kl.AUC(), kl.AUC(curve="PR")])
    with pytest.raises(ValueError, match="BinaryAccuracy and AUC objects"):
        kl.BinaryMetricGroup([kl.AUC(), object()])


def test_validation_comes_before_the_device_check():
    """CPU tensors: a shape mistake is a ValueError, well-formed input reaches the device check (no CPU fallback)."""
    y, p = torch.zeros(4), torch.zeros(5)
    for m in (kl.AUC(), kl.BinaryAccuracy(), kl.BinaryMetricGroup([kl.BinaryAccuracy(), kl.AUC()])):
        with pytest.raises(ValueError, match="same number of elements"):
            m.update_state(y, p)
        with pytest.raises(ValueError, match="sample_weight"):
            m.update_state(y, torch.zeros(4, 1), sample_weight=torch.ones(3))
        with pytest.raises(L.KrsError, match="no CPU fallback"):
            m.update_state(y, torch.zeros(4, 1), sample_weight=torch.ones(4))


def test_header_constants_match_the_host_module():
    header = open(os.path.join(os.path.dirname(HERE), "include", "krs.h")).read()
    value = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))  # noqa: E731
    assert value("KRS_BINARY_METRIC_MAX_AUCS") == metric_ops.MAX_AUCS == 4
    assert value("KRS_BINARY_METRIC_MAX_THRESHOLDS") == metric_ops.MAX_THRESHOLDS == 2048
    assert value("KRS_BINARY_METRIC_CHUNK") == metric_ops.BINARY_CHUNK
    assert "krs_binary_metrics" in L.SYMBOLS and "krs_binary_metrics_workspace_bytes" in L.SYMBOLS


def test_workspace_size_and_argument_checks_without_a_device():
    """Host-only entry points: the workspace formula, and the argument checks that return before any launch."""
    import ctypes as C

    from keras_rs_amd.build import build

    build()
    lib = L.lib()
    chunk, groups = metric_ops.BINARY_CHUNK, 256
    ts = (C.c_int * 2)(200, 2048)
    assert lib.krs_binary_metrics_workspace_bytes(0, 2, ts) == 0
    assert lib.krs_binary_metrics_workspace_bytes(1, 0, None) == 4 * 2 * groups
    for n, g in ((1, 1), (chunk, 1), (chunk + 1, 2), (groups * chunk + 1, groups), (1 << 33, groups)):
        assert lib.krs_binary_metrics_workspace_bytes(n, 2, ts) == 4 * (2 * groups + g * 2 * (201 + 2049))
    state = (C.c_void_p * 1)(1)

    def call(n_aucs, t, thresholds=None, acc_state=None):
        return lib.krs_binary_metrics(None, L.F32, None, None, 1.0, 0, 0.5, acc_state, n_aucs, thresholds,
                                      (C.c_int * 1)(t), (C.c_int * 1)(0), state, None, 0, None)

    assert call(1, 200) == 0                                     # n = 0: checked, nothing launched
    for t in (1, 0, 2049):
        assert call(1, t) == -1 and b"KRS_BINARY_METRIC_MAX_THRESHOLDS" in lib.krs_last_error()
    assert call(1, 2) == -1 and b"even thresholds" in lib.krs_last_error()
    assert call(1, 2, (C.c_void_p * 1)(1)) == 0
    assert call(5, 200) == -1 and b"KRS_BINARY_METRIC_MAX_AUCS" in lib.krs_last_error()
    assert call(0, 200) == -1 and call(0, 200, acc_state=1) == 0
