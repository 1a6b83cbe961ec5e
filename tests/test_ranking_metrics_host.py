"""Host-side checks of the ranking metrics (K10): the float64 restatement the GPU tests compare against reproduces
every value of the reference's own tests and none of those values depends on how score ties are broken, the
reference's ValueErrors, config round trips, the group's agreement check, and the C ABI's symbols and limits -- none
of it needs a GPU."""

import json
import os

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import metrics
from tests import ranking_metric_restatement as MR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ranking_metrics.json")))
KINDS = {"DCG": "dcg", "NDCG": "ndcg", "MeanAveragePrecision": "map", "MeanReciprocalRank": "mrr",
         "PrecisionAtK": "precision", "RecallAtK": "recall"}
CLASSES = [getattr(metrics, n) for n in KINDS]
GAINS = {"default": MR.default_gain, "linear": lambda y: y}
DISCOUNTS = {"default": MR.default_discount, "inverse": lambda r: 1.0 / r}


def restated_results(c, **order):
    """result() after each update of a golden case, from the restatement."""
    mean, out = MR.Mean(), []
    for u in c["updates"]:
        y = np.asarray(u["y_true"], dtype=np.float64)
        w = MR.broadcast_weight(u["sample_weight"], y.shape)
        y2, s2 = np.atleast_2d(y), np.atleast_2d(np.asarray(u["y_pred"], dtype=np.float32))
        m2 = None if u["mask"] is None else np.atleast_2d(np.asarray(u["mask"]))
        v, lw, _ = MR.metric(KINDS[c["metric"]], s2, y2, m2, w, c["k"], gain_fn=GAINS[c["gain"]],
                             discount_fn=DISCOUNTS[c["discount"]], **order)
        mean.update(v, lw)
        out.append(mean.result())
    return out


def test_golden_file_covers_every_metric_and_case():
    seen = {(c["metric"], c["case"].split("/")[0]) for c in GOLD["cases"]}
    for name in KINDS:
        for group in ("unbatched", "batched", "batched_sample_weight", "2d_sample_weight", "masking", "k",
                      "statefulness"):
            assert (name, group) in seen
    assert ("DCG", "alternative_gain_rank_discount_fns") in seen
    assert ("NDCG", "alternative_gain_rank_discount_fns") in seen
    for c in GOLD["cases"]:
        assert c["source"].split(":")[0].endswith("_test.py") and c["source"].split(":")[1]
        for u in c["updates"]:
            assert u["atol"] == 1e-6 and u["rtol"] in (1e-6, 1e-5)


@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: f"{c['metric']}-{c['case']}")
def test_restatement_reproduces_reference_values(c):
    for got, u in zip(restated_results(c), c["updates"]):
        assert abs(got - u["expected"]) <= u["atol"] + u["rtol"] * abs(u["expected"]), (got, u["expected"])


@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: f"{c['metric']}-{c['case']}")
def test_golden_values_do_not_depend_on_the_tie_order(c):
    up = restated_results(c, ties="ascending")
    down = restated_results(c, ties="descending")
    # (equal up to the float64 rounding of a sum taken in another order)
    assert np.allclose(up, down, rtol=1e-13, atol=1e-13)
    for seed in (1, 2):
        assert np.allclose(restated_results(c, shuffle_ties=True, seed=seed), up, rtol=1e-13, atol=1e-13)


def test_restatement_tie_rule():
    s = np.array([[1.0, 2.0, 1.0, 1.0, -0.0, 0.0, 5.0]], dtype=np.float32)
    valid = np.array([[True, True, True, True, True, True, False]])
    assert MR.rank_order(s, valid).tolist() == [[1, 0, 2, 3, 4, 5, 6]]
    assert MR.rank_order(s, valid, ties="descending").tolist() == [[1, 3, 2, 0, 5, 4, 6]]
    # the hash: every tie key fits 20 bits, differs between draws, and is a function of (seed, draw, row, index)
    a, b = MR.tie_r20(7, 0, 3, 8), MR.tie_r20(7, 1, 3, 8)
    assert a.shape == (3, 8) and int(a.max()) < 2 ** 20 and (a != b).any()
    assert (MR.tie_r20(7, 0, 3, 8) == a).all() and (MR.tie_r20(8, 0, 3, 8) != a).any()
    # the first output of splitmix64 seeded with 0 (its published test vector)
    assert MR._mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("cls", CLASSES)
def test_k_must_be_a_positive_integer(cls):
    for k in (0, -5, 3.5):
        with pytest.raises(ValueError, match="`k` should be a positive integer"):
            cls(k=k)


@pytest.mark.parametrize("cls", CLASSES)
def test_only_float32(cls):
    with pytest.raises(ValueError, match="float32"):
        cls(dtype="float64")
    assert cls(dtype="float32").get_config()["dtype"] == "float32"


@pytest.mark.parametrize("cls", CLASSES)
def test_input_errors_before_any_device_check(cls):
    m = cls()
    x = torch.ones((2, 3, 4))
    with pytest.raises(ValueError, match="`y_true` should have a rank from"):
        m.update_state(x, x)
    with pytest.raises(ValueError, match="`y_true` should have a rank from"):
        m.update_state(torch.ones(()), torch.ones(()))
    with pytest.raises(ValueError, match="same shape"):
        m.update_state(torch.ones((2, 5)), torch.ones((2, 4)))
    with pytest.raises(ValueError, match="`y_pred` should have a rank from"):
        m.update_state(torch.ones((2, 5)), torch.ones((2, 5, 1)))
    with pytest.raises(ValueError, match="same shape"):
        m.update_state({"labels": torch.ones((2, 5)), "mask": torch.ones((2, 4), dtype=torch.bool)}, torch.ones((2, 5)))
    with pytest.raises(ValueError, match="`mask` should have a rank from"):
        m.update_state({"labels": torch.ones((2, 5)), "mask": torch.ones((2, 5, 1), dtype=torch.bool)},
                       torch.ones((2, 5)))
    with pytest.raises(ValueError, match='"labels"'):
        m.update_state({"mask": torch.ones((2, 5), dtype=torch.bool)}, torch.ones((2, 5)))
    with pytest.raises(ValueError, match="`sample_weight` should have a rank from"):
        m.update_state(torch.ones((2, 5)), torch.ones((2, 5)), sample_weight=torch.ones((2, 5, 1)))
    with pytest.raises(ValueError, match="`sample_weight` should have a rank from"):
        m.update_state(torch.ones(5), torch.ones(5), sample_weight=torch.ones((1, 5)))
    for bad in (torch.ones(3), torch.ones((2, 4)), torch.ones((5, 2))):
        with pytest.raises(ValueError, match="`sample_weight` of shape"):
            m.update_state(torch.ones((2, 5)), torch.ones((2, 5)), sample_weight=bad)
    with pytest.raises(ValueError, match="`sample_weight` of shape"):
        m.update_state(torch.ones(5), torch.ones(5), sample_weight=torch.ones(4))


@pytest.mark.parametrize("cls", CLASSES)
def test_cpu_tensors_are_refused(cls):
    with pytest.raises(L.KrsError, match="no CPU fallback"):
        cls().update_state(torch.ones((2, 5)), torch.ones((2, 5)))


@pytest.mark.parametrize("cls", CLASSES)
def test_config_round_trip(cls):
    m = cls(k=7, shuffle_ties=False, seed=11, name="my_metric")
    cfg = m.get_config()
    assert {"name": "my_metric", "dtype": "float32", "k": 7, "shuffle_ties": False, "seed": 11}.items() <= cfg.items()
    again = cls.from_config(cfg)
    assert again.get_config() == cfg and type(again) is cls
    default = cls().get_config()
    assert default["k"] is None and default["shuffle_ties"] is True and default["seed"] is None


@pytest.mark.parametrize("cls", [metrics.DCG, metrics.NDCG])
def test_gain_and_discount_functions_in_the_config(cls):
    cfg = cls().get_config()
    assert cfg["gain_fn"] == "default_gain_fn" and cfg["rank_discount_fn"] == "default_rank_discount_fn"
    again = cls.from_config(cfg)
    assert again.gain_fn is metrics.default_gain_fn and again.rank_discount_fn is metrics.default_rank_discount_fn

    def linear(label):
        return label

    cfg = cls(gain_fn=linear).get_config()
    assert cfg["gain_fn"] is linear and cls.from_config(cfg).gain_fn is linear
    with pytest.raises(ValueError, match="gain_fn"):
        cls(gain_fn="no_such_function")


def test_default_names_follow_keras():
    assert metrics.DCG().name == "dcg" and metrics.NDCG().name == "ndcg"
    assert metrics.MeanAveragePrecision().name == "mean_average_precision"
    assert metrics.MeanReciprocalRank().name == "mean_reciprocal_rank"
    assert metrics.PrecisionAtK().name == "precision_at_k" and metrics.RecallAtK().name == "recall_at_k"


def test_base_is_abstract_and_result_starts_at_zero():
    with pytest.raises(TypeError):
        metrics.RankingMetric()
    m = metrics.NDCG()
    assert float(m.result()) == 0.0 and m.result().dtype == torch.float32 and m.result().dim() == 0
    m.reset_state()
    assert float(m.result()) == 0.0


def test_seed_none_is_drawn_from_the_default_generator():
    torch.manual_seed(1234)
    a = metrics.NDCG()._seed_value
    b = metrics.NDCG()._seed_value
    torch.manual_seed(1234)
    assert metrics.NDCG()._seed_value == a and a != b
    assert metrics.NDCG(seed=5)._seed_value == 5


def test_group_members_must_agree():
    ok = metrics.RankingMetricGroup([metrics.NDCG(k=10, seed=3), metrics.MeanReciprocalRank(seed=3)])
    assert [m.name for m in ok.metrics] == ["ndcg", "mean_reciprocal_rank"]
    with pytest.raises(ValueError, match="agree on `shuffle_ties` and `seed`"):
        metrics.RankingMetricGroup([metrics.NDCG(seed=3), metrics.MeanReciprocalRank(seed=4)])
    with pytest.raises(ValueError, match="agree on `shuffle_ties` and `seed`"):
        metrics.RankingMetricGroup([metrics.NDCG(seed=3, shuffle_ties=False), metrics.RecallAtK(seed=3)])
    with pytest.raises(ValueError, match="`gain_fn` and `rank_discount_fn`"):
        metrics.RankingMetricGroup([metrics.NDCG(seed=3, gain_fn=lambda y: y), metrics.DCG(seed=3)])
    with pytest.raises(ValueError, match="1 to 8"):
        metrics.RankingMetricGroup([metrics.RecallAtK(k=k, seed=0) for k in range(1, 10)])
    with pytest.raises(ValueError, match="1 to 8"):
        metrics.RankingMetricGroup([])
    with pytest.raises(L.KrsError, match="no CPU fallback"):
        ok.update_state(torch.ones((2, 5)), torch.ones((2, 5)))


def test_symbols_listed():
    for name in ("krs_ranking_metrics", "krs_ranking_metrics_accumulate",
                 "krs_ranking_metrics_accumulate_workspace_bytes"):
        assert name in L.SYMBOLS


def _stage_a(n_specs, list_len, kinds=None):
    import ctypes as C

    kinds = (C.c_int * 9)(*(kinds or [0] * 9))
    ks = (C.c_int * 9)(*([0] * 9))
    return L.lib().krs_ranking_metrics(8, list_len, 0, 8, None, None, 0, 0, 1.0, None, None, 0, 0, 0, None, kinds, ks,
                                       n_specs, 1, list_len, 8, 8, None, None)


def test_limits_are_refused_without_a_device():
    from keras_rs_amd.build import build

    build()
    assert _stage_a(1, 4097) == -1
    msg = L.lib().krs_last_error().decode()
    assert "4097" in msg and "4096" in msg
    assert _stage_a(1, 0) == -1
    assert _stage_a(9, 16) == -1
    msg = L.lib().krs_last_error().decode()
    assert "9" in msg and "8" in msg and "KRS_METRIC_MAX_SPECS" in msg
    assert _stage_a(0, 16) == -1
    assert _stage_a(2, 16, kinds=[0, 6] + [0] * 7) == -1
    assert "metric kind 6" in L.lib().krs_last_error().decode()
    import ctypes as C

    rc = L.lib().krs_ranking_metrics_accumulate(8, 8, (C.c_int * 9)(), 9, 1, (C.c_void_p * 9)(), None, None, None,
                                                None, 0, None)
    assert rc == -1 and "KRS_METRIC_MAX_SPECS" in L.lib().krs_last_error().decode()
    # stage B's workspace: none for one workgroup's 1024 lists, 20 floats per workgroup of 1024 lists above, 256 at most
    size = L.lib().krs_ranking_metrics_accumulate_workspace_bytes
    assert [size(b) for b in (0, 1, 1024, 1025, 2048, 2049, 65536, 10 ** 7)] == [0, 0, 0, 160, 160, 240, 5120, 20480]
