"""Host-side checks of the ranking losses (K9): the float64 restatement the GPU tests compare against reproduces every
value of the reference's own tests, the reference's ValueErrors, config round trips, and the C ABI's symbols and its
list-length limit -- none of it needs a GPU."""

import json
import os

import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import losses
from tests import ranking_restatement as RR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ranking_losses.json")))
KINDS = {"PairwiseHingeLoss": "hinge", "PairwiseLogisticLoss": "logistic", "PairwiseSoftZeroOneLoss": "soft_zero_one",
         "PairwiseMeanSquaredError": "mse", "ListMLELoss": "listmle"}
CLASSES = [getattr(losses, n) for n in KINDS]


def golden_case(c):
    """(labels, scores, mask, sample_weight) of a golden case as float64 / bool tensors, rank as in the case."""
    y = torch.tensor(GOLD["labels"], dtype=torch.float64)
    s = torch.tensor(GOLD["scores"], dtype=torch.float64)
    m = None if c["mask"] is None else torch.tensor(c["mask"])
    w = None if c["sample_weight"] is None else torch.tensor(c["sample_weight"], dtype=torch.float64)
    if c["rank"] == 1:
        y, s = y[0], s[0]
    return y, s, m, w


def test_golden_file_covers_every_loss_and_case():
    seen = {(c["loss"], c["case"]) for c in GOLD["cases"]}
    for name in KINDS:
        for case in ("unbatched", "batched", "temperature", "sum_over_batch_size", "scalar_sample_weight"):
            assert (name, case) in seen
        if name != "ListMLELoss":
            assert (name, "itemwise_sample_weight") in seen and (name, "mask") in seen


@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: f"{c['loss']}-{c['case']}")
def test_restatement_reproduces_reference_values(c):
    y, s, m, w = golden_case(c)
    if y.dim() == 1:
        y, s = y[None], s[None]
    v = RR.unreduced(KINDS[c["loss"]], s, y, m, c["temperature"])
    got = RR.reduce(v, w, c["reduction"])
    torch.testing.assert_close(got, torch.tensor(c["expected"], dtype=torch.float64), atol=1e-5, rtol=0)


@pytest.mark.parametrize("cls", CLASSES)
def test_temperature_must_be_positive(cls):
    for t in (0.0, -1.0):
        with pytest.raises(ValueError, match="positive float"):
            cls(temperature=t)


@pytest.mark.parametrize("cls", CLASSES)
def test_bad_reduction(cls):
    with pytest.raises(ValueError, match="reduction"):
        cls(reduction="max")


@pytest.mark.parametrize("cls", CLASSES)
def test_input_errors_before_any_device_check(cls):
    loss = cls()
    x = torch.ones((2, 3, 4))
    with pytest.raises(ValueError, match="rank"):
        loss(x, x)
    with pytest.raises(ValueError, match="rank"):
        loss(torch.ones(()), torch.ones(()))
    with pytest.raises(ValueError, match="same shape"):
        loss(torch.ones((2, 5)), torch.ones((2, 4)))
    with pytest.raises(ValueError, match="same shape"):
        loss({"labels": torch.ones((2, 5)), "mask": torch.ones((2, 4), dtype=torch.bool)}, torch.ones((2, 5)))
    with pytest.raises(ValueError, match="rank"):
        loss({"labels": torch.ones((2, 5)), "mask": torch.ones((2, 5, 1), dtype=torch.bool)}, torch.ones((2, 5)))
    with pytest.raises(ValueError, match='"labels"'):
        loss({"mask": torch.ones((2, 5), dtype=torch.bool)}, torch.ones((2, 5)))
    with pytest.raises(ValueError, match="sample_weight"):
        loss(torch.ones((2, 5)), torch.ones((2, 5)), sample_weight=torch.ones(3))


@pytest.mark.parametrize("cls", CLASSES)
def test_cpu_tensors_are_refused(cls):
    with pytest.raises(L.KrsError, match="no CPU fallback"):
        cls()(torch.ones((2, 5)), torch.ones((2, 5)))


@pytest.mark.parametrize("cls", CLASSES)
def test_config_round_trip(cls):
    loss = cls(temperature=0.8, reduction="sum", name="my_loss")
    cfg = loss.get_config()
    assert cfg["temperature"] == 0.8 and cfg["reduction"] == "sum" and cfg["name"] == "my_loss"
    again = cls.from_config(cfg)
    assert again.get_config() == cfg
    assert cls().get_config()["reduction"] == "sum_over_batch_size"


def test_default_names_follow_keras():
    assert losses.ListMLELoss().name == "list_mle_loss"
    assert losses.PairwiseHingeLoss().name == "pairwise_hinge_loss"
    assert losses.PairwiseMeanSquaredError().name == "pairwise_mean_squared_error"


def test_pairwise_base_is_abstract():
    with pytest.raises(TypeError):
        losses.PairwiseLoss()


def test_symbols_listed():
    assert "krs_pairwise_loss" in L.SYMBOLS and "krs_listmle_loss" in L.SYMBOLS


@pytest.mark.parametrize("entry", ["krs_pairwise_loss", "krs_listmle_loss"])
def test_list_longer_than_4096_is_refused_with_the_limit(entry):
    from keras_rs_amd.build import build

    build()
    fn = getattr(L.lib(), entry)
    args = [8, 4097, 0, 8, None, None, 1.0, 1.0, 1, 4097, 8, None, None]
    if entry == "krs_pairwise_loss":
        args = [1] + args
    rc = fn(*args)
    assert rc == -1
    msg = L.lib().krs_last_error().decode()
    assert "4097" in msg and "4096" in msg
