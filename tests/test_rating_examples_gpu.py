"""The three rating examples (examples/basic_ranking.py, listwise_ranking.py, multi_task.py) at their smallest
setting: the step-0 loss is bit-equal to the loss object called on the recorded predictions, the metric equals the
float64 restatement on the recorded predictions, and the loss falls on the learnable synthetic target."""

import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import keras_rs_amd.layers as kl
from tests import regression_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example(name):
    spec = importlib.util.spec_from_file_location(f"{name}_example", os.path.join(ROOT, "examples", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rmse64(recorded, epoch):
    """sqrt(sum e^2 / count) in float64 over the recorded (epoch, y_true [B], y_pred [B, 1]) steps of one epoch"""
    total = count = 0.0
    for e, y, p in recorded:
        if e == epoch:
            s = R.reference64(p.float().cpu().numpy().reshape(-1, 1), y.cpu().numpy().reshape(-1, 1), None, "mse", 1.0,
                              "sum")["sums"]
            total, count = total + s[0], count + s[2]
    return math.sqrt(total / count)


def test_basic_ranking():
    run = _example("basic_ranking").main(epochs=2, rows=1024, batch=256, num_users=50, num_movies=40, embedding_dim=16,
                                         quiet=True)
    losses = [float(v) for v in run["losses"]]
    print("loss:", " ".join(f"{x:.4f}" for x in losses))
    assert len(losses) == 8 and all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]
    _, y0, p0 = run["recorded"][0]
    assert tuple(y0.shape) == (256,) and tuple(p0.shape) == (256, 1)
    assert torch.equal(run["losses"][0], kl.MeanSquaredError()(y0, p0))
    np.testing.assert_allclose(losses[0], R.reference64(p0.cpu().numpy(), y0.cpu().numpy().reshape(-1, 1), None, "mse",
                                                        1.0, "sum_over_batch_size")["loss"], rtol=1e-5)
    np.testing.assert_allclose(float(run["rmse"]), _rmse64(run["recorded"], run["last_epoch"]), rtol=1e-5)


def test_listwise_ranking():
    run = _example("listwise_ranking").main(epochs=2, lists=512, batch=128, num_users=40, num_movies=30,
                                            embedding_dim=16, quiet=True)
    from keras_rs_amd.losses import PairwiseHingeLoss

    for name, loss_fn in (("mse", kl.MeanSquaredError()), ("hinge", PairwiseHingeLoss())):
        part = run[name]
        losses = [float(v) for v in part["losses"]]
        print(name, "loss:", " ".join(f"{x:.4f}" for x in losses), "ndcg", float(part["ndcg"]))
        assert len(losses) == 8 and all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]
        y0, p0 = part["recorded"][0]
        assert tuple(y0.shape) == tuple(p0.shape) == (128, 5)
        assert torch.equal(part["losses"][0], loss_fn(y0, p0))
        assert 0.0 < float(part["ndcg"]) <= 1.0
    y0, p0 = run["mse"]["recorded"][0]
    np.testing.assert_allclose(float(run["mse"]["losses"][0]),
                               R.reference64(p0.cpu().numpy(), y0.cpu().numpy(), None, "mse", 1.0,
                                             "sum_over_batch_size")["loss"], rtol=1e-5)


@pytest.mark.parametrize("stored", [False, True])
def test_multi_task(stored):
    run = _example("multi_task").main(epochs=2, rows=1024, batch=256, num_users=50, num_movies=40, embedding_dim=16,
                                      stored=stored, quiet=True)
    for key in ("total", "ranking", "retrieval"):
        losses = [float(v[key]) for v in run["losses"]]
        print(key, "loss:", " ".join(f"{x:.4f}" for x in losses))
        assert len(losses) == 8 and all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]
    _, y0, p0 = run["recorded"][0]
    assert torch.equal(run["losses"][0]["ranking"], kl.MeanSquaredError()(y0, p0))
    first = run["losses"][0]
    assert float(first["total"]) == pytest.approx(float(first["ranking"]) + float(first["retrieval"]), rel=1e-6)
    np.testing.assert_allclose(float(run["rmse"]), _rmse64(run["recorded"], run["last_epoch"]), rtol=1e-5)
    ev = run["evaluation"]
    assert math.isfinite(float(ev["rmse"])) and 0.0 <= float(ev["top_10_accuracy"]) <= 1.0
