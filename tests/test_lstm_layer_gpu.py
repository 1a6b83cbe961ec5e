"""layers.LSTM on the GPU: the whole layer (input projection + K25 + the weight-gradient products) against the float64
reference (tests/lstm_reference.py `layer`, its bounds), unit_forget_bias, the shapes of return_sequences /
return_state, the refusals, a captured training step against the eager one, and the example with --cell lstm."""

import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from keras_rs_amd import layers as kl
from keras_rs_amd import recurrent_ops as G
from tests import lstm_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _holes(b, l):
    v = np.ones((b, l), dtype=bool)
    for x in range(b):
        v[x, x % 3::3] = False                             # (rows 0, 3, ..: the first step is masked)
    return v


@pytest.mark.parametrize("policy,b,l,d,u", [("mixed_bfloat16", 33, 7, 24, 50), ("float32", 5, 7, 12, 40)])
def test_lstm_layer_against_float64(policy, b, l, d, u):
    torch.manual_seed(3)
    rng = np.random.default_rng(b * 1000 + u)
    bf16 = policy == "mixed_bfloat16"
    rep = R.round_bf16 if bf16 else (lambda a: a.astype(np.float32).astype(np.float64))
    x = rng.standard_normal((b, l, d)).astype(np.float32).astype(np.float64)
    h0, c0 = rep(rng.standard_normal((b, u)) * 0.5), rep(rng.standard_normal((b, u)))
    dhs, dh_last, dc_last = (rep(rng.standard_normal(s)) for s in ((b, l, u), (b, u), (b, u)))
    valid = _holes(b, l)
    dev = lambda a, dt=torch.float32: torch.from_numpy(a).to(dt).to(DEV)
    layer = kl.LSTM(u, return_sequences=True, return_state=True, dtype=policy, device=DEV)
    xg, h0g, c0g = (dev(a).requires_grad_(True) for a in (x, h0, c0))
    layer(xg, initial_state=[h0g, c0g], mask=dev(valid, torch.bool))             # (builds the weights)
    assert [tuple(w.shape) for w in layer.weights] == [(d, 4 * u), (u, 4 * u), (4 * u,)]
    layer.bias.data.normal_(0.0, 0.3)
    hs, h, c = layer(xg, initial_state=[h0g, c0g], mask=dev(valid, torch.bool))
    assert hs.shape == (b, l, u) and h.shape == c.shape == (b, u) and hs.dtype == c.dtype == layer.compute_dtype
    assert G.lstm_last_route() == ((G.FAST, 64) if bf16 else (G.GENERIC, 0))
    grads = torch.autograd.grad((hs, h, c), [xg] + layer.weights + [h0g, c0g],
                                tuple(dev(g, hs.dtype) for g in (dhs, dh_last, dc_last)))
    got = dict(zip(("hs", "h", "c", "dx", "dkernel", "drk", "dbias", "dh0", "dc0"), (hs, h, c) + tuple(grads)))
    w = [p.detach().double().cpu().numpy() for p in layer.weights]
    args = (x, w[0], w[1], w[2], valid, h0, c0, dhs, dh_last, dc_last)
    ref = R.layer(*args)
    bound, _ = R.bounds(ref, R.layer(*args, bf16=True) if bf16 else ref, bf16)
    worst = {}
    for key, g in got.items():
        err = np.abs(g.detach().double().cpu().numpy() - ref[key])
        worst[key] = float(np.where(err == 0.0, 0.0, err / bound[key]).max())
        print(f"{policy}: {key}: worst error / bound = {worst[key]:.3f}")
    assert max(worst.values()) <= 1.0, worst


def test_unit_forget_bias_shapes_and_refusals():
    u = 6
    x = torch.randn(3, 5, 8, device=DEV)
    ones = kl.LSTM(u, bias_initializer="zeros", device=DEV)
    assert ones(x).shape == (3, u)
    assert torch.equal(ones.bias.detach().cpu(), torch.cat([torch.zeros(u), torch.ones(u), torch.zeros(2 * u)]))
    flat = kl.LSTM(u, unit_forget_bias=False, return_sequences=True, return_state=True, device=DEV)
    out, h, c = flat(x)
    assert not flat.bias.any() and out.shape == (3, 5, u) and h.shape == c.shape == (3, u)
    assert flat.compute_output_shape((3, 5, 8)) == ((3, 5, u), (3, u), (3, u))
    assert ones.compute_output_shape((3, 5, 8)) == (3, u)
    assert kl.LSTM.from_config(flat.get_config()).get_config() == flat.get_config() and "LSTM" in kl.__all__
    with pytest.raises(ValueError, match="units"):
        kl.LSTM(0)
    for kwargs, word in ((dict(activation="relu"), "activation"), (dict(recurrent_activation="tanh"), "recurrent_activation"),
                         (dict(dropout=0.1), "dropout"), (dict(recurrent_dropout=0.1), "recurrent_dropout"),
                         (dict(go_backwards=True), "go_backwards"), (dict(stateful=True), "stateful"),
                         (dict(unroll=True), "unroll")):
        with pytest.raises(NotImplementedError, match=word):
            kl.LSTM(4, **kwargs)


def test_a_captured_training_step_replays_the_eager_step_bit_for_bit():
    torch.manual_seed(11)
    b, l, d, u = 65, 7, 24, 128
    layer = kl.LSTM(u, return_sequences=True, return_state=True, dtype="mixed_bfloat16", device=DEV)
    x = torch.randn(b, l, d, device=DEV).requires_grad_(True)
    valid = torch.from_numpy(_holes(b, l)).to(DEV)
    layer(x, mask=valid)
    dhs, dh, dc = (torch.randn(*s, device=DEV).bfloat16() for s in ((b, l, u), (b, u), (b, u)))

    def step():
        outs = layer(x, mask=valid)
        return tuple(outs) + torch.autograd.grad(outs, [x] + layer.weights, (dhs, dh, dc))

    eager = [o.detach().clone() for o in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                             # (warm-up outside the capture: allocations, attributes)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(3):
        for o in outs:
            o.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o.detach(), e) for o, e in zip(outs, eager))


def test_the_sequential_retrieval_example_trains_and_serves_with_an_lstm():
    spec = importlib.util.spec_from_file_location("sequential_retrieval_example",
                                                  os.path.join(ROOT, "examples", "sequential_retrieval.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    run = ex.main(steps=8, batch=64, vocabulary_size=200, hidden_dim=32, dtype="bf16", cell="lstm", quiet=True)
    losses = run["losses"]
    assert len(losses) == 8 and all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    assert G.lstm_last_route() == (G.FAST, 32) and isinstance(run["model"].lstm, kl.LSTM)
    pred = run["outputs"]["predictions"]
    assert pred.shape == (64, 10) and int(pred.min()) >= 0 and int(pred.max()) <= 200
