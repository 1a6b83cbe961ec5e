"""layers.GRU and examples/sequential_retrieval.py on the GPU: the layer (input projection + K20 + the weight-gradient
products) against the float64 restatement of the whole layer, under autograd.grad on subsets of its inputs, and the
example end to end.

Bounds of the layer comparisons.  float32 policy: the project's standing rtol = atol = 1e-5 against float64, element by
element, for every output and gradient (the configurations below keep B L <= 455 tokens and O(1) entries, so an fp32
sum of that many products stays inside it, as the table's fp32 cases do at 1089 tokens).  mixed_bfloat16: as in
tests/gru_cases.py, from the restatement alone: E is the largest distance between tests/gru_restatement.py's
`layer(bf16=True)`, which rounds where the layer rounds, and the exact one; a result must be within 2 E + 2^-8 |ref|."""

import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from keras_rs_amd import layers as kl
from keras_rs_amd import recurrent_ops as G
from tests import gru_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("hs", "h_last", "dx", "dkernel", "drk", "dbias", "dh0")


def _mask(kind, b, l):
    if kind == "none":
        return None
    pos = np.arange(l)[None, :]
    lengths = np.array([max(1, l - (x % 4 + 1) * l // 5) for x in range(b)])[:, None]
    if kind == "right":
        return pos < lengths
    if kind == "left":
        return pos >= l - lengths
    holes = np.ones((b, l), dtype=bool)
    for x in range(b):
        holes[x, x % 3::3] = False                         # (row 0, 3, ..: the first step is masked)
    return holes


def _bounds(policy, ref, rounded):
    out = {}
    for key in KEYS:
        if ref[key] is None:
            continue
        if policy == "float32":
            out[key] = 1e-5 + 1e-5 * np.abs(ref[key])
        else:
            e = float(np.abs(rounded[key] - ref[key]).max(initial=0.0))
            out[key] = 2.0 * e + 2.0 ** -8 * np.abs(ref[key])
    return out


def _check(what, got, ref, bound):
    worst = 0.0
    for key in KEYS:
        if ref[key] is None:
            continue
        g = got[key].detach().double().cpu().numpy()
        assert g.shape == ref[key].shape and np.isfinite(g).all(), f"{what}: {key}"
        err = np.abs(g - ref[key])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.where(err == 0.0, 0.0, err / bound[key]).max(initial=0.0))
        print(f"{what}: {key}: worst error / bound = {ratio:.3f}")
        worst = max(worst, ratio)
    assert worst <= 1.0, what


CONFIGS = [  # b, l, d, u, mask, h0, use_bias
    (33, 7, 24, 32, "none", False, True),
    (65, 7, 24, 50, "holes", True, True),
    (3, 33, 24, 128, "left", True, False),
    (31, 2, 24, 160, "right", False, True),
]


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
@pytest.mark.parametrize("b,l,d,u,mask,with_h0,use_bias", CONFIGS)
def test_gru_layer_against_float64(policy, b, l, d, u, mask, with_h0, use_bias):
    torch.manual_seed(3)
    rng = np.random.default_rng(b * 1000 + u)
    layer = kl.GRU(u, return_sequences=True, return_state=True, use_bias=use_bias, dtype=policy, device=DEV)
    bf16 = policy == "mixed_bfloat16"
    rep = R.round_bf16 if bf16 else (lambda a: a.astype(np.float32).astype(np.float64))
    x = rng.standard_normal((b, l, d)).astype(np.float32).astype(np.float64)
    h0 = rep(rng.standard_normal((b, u))) if with_h0 else None
    dhs, dh_last = rep(rng.standard_normal((b, l, u))), rep(rng.standard_normal((b, u)))
    valid = _mask(mask, b, l)
    dev = lambda a, dt=torch.float32: None if a is None else torch.from_numpy(a).to(dt).to(DEV)
    xg = dev(x).requires_grad_(True)
    h0g = None if h0 is None else dev(h0).requires_grad_(True)
    layer(xg, initial_state=h0g, mask=dev(valid, torch.bool))                   # (builds the weights)
    assert [tuple(w.shape) for w in layer.weights] == [(d, 3 * u), (u, 3 * u)] + ([(2, 3 * u)] if use_bias else [])
    if use_bias:
        layer.bias.data.normal_(0.0, 0.3)
    hs, state = layer(xg, initial_state=h0g, mask=dev(valid, torch.bool))
    assert hs.shape == (b, l, u) and state.shape == (b, u) and hs.dtype == state.dtype == layer.compute_dtype
    assert G.last_route()[0] == (G.FAST if bf16 and u <= 128 else G.GENERIC)
    leaves = [xg] + layer.weights + ([h0g] if h0g is not None else [])
    grads = list(torch.autograd.grad((hs, state), leaves, (dev(dhs, hs.dtype), dev(dh_last, hs.dtype))))
    got = {"hs": hs, "h_last": state, "dx": grads[0], "dkernel": grads[1], "drk": grads[2],
           "dbias": grads[3] if use_bias else None, "dh0": grads[-1] if h0g is not None else None}
    w = [p.detach().double().cpu().numpy() for p in layer.weights]
    args = (x, w[0], w[1], w[2] if use_bias else None, valid, h0, dhs, dh_last)
    ref = R.layer(*args)
    if h0 is None:
        ref["dh0"] = None
    rounded = R.layer(*args, bf16=True) if bf16 else None
    _check(f"{policy} b{b} l{l} d{d} u{u} {mask}", got, ref, _bounds(policy, ref, rounded))


def test_return_sequences_off_returns_the_last_output_and_the_state():
    torch.manual_seed(5)
    b, l, d, u = 33, 7, 24, 50
    x = torch.randn(b, l, d, device=DEV)
    valid = torch.from_numpy(_mask("right", b, l)).to(DEV)
    valid[1] = False                                                             # one all-padding sequence
    h0 = torch.randn(b, u, device=DEV)
    seq = kl.GRU(u, return_sequences=True, return_state=True, dtype="mixed_bfloat16", device=DEV)
    last = kl.GRU(u, return_state=True, dtype="mixed_bfloat16", device=DEV)
    plain = kl.GRU(u, dtype="mixed_bfloat16", device=DEV)
    hs, state = seq(x, initial_state=h0, mask=valid)
    for other in (last, plain):
        other(x)
        other.load_state_dict(seq.state_dict())
    out, state2 = last(x, initial_state=h0, mask=valid)
    assert torch.equal(out, hs[:, -1]) and torch.equal(state2, state) and torch.equal(plain(x, h0, valid), out)
    assert not out[1].any() and torch.equal(state[1], h0[1].to(state.dtype))     # zeros out, the state carried
    assert torch.equal(plain(x, [h0], valid), out)                               # (Keras passes states as a list)


def test_autograd_grad_on_a_subset_of_inputs():
    g = torch.Generator().manual_seed(9)
    b, l, u = 33, 7, 64
    mk = lambda *s: torch.randn(*s, generator=g).bfloat16().to(DEV).requires_grad_(True)
    xz, rk, h0 = mk(b, l, 3 * u), mk(u, 3 * u), mk(b, u)
    rb = torch.randn(3 * u, generator=g).to(DEV).requires_grad_(True)
    dhs = torch.randn(b, l, u, generator=g).bfloat16().to(DEV)
    run = lambda *a: G.gru(*a[:3], initial_state=a[3], return_sequences=True)[0]
    full = torch.autograd.grad(run(xz, rk, rb, h0), (xz, rk, rb, h0), dhs)
    for subset in ((0,), (1,), (2,), (3,), (0, 3), (1, 2)):
        leaves = [(xz, rk, rb, h0)[i] for i in subset]
        got = torch.autograd.grad(run(xz, rk, rb, h0), leaves, dhs)
        assert all(torch.equal(a, full[i]) for a, i in zip(got, subset)), subset
    got = torch.autograd.grad(run(xz.detach(), rk, rb, h0.detach()), (rk, rb), dhs)    # inputs that need no gradient
    assert torch.equal(got[0], full[1]) and torch.equal(got[1], full[2])
    # gradients arriving at the final state only, at the sequence output only, and at both add up (to rounding)
    hs, state = G.gru(xz, rk, rb, initial_state=h0, return_sequences=True)
    dlast = torch.randn(b, u, generator=g).bfloat16().to(DEV)
    both = torch.autograd.grad((hs, state), xz, (dhs, dlast), retain_graph=True)[0].float()
    one = torch.autograd.grad(hs, xz, dhs, retain_graph=True)[0].float()
    two = torch.autograd.grad(state, xz, dlast)[0].float()
    assert (both - (one + two)).abs().max().item() <= 2.0 ** -6 * both.abs().max().item()


# ---- the example ----------------------------------------------------------------------------------------------------
def _example():
    spec = importlib.util.spec_from_file_location("sequential_retrieval_example",
                                                  os.path.join(ROOT, "examples", "sequential_retrieval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _loss64(q, c):
    """The in-batch softmax loss in float64: mean_i (logsumexp_j s_ij - s_ii), s = q c^T."""
    s = q @ c.T
    m = s.max(axis=1, keepdims=True)
    return float(np.mean(m[:, 0] + np.log(np.exp(s - m).sum(axis=1)) - np.diag(s)))


@pytest.mark.parametrize("fused", [False, True])
def test_sequential_retrieval_matches_float64_at_step_0_lowers_its_loss_and_serves(fused):
    ex = _example()
    b, v, d = 64, 200, 32
    run = ex.main(steps=8, batch=b, vocabulary_size=v, hidden_dim=d, dtype="bf16", fused=fused, quiet=True)
    losses = run["losses"]
    print("loss:", " ".join(f"{x:.4f}" for x in losses))
    assert len(losses) == 8 and all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]
    assert G.last_route() == (G.FAST, 32)
    # step 0 against float64 on the same weights
    ctx, label = run["context"].cpu().numpy(), run["label"].cpu().numpy()
    assert (ctx[:, -1] == 0).any() and (ctx[:, 0] != 0).all()                    # right padding, as the reference pads
    table, kernel, rk, bias, cand = (w.double().cpu().numpy() for w in run["initial_weights"])
    args = (table[ctx], kernel, rk, bias, None, None, None, np.zeros((b, d)))
    q64 = R.layer(*args)["h_last"]
    e = float(np.abs(R.layer(*args, bf16=True)["h_last"] - q64).max())
    bq = 2.0 * e + 2.0 ** -8 * np.abs(q64)                                       # the bf16 bound on the query embeddings
    c64 = cand[label]
    # propagated through s = q c^T (c rounded to bf16: 2^-9 relative) and the loss (its gradient's 1-norm over a row of
    # scores is at most 2); the unfused path rounds the scores to bf16 too, the fused one keeps them in fp32
    ds = bq @ np.abs(c64).T + (np.abs(q64) + bq) @ (2.0 ** -9 * np.abs(c64)).T
    if not fused:
        ds = ds + 2.0 ** -8 * (np.abs(q64 @ c64.T) + ds)
    bound = float(np.mean(2.0 * ds.max(axis=1))) + 1e-5
    want = _loss64(q64, c64)
    print(f"step-0 loss {losses[0]:.6f}, float64 {want:.6f}: error / bound = {abs(losses[0] - want) / bound:.3f} (bound {bound:.2e})")
    assert abs(losses[0] - want) <= bound
    # serving
    pred = run["outputs"]["predictions"]
    assert pred.shape == (b, 10) and int(pred.min()) >= 0 and int(pred.max()) <= v
    model = run["model"]
    tab = model.candidate_model.weights[0].detach().to(torch.bfloat16)
    ids = torch.arange(v + 1, device=DEV, dtype=torch.int32)
    restated = kl.BruteForceRetrieval(tab, ids, k=10, return_scores=False, device=DEV)(run["outputs"]["query_embeddings"])
    assert torch.equal(pred, restated)
