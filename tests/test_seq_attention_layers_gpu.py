"""MultiHeadAttention, TransformerDecoder and examples/sas_rec.py on the GPU: against a float64 torch-CPU composition of
the same weights, under autograd.grad on a subset of inputs, with training-mode dropout (reproducible per draw, captured
in a HIP graph), and the example end to end.

Tolerances of the layer comparisons.  float32 policy: the project's standing 1e-5 per fused op, eight
ops in a chain here (three projections side by side, attention, output projection, two norms, two Dense) and a layer
norm that can double an absolute error of an O(1) row: 2e-4, absolute plus relative.  mixed_bfloat16: every op rounds
its O(1) output to bf16, half an ulp 2^-9 relative, and the attention stays within about 2^-8 (the K19 matrix test);
ten roundings in a chain, doubled by the norms: 10 * 2 * 2^-9 = 4e-2.  Gradients: the backward walks the same ten ops
again, rounding each intermediate gradient to bf16, and what it multiplies them with are the saved activations, which
carry the forward's ten roundings: twenty in a chain, 8e-2 (float32: 4e-4), taken relative to the largest entry of the
gradient, because every backward product mixes the entries of a row.  A wrong mask, head layout or residual order is an
O(1) error; the float32 runs, the same code path at one-hundredth of the tolerance, are the sharp check of the
arithmetic."""

import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from keras_rs_amd import layers as kl
from keras_rs_amd import sequence_ops as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"float32": 2e-4, "mixed_bfloat16": 4e-2}


def _close(what, got, ref, tol):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = ((got - ref).abs() / (tol + tol * ref.abs())).max().item()
    print(f"{what}: worst error / bound = {err:.3f}")
    assert math.isfinite(err) and err <= 1.0, what


def _mask(b, l, left=False):
    lengths = torch.tensor([max(1, l - (x * l) // 3) for x in range(b)])
    pos = torch.arange(l)[None, :]
    return (pos >= (l - lengths)[:, None]) if left else (pos < lengths[:, None])


# ---- float64 compositions on the CPU --------------------------------------------------------------------------------
def _attention64(q, k, v, mask, causal):
    """[B, L, H, Dh] float64; K19's rule for a row with no allowed key (zero output, no gradient)."""
    b, l, h, dh = q.shape
    ok = torch.ones(b, 1, l, l, dtype=torch.bool)
    if causal:
        ok = ok & torch.tril(torch.ones(l, l, dtype=torch.bool))
    if mask is not None:
        ok = ok & mask.reshape(b, 1, 1, l)
    s = torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(dh)
    dead = ~ok.any(-1, keepdim=True)
    s = s.masked_fill(~ok, -math.inf).masked_fill(dead, 0.0)
    p = torch.softmax(s, dim=-1) * ok
    return torch.einsum("bhij,bjhd->bihd", p, v)


def _mha64(w, x, mask, causal):
    wq, bq, wk, bk, wv, bv, wo, bo = w
    q = torch.einsum("bld,dhe->blhe", x, wq) + bq
    k = torch.einsum("bld,dhe->blhe", x, wk) + bk
    v = torch.einsum("bld,dhe->blhe", x, wv) + bv
    return torch.einsum("blhe,hed->bld", _attention64(q, k, v, mask, causal), wo) + bo


def _decoder64(w, x, mask, normalize_first, eps):
    ln = lambda t, g, b: torch.nn.functional.layer_norm(t, (t.shape[-1],), g, b, eps)
    att, (g1, b1), (k1, c1, k2, c2), (g2, b2) = w[:8], w[8:10], w[10:14], w[14:16]
    res = x
    y = ln(x, g1, b1) if normalize_first else x
    y = _mha64(att, y, mask, True) + res
    if not normalize_first:
        y = ln(y, g1, b1)
    res = y
    z = ln(y, g2, b2) if normalize_first else y
    z = (torch.relu(z @ k1 + c1) @ k2 + c2) + res
    return z if normalize_first else ln(z, g2, b2)


def _w64(layer):
    return [w.detach().double().cpu().requires_grad_(True) for w in layer.weights]


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
@pytest.mark.parametrize("heads,key_dim,l", [(2, 16, 37), (1, 50, 50)])
def test_multi_head_attention_against_float64(policy, heads, key_dim, l):
    torch.manual_seed(3)
    b, d = 3, heads * key_dim
    layer = kl.MultiHeadAttention(heads, key_dim, dropout=0.3, seed=1, dtype=policy, device=DEV)
    x = torch.randn(b, l, d)
    mask = _mask(b, l, left=True)
    xg = x.to(DEV).requires_grad_(True)
    out = layer(xg, padding_mask=mask.to(DEV), use_causal_mask=True)            # (not training: no dropout)
    assert out.shape == (b, l, d) and out.dtype == layer.compute_dtype
    for bias in (layer.query_bias, layer.key_bias, layer.value_bias, layer.output_bias):
        bias.data.normal_(0.0, 0.1)
    out = layer(xg, padding_mask=mask.to(DEV), use_causal_mask=True)
    up = torch.randn(b, l, d)
    grads = torch.autograd.grad(out, [xg] + layer.weights, up.to(DEV).to(out.dtype))
    w = _w64(layer)
    x64 = x.double().requires_grad_(True)
    ref = _mha64(w, x64, mask, True)
    ref_grads = torch.autograd.grad(ref, [x64] + w, up.double())
    tol = TOL[policy]
    _close("out", out, ref, tol)
    for name, g, r in zip(["dx"] + [f"dw{i}" for i in range(8)], grads, ref_grads):
        _close(name, g, r, 2 * tol * max(1.0, r.abs().max().item()))


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
@pytest.mark.parametrize("normalize_first", [False, True])
def test_transformer_decoder_against_float64(policy, normalize_first):
    torch.manual_seed(5)
    b, l, d = 2, 45, 48
    layer = kl.TransformerDecoder(64, num_heads=3, dropout=0.2, normalize_first=normalize_first, seed=2, dtype=policy,
                                  device=DEV)
    x = torch.randn(b, l, d)
    mask = _mask(b, l)
    xg = x.to(DEV).requires_grad_(True)
    layer(xg, decoder_padding_mask=mask.to(DEV))
    for wt in layer.weights:
        if wt.dim() == 1 or wt.shape == (3, 16):
            wt.data.add_(torch.randn_like(wt) * 0.1)
    out = layer(xg, decoder_padding_mask=mask.to(DEV))
    up = torch.randn(b, l, d)
    grads = torch.autograd.grad(out, [xg] + layer.weights, up.to(DEV).to(out.dtype))
    w = _w64(layer)
    x64 = x.double().requires_grad_(True)
    ref = _decoder64(w, x64, mask, normalize_first, 1e-5)
    ref_grads = torch.autograd.grad(ref, [x64] + w, up.double())
    tol = TOL[policy]
    _close("out", out, ref, tol)
    for name, g, r in zip(["dx"] + [f"dw{i}" for i in range(16)], grads, ref_grads):
        _close(name, g, r, 2 * tol * max(1.0, r.abs().max().item()))


def test_autograd_grad_on_a_subset_of_inputs():
    g = torch.Generator().manual_seed(9)
    mk = lambda: torch.randn(2, 70, 2, 32, generator=g).bfloat16().to(DEV).requires_grad_(True)
    q, k, v = mk(), mk(), mk()
    dout = torch.randn(2, 70, 2, 32, generator=g).bfloat16().to(DEV)
    draw = torch.zeros(1, dtype=torch.int64, device=DEV)
    kw = dict(causal=True, dropout_p=0.2, seed=8)
    full = torch.autograd.grad(S.seq_attention(q, k, v, draw=draw.clone(), **kw), (q, k, v), dout)
    for subset in ((0,), (1,), (2,), (0, 2), (1, 2)):
        leaves = [(q, k, v)[i] for i in subset]
        got = torch.autograd.grad(S.seq_attention(q, k, v, draw=draw.clone(), **kw), leaves, dout)
        assert all(torch.equal(a, full[i]) for a, i in zip(got, subset)), subset
    qd = q.detach()                                                               # an input that needs no gradient
    got = torch.autograd.grad(S.seq_attention(qd, k, v, draw=draw.clone(), **kw), (k, v), dout)
    assert torch.equal(got[0], full[1]) and torch.equal(got[1], full[2])


def test_training_dropout_reproduces_per_draw_and_moves_on():
    torch.manual_seed(11)
    layer = kl.MultiHeadAttention(2, 32, dropout=0.5, seed=6, dtype="mixed_bfloat16", device=DEV)
    x = torch.randn(2, 40, 64, device=DEV)
    plain = layer(x)
    counter = layer.draw_counter()
    assert counter.item() == 0                                                    # (an inference call draws nothing)
    a = layer(x, training=True)
    assert counter.item() == 1
    z = layer(x, training=True)
    assert counter.item() == 2
    counter.zero_()
    again = layer(x, training=True)
    assert torch.equal(a, again) and not torch.equal(a, z) and not torch.equal(a, plain)
    other = kl.MultiHeadAttention(2, 32, dropout=0.5, seed=7, dtype="mixed_bfloat16", device=DEV)
    other(x)
    other.load_state_dict(layer.state_dict())
    assert torch.equal(other(x), plain) and not torch.equal(other(x, training=True), a)   # another seed, another mask


def test_a_captured_training_step_replays_with_the_counter_advancing():
    g = torch.Generator().manual_seed(13)
    mk = lambda: torch.randn(2, 66, 2, 64, generator=g).bfloat16().to(DEV)
    q0, k0, v0 = mk(), mk(), mk()
    target = mk()
    valid = _mask(2, 66).to(DEV)
    q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
    draw = torch.zeros(1, dtype=torch.int64, device=DEV)

    def step():
        out = S.seq_attention(q, k, v, key_valid=valid, causal=True, dropout_p=0.25, seed=21, draw=draw)
        loss = (out.float() - target.float()).square().mean()
        grads = torch.autograd.grad(loss, (q, k, v))
        with torch.no_grad():
            for p, gr in zip((q, k, v), grads):
                p.sub_(gr * 8.0)

    def reset():
        with torch.no_grad():
            q.copy_(q0), k.copy_(k0), v.copy_(v0), draw.zero_()

    eager = []
    for _ in range(3):
        step()
        eager.append([t.detach().clone() for t in (q, k, v)] + [draw.clone()])
    assert not torch.equal(eager[0][0], eager[1][0]) and eager[2][3].item() == 3
    reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    reset()
    for n in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((q, k, v, draw), eager[n]):
            assert torch.equal(got.detach(), want), f"replay {n}"


# ---- the example ----------------------------------------------------------------------------------------------------
def _sas_rec():
    spec = importlib.util.spec_from_file_location("sas_rec_example", os.path.join(ROOT, "examples", "sas_rec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sas_rec_lowers_its_loss_and_serves_the_last_token():
    ex = _sas_rec()
    run = ex.main(steps=30, batch=64, vocabulary_size=500, length=50, hidden_dim=50, num_heads=1, num_layers=2,
                  dtype="bf16", quiet=True)
    losses = run["losses"]
    print("loss:", " ".join(f"{x:.3f}" for x in losses))
    assert all(math.isfinite(x) for x in losses) and np.mean(losses[-5:]) < np.mean(losses[:5])
    out, inputs, model = run["outputs"], run["inputs"], run["model"]
    mask = inputs["padding_mask"].cpu().numpy()
    assert (~mask[:, 0]).any() and mask[:, -1].all()                              # left padding: fully masked rows exist
    last = np.array([np.nonzero(row)[0].max() for row in mask])
    emb = out["item_sequence_embedding"]
    assert emb.shape == (64, 50, 50) and torch.isfinite(emb.float()).all()
    query = emb[torch.arange(64, device=DEV), torch.from_numpy(last).to(DEV)]
    table = model.item_embedding.weights[0].detach().to(emb.dtype)
    ids = torch.arange(500, device=DEV, dtype=torch.int32)
    restated = kl.BruteForceRetrieval(table, ids, k=10, return_scores=False, device=DEV)(query)
    assert out["predictions"].shape == (64, 10) and torch.equal(out["predictions"], restated)
