"""LayerNormalization, TransformerDecoder and norm_ops.residual_layer_norm on the GPU: the layer with center / scale off
against float64; the decoder block on K22 (FUSE_NORM on) against the torch composition (off) in eval mode; training-mode
dropout (reproducible per (seed, draw), captured in a HIP graph); autograd.grad on subsets of the inputs.

Tolerances of the decoder comparison are those of tests/test_seq_attention_layers_gpu.py (2e-4 under float32, 4e-2 under
mixed_bfloat16, gradients twice that relative to their largest entry): both sides are the same ten-op chain and differ
only in where the glue rounds."""

import math

import pytest
import torch

from keras_rs_amd import layers as kl
from keras_rs_amd import norm_ops
from keras_rs_amd.layers import sequence

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {"float32": 2e-4, "mixed_bfloat16": 4e-2}


def _close(what, got, ref, tol):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = ((got - ref).abs() / (tol + tol * ref.abs())).max().item()
    print(f"{what}: worst error / bound = {err:.3f}")
    assert math.isfinite(err) and err <= 1.0, what


@pytest.fixture
def fuse_switch():
    old = sequence.FUSE_NORM
    yield lambda on: setattr(sequence, "FUSE_NORM", bool(on))
    sequence.FUSE_NORM = old


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
@pytest.mark.parametrize("center,scale", [(True, True), (False, True), (True, False), (False, False)])
def test_layer_normalization_against_float64(policy, center, scale):
    torch.manual_seed(3)
    layer = kl.LayerNormalization(1e-5, center=center, scale=scale, dtype=policy, device=DEV)
    x = torch.randn(3, 21, 50)
    xc = x.to(DEV).to(layer.compute_dtype).requires_grad_(True)
    layer(xc)
    for w in layer.weights:
        w.data.add_(torch.randn_like(w) * 0.3)
    out = layer(xc)
    assert out.shape == x.shape and out.dtype == layer.compute_dtype
    assert norm_ops.last_route()[0] in (norm_ops.VEC, norm_ops.ELEM)            # it ran on K22
    up = torch.randn(3, 21, 50).to(layer.compute_dtype)
    grads = torch.autograd.grad(out, [xc] + layer.weights, up.to(DEV))
    x64 = xc.detach().double().cpu().requires_grad_(True)
    w64 = [w.detach().double().cpu().requires_grad_(True) for w in layer.weights]
    gamma = w64[0] if scale else None
    beta = w64[-1] if center else None
    ref = torch.nn.functional.layer_norm(x64, (50,), gamma, beta, 1e-5)
    ref_grads = torch.autograd.grad(ref, [x64] + w64, up.double())
    tol = 1e-5 if policy == "float32" else 2.0 ** -7        # one op: the standing fp32 tolerance; two bf16 roundings
    _close("out", out, ref, tol)
    for name, g, r in zip(["dx", "dw0", "dw1"], grads, ref_grads):
        _close(name, g, r, tol * max(1.0, r.abs().max().item()))


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
@pytest.mark.parametrize("normalize_first", [False, True])
def test_transformer_decoder_fused_against_the_torch_composition(policy, normalize_first, fuse_switch):
    torch.manual_seed(5)
    b, l, d = 2, 45, 48
    layer = kl.TransformerDecoder(64, num_heads=3, dropout=0.2, normalize_first=normalize_first, seed=2, dtype=policy,
                                  device=DEV)
    x = torch.randn(b, l, d)
    lengths = torch.tensor([l, l - 13])
    mask = (torch.arange(l)[None, :] < lengths[:, None]).to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    layer(xg, decoder_padding_mask=mask)
    for wt in layer.weights:
        if wt.dim() == 1 or wt.shape == (3, 16):
            wt.data.add_(torch.randn_like(wt) * 0.1)
    up = torch.randn(b, l, d).to(DEV).to(layer.compute_dtype)
    runs = {}
    for on in (True, False):
        fuse_switch(on)
        out = layer(xg, decoder_padding_mask=mask)
        runs[on] = (out, torch.autograd.grad(out, [xg] + layer.weights, up))
    assert layer.draw_counter().item() == 0                                     # (eval mode draws nothing)
    tol = TOL[policy]
    _close("out", runs[True][0], runs[False][0], tol)
    for name, g, r in zip(["dx"] + [f"dw{i}" for i in range(16)], runs[True][1], runs[False][1]):
        _close(name, g, r, 2 * tol * max(1.0, r.abs().max().item()))


@pytest.mark.parametrize("normalize_first", [False, True])
def test_training_dropout_reproduces_per_seed_and_draw_and_moves_on(normalize_first):
    torch.manual_seed(11)
    mk = lambda seed: kl.TransformerDecoder(64, num_heads=2, dropout=0.5, normalize_first=normalize_first, seed=seed,
                                            dtype="mixed_bfloat16", device=DEV)
    layer = mk(6)
    x = torch.randn(2, 40, 64, device=DEV)
    plain = layer(x)
    own, attn = layer.draw_counter(), layer.self_attention.draw_counter()
    assert own.item() == 0 and attn.item() == 0
    a = layer(x, training=True)
    assert own.item() == 2 and attn.item() == 1                                  # two residual dropouts, one attention
    z = layer(x, training=True)
    assert own.item() == 4 and attn.item() == 2
    own.zero_(), attn.zero_()
    again = layer(x, training=True)
    assert torch.equal(a, again) and not torch.equal(a, z) and not torch.equal(a, plain)
    own.zero_()                                                                   # (the attention's counter stays at 1)
    assert not torch.equal(layer(x, training=True), a)
    other = mk(7)
    other(x)
    other.load_state_dict(layer.state_dict())
    assert torch.equal(other(x), plain) and not torch.equal(other(x, training=True), a)   # another seed, another mask


def test_the_two_residual_dropouts_draw_different_masks():
    x = torch.ones(64, 128, dtype=torch.bfloat16, device=DEV)
    draw = torch.zeros(1, dtype=torch.int64, device=DEV)
    kw = dict(epsilon=0.0, dropout_p=0.5, norm=False)
    a = norm_ops.residual_layer_norm(x, seed=9 + sequence._ATTN_RESIDUAL_SEED, draw=draw.clone(), **kw)
    b = norm_ops.residual_layer_norm(x, seed=9 + sequence._FF_RESIDUAL_SEED, draw=draw.clone(), **kw)
    assert set(a.unique().tolist()) == {0.0, 2.0} and 0.4 < (a != b).float().mean().item() < 0.6


def test_a_captured_training_step_of_a_block_replays_with_the_counters_advancing():
    torch.manual_seed(13)
    layer = kl.TransformerDecoder(96, num_heads=2, dropout=0.25, normalize_first=True, seed=21, dtype="mixed_bfloat16",
                                  device=DEV)
    x = torch.randn(2, 66, 64, device=DEV)
    target = torch.randn(2, 66, 64, device=DEV)
    mask = (torch.arange(66)[None, :] < torch.tensor([66, 40])[:, None]).to(DEV)
    layer(x, decoder_padding_mask=mask)
    weights = layer.weights
    start = [w.detach().clone() for w in weights]
    counters = (layer.draw_counter(), layer.self_attention.draw_counter())

    def step():
        out = layer(x, decoder_padding_mask=mask, training=True)
        loss = (out.float() - target).square().mean()
        grads = torch.autograd.grad(loss, weights)
        with torch.no_grad():
            for p, gr in zip(weights, grads):
                p.sub_(gr.to(p.dtype) * 0.5)

    def reset():
        with torch.no_grad():
            for p, s in zip(weights, start):
                p.copy_(s)
            for c in counters:
                c.zero_()

    eager = []
    for _ in range(3):
        step()
        eager.append([w.detach().clone() for w in weights] + [c.clone() for c in counters])
    assert not torch.equal(eager[0][0], eager[1][0]) and eager[2][-2].item() == 6 and eager[2][-1].item() == 3
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
        for got, want in zip(list(weights) + list(counters), eager[n]):
            assert torch.equal(got.detach(), want), f"replay {n}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_autograd_grad_on_subsets_of_the_inputs(dtype):
    g = torch.Generator().manual_seed(9)
    shape = (3, 23, 50)
    x, res = (torch.randn(shape, generator=g).to(dtype).to(DEV).requires_grad_(True) for _ in range(2))
    gamma, beta = (torch.randn(50, generator=g).to(DEV).requires_grad_(True) for _ in range(2))
    dy, dsum = (torch.randn(shape, generator=g).to(dtype).to(DEV) for _ in range(2))
    draw = torch.zeros(1, dtype=torch.int64, device=DEV)
    kw = dict(epsilon=1e-5, dropout_p=0.2, seed=8, return_sum=True)
    leaves = (x, res, gamma, beta)
    call = lambda *a: norm_ops.residual_layer_norm(*a, draw=draw.clone(), **kw)
    full = torch.autograd.grad(call(*leaves), leaves, (dy, dsum))
    for subset in ((0,), (1,), (2,), (3,), (0, 1), (2, 3), (0, 3), (1, 2)):
        got = torch.autograd.grad(call(*leaves), [leaves[i] for i in subset], (dy, dsum))
        assert all(torch.equal(a, full[i]) for a, i in zip(got, subset)), subset
    got = torch.autograd.grad(call(x.detach(), res, gamma.detach(), beta), (res, beta), (dy, dsum))
    assert torch.equal(got[0], full[1]) and torch.equal(got[1], full[3])
    # only one of the two outputs reaches the loss
    y, s = call(*leaves)
    only_y = torch.autograd.grad(y, leaves, dy)
    y, s = call(*leaves)
    only_s = torch.autograd.grad(s, (x, res), dsum, allow_unused=True)
    assert torch.equal(only_s[1], dsum) and torch.equal(only_y[3], full[3]) and torch.equal(only_y[2], full[2])
    keep = only_s[0] != 0
    assert torch.equal(only_s[0][keep].float(), (dsum.float() * 1.25).to(dtype)[keep].float())
    # the add form: without dropout both inputs take dsum itself; any leading shape; no gradient, nothing saved
    a = norm_ops.residual_layer_norm(x, res, epsilon=0.0, norm=False)
    gx, gr = torch.autograd.grad(a, (x, res), dsum)
    assert torch.equal(a, (x.float() + res.float()).to(dtype)) and torch.equal(gx, dsum) and torch.equal(gr, dsum)
    with torch.no_grad():
        flat = norm_ops.residual_layer_norm(x.reshape(-1, 50), None, gamma, beta, epsilon=1e-5)
        deep = norm_ops.residual_layer_norm(x.reshape(3, 23, 1, 50), None, gamma, beta, epsilon=1e-5)
    assert torch.equal(flat.reshape(shape), deep.reshape(shape)) and not flat.requires_grad
    # with p = 0, dx and dres are one tensor
    y = norm_ops.residual_layer_norm(x, res, gamma, beta, epsilon=1e-5)
    gx, gr = torch.autograd.grad(y, (x, res), dy)
    assert torch.equal(gx, gr)
