"""Dense.quantize("int8") and FeatureCross.quantize("int8") (K18) on the GPU, against the numpy restatement of their call
sequences (tests/gemm_q8_restatement.py) and against the float64 result of the FLOAT weights.

  * Dense at fp32 with a linear, ReLU or exact callable activation: bit-equal to the restatement (z + bias is one correctly
    rounded fp32 add on both sides).  Sigmoid / tanh and bf16 output: tests/test_gemm_q8_gpu.py's bound,
    gamma(3 + 8) * E + act_err [+ half a bf16 ulp].
  * FeatureCross: the low-rank product h is bit-equal to the restatement (so the second quantizer sees the same rows and the
    second integer product is the same); the output is held to that bound with the cross form's envelope.  The cross form is
    NOT asserted bit-equal even with a linear or ReLU pre-activation at fp32: the contract pins z, not how the epilogue's
    x0 * (v + diag_scale * x) + x is rounded, and the compiler may contract its multiply-adds (krs_gemm's own tests bound
    that form for the same reason).  Bit-equality is asserted where the arithmetic is pinned: z, z + bias, ReLU of it.
  * Against float64 on the float weights, the derived quantization bound (gemm_q8_restatement.quantization_bound) propagated
    through the call: activations here have Lipschitz constant <= 1, the cross form multiplies by |x0|, and the low-rank
    layer's first error passes through |kernel|:  B = B2(h^, K) + (B1(x, U) [+ half a bf16 ulp of h]) . |K|.
  * state: .bfloat16() keeps the steps fp32, a checkpoint round trip reproduces the outputs, the refusals, and an unquantized
    layer still returns exactly what dense_ops.gemm returns.
"""

import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import gemm_q8_restatement as RS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24
GAMMA = 11 * U32 / (1.0 - 11 * U32)          # the product's three roundings + the epilogue's eight operations
ACT_ERR = 1e-5
ACTS = {"linear": RS.ACT_NONE, None: RS.ACT_NONE, "relu": RS.ACT_RELU, "sigmoid": RS.ACT_SIGMOID, "tanh": RS.ACT_TANH}


def _leaky(v):
    return torch.where(v > 0, v, v * 0.25)       # a callable no kernel fuses; * 0.25 is exact


def _np_act(v, act):
    if act is _leaky:
        return np.where(v > 0, v, v * 0.25)
    return RS.activation(v, ACTS[act])


def _np(t):
    return t.detach().float().cpu().numpy()


def _x(m, d, seed, dtype=torch.float32):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn((m, d), generator=g, device=DEV)
    x[m // 2] *= 30.0                                # rows of different scale: the per-row steps differ
    return x.to(dtype)


def _half_ulp(v, bf16):
    return np.abs(v) * 2.0 ** -8 if bf16 else 0.0


@pytest.mark.parametrize("act", ["linear", "relu", "sigmoid", "tanh", _leaky], ids=["linear", "relu", "sigmoid", "tanh", "callable"])
@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_quantized_dense_follows_the_restatement_and_the_float_layer(act, policy):
    import keras_rs_amd.layers as kl

    bf16 = policy != "float32"
    m, d, units = 70, 48, 24
    layer = kl.Dense(units, activation=act, bias_initializer=kl.base.RandomUniform(-0.5, 0.5, seed=3), dtype=policy)
    x = _x(m, d, 11)
    with torch.no_grad():
        layer(x)                                     # (builds the float layer)
    w, b = _np(layer.kernel), _np(layer.bias)
    layer.quantize("int8")
    y = layer(x)
    assert not y.requires_grad and y.dtype == (torch.bfloat16 if bf16 else torch.float32) and tuple(y.shape) == (m, units)
    wq, wstep = RS.quantize_kernel(w)
    assert (layer.kernel_q.cpu().numpy() == wq).all() and (layer.kernel_step.cpu().numpy() == wstep).all()
    z, _, astep = RS.dense(_np(x), wq, wstep)
    pre = z.astype(np.float64) + b
    ref = _np_act(pre, act)
    got = _np(y).astype(np.float64)
    if not bf16 and act in ("linear", "relu", _leaky):
        assert (_np(y).view(np.uint32) == ref.astype(np.float32).view(np.uint32)).all()
    else:
        env = np.abs(z) + np.abs(b) + (1.0 if act == "sigmoid" else 0.0)
        tol = GAMMA * env + (ACT_ERR if act in ("sigmoid", "tanh") else 0.0) + _half_ulp(ref, bf16)
        assert (np.abs(got - ref) <= tol).all(), float((np.abs(got - ref) / tol).max())
    # against the float weights in float64: the quantization bound through an activation of Lipschitz constant <= 1
    exact = _np_act(_np(x).astype(np.float64) @ w.astype(np.float64) + b, act)
    qb = (RS.quantization_bound(_np(x), w, astep, wstep) + GAMMA * (np.abs(z) + np.abs(b) + 1.0)
          + (ACT_ERR if act in ("sigmoid", "tanh") else 0.0) + _half_ulp(exact, bf16))
    assert (np.abs(got - exact) <= qb).all(), float((np.abs(got - exact) / qb).max())


@pytest.mark.parametrize("act", [None, "relu", "tanh", _leaky], ids=["linear", "relu", "tanh", "callable"])
@pytest.mark.parametrize("projection,diag,policy", [(None, 0.0, "float32"), (16, 0.5, "float32"), (16, 0.0, "mixed_bfloat16"),
                                                    (None, 0.25, "mixed_bfloat16")],
                         ids=["full", "lowrank_diag", "lowrank_bf16", "full_diag_bf16"])
def test_quantized_feature_cross_follows_the_restatement_and_the_float_layer(projection, diag, policy, act):
    import keras_rs_amd.layers as kl
    from keras_rs_amd import dense_ops as D

    bf16 = policy != "float32"
    cd = torch.bfloat16 if bf16 else torch.float32
    m, d = 40, 48
    layer = kl.FeatureCross(projection_dim=projection, diag_scale=diag, pre_activation=act,
                            bias_initializer=kl.base.RandomUniform(-0.5, 0.5, seed=5), dtype=policy)
    x0, x = _x(m, d, 21, cd), _x(m, d, 22, cd)
    with torch.no_grad():
        layer(x0, x)
    down = None if projection is None else _np(layer.down_kernel)
    kern, b = _np(layer.kernel), _np(layer.bias)
    layer.quantize("int8")
    y = layer(x0, x)
    assert not y.requires_grad and y.dtype == cd and tuple(y.shape) == (m, d)
    x0n, xn = _np(x0).astype(np.float64), _np(x)
    # the restated call sequence
    h_hat, b1 = xn, 0.0
    if projection is not None:
        dq, dstep = RS.quantize_kernel(down)
        z1, _, astep1 = RS.dense(xn, dq, dstep)
        h_hat = RS.to_bf16(z1) if bf16 else z1
        h_dev, _ = D.gemm_q8(x, layer.down_kernel_q, layer.down_kernel_step, out_dtype=cd)
        assert (_np(h_dev).view(np.uint32) == h_hat.view(np.uint32)).all(), "the low-rank product is not the restatement's"
        b1 = RS.quantization_bound(xn, down, astep1, dstep) + _half_ulp(xn.astype(np.float64) @ down.astype(np.float64), bf16)
    kq, kstep = RS.quantize_kernel(kern)
    z2, _, astep2 = RS.dense(h_hat, kq, kstep)
    u = _np_act(z2.astype(np.float64) + b, act)
    ref = x0n * (u + diag * xn) + xn
    got = _np(y).astype(np.float64)
    act_err = ACT_ERR if act == "tanh" else 0.0
    u_round = _half_ulp(u, bf16) if act is _leaky else 0.0      # the callable's output is rounded to the compute dtype
    env = np.abs(x0n) * (np.abs(z2) + np.abs(b) + np.abs(diag * xn)) + np.abs(xn)
    tol = GAMMA * env + np.abs(x0n) * (act_err + u_round) + _half_ulp(ref, bf16)
    assert (np.abs(got - ref) <= tol).all(), float((np.abs(got - ref) / np.maximum(tol, 1e-300)).max())
    # against the float weights in float64
    h_true = xn.astype(np.float64) if projection is None else xn.astype(np.float64) @ down.astype(np.float64)
    exact = x0n * (_np_act(h_true @ kern.astype(np.float64) + b, act) + diag * xn) + xn
    b_total = RS.quantization_bound(h_hat, kern, astep2, kstep) + (b1 @ np.abs(kern.astype(np.float64)) if projection is not None else 0.0)
    qb = np.abs(x0n) * (b_total + act_err + _half_ulp(u, bf16)) + GAMMA * (env + np.abs(x0n)) + _half_ulp(exact, bf16)
    assert (np.abs(got - exact) <= qb).all(), float((np.abs(got - exact) / qb).max())


def test_quantized_layers_keep_fp32_steps_round_trip_a_checkpoint_and_refuse_what_they_must():
    import keras_rs_amd.layers as kl

    x = _x(33, 32, 5)
    dense = kl.Dense(16, activation="relu", dtype="float32")
    cross = kl.FeatureCross(projection_dim=16, dtype="float32")
    with torch.no_grad():
        dense(x), cross(x, x)
    # a kernel with an infinity: ValueError, and the layer still runs in float
    kept = dense.kernel.detach().clone()
    with torch.no_grad():
        dense.kernel[0, 0] = float("inf")
    with pytest.raises(ValueError, match="infinity"):
        dense.quantize("int8")
    assert dense.quantization_mode is None and dense.kernel is not None
    with torch.no_grad():
        dense.kernel.copy_(kept)
    dense.quantize("int8"), cross.quantize("int8")
    for layer in (dense, cross):
        with pytest.raises(RuntimeError, match="already quantized"):
            layer.quantize("int8")
    yd, yc = dense(x), cross(x, x)
    # an input that requires grad is refused by name while grad mode is on, and served under no_grad
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match=dense.name):
        dense(xg)
    with pytest.raises(RuntimeError, match=cross.name):
        cross(x, xg)
    with torch.no_grad():
        assert torch.equal(dense(xg), yd) and torch.equal(cross(xg, xg), yc)
    # a checkpoint round trip through a second layer quantized the same way reproduces the outputs
    dense2 = kl.Dense(16, activation="relu", dtype="float32")
    cross2 = kl.FeatureCross(projection_dim=16, dtype="float32")
    with torch.no_grad():
        dense2(x), cross2(x, x)
    dense2.quantize("int8"), cross2.quantize("int8")
    assert not torch.equal(dense2(x), yd)
    dense2.load_state_dict(dense.state_dict()), cross2.load_state_dict(cross.state_dict())
    assert torch.equal(dense2(x), yd) and torch.equal(cross2(x, x), yc)
    # a dtype cast keeps the steps fp32 and the layer serving
    steps = dense.kernel_step.clone()
    dense.bfloat16(), cross.bfloat16()
    assert dense.kernel_step.dtype == cross.kernel_step.dtype == cross.down_kernel_step.dtype == torch.float32
    assert torch.equal(dense.kernel_step, steps) and dense.kernel_q.dtype == torch.int8
    assert torch.isfinite(dense(x)).all() and torch.isfinite(cross(x, x)).all()
    # a NaN in the input poisons its row and no other
    bad = x.clone()
    bad[7, 3] = float("nan")
    yb = dense2(bad)
    assert torch.isnan(yb[7]).all() and torch.equal(torch.cat([yb[:7], yb[8:]]), torch.cat([yd[:7], yd[8:]]))
    # the same through FeatureCross: the NaN row of x passes the low-rank product as a NaN row of h, is marked again by the
    # second quantizer and comes out of the cross epilogue as NaNs
    for y_bad in (cross2(x, bad), cross2(bad, bad)):
        assert torch.isnan(y_bad[7]).all() and torch.equal(torch.cat([y_bad[:7], y_bad[8:]]), torch.cat([yc[:7], yc[8:]]))
    relu_cross = kl.FeatureCross(pre_activation="relu", dtype="float32")         # full rank; ReLU would turn a NaN into 0
    with torch.no_grad():
        relu_cross(x, x)
    relu_cross.quantize("int8")
    good = relu_cross(x * 0.0 + 1.0, x)
    y_bad = relu_cross(x * 0.0 + 1.0, bad)                                       # (x0 = 1 everywhere: only the rule can make NaNs)
    assert torch.isnan(y_bad[7]).all() and torch.equal(torch.cat([y_bad[:7], y_bad[8:]]), torch.cat([good[:7], good[8:]]))


def test_an_unquantized_layer_returns_what_it_returned_before():
    import keras_rs_amd.layers as kl
    from keras_rs_amd import dense_ops as D

    x = _x(65, 40, 9)
    for policy, cd in (("float32", torch.float32), ("mixed_bfloat16", torch.bfloat16)):
        layer = kl.Dense(24, activation="relu", dtype=policy)
        with torch.no_grad():
            y = layer(x)
            want, _ = D.gemm(x.to(cd), layer.kernel.to(cd), bias=layer.bias, act=RS.ACT_RELU)
        assert layer.quantization_mode is None and torch.equal(y, want)
        y_grad = layer(x.clone().requires_grad_(True))
        assert y_grad.requires_grad


def test_the_example_serves_a_small_batch_with_int8_tables_and_int8_layers():
    import keras_rs_amd.layers as kl

    spec = importlib.util.spec_from_file_location("dlrm_dcn_v2", os.path.join(ROOT, "examples", "dlrm_dcn_v2.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    batch, dim = 64, 16
    hots = [3, 1, 2, 5, 1, 2]
    model = ex.build_model(batch, [500, 70, 300, 900, 60, 40], hots, embedding_dim=dim, projection=16, cross_layers=2,
                           bottom=(32, dim), top=(32, 16, 1), table_optimizer=kl.SGD(0.1))
    x, _ = ex.synthetic_batch(batch, 13, 40, hots, DEV, seed=4)
    diff, nbytes, qbytes, diff_all = ex.quantize_and_compare(model, x, dense=True)
    print(f"largest |prediction difference|: int8 tables {diff:.3e}, int8 tables + layers {diff_all:.3e}; "
          f"table bytes {nbytes} -> {qbytes}")
    assert np.isfinite(diff) and np.isfinite(diff_all) and 0 < qbytes < nbytes
    assert 0.0 <= diff <= 1.0 and 0.0 <= diff_all <= 1.0            # (predictions are probabilities)
    quantized = [m for m in model.modules() if isinstance(m, (kl.Dense, kl.FeatureCross))]
    assert len(quantized) == 2 + 2 + 3 and all(m.quantization_mode == "int8" for m in quantized)
    # the three-entry form is what it was
    model2 = ex.build_model(batch, [500, 70, 300, 900, 60, 40], hots, embedding_dim=dim, projection=16, cross_layers=2,
                            bottom=(32, dim), top=(32, 16, 1), table_optimizer=kl.SGD(0.1))
    assert len(ex.quantize_and_compare(model2, x)) == 3
