"""K19 without a GPU: the float64 restatement against torch's own scaled_dot_product_attention; the host planner under
the sanitizers, and the routes the case table claims; the dropout hash; the bounds of the table (they hold for a
result that rounds where the fast path rounds, and they reject six deliberate defects); the layers' host logic."""

import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from keras_rs_amd import layers
from tests import seq_attention_cases as T
from tests import seq_attention_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in T.CASES]


# ---- (a) the restatement against torch's CPU attention in float64 ------------------------------------------------------
@pytest.mark.parametrize("index", range(len(T.CASES)), ids=IDS)
def test_restatement_agrees_with_torch_sdpa_in_float64(index):
    case = T.CASES[index]._replace(p=0.0)
    t = T.inputs_of(case, index)
    ref = T.reference(case, t)
    live = np.isfinite(ref["lse"])                                                    # [B, H, L]
    ok = np.broadcast_to(R.allowed_mask(case.b, case.l, t["key_valid"], case.causal), (case.b, 1, case.l, case.l)).copy()
    # torch gives NaN to a row with no allowed key: let such a row see itself and take no part (its dout is zeroed)
    dead_rows = ~ok.any(axis=-1)                                                      # [B, 1, L]
    idx = np.arange(case.l)
    ok[:, :, idx, idx] |= dead_rows
    q, k, v = (torch.from_numpy(t[n]).permute(0, 2, 1, 3).clone().requires_grad_(True) for n in ("q", "k", "v"))
    dout = torch.from_numpy(np.where(live.transpose(0, 2, 1)[..., None], t["dout"], 0.0)).permute(0, 2, 1, 3)
    out = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=torch.from_numpy(ok), scale=t["scale"])
    gq, gk, gv = torch.autograd.grad(out, (q, k, v), dout)
    back = lambda x: x.detach().permute(0, 2, 1, 3).numpy()
    rows = live.transpose(0, 2, 1)                                                    # [B, L, H]
    assert np.abs(back(out) - ref["out"])[rows].max(initial=0.0) <= 1e-12
    assert (ref["out"][~rows] == 0).all() and np.isneginf(ref["lse"][~live]).all()
    for name, got in (("dq", gq), ("dk", gk), ("dv", gv)):
        assert np.abs(back(got) - ref[name]).max() <= 1e-12, name


# ---- (b) the planner ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tests/host/seq_attn_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("seq_attn_plan") / "seq_attn_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "seq_attn_plan_check.cpp"),
                    "-o", exe], check=True)

    def ask(args):
        run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
        lines = run.stdout.strip().splitlines()
        assert "0 failed checks" in lines[-1]
        return lines[:-1]

    return ask


def test_the_planner_keeps_its_invariants_over_the_grid_under_the_sanitizers(planner):
    assert planner([]) == []


def _aligned(case):
    ld = case.h * case.dh if case.pad < 0 else 3 * case.h * case.dh + case.pad
    return int(ld % 8 == 0 and (case.h * case.dh) % 8 == 0)


def test_the_claimed_routes_are_the_planners_and_reach_every_build(planner):
    args = []
    for c in T.CASES:
        args += [c.b, c.h, c.l, c.dh, 1 if c.dtype == "bf16" else 0, _aligned(c)]
    lines = planner(args)
    assert len(lines) == len(T.CASES)
    reached = set()
    for c, line in zip(T.CASES, lines):
        status, kernel, dpad, vec, oblocks, groups = map(int, line.split())
        assert (status, kernel, dpad, vec) == (0, c.route, c.dpad, c.vec), c.name
        assert groups == (math.ceil(c.l / 128) * c.b * c.h if kernel == T.FAST else c.b * c.h * c.l)
        reached.add((kernel, c.dtype, dpad, vec))
        reached.add((kernel, c.dtype, dpad, c.causal, c.mask != "none", c.p > 0))
    flags = [(c, m, d) for c in (False, True) for m in (False, True) for d in (False, True)]
    want = {(T.FAST, "bf16", dpad, vec) for dpad in (32, 64, 128) for vec in (0, 1)}
    want |= {(T.GENERIC, "bf16", 0, 0), (T.GENERIC, "fp32", 0, 0)}
    want |= {(T.FAST, "bf16", dpad, *f) for dpad in (32, 64, 128) for f in flags}
    want |= {(T.GENERIC, dt, 0, *f) for dt in ("bf16", "fp32") for f in flags}
    assert want <= reached, sorted(want - reached, key=str)


def test_the_table_is_the_stated_matrix():
    assert len(set(IDS)) == len(T.CASES) and all(c.b <= 3 and c.h <= 3 for c in T.CASES)
    bf16 = [c for c in T.CASES if c.dtype == "bf16"]
    fp32 = [c for c in T.CASES if c.dtype == "fp32"]
    assert {c.l for c in bf16} == {c.l for c in fp32} == set(T.LENGTHS)
    assert {c.dh for c in bf16} == set(T.BF16_FAST_DH) | set(T.BF16_GENERIC_DH) and {c.dh for c in fp32} == set(T.FP32_DH)
    assert {c.mask for c in T.CASES} == set(T.MASKS) and {c.p for c in T.CASES} == {0.0, 0.2}
    assert any(c.pad >= 0 and c.pad % 8 for c in bf16) and any(c.pad >= 0 and c.pad % 8 == 0 for c in bf16)
    # fully masked rows exist: left padding under the causal mask, and an all-padding sequence
    dead = lambda c: (~np.isfinite(T.reference(c, T.inputs_of(c))["lse"])).any()
    assert any(c.mask == "left" and c.causal and dead(c) for c in bf16) and any(c.mask == "allpad" and dead(c) for c in T.CASES)


# ---- (c) the dropout hash -------------------------------------------------------------------------------------------
def test_the_hash_is_the_headers_and_the_planner_headers(planner):
    seed, draw = 0x1234_5678_9ABC_DEF0, (7 << 32) + 5
    h = R.dropout_hash(seed, draw, 3, 2, 40)
    points = [(0, 0, 0), (5, 39, 17), (2, 1, 38), (4, 20, 20)]
    args = []
    for bh, i, j in points:
        args += ["hash", seed, draw, bh, i, j]
    got = [int(x) for x in planner(args)]
    assert got == [int(h[bh // 2, bh % 2, i, j]) for bh, i, j in points]
    # written out once more, in plain Python integers
    def mix(x):
        x ^= x >> 16
        x = x * 0x7FEB352D & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ x >> 16
    bh, i, j = points[1]
    base = mix(mix(mix(mix(mix((seed & 0xFFFFFFFF) ^ 0x9E3779B9) ^ (seed >> 32)) ^ (draw & 0xFFFFFFFF)) ^ (draw >> 32)) ^ bh)
    assert got[1] == mix((base + ((i << 12) | j)) & 0xFFFFFFFF)


@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_the_hash_keeps_its_share_and_draws_are_independent(p):
    n = 2 ** 20
    thr = R.drop_threshold(p)
    assert thr == math.floor(float(np.float32(p)) * 2 ** 32)
    a = R.dropout_hash(99, 4, 2, 2, 512) >= np.uint64(thr)             # 2 * 2 * 512 * 512 = 2^20 positions
    z = R.dropout_hash(99, 5, 2, 2, 512) >= np.uint64(thr)
    assert a.size == n
    pf = thr / 2 ** 32
    assert abs(a.mean() - (1 - pf)) <= 4 * math.sqrt(pf * (1 - pf) / n)
    d = 2 * pf * (1 - pf)
    assert abs((a != z).mean() - d) <= 4 * math.sqrt(d * (1 - d) / n)
    kf = R.keep_factor(99, 4, 2, 2, 512, p)
    assert set(np.unique(kf)) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}


# ---- (d), (e) the bounds --------------------------------------------------------------------------------------------
def _rounded(case, t, defect=None):
    kw = T.kwargs_of(case, t)
    bf16 = case.dtype == "bf16"
    f = R.forward(t["q"], t["k"], t["v"], bf16=bf16, defect=defect, **kw)
    g = R.backward(t["q"], t["k"], t["v"], t["dout"], bf16=bf16, defect=defect, fwd=f, **kw)
    return {"out": f["out"], "lse": f["lse"], **g}


def test_c_is_twice_the_smallest_that_holds_the_rounding_restatement():
    worst = 0.0
    for index, case in enumerate(T.CASES):
        if case.dtype == "bf16":
            t = T.inputs_of(case, index)
            ref = T.reference(case, t)
            worst = max(worst, T.worst_ratio(_rounded(case, t), ref, T.bounds(case, t, ref, c=1.0)))
    print(f"worst ratio of the rounding restatement at C = 1: {worst:.4f} (header: {T.OBSERVED_MAX}, C = {T.C})")
    assert worst <= T.OBSERVED_MAX <= T.C / 2 <= 1.01 * T.OBSERVED_MAX


def test_fp32_cases_keep_the_standing_tolerance():
    case = next(c for c in T.CASES if c.dtype == "fp32")
    t = T.inputs_of(case)
    ref = T.reference(case, t)
    bound = T.bounds(case, t, ref)
    assert T.FP32_TOL == 1e-5 and np.array_equal(bound["out"], 1e-5 + 1e-5 * np.abs(ref["out"]))


def _applies(defect, case, t):
    ok = np.broadcast_to(R.allowed_mask(case.b, case.l, t["key_valid"], case.causal), (case.b, 1, case.l, case.l))
    if defect == "causal_edge":
        return case.causal and ok[:, :, np.arange(case.l), np.arange(case.l)].any()
    if defect == "heads":
        return case.h > 1 and ok.any()
    if defect == "no_key_valid":
        free = np.broadcast_to(R.allowed_mask(case.b, case.l, None, case.causal), ok.shape)
        return bool((free & ~ok)[ok.any(axis=-1)].any()) or bool((free.any(axis=-1) & ~ok.any(axis=-1)).any())
    if defect == "draw":
        return case.p > 0 and ok.sum() >= 64
    if defect == "no_scale":
        return bool((ok.sum(axis=-1) >= 2).any())          # (a row with one allowed key has P = 1 at any scale)
    if defect == "no_delta":
        return bool(ok.any())
    raise AssertionError(defect)


@pytest.mark.parametrize("defect", ["causal_edge", "heads", "no_key_valid", "draw", "no_scale", "no_delta"])
def test_the_bounds_would_not_hide_a_defect(defect):
    applied = 0
    for index, case in enumerate(T.CASES):
        t = T.inputs_of(case, index)
        if not _applies(defect, case, t):
            continue
        ref = T.reference(case, t)
        ratio = T.worst_ratio(_rounded(case, t, defect), ref, T.bounds(case, t, ref))
        assert ratio > 1.0, f"{defect} stays inside the bound of {case.name} (worst ratio {ratio:.3f})"
        applied += 1
    assert applied >= 10


# ---- (f) the layers' host logic -------------------------------------------------------------------------------------
def test_multi_head_attention_weights_config_and_refusals():
    mha = layers.MultiHeadAttention(num_heads=3, key_dim=5, dropout=0.1, seed=4, device="cpu")
    mha.build((2, 7, 12))
    shapes = [tuple(w.shape) for w in mha.weights]
    assert shapes == [(12, 3, 5), (3, 5)] * 3 + [(3, 5, 12), (12,)]
    assert [w is x for w, x in zip(mha.weights, (mha.query_kernel, mha.query_bias, mha.key_kernel, mha.key_bias,
                                                  mha.value_kernel, mha.value_bias, mha.output_kernel, mha.output_bias))]
    lim = math.sqrt(6.0 / (3 * 12 + 5 * 12))               # glorot_uniform with Keras' fans of a [d, H, Dh] kernel
    assert 0.8 * lim < mha.query_kernel.abs().max().item() <= lim
    nobias = layers.MultiHeadAttention(2, 4, use_bias=False, device="cpu")
    nobias.build((1, 3, 8))
    assert [tuple(w.shape) for w in nobias.weights] == [(8, 2, 4)] * 3 + [(2, 4, 8)]
    cfg = mha.get_config()
    again = layers.MultiHeadAttention.from_config(cfg)
    assert again.get_config() == cfg and cfg["num_heads"] == 3 and cfg["key_dim"] == 5 and cfg["seed"] == 4
    x = torch.zeros(2, 7, 12)
    with pytest.raises(NotImplementedError, match="attention_mask"):
        mha(x, attention_mask=torch.ones(2, 7, 7))
    with pytest.raises(NotImplementedError, match="return_attention_scores"):
        mha(x, return_attention_scores=True)
    with pytest.raises(NotImplementedError, match="differ"):
        mha(x, torch.zeros(2, 9, 12))
    with pytest.raises(NotImplementedError, match="value_dim"):
        layers.MultiHeadAttention(2, 8, value_dim=4)
    assert layers.MultiHeadAttention(2, 8, value_dim=8).value_dim == 8
    with pytest.raises(ValueError, match="dropout"):
        layers.MultiHeadAttention(2, 8, dropout=1.0)


def test_transformer_decoder_weights_config_and_refusals():
    dec = layers.TransformerDecoder(intermediate_dim=20, num_heads=2, dropout=0.1, normalize_first=True,
                                    layer_norm_epsilon=1e-5, device="cpu")
    dec.build((2, 7, 12))
    shapes = [tuple(w.shape) for w in dec.weights]
    assert shapes == [(12, 2, 6), (2, 6)] * 3 + [(2, 6, 12), (12,)] + [(12,), (12,)] + [(12, 20), (20,), (20, 12), (12,)] \
        + [(12,), (12,)]
    assert dec.self_attention.key_dim == 6
    cfg = dec.get_config()
    assert layers.TransformerDecoder.from_config(cfg).get_config() == cfg
    assert cfg["normalize_first"] is True and cfg["activation"] == "relu" and cfg["intermediate_dim"] == 20
    with pytest.raises(NotImplementedError, match="encoder_sequence"):
        dec(torch.zeros(2, 7, 12), torch.zeros(2, 7, 12))
    with pytest.raises(ValueError, match="multiple"):
        layers.TransformerDecoder(8, num_heads=5, device="cpu").build((1, 4, 12))
    assert {"MultiHeadAttention", "TransformerDecoder"} <= set(layers.__all__)
