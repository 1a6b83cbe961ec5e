"""K20 without a GPU: the float64 restatement (forward and hand-written backward) against torch.nn.GRU and against torch
autograd through a plain per-step loop; the host planner under the sanitizers, and the routes the case table claims;
the C ABI's four entries; the bounds of the table (recomputed, and rejecting seven deliberate defects); the layer's host
logic."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers
from keras_rs_amd.layers import base
from tests import gru_cases as T
from tests import gru_restatement as R
from tests.test_capi_symbols import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in T.CASES]
GRU_SYMBOLS = ("krs_gru_reserve_bytes", "krs_gru_fwd", "krs_gru_bwd", "krs_gru_last_route")


def _to_torch_order(m, u):
    """columns (or entries) z | r | h -> torch's r | z | n."""
    return np.concatenate([m[..., u:2 * u], m[..., :u], m[..., 2 * u:]], axis=-1)


def _torch_gru(t, u):
    """torch.nn.GRU in float64 whose input IS xz: weight_ih is the permutation from Keras' gate order to torch's, so the
    gradient at its input is dxz in Keras' order."""
    gru = torch.nn.GRU(3 * u, u, batch_first=True, bias=True).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.from_numpy(_to_torch_order(np.eye(3 * u), u).T.copy()))
        gru.bias_ih_l0.zero_()
        gru.weight_hh_l0.copy_(torch.from_numpy(_to_torch_order(t["rk"], u).T.copy()))
        gru.bias_hh_l0.copy_(torch.from_numpy(_to_torch_order(np.zeros(3 * u) if t["rb"] is None else t["rb"], u)))
    return gru


def _from_torch(gru, u):
    """(drk [U, 3U], drb [3U]) in Keras' order from torch's weight_hh / bias_hh gradients (r | z | n rows)."""
    back = lambda m: np.concatenate([m[..., u:2 * u], m[..., :u], m[..., 2 * u:]], axis=-1)
    return back(gru.weight_hh_l0.grad.numpy().T), back(gru.bias_hh_l0.grad.numpy())


# ---- (a) the restatement against torch.nn.GRU in float64 ---------------------------------------------------------------
UNMASKED = [i for i, c in enumerate(T.CASES) if c.mask == "none"]
RIGHT = [i for i, c in enumerate(T.CASES) if c.mask == "right"]


@pytest.mark.parametrize("index", UNMASKED, ids=[IDS[i] for i in UNMASKED])
def test_restatement_agrees_with_torch_gru_in_float64(index):
    case = T.CASES[index]
    t, ref = T.TABLE[index][0], T.TABLE[index][1]
    u = case.u
    gru = _torch_gru(t, u)
    xz = torch.from_numpy(t["xz"]).requires_grad_(True)
    h0 = torch.zeros(case.b, u, dtype=torch.float64) if t["h0"] is None else torch.from_numpy(t["h0"])
    h0 = h0.clone().requires_grad_(True)
    out, hn = gru(xz, h0[None])
    loss = 0.0
    if t["dhs"] is not None:
        loss = loss + (out * torch.from_numpy(t["dhs"])).sum()
    if t["dh_last"] is not None:
        loss = loss + (hn[0] * torch.from_numpy(t["dh_last"])).sum()
    loss.backward()
    drk, drb = _from_torch(gru, u)
    assert np.abs(out.detach().numpy() - ref["hs"]).max() <= 1e-12
    assert np.abs(hn[0].detach().numpy() - ref["h_last"]).max() <= 1e-12
    assert np.abs(xz.grad.numpy() - ref["dxz"]).max() <= 1e-12
    assert np.abs(h0.grad.numpy() - ref["dh0"]).max() <= 1e-12
    assert np.abs(drk - ref["drk"]).max() <= 1e-12 * max(1.0, np.abs(ref["drk"]).max())
    assert np.abs(drb - ref["drb"]).max() <= 1e-12 * max(1.0, np.abs(ref["drb"]).max())


@pytest.mark.parametrize("index", RIGHT, ids=[IDS[i] for i in RIGHT])
def test_right_padding_agrees_with_torch_packed_sequences(index):
    # pack_padded_sequence stops every row at its length: its final state is the state carried through the padding,
    # and its (zero-padded) outputs equal the restatement's at the valid steps
    case = T.CASES[index]
    t, ref = T.TABLE[index][0], T.TABLE[index][1]
    u = case.u
    lengths = torch.from_numpy(t["valid"].sum(axis=1).astype(np.int64))
    gru = _torch_gru(t, u)
    xz = torch.from_numpy(t["xz"]).requires_grad_(True)
    h0 = torch.zeros(case.b, u, dtype=torch.float64) if t["h0"] is None else torch.from_numpy(t["h0"])
    packed = torch.nn.utils.rnn.pack_padded_sequence(xz, lengths, batch_first=True, enforce_sorted=False)
    out, hn = gru(packed, h0[None])
    out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=case.l)
    v = t["valid"].astype(bool)
    assert np.abs(hn[0].detach().numpy() - ref["h_last"]).max() <= 1e-12
    assert np.abs(out.detach().numpy() - ref["hs"])[v].max() <= 1e-12
    # the gradient of the final state alone (the masked outputs repeat the last valid one: the loop test covers that)
    dlast = torch.from_numpy(np.random.default_rng(index).standard_normal((case.b, u)))
    (gx,) = torch.autograd.grad(hn[0], xz, dlast)
    f = R.forward(t["xz"], t["rk"], t["rb"], t["valid"], t["h0"])
    g = R.backward(t["rk"], t["valid"], t["h0"], f, None, dlast.numpy())
    assert np.abs(gx.numpy() - g["dxz"]).max() <= 1e-12


# ---- (b) every mask against torch autograd through a plain per-step loop ---------------------------------------------
@pytest.mark.parametrize("index", range(len(T.CASES)), ids=IDS)
def test_restatement_agrees_with_torch_autograd_through_a_masked_loop(index):
    case = T.CASES[index]
    t, ref = T.TABLE[index][0], T.TABLE[index][1]
    leaves, hs, h_last = R.torch_loop(t)
    loss = 0.0
    if t["dhs"] is not None:
        loss = loss + (hs * torch.from_numpy(t["dhs"])).sum()
    if t["dh_last"] is not None:
        loss = loss + (h_last * torch.from_numpy(t["dh_last"])).sum()
    grads = torch.autograd.grad(loss, [leaves[k] for k in ("xz", "h0", "rk", "rb")], allow_unused=True)
    got = {"hs": hs, "h_last": h_last, "dxz": grads[0], "dh0": grads[1], "drk": grads[2], "drb": grads[3]}
    for key in T.OUTPUTS:
        g = np.zeros_like(ref[key]) if got[key] is None else got[key].detach().numpy()
        assert np.abs(g - ref[key]).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(ref[key]).max(initial=0.0)), key
    if case.mask == "first":       # zeros before the first valid step although h0 is not zero
        assert t["h0"] is not None and not ref["hs"][:, 0].any() and np.abs(ref["h_last"]).max() > 0
    if case.mask == "allpad":      # the all-padding sequence: zero outputs, the state is h0 (or zero)
        assert not ref["hs"][1].any()
        assert np.array_equal(ref["h_last"][1], np.zeros(case.u) if t["h0"] is None else t["h0"][1])


# ---- (c) the planner ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tests/host/gru_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("gru_plan") / "gru_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "gru_plan_check.cpp"),
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


def test_the_claimed_routes_are_the_planners_and_reach_every_build(planner):
    args = []
    for c in T.CASES:
        args += [c.b, c.l, c.u, 1 if c.dtype == "bf16" else 0]
    lines = planner(args)
    assert len(lines) == len(T.CASES)
    reached = set()
    for c, line in zip(T.CASES, lines):
        status, kernel, upad, rows, threads, groups, lds_fwd, lds_bwd = map(int, line.split())
        assert (status, kernel, upad) == (0, c.route, c.upad), c.name
        assert upad == 0 or upad >= c.u
        assert rows * groups >= c.b > rows * (groups - 1) and max(lds_fwd, lds_bwd) <= 160 * 1024
        reached.add((kernel, c.dtype, upad))
        reached.add((kernel, c.dtype, upad, c.mask != "none", groups > 1))
    want = {(T.FAST, "bf16", upad) for upad in (32, 64, 128)} | {(T.GENERIC, "bf16", 0), (T.GENERIC, "fp32", 0)}
    # every kernel build with and without a mask, on one workgroup and on several
    want |= {(T.FAST, "bf16", upad, m, g) for upad in (32, 64, 128) for m in (False, True) for g in (False, True)}
    want |= {(T.GENERIC, dt, 0, m, True) for dt in ("bf16", "fp32") for m in (False, True)}
    assert want <= reached, sorted(want - reached, key=str)


def test_the_table_is_the_stated_matrix():
    assert len(set(IDS)) == len(T.CASES) and all(c.b <= 65 for c in T.CASES)
    bf16 = [c for c in T.CASES if c.dtype == "bf16"]
    fp32 = [c for c in T.CASES if c.dtype == "fp32"]
    assert {c.b for c in T.CASES} == set(T.BATCHES) and {c.l for c in T.CASES} == set(T.LENGTHS)
    assert {c.u for c in bf16} == set(T.BF16_FAST_U) | set(T.BF16_GENERIC_U) and {c.u for c in fp32} == set(T.FP32_U)
    assert {c.mask for c in T.CASES} == set(T.MASKS) and {c.grad for c in T.CASES} == set(T.GRADS)
    assert {c.h0 for c in T.CASES} == {False, True} and {c.bias for c in T.CASES} == {False, True}
    assert any(c.pad >= 0 and c.pad % 8 for c in bf16) and any(c.pad >= 0 and c.pad % 8 == 0 for c in bf16)
    assert any(c.mask == "first" and c.h0 and c.route == T.FAST for c in T.CASES)
    assert any(c.mask == "first" and c.h0 and c.route == T.GENERIC for c in T.CASES)
    assert any(c.pad >= 0 for c in fp32) and any(c.sticky for c in bf16)


# ---- (d) the C ABI --------------------------------------------------------------------------------------------------
def test_the_four_entries_are_declared_bound_and_exported():
    from keras_rs_amd.build import build

    protos = header_prototypes(open(os.path.join(ROOT, "include", "krs.h")).read())
    build()
    lib = L.lib()
    for name in GRU_SYMBOLS:
        assert name in protos, f"{name} is not declared in include/krs.h"
        assert name in L.PROTOTYPES, f"{name} has no row in _lib.PROTOTYPES"
        (ret, args), (restype, argtypes) = protos[name], L.PROTOTYPES[name]
        assert restype is ret and len(args) == len(argtypes) and all(a is b for a, b in zip(args, argtypes)), name
        fn = getattr(lib, name, None)
        assert fn is not None, f"libkrs_hip.so does not export {name}"
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    # the host-only entries answer without a GPU
    assert lib.krs_gru_reserve_bytes(3, 7, 50, L.BF16) == 3 * 7 * 4 * 50 * 2
    assert lib.krs_gru_reserve_bytes(3, 7, 50, L.F32) == 3 * 7 * 4 * 50 * 4
    assert lib.krs_gru_reserve_bytes(0, 7, 50, L.F32) == 0
    kernel, upad = C.c_int(-1), C.c_int(-1)
    assert lib.krs_gru_last_route(C.addressof(kernel), C.addressof(upad)) == kernel.value
    assert (kernel.value, upad.value) in {(0, 0), (1, 32), (1, 64), (1, 128), (2, 0)}


# ---- (e) the bounds -------------------------------------------------------------------------------------------------
def test_the_recorded_rounding_distance_is_the_tables():
    worst, where = 0.0, None
    for index, case in enumerate(T.CASES):
        if case.dtype != "bf16":
            continue
        t, ref = T.TABLE[index][0], T.TABLE[index][1]
        e = T.rounding_distance(case, t, ref)
        for key in T.OUTPUTS:
            top = float(np.abs(ref[key]).max(initial=0.0))
            if e[key] > 0.0 and e[key] / top > worst:
                worst, where = e[key] / top, (case.name, key)
    print(f"largest E / max |ref| of the rounding restatement: {worst:.5f} at {where} (header: {T.OBSERVED_MAX_E})")
    assert worst == T.MAX_E and worst <= T.OBSERVED_MAX_E <= 1.05 * worst
    # the rounding restatement itself is inside every bound, with the factor 2 to spare
    for index, case in enumerate(T.CASES):
        t, ref, bound, _ = T.TABLE[index]
        if case.dtype == "bf16":
            assert T.worst_ratio(T.compute(case, t, bf16=True), ref, bound) <= 0.5


def test_fp32_cases_keep_the_standing_tolerance():
    index = next(i for i, c in enumerate(T.CASES) if c.dtype == "fp32")
    _, ref, bound, _ = T.TABLE[index]
    assert T.FP32_TOL == 1e-5 and np.array_equal(bound["hs"], 1e-5 + 1e-5 * np.abs(ref["hs"]))


def _applies(defect, case, t):
    v = t["valid"]
    if defect in ("mask_zero_state", "mask_out_state"):
        if v is None:
            return False
        masked_then_valid = any((row == 0).any() and row[np.argmax(row == 0):].any() for row in v)
        if defect == "mask_zero_state":
            return masked_then_valid
        return t["h0"] is not None and bool((v[:, 0] == 0).any())
    if defect == "rbh_outside":
        return t["rb"] is not None
    if defect == "round_state":
        return case.l >= 2
    return True


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_the_bounds_would_not_hide_a_defect(defect):
    caught = applied = 0
    for index, case in enumerate(T.CASES):
        t, ref, bound, _ = T.TABLE[index]
        if not _applies(defect, case, t):
            continue
        applied += 1
        ratio = T.worst_ratio(T.compute(case, t, bf16=case.dtype == "bf16", defect=defect), ref, bound)
        caught += ratio > 1.0
    print(f"{defect}: outside the bound on {caught} of the {applied} cases it applies to")
    assert applied >= 3 and caught >= 1
    if defect != "round_state":        # (a gross defect shows on many cases, not on one lucky draw)
        assert caught >= 3


def test_rounding_the_state_every_step_is_caught_by_the_sticky_case():
    index = next(i for i, c in enumerate(T.CASES) if c.sticky)
    case = T.CASES[index]
    t, ref, bound, _ = T.TABLE[index]
    good = T.worst_ratio(T.compute(case, t, bf16=True), ref, bound, keys=("hs", "h_last"))
    bad = T.worst_ratio(T.compute(case, t, bf16=True, defect="round_state"), ref, bound, keys=("hs", "h_last"))
    print(f"{case.name}: forward error / bound {good:.3f} with the state in fp32, {bad:.3f} rounded every step")
    assert good <= 0.5 and bad > 1.0


# ---- (f) the layer's host logic -------------------------------------------------------------------------------------
def test_gru_weights_config_and_refusals():
    gru = layers.GRU(5, return_sequences=True, return_state=True, device="cpu")
    gru.build((2, 7, 12))
    assert [tuple(w.shape) for w in gru.weights] == [(12, 15), (5, 15), (2, 15)]
    assert all(w is x for w, x in zip(gru.weights, (gru.kernel, gru.recurrent_kernel, gru.bias)))
    assert gru.bias.dtype == torch.float32 and not gru.bias.any()
    nobias = layers.GRU(4, use_bias=False, device="cpu")
    nobias.build((1, 3, 8))
    assert [tuple(w.shape) for w in nobias.weights] == [(8, 12), (4, 12)] and nobias.bias is None
    cfg = gru.get_config()
    again = layers.GRU.from_config(cfg)
    assert again.get_config() == cfg
    assert cfg["units"] == 5 and cfg["return_sequences"] is True and cfg["return_state"] is True and cfg["reset_after"] is True
    assert cfg["activation"] == "tanh" and cfg["recurrent_activation"] == "sigmoid"
    assert cfg["recurrent_initializer"]["class_name"] == "Orthogonal"
    assert gru.compute_output_shape((2, 7, 12)) == (2, 7, 5) and nobias.compute_output_shape((1, 3, 8)) == (1, 4)
    for kwargs, word in ((dict(reset_after=False), "reset_after"), (dict(activation="relu"), "activation"),
                         (dict(recurrent_activation="tanh"), "recurrent_activation"), (dict(dropout=0.1), "dropout"),
                         (dict(recurrent_dropout=0.1), "recurrent_dropout"), (dict(go_backwards=True), "go_backwards"),
                         (dict(stateful=True), "stateful"), (dict(unroll=True), "unroll")):
        with pytest.raises(NotImplementedError, match=word):
            layers.GRU(4, **kwargs)
    with pytest.raises(ValueError, match="units"):
        layers.GRU(0)
    with pytest.raises(ValueError, match=r"\[B, L, D\]"):
        gru(torch.zeros(2, 12))
    assert "GRU" in layers.__all__ and layers.GRU is gru.__class__


def test_the_orthogonal_initializer():
    for shape in ((32, 96), (96, 32), (8, 8)):
        w = base.get_initializer("orthogonal")(shape, torch.float64)
        small = min(shape)
        gram = w.t() @ w if shape[0] >= shape[1] else w @ w.t()
        assert tuple(w.shape) == shape and torch.allclose(gram, torch.eye(small, dtype=torch.float64), atol=1e-12)
    a, z = base.Orthogonal(gain=2.0, seed=3), base.get_initializer({"class_name": "Orthogonal", "config": {"gain": 2.0, "seed": 3}})
    assert torch.equal(a((4, 12)), z((4, 12))) and a.serialize() == z.serialize()
    assert torch.allclose(a((4, 12)) @ a((4, 12)).t(), 4.0 * torch.eye(4), atol=1e-5)
    with pytest.raises(ValueError):
        a((5,))
