"""K25 (csrc/lstm.hip) through recurrent_ops.lstm against the float64 reference (tests/lstm_reference.py), every output
within the bound stated there; the route each call took against the planner's rule; one call twice for bit-identity."""

from typing import NamedTuple

import numpy as np
import pytest
import torch

from keras_rs_amd import recurrent_ops as G
from tests import lstm_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


class Case(NamedTuple):
    dtype: str          # "bf16" | "fp32"
    b: int
    l: int
    u: int
    mask: str           # none | right | left | holes | allpad
    init: bool          # (h0, c0) given
    grad: str           # where gradients arrive: seq | h | c | all
    pad: int = -1       # >= 0: xz is a view of a [B L, 4U + pad] buffer
    sticky: bool = False    # xz_f shifted by +6: f ~ 0.9975


CASES = [
    # the per-u sweep: every upad with ragged unit counts and the tight LDS case, the generic route, fp32
    Case("bf16", 1, 1, 8, "none", False, "seq"),
    Case("bf16", 33, 7, 33, "right", True, "all"),
    Case("bf16", 65, 2, 64, "left", False, "h"),
    Case("bf16", 33, 7, 65, "holes", True, "c"),
    Case("bf16", 65, 7, 128, "allpad", True, "all"),
    Case("bf16", 33, 2, 160, "right", True, "all"),
    Case("fp32", 65, 7, 8, "left", True, "all"),
    Case("fp32", 33, 2, 50, "none", False, "c"),
    Case("fp32", 1, 7, 200, "holes", True, "seq"),
    # cross-cutting
    Case("bf16", 33, 7, 128, "none", False, "seq"),
    Case("bf16", 65, 1, 33, "allpad", False, "h"),
    Case("bf16", 33, 7, 50, "right", True, "all", pad=5),          # a token stride that is no whole 16-byte chunk
    Case("fp32", 33, 7, 50, "allpad", True, "h", pad=3),
    Case("bf16", 33, 33, 32, "none", True, "all", sticky=True),
]
IDS = [f"{c.dtype}-b{c.b}l{c.l}u{c.u}-{c.mask}-{'init' if c.init else 'zero'}-{c.grad}"
       + (f"-pad{c.pad}" if c.pad >= 0 else "") + ("-sticky" if c.sticky else "") for c in CASES]


def _valid(case):
    b, l = case.b, case.l
    if case.mask == "none":
        return None
    v = np.zeros((b, l), dtype=np.uint8)
    for x in range(b):
        n = max(1, l - ((x % 4 + 1) * l) // 5)
        if case.mask in ("right", "allpad"):
            v[x, :n] = 1
        elif case.mask == "left":
            v[x, l - n:] = 1
        else:
            v[x, :] = 1
            v[x, 1 + x % 3:l - 1:3] = 0
    if case.mask == "allpad":
        v[b // 2] = 0
    return v


def _inputs(case, seed):
    rng = np.random.default_rng(seed)
    b, l, u = case.b, case.l, case.u
    rep = R.round_bf16 if case.dtype == "bf16" else (lambda x: x.astype(np.float32).astype(np.float64))
    xz = rng.standard_normal((b, l, 4 * u))
    if case.sticky:
        xz[:, :, u:2 * u] += 6.0
    t = {"xz": rep(xz), "rk": rep(rng.standard_normal((u, 4 * u)) / np.sqrt(u)), "valid": _valid(case)}
    h0, c0 = rep(rng.standard_normal((b, u)) * 0.5), rep(rng.standard_normal((b, u)))
    t["h0"], t["c0"] = (h0, c0) if case.init else (None, None)
    grads = {"dhs": rep(rng.standard_normal((b, l, u))), "dh_last": rep(rng.standard_normal((b, u))),
             "dc_last": rep(rng.standard_normal((b, u)))}
    want = {"seq": ("dhs",), "h": ("dh_last",), "c": ("dc_last",), "all": tuple(grads)}[case.grad]
    t.update({k: (g if k in want else None) for k, g in grads.items()})
    return t


def _run(case, t):
    dt = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    dev = lambda a: None if a is None else torch.from_numpy(a).to(dt).to(DEV)
    b, l, u4 = t["xz"].shape
    xz = dev(t["xz"])
    if case.pad >= 0:
        leaf = torch.full((b * l, u4 + case.pad), NAN, dtype=dt, device=DEV)
        leaf[:, :u4] = xz.reshape(b * l, u4)
        leaf.requires_grad_(True)
        xz = leaf[:, :u4].view(b, l, u4)
        assert xz.stride(1) == u4 + case.pad
    else:
        leaf = xz.requires_grad_(True)
    rk = dev(t["rk"]).requires_grad_(True)
    init = None if t["h0"] is None else (dev(t["h0"]).requires_grad_(True), dev(t["c0"]).requires_grad_(True))
    valid = None if t["valid"] is None else torch.from_numpy(t["valid"]).to(DEV)
    hs, h, c = G.lstm(xz, rk, mask=valid, initial_state=init, return_sequences=True)
    route_fwd = G.lstm_last_route()
    pairs = [(o, dev(t[k])) for o, k in ((hs, "dhs"), (h, "dh_last"), (c, "dc_last")) if t[k] is not None]
    grads = torch.autograd.grad([o for o, _ in pairs], [leaf, rk] + list(init or ()), [g for _, g in pairs])
    dxz = grads[0]
    if case.pad >= 0:
        assert not dxz[:, u4:].any()                      # the padding columns took no part
        dxz = dxz[:, :u4].reshape(b, l, u4)
    got = {"hs": hs, "h": h, "c": c, "dxz": dxz, "drk": grads[1]}
    if init is not None:
        got["dh0"], got["dc0"] = grads[2], grads[3]
    return {k: v.detach().double().cpu().numpy() for k, v in got.items()}, route_fwd, G.lstm_last_route()


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_every_output_against_float64_on_the_planned_route_twice(index):
    case = CASES[index]
    t = _inputs(case, 2500 + index)
    args = (t["xz"], t["rk"], t["valid"], t["h0"], t["c0"], t["dhs"], t["dh_last"], t["dc_last"])
    ref = R.lstm(*args)
    bf16 = case.dtype == "bf16"
    bound, e = R.bounds(ref, R.lstm(*args, bf16=True) if bf16 else ref, bf16)
    got, route_fwd, route_bwd = _run(case, t)
    fast = bf16 and case.u <= 128
    assert route_fwd == route_bwd == ((G.FAST, 32 if case.u <= 32 else 64 if case.u <= 64 else 128) if fast
                                      else (G.GENERIC, 0))
    worst = {}
    for key, g in got.items():
        assert g.shape == ref[key].shape and np.isfinite(g).all(), key
        err = np.abs(g - ref[key])
        worst[key] = float(np.where(err == 0.0, 0.0, err / bound[key]).max(initial=0.0))
        print(f"{IDS[index]}: {key}: E = {e[key]:.3e}, worst error / bound = {worst[key]:.3f}")
    assert max(worst.values()) <= 1.0, worst
    if case.mask == "allpad":                             # the all-padding sequence: zero outputs, the states carried
        row = case.b // 2
        assert not got["hs"][row].any()
        assert np.array_equal(got["h"][row], t["h0"][row] if case.init else np.zeros(case.u))
    again, _, _ = _run(case, t)
    for key in got:
        assert np.array_equal(got[key], again[key]), key
