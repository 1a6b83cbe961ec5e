"""K20 (csrc/gru.hip) on every case of tests/gru_cases.py against the float64 restatement, within the case's stated bound;
the route each call took; bit-identical repeats; the inference forward (no reserve) against the training forward; a
forward + backward captured into a graph; the C ABI called directly.  Each comparison prints its worst error / bound
ratio before it asserts."""

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import recurrent_ops as G
from tests import gru_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KRS_ERR_INVALID, KRS_ERR_UNSUPPORTED = -1, -2
NAN = float("nan")


def _dtype(case):
    return torch.bfloat16 if case.dtype == "bf16" else torch.float32


def _device_inputs(case, t):
    """xz (a leaf, or a view of a wider leaf), rk, rb, h0 as leaves; valid, dhs, dh_last."""
    dt = _dtype(case)
    dev = lambda a, d=dt: None if a is None else torch.from_numpy(a).to(d).to(DEV)
    xz = dev(t["xz"])
    b, l, u3 = xz.shape
    if case.pad >= 0:
        wide = torch.full((b * l, u3 + case.pad), NAN, dtype=dt, device=DEV)
        wide[:, :u3] = xz.reshape(b * l, u3)
        wide.requires_grad_(True)
        xz_leaf, xz = wide, wide[:, :u3].view(b, l, u3)
        assert xz.stride(1) == u3 + case.pad
    else:
        xz_leaf = xz.requires_grad_(True)
    rk = dev(t["rk"]).requires_grad_(True)
    rb = None if t["rb"] is None else dev(t["rb"], torch.float32).requires_grad_(True)
    h0 = None if t["h0"] is None else dev(t["h0"]).requires_grad_(True)
    valid = None if t["valid"] is None else torch.from_numpy(t["valid"]).to(DEV)
    return xz_leaf, xz, rk, rb, h0, valid, dev(t["dhs"]), dev(t["dh_last"])


def _run(case, t):
    xz_leaf, xz, rk, rb, h0, valid, dhs, dh_last = _device_inputs(case, t)
    hs, h_last = G.gru(xz, rk, rb, mask=valid, initial_state=h0, return_sequences=True)
    route_fwd = G.last_route()
    leaves = [x for x in (xz_leaf, rk, rb, h0) if x is not None]
    outs, gouts = [], []
    if dhs is not None:
        outs.append(hs), gouts.append(dhs)
    if dh_last is not None:
        outs.append(h_last), gouts.append(dh_last)
    got_grads = torch.autograd.grad(outs, leaves, gouts)
    route_bwd = G.last_route()
    it = iter(got_grads)
    dxz = next(it)
    if case.pad >= 0:
        b, l, u3 = xz.shape
        assert not dxz[:, u3:].any()                      # the padding columns took no part
        dxz = dxz[:, :u3].reshape(b, l, u3)
    drk = next(it)
    drb = next(it) if rb is not None else torch.zeros(3 * case.u)
    dh0 = next(it) if h0 is not None else None
    got = {"hs": hs.detach(), "h_last": h_last.detach(), "dxz": dxz, "drk": drk, "drb": drb, "dh0": dh0}
    return {k: (None if v is None else v.double().cpu().numpy()) for k, v in got.items()}, route_fwd, route_bwd


def _keys(got):
    return tuple(k for k in T.OUTPUTS if got[k] is not None)


@pytest.mark.parametrize("index", range(len(T.CASES)), ids=[c.name for c in T.CASES])
def test_every_case_against_float64_on_the_claimed_route(index):
    case = T.CASES[index]
    t, ref, bound, _ = T.TABLE[index]
    got, route_fwd, route_bwd = _run(case, t)
    assert route_fwd == route_bwd == (case.route, case.upad)
    keys = _keys(got)
    if t["rb"] is None:
        keys = tuple(k for k in keys if k != "drb")
    for key in keys:
        print(f"{case.name}: {key}: worst error / bound = {T.worst_ratio(got, ref, bound, keys=(key,)):.3f}")
    assert T.worst_ratio(got, ref, bound, keys=keys) <= 1.0
    if case.mask == "allpad":
        assert not got["hs"][1].any()                     # the all-padding sequence: zero outputs, exactly


@pytest.mark.parametrize("index", [i for i, c in enumerate(T.CASES) if not c.h0 and c.l >= 7][:4])
def test_dh0_of_an_absent_initial_state_is_that_of_a_zero_one(index):
    case = T.CASES[index]._replace(h0=True)
    t = dict(T.TABLE[index][0])
    ref, bound = T.TABLE[index][1], T.TABLE[index][2]
    t["h0"] = np.zeros((case.b, case.u))
    got, _, _ = _run(case, t)
    ratio = T.worst_ratio(got, ref, bound, keys=("dh0", "hs", "h_last"))
    print(f"{case.name}: dh0 through a zero initial state: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("index", range(len(T.CASES)), ids=[c.name for c in T.CASES])
def test_two_calls_are_bit_identical(index):
    case = T.CASES[index]
    t = T.TABLE[index][0]
    a, _, _ = _run(case, t)
    z, _, _ = _run(case, t)
    for key in _keys(a):
        assert np.array_equal(a[key], z[key]), key


@pytest.mark.parametrize("index", range(len(T.CASES)), ids=[c.name for c in T.CASES])
def test_the_inference_forward_equals_the_training_forward_bit_for_bit(index):
    case = T.CASES[index]
    t = T.TABLE[index][0]
    _, xz, rk, rb, h0, valid, _, _ = _device_inputs(case, t)
    hs, h_last = G.gru(xz, rk, rb, mask=valid, initial_state=h0, return_sequences=True)
    assert hs.requires_grad and G.last_route() == (case.route, case.upad)
    with torch.no_grad():
        hs_i, h_last_i = G.gru(xz, rk, rb, mask=valid, initial_state=h0, return_sequences=True)
        out_i, state_i = G.gru(xz, rk, rb, mask=valid, initial_state=h0)         # no sequence output at all
    assert torch.equal(hs.detach(), hs_i) and torch.equal(h_last.detach(), h_last_i) and torch.equal(state_i, h_last_i)
    assert torch.equal(out_i, hs_i[:, -1])


def test_forward_and_backward_replay_from_a_graph_bit_for_bit():
    index = next(i for i, c in enumerate(T.CASES) if c.route == T.FAST and c.mask == "holes" and c.h0 and c.bias and c.grad == "both")
    case = T.CASES[index]
    t = T.TABLE[index][0]
    eager, _, _ = _run(case, t)
    xz_leaf, xz, rk, rb, h0, valid, dhs, dh_last = _device_inputs(case, t)
    leaves = [xz_leaf, rk, rb, h0]

    def step():
        hs, h_last = G.gru(xz, rk, rb, mask=valid, initial_state=h0, return_sequences=True)
        return (hs, h_last) + torch.autograd.grad((hs, h_last), leaves, (dhs, dh_last))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                            # (warm-up outside the capture: allocations, attributes)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for o in outs:
        o.detach().fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    got = dict(zip(("hs", "h_last", "dxz", "drk", "drb", "dh0"), (o.detach().double().cpu().numpy() for o in outs)))
    got["dxz"] = got["dxz"].reshape(eager["dxz"].shape)
    for key in T.OUTPUTS:
        assert np.array_equal(got[key], eager[key]), key


# ---- the C ABI directly ---------------------------------------------------------------------------------------------
def _abi_tensors(b=5, l=6, u=40, dt=torch.bfloat16, seed=7):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *shape: torch.randn(*shape, generator=g).to(dt).to(DEV)
    return mk(b, l, 3 * u), mk(u, 3 * u) * 0.2


def _fwd(lib, xz, rk, hs, h_last, reserve=None, *, b=None, l=None, u=None, dtype=None, ld=None, null_xz=False,
         null_rk=False):
    B, Lq, U3 = xz.shape
    return lib.krs_gru_fwd(None if null_xz else L.ptr(xz), U3 if ld is None else ld, None if null_rk else L.ptr(rk),
                           None, None, None,
                           L.fdtype(xz) if dtype is None else dtype, B if b is None else b, Lq if l is None else l,
                           U3 // 3 if u is None else u, L.ptr(hs), L.ptr(h_last), L.ptr(reserve), L.stream_ptr())


def test_abi_refusals_and_no_ops():
    lib = L.lib()
    xz, rk = _abi_tensors()
    b, l, u3 = xz.shape
    u = u3 // 3
    hs = torch.full((b, l, u), NAN, dtype=xz.dtype, device=DEV)
    h_last = torch.full((b, u), NAN, dtype=xz.dtype, device=DEV)
    reserve = torch.full((b, l, 4 * u), NAN, dtype=xz.dtype, device=DEV)
    err = lambda: lib.krs_last_error().decode()
    assert _fwd(lib, xz, rk, hs, h_last, u=1025, ld=4096) == KRS_ERR_UNSUPPORTED and "1024" in err() and G.last_route() == (0, 0)
    assert _fwd(lib, xz, rk, hs, h_last, null_xz=True) == KRS_ERR_INVALID
    assert _fwd(lib, xz, rk, hs, h_last, null_rk=True) == KRS_ERR_INVALID
    assert _fwd(lib, xz, rk, None, None) == KRS_ERR_INVALID
    assert _fwd(lib, xz, rk, None, h_last, reserve) == KRS_ERR_INVALID        # a reserve without hs
    assert _fwd(lib, xz, rk, hs, h_last, b=-1) == KRS_ERR_INVALID
    assert _fwd(lib, xz, rk, hs, h_last, l=-1) == KRS_ERR_INVALID
    assert _fwd(lib, xz, rk, hs, h_last, u=0) == KRS_ERR_INVALID
    assert _fwd(lib, xz, rk, hs, h_last, dtype=L.I8) == KRS_ERR_INVALID
    assert _fwd(lib, xz, rk, hs, h_last, ld=u3 - 1) == KRS_ERR_INVALID
    assert _fwd(lib, xz, rk, hs, h_last, b=0) == 0 and G.last_route() == (0, 0)
    assert _fwd(lib, xz, rk, hs, h_last, l=0) == 0 and G.last_route() == (0, 0)
    bwd = lambda **kw: lib.krs_gru_bwd(L.ptr(rk), None, None, L.ptr(hs), L.ptr(reserve), None, L.ptr(h_last), L.BF16,
                                       kw.get("b", b), kw.get("l", l), kw.get("u", u), L.ptr(reserve), L.ptr(reserve),
                                       None, None, L.stream_ptr())
    assert bwd(b=0) == 0 and bwd(l=0) == 0 and G.last_route() == (0, 0)
    assert bwd(u=1025) == KRS_ERR_UNSUPPORTED and "1024" in err()
    assert lib.krs_gru_bwd(L.ptr(rk), None, None, L.ptr(hs), None, None, None, L.BF16, b, l, u, L.ptr(reserve),
                           L.ptr(reserve), None, None, L.stream_ptr()) == KRS_ERR_INVALID
    torch.cuda.synchronize()
    for x in (hs, h_last, reserve):                        # no refused call and no no-op launched anything
        assert torch.isnan(x.float()).all()
    assert lib.krs_gru_reserve_bytes(b, l, u, L.BF16) == reserve.numel() * 2


def test_abi_inference_writes_nothing_but_the_outputs():
    lib = L.lib()
    xz, rk = _abi_tensors()
    b, l, u3 = xz.shape
    u = u3 // 3
    hs = torch.full((b, l, u), NAN, dtype=xz.dtype, device=DEV)
    h_last = torch.full((b, u), NAN, dtype=xz.dtype, device=DEV)
    assert _fwd(lib, xz, rk, hs, h_last) == 0 and G.last_route() == (T.FAST, 64)
    only_last = torch.full((b, u), NAN, dtype=xz.dtype, device=DEV)
    assert _fwd(lib, xz, rk, None, only_last) == 0
    hs_t = torch.full_like(hs, NAN)
    reserve = torch.full((b, l, 4 * u), NAN, dtype=xz.dtype, device=DEV)
    assert _fwd(lib, xz, rk, hs_t, torch.empty_like(h_last), reserve) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(hs.float()).all() and torch.isfinite(reserve.float()).all()
    assert torch.equal(hs, hs_t) and torch.equal(h_last, only_last) and torch.equal(h_last, hs[:, -1])
