"""krs_dot_interaction_fwd / _bwd_accumulate (K4) on every kernel build and route of
keras_rs_amd/csrc/dot_interaction.hip: the kernel each case ran is asserted from krs_dot_interaction_last_route, and every
element of its result is held to a float64 restatement of the operation (tests/dot_interaction_restatement.py, plain
numpy, no oracle/).

One table drives everything (tests/dot_interaction_cases.py; its coverage is checked without a GPU by
tests/test_dot_interaction_routes_host.py).  The test goes through the C ABI, so it owns the buffers: every buffer has a
row before and a row after the batch, and the output and the gradients have lead, gap and tail columns around what the
entry owns, all pre-filled with 7.0; the inputs carry NaN there.  Per case:

  * route: dot_last_route() equals the case's expected record;
  * every element: |got - ref| <= (n + 2) * 2^-24 * S + r * |ref|, n = D forward and F (+ 1 with an existing gradient)
    backward, S the magnitude sum of the restatement, r = 0 (fp32) or 2^-8 * 1.01 (bf16, one rounding of an fp32 sum); the
    block backward in bf16 adds r * |partial sum| per earlier chunk of 128 features.  The masked part of the [F, F]
    layout is exactly zero.  tests/test_dot_interaction_routes_host.py checks on the CPU that the restatement's own fp32
    evaluation stays inside this bound for every small case;
  * the sentinel rows and columns are untouched, bit for bit, and nothing is NaN (a read outside a feature would be);
  * a second call gives the same bits.
"""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import dot_interaction_restatement as RS
from tests.dot_interaction_cases import CASES, ES, feature_layout, inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
OUT_LEAD, OUT_TAIL = 3, 5


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@functools.lru_cache(maxsize=4)
def _reference(name):
    c = next(k for k in CASES if k.name == name)
    h = inputs(name)
    X = h["X"].astype(np.float64)
    bf16 = c.dtype == "bf16"
    if c.direction == "fwd":
        ref, S = RS.forward(X, c.self_i, c.skip)
        return ref, RS.bound(ref, S, c.D, bf16)
    chunked = c.route["kernel"] == "bwd_block"
    ex = None if h["existing"] is None else h["existing"].astype(np.float64)
    ref, S, partial = RS.backward(X, h["G"].astype(np.float64), c.self_i, c.skip, ex, c.mask, chunked)
    return ref, RS.bound(ref, S, c.F + (1 if c.mask else 0), bf16, partial if bf16 else None)


def _feature_buffers(c, values, fill):
    """the buffers of the F features under the case's layout, `values` [B, F, D] (or None) in the feature slots and `fill`
    everywhere else: (buffers to keep alive, pointers, row strides, [(buffer index, column)] per feature)"""
    dt = TORCH_DT[c.dtype]
    lead, cols, widths = feature_layout(c)
    if c.layout == "concat":
        bufs = [torch.full((c.B + 2, widths[0]), fill, dtype=dt)]
        where = [(0, col) for col in cols]
    else:
        bufs = [torch.full((c.B + 2, w), fill, dtype=dt) for w in widths]
        where = [(f, lead) for f in range(c.F)]
    if values is not None:
        v = torch.from_numpy(values).to(dt)
        for f, (k, col) in enumerate(where):
            bufs[k][1:c.B + 1, col:col + c.D] = v[:, f]
    return where, lead, widths, bufs


def _run(c, h):
    """One call of case c on fresh buffers: (result buffers on the host, their feature map, route)."""
    from keras_rs_amd import _lib as L
    from keras_rs_amd import dense_ops as D

    dt, es = TORCH_DT[c.dtype], ES[c.dtype]
    where, lead, widths, xb = _feature_buffers(c, h["X"], float("nan"))
    xb = [b.to(DEV) for b in xb]

    def tables(bufs):
        ptrs = [bufs[k].data_ptr() + (bufs[k].stride(0) + col) * es for k, col in where]
        lds = [bufs[k].stride(0) for k, _ in where]
        return (C.c_void_p * c.F)(*ptrs), (C.c_int64 * c.F)(*lds)

    ptrs, lds = tables(xb)
    ow = OUT_LEAD + c.cols + OUT_TAIL
    stream = L.stream_ptr()
    if c.direction == "fwd":
        out = torch.full((c.B + 2, ow), 7.0, dtype=dt, device=DEV)
        rc = L.lib().krs_dot_interaction_fwd(ptrs, lds, c.F, c.B, c.D, L.fdtype(out), int(c.self_i), int(c.skip),
                                             out.data_ptr() + (ow + OUT_LEAD) * es, ow, stream)
        L.check(rc, "krs_dot_interaction_fwd")
        route = D.dot_last_route()
        torch.cuda.synchronize()
        return [out.cpu()], route
    g = torch.full((c.B + 2, ow), float("nan"), dtype=dt)
    g[1:c.B + 1, OUT_LEAD:OUT_LEAD + c.cols] = torch.from_numpy(h["G"]).to(dt)
    g = g.to(DEV)
    existing = None
    if c.mask:
        existing = np.full((c.B, c.F, c.D), 7.0, dtype=np.float32)
        for f in range(min(c.F, 64)):
            if (c.mask >> f) & 1:
                existing[:, f] = h["existing"][:, f]
    _, _, _, gb = _feature_buffers(c, existing, 7.0)
    gb = [b.to(DEV) for b in gb]
    gptrs, glds = tables(gb)
    rc = L.lib().krs_dot_interaction_bwd_accumulate(ptrs, lds, c.F, c.B, c.D, L.fdtype(g), int(c.self_i), int(c.skip),
                                                    g.data_ptr() + (ow + OUT_LEAD) * es, ow, gptrs, glds, c.mask, stream)
    L.check(rc, "krs_dot_interaction_bwd_accumulate")
    route = D.dot_last_route()
    torch.cuda.synchronize()
    return [b.cpu() for b in gb], route


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_route_against_float64(case):
    c, h = case, inputs(case.name)
    ref, tol = _reference(c.name)
    bufs, route = _run(c, h)
    assert route == c.route

    seven = _bits(torch.full((1,), 7.0, dtype=TORCH_DT[c.dtype]))[0]
    if c.direction == "fwd":
        got = bufs[0][1:c.B + 1, OUT_LEAD:OUT_LEAD + c.cols]
        owned = [torch.zeros(bufs[0].shape, dtype=torch.bool)]
        owned[0][1:c.B + 1, OUT_LEAD:OUT_LEAD + c.cols] = True
    else:
        where, _, _, _ = _feature_buffers(c, None, 0.0)
        got = torch.stack([bufs[k][1:c.B + 1, col:col + c.D] for k, col in where], dim=1)
        owned = [torch.zeros(b.shape, dtype=torch.bool) for b in bufs]
        for k, col in where:
            owned[k][1:c.B + 1, col:col + c.D] = True
    for b, own in zip(bufs, owned):
        assert bool((_bits(b)[~own] == seven).all()), "a sentinel row or column was written"
    assert bool(got.isfinite().all()), "a value from outside a feature (NaN) reached the result"

    err = np.abs(got.double().numpy() - ref)
    exact_zero = tol == 0
    assert (err[exact_zero] == 0).all(), "the masked part of the [F, F] layout is not zero"
    worst = float((err[~exact_zero] / tol[~exact_zero]).max()) if (~exact_zero).any() else 0.0
    build = "/".join(f"{k}={v}" for k, v in c.route.items() if k in ("kernel", "dtype", "ks", "fr", "self", "multi", "acc", "ng"))
    print(f"RATIO {build} {worst:.3f} {c.name}")
    assert worst <= 1.0, c.name

    bufs2, route2 = _run(c, h)        # a second call gives the same bits
    assert route2 == c.route
    for b, b2 in zip(bufs, bufs2):
        assert torch.equal(_bits(b), _bits(b2))
