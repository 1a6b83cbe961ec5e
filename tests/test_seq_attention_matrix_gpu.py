"""K19 (csrc/seq_attention.hip) on every case of tests/seq_attention_cases.py against the float64 restatement, within the
case's stated bound; the route each call took; the fully-masked-row rule; bit-identical repeats; the fast route
against the generic one; the C ABI called directly; and the memory contract.  Each comparison prints its worst
error / bound ratio before it asserts."""

import math

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import sequence_ops as S
from tests import seq_attention_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KRS_ERR_INVALID, KRS_ERR_UNSUPPORTED, KRS_ERR_WORKSPACE = -1, -2, -4
NAN = float("nan")


def _dtype(case):
    return torch.bfloat16 if case.dtype == "bf16" else torch.float32


def _device_inputs(case, t):
    """q, k, v (leaves, or views of one packed leaf), dout, key_valid, draw on the device; and the leaf list."""
    dt = _dtype(case)
    q, k, v, dout = (torch.from_numpy(t[n]).to(dt).to(DEV) for n in ("q", "k", "v", "dout"))
    kv = None if t["key_valid"] is None else torch.from_numpy(t["key_valid"]).to(DEV)
    draw = torch.tensor([t["draw"]], dtype=torch.int64, device=DEV)
    if case.pad < 0:
        for x in (q, k, v):
            x.requires_grad_(True)
        return q, k, v, dout, kv, draw, None
    b, l, h, dh = q.shape
    hd = h * dh
    packed = torch.full((b * l, 3 * hd + case.pad), NAN, dtype=dt, device=DEV)
    for x, src in enumerate((q, k, v)):
        packed[:, x * hd:(x + 1) * hd] = src.reshape(b * l, hd)
    packed.requires_grad_(True)
    views = [packed[:, x * hd:(x + 1) * hd].view(b, l, h, dh) for x in range(3)]
    assert all(x.stride(1) == 3 * hd + case.pad for x in views)
    return views[0], views[1], views[2], dout, kv, draw, packed


def _run(case, t):
    q, k, v, dout, kv, draw, packed = _device_inputs(case, t)
    out, lse = S.seq_attention(q, k, v, key_valid=kv, causal=case.causal, scale=t["scale"], dropout_p=case.p,
                               seed=t["seed"], draw=draw, return_lse=True)
    route_fwd = S.last_route()
    leaves = (q, k, v) if packed is None else (packed,)
    grads = torch.autograd.grad(out, leaves, dout)
    route_bwd = S.last_route()
    if packed is not None:
        b, l, h, dh = q.shape
        hd = h * dh
        grads = [grads[0][:, x * hd:(x + 1) * hd].reshape(b, l, h, dh) for x in range(3)]
    assert int(draw.item()) == t["draw"] + (1 if case.p > 0 else 0)
    got = {"out": out.detach(), "lse": lse, "dq": grads[0], "dk": grads[1], "dv": grads[2]}
    return {key: val.double().cpu().numpy() for key, val in got.items()}, route_fwd, route_bwd


@pytest.mark.parametrize("index", range(len(T.CASES)), ids=[c.name for c in T.CASES])
def test_every_case_against_float64_on_the_claimed_route(index):
    case = T.CASES[index]
    t = T.inputs_of(case, index)
    got, route_fwd, route_bwd = _run(case, t)
    assert route_fwd == route_bwd == (case.route, case.dpad)
    ref = T.reference(case, t)
    ratio = T.worst_ratio(got, ref, T.bounds(case, t, ref))
    print(f"{case.name}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # rows with no allowed key: exactly zero, lse = -inf; nothing anywhere is NaN
    dead = ~np.isfinite(ref["lse"])                                          # [B, H, L]
    assert np.array_equal(np.isneginf(got["lse"]), dead)
    assert not got["out"].transpose(0, 2, 1, 3)[dead].any() and not got["dq"].transpose(0, 2, 1, 3)[dead].any()
    assert all(np.isfinite(got[key]).all() for key in ("out", "dq", "dk", "dv"))


def test_fully_masked_rows_add_nothing_to_any_gradient():
    # left padding under the causal mask: the gradient of the padded rows' upstream dout must not matter at all
    case = T.Case("dead-rows", "bf16", 2, 2, 65, 64, True, "left", 0.2, -1, T.FAST, 64, 1)
    t = T.inputs_of(case, 501)
    dead = ~np.isfinite(T.reference(case, t)["lse"])
    assert dead.any() and not dead.all()
    base, _, _ = _run(case, t)
    t2 = dict(t)
    t2["dout"] = np.where(dead.transpose(0, 2, 1)[..., None], 64.0, t["dout"])
    other, _, _ = _run(case, t2)
    for key in ("dq", "dk", "dv"):
        assert np.array_equal(base[key], other[key]), key


@pytest.mark.parametrize("index", [i for i, c in enumerate(T.CASES) if c.l >= 127 and c.p > 0][:4])
def test_two_calls_are_bit_identical(index):
    case = T.CASES[index]
    t = T.inputs_of(case, index)
    a, _, _ = _run(case, t)
    z, _, _ = _run(case, t)
    for key in a:
        assert np.array_equal(a[key], z[key], equal_nan=True), key


def test_fast_and_generic_routes_agree_on_a_shared_case():
    # Dh = 128 on the fast route against the same data zero-padded to Dh = 160, which the generic route takes
    case = T.SHARED_FAST_GENERIC
    t = T.inputs_of(case, 977)
    fast, route, _ = _run(case, t)
    assert route == (T.FAST, 128)
    wide = case._replace(dh=160, route=T.GENERIC, dpad=0, vec=0)
    tw = dict(t)
    for name in ("q", "k", "v", "dout"):
        tw[name] = np.concatenate([t[name], np.zeros(t[name].shape[:3] + (32,))], axis=-1)
    gen, route, _ = _run(wide, tw)
    assert route == (T.GENERIC, 0)
    ref = T.reference(case, t)
    bound = T.bounds(case, t, ref)
    gen = {key: (val if key == "lse" else val[..., :128]) for key, val in gen.items()}
    for name, got in (("fast", fast), ("generic", gen)):
        ratio = T.worst_ratio(got, ref, bound)
        print(f"shared case, {name}: worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0
    # each within the bound of the reference, so within twice the bound of each other
    assert T.worst_ratio(fast, {k: gen[k] for k in gen}, {k: 2 * bound[k] for k in bound}) <= 1.0


# ---- the C ABI directly ---------------------------------------------------------------------------------------------
def _abi_tensors(b=2, h=2, l=40, dh=64, dt=torch.bfloat16, seed=7):
    g = torch.Generator().manual_seed(seed)
    mk = lambda: torch.randn(b, l, h, dh, generator=g).to(dt).to(DEV)
    return mk(), mk(), mk(), mk()


def _fwd(lib, q, k, v, out, lse, *, b=None, h=None, l=None, dh=None, dtype=None, kv=None, causal=1, p=0.0, draw=None,
         ld=None, scale=0.125):
    B, Lq, H, Dh = k.shape
    b, h, l, dh = (B if b is None else b), (H if h is None else h), (Lq if l is None else l), (Dh if dh is None else dh)
    ld = H * Dh if ld is None else ld
    return lib.krs_seq_attn_fwd(L.ptr(q), ld, L.ptr(k), ld, L.ptr(v), ld, L.fdtype(k) if dtype is None else dtype, b, h, l,
                                dh, L.ptr(kv), causal, scale, p, 11, L.ptr(draw), L.ptr(out), ld, L.ptr(lse), None, 0,
                                L.stream_ptr())


def _bwd(lib, q, k, v, out, dout, lse, dq, dk, dv, ws, ws_bytes, *, causal=1, p=0.0, draw=None, scale=0.125):
    B, Lq, H, Dh = q.shape
    ld = H * Dh
    return lib.krs_seq_attn_bwd(L.ptr(q), ld, L.ptr(k), ld, L.ptr(v), ld, L.fdtype(q), B, H, Lq, Dh, None, causal, scale, p,
                                11, L.ptr(draw), L.ptr(out), ld, L.ptr(dout), ld, L.ptr(lse), L.ptr(dq), ld, L.ptr(dk), ld,
                                L.ptr(dv), ld, L.ptr(ws), ws_bytes, L.stream_ptr())


def test_abi_nan_filled_workspace_and_outputs_and_each_gradient_alone():
    lib = L.lib()
    q, k, v, dout = _abi_tensors()
    b, l, h, dh = q.shape
    out = torch.full_like(q, NAN)
    lse = torch.full((b, h, l), NAN, dtype=torch.float32, device=DEV)
    assert _fwd(lib, q, k, v, out, lse) == 0
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    size = lib.krs_seq_attn_workspace_bytes(b, h, l, dh, L.BF16)
    assert size >= b * h * l * 4
    full = [torch.full_like(q, NAN) for _ in range(3)]
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device=DEV)            # (all-ones bytes: NaN as fp32)
    assert _bwd(lib, q, k, v, out, dout, lse, *full, ws, size) == 0
    assert all(torch.isfinite(g.float()).all() for g in full)
    for x in range(3):
        alone = [torch.full_like(q, NAN) if y == x else None for y in range(3)]
        ws = torch.full((size,), 0xFF, dtype=torch.uint8, device=DEV)
        assert _bwd(lib, q, k, v, out, dout, lse, *alone, ws, size) == 0
        assert torch.equal(alone[x], full[x])
    assert _bwd(lib, q, k, v, out, dout, lse, None, None, None, ws, size) == KRS_ERR_INVALID
    assert _bwd(lib, q, k, v, out, dout, lse, *full, ws, size - 256) == KRS_ERR_WORKSPACE
    assert _bwd(lib, q, k, v, out, dout, lse, *full, None, 0) == KRS_ERR_WORKSPACE


def test_abi_refusals_and_no_ops():
    lib = L.lib()
    q, k, v, _ = _abi_tensors()
    b, l, h, dh = q.shape
    out = torch.full_like(q, NAN)
    lse = torch.full((b, h, l), NAN, dtype=torch.float32, device=DEV)
    route = lambda: S.last_route()
    err = lambda: lib.krs_last_error().decode()
    assert _fwd(lib, q, k, v, out, lse, l=4097) == KRS_ERR_UNSUPPORTED and "4096" in err() and route() == (0, 0)
    assert _fwd(lib, q, k, v, out, lse, dh=257, ld=4096) == KRS_ERR_UNSUPPORTED and "256" in err()
    assert _fwd(lib, q, k, v, out, lse, b=2 ** 21, l=1024) == KRS_ERR_UNSUPPORTED and "2^31" in err()
    assert _fwd(lib, None, k, v, out, lse) == KRS_ERR_INVALID
    assert _fwd(lib, q, k, v, None, lse) == KRS_ERR_INVALID
    assert _fwd(lib, q, k, v, out, None) == KRS_ERR_INVALID
    assert _fwd(lib, q, k, v, out, lse, b=-1) == KRS_ERR_INVALID
    assert _fwd(lib, q, k, v, out, lse, l=-1) == KRS_ERR_INVALID
    assert _fwd(lib, q, k, v, out, lse, dh=0) == KRS_ERR_INVALID
    assert _fwd(lib, q, k, v, out, lse, h=0) == KRS_ERR_INVALID
    assert _fwd(lib, q, k, v, out, lse, dtype=L.I8) == KRS_ERR_INVALID
    assert _fwd(lib, q, k, v, out, lse, dtype=7) == KRS_ERR_INVALID
    assert _fwd(lib, q, k, v, out, lse, p=1.0) == KRS_ERR_INVALID
    assert _fwd(lib, q, k, v, out, lse, p=-0.1) == KRS_ERR_INVALID
    assert _fwd(lib, q, k, v, out, lse, p=math.nan) == KRS_ERR_INVALID
    assert _fwd(lib, q, k, v, out, lse, p=0.5, draw=None) == KRS_ERR_INVALID      # dropout without its counter
    assert _fwd(lib, q, k, v, out, lse, ld=h * dh - 1) == KRS_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all() and torch.isnan(lse).all()              # no refused call launched anything
    assert _fwd(lib, q, k, v, out, lse, b=0) == 0 and route() == (0, 0)
    assert _fwd(lib, q, k, v, out, lse, l=0) == 0
    assert lib.krs_seq_attn_fwd(None, 8, None, 8, None, 8, L.BF16, 0, 1, 5, 8, None, 0, 1.0, 0.0, 0, None, None, 8, None,
                                None, 0, None) == 0
    assert lib.krs_seq_attn_bwd(None, 8, None, 8, None, 8, L.BF16, 0, 1, 5, 8, None, 0, 1.0, 0.0, 0, None, None, 8, None,
                                8, None, q.data_ptr(), 8, None, 8, None, 8, None, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()
    assert lib.krs_seq_attn_workspace_bytes(0, 2, 5, 8, L.BF16) == 0


def test_memory_stays_linear_in_the_sequence_length():
    # B = 64, H = 2, L = 1024, Dh = 64, bf16: one fp32 score tensor alone would be 512 MiB
    b, h, l, dh = 64, 2, 1024, 64
    g = torch.Generator(device=DEV).manual_seed(5)
    q, k, v = (torch.randn(b, l, h, dh, device=DEV, generator=g).to(torch.bfloat16).requires_grad_(True) for _ in range(3))
    dout = torch.randn(b, l, h, dh, device=DEV, generator=g).to(torch.bfloat16)
    tensor_bytes = 8 * q.numel() * 2 + b * h * l * 4                              # q k v out dout dq dk dv, lse
    budget = 2 * (tensor_bytes + S.seq_attn_workspace_bytes(b, h, l, dh))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = S.seq_attention(q, k, v, causal=True)
    grads = torch.autograd.grad(out, (q, k, v), dout)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - (before - 4 * q.numel() * 2)       # (q, k, v, dout were allocated before)
    print(f"peak {used / 2**20:.1f} MiB, budget {budget / 2**20:.1f} MiB, one fp32 score tensor {b * h * l * l * 4 / 2**20:.0f} MiB")
    assert used <= budget < b * h * l * l * 4
    assert S.last_route() == (T.FAST, 64) and all(torch.isfinite(x.float()).all() for x in grads)
