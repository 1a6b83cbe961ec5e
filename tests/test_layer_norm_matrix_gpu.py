"""K22 on the GPU, through the C ABI: every case of tests/layer_norm_cases.py against the float64 reference on the route
the table claims, forward and backward; the kept set; bit-identical calls; each gradient alone on NaN-filled buffers;
the two routes on one shape; refusals and no-ops."""

import ctypes as C

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import norm_ops
from tests import layer_norm_cases as T
from tests import layer_norm_restatement as R

pytestmark = pytest.mark.gpu
IDS = [c.name for c in T.CASES]
DEV = "cuda:0"


def _matrix(a, case, fill=None):
    """The first d columns of an [n, d + pad] device buffer (the rest NaN), holding a (or `fill` everywhere when a is None)."""
    dt = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    buf = torch.full((case.n, case.d + case.pad), float("nan"), dtype=dt, device=DEV)
    view = buf[:, :case.d]
    if a is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dt))
    elif fill is not None:
        view.fill_(fill)
    return view


def _vector(a):
    return None if a is None else torch.from_numpy(a.astype(np.float32)).to(DEV)


def _host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def run_case(case, t, *, want=("dx", "dres", "dgamma", "dbeta"), nan_fill=True):
    """One forward and one backward call on the case's matrices; {key: float64 array}, and the routes of both calls."""
    ld = case.d + case.pad
    dtc = L.BF16 if case.dtype == "bf16" else L.F32
    norm = case.form != "add"
    fill = float("nan") if nan_fill else 0.0
    x, res = _matrix(t["x"], case), (None if t["residual"] is None else _matrix(t["residual"], case))
    gamma, beta = _vector(t["gamma"]), _vector(t["beta"])
    draw = torch.tensor([t["draw"]], dtype=torch.int64, device=DEV) if case.p > 0 else None
    y = _matrix(None, case, fill) if norm else None
    s = _matrix(None, case, fill) if case.form != "norm" else None
    mean = torch.full((case.n,), fill, dtype=torch.float32, device=DEV) if norm else None
    rstd = torch.full((case.n,), fill, dtype=torch.float32, device=DEV) if norm else None
    lib = L.lib()
    rc = lib.krs_ln_fwd(L.ptr(x), ld, L.ptr(res), ld, L.ptr(gamma), L.ptr(beta), dtc, case.n, case.d, case.eps, case.p,
                        t["seed"], L.ptr(draw), L.ptr(y), ld, L.ptr(s), ld, L.ptr(mean), L.ptr(rstd), L.stream_ptr())
    L.check(rc, "krs_ln_fwd")
    routes = [norm_ops.last_route()]
    out = {"s": _host(x if s is None else s)}
    if norm:
        out.update(y=_host(y), mean=_host(mean), rstd=_host(rstd))
    saved = x if s is None else s
    dy = None if t["dy"] is None else _matrix(t["dy"], case)
    dsum = None if t["dsum"] is None else _matrix(t["dsum"], case)
    bufs = {"dx": _matrix(None, case, fill) if "dx" in want else None,
            "dres": _matrix(None, case, fill) if "dres" in want else None,
            "dgamma": torch.full((case.d,), fill, dtype=torch.float32, device=DEV) if (norm and "dgamma" in want) else None,
            "dbeta": torch.full((case.d,), fill, dtype=torch.float32, device=DEV) if (norm and "dbeta" in want) else None}
    size = norm_ops.ln_workspace_bytes(case.n, case.d)
    ws = torch.full((size // 4,), fill, dtype=torch.float32, device=DEV)
    rc = lib.krs_ln_bwd(L.ptr(saved), ld, L.ptr(dy), ld, L.ptr(dsum), ld, L.ptr(gamma), L.ptr(mean), L.ptr(rstd), dtc, case.n,
                        case.d, case.p, t["seed"], L.ptr(draw), L.ptr(bufs["dx"]), ld, L.ptr(bufs["dres"]), ld,
                        L.ptr(bufs["dgamma"]), L.ptr(bufs["dbeta"]), L.ptr(ws), size, L.stream_ptr())
    L.check(rc, "krs_ln_bwd")
    routes.append(norm_ops.last_route())
    out.update({k: _host(v) for k, v in bufs.items() if v is not None})
    return out, routes


@pytest.mark.parametrize("index", range(len(T.CASES)), ids=IDS)
def test_every_case_against_float64_on_the_claimed_route(index):
    case = T.CASES[index]
    t, ref, bound = T.reference_of(index)
    got, routes = run_case(case, t)
    assert routes == [(case.route, case.lanes, case.vec)] * 2, routes
    assert set(got) == set(ref)
    ratio, where = T.worst_ratio(got, ref, bound)
    print(f"{case.name}: worst error over bound {ratio:.4f} at {where}")
    assert ratio <= 1.0, f"{case.name}: worst error over bound {ratio:.4f} at {where}"
    if case.p > 0:                                   # the kept set is the restatement's exactly
        kept = R.kept(t["seed"], t["draw"], case.n, case.d, case.p)
        if t["residual"] is None:                    # s = round(x / (1 - p)) where kept, 0 where dropped
            live = t["x"] != 0
            assert np.array_equal((got["s"] != 0)[live], kept[live])
        live = got["dres"] != 0                      # dx = round(ds / (1 - p)) where kept, 0 where dropped
        assert np.array_equal((got["dx"] != 0)[live], kept[live])
    if case.special == "const":                      # variance 0: y = beta exactly, everything finite
        want = np.zeros(case.d) if t["beta"] is None else t["beta"]
        assert np.array_equal(got["y"][0], R.round_to(want, case.dtype)) and got["mean"][0] == 1.5


REPEAT = [i for i, c in enumerate(T.CASES) if c.form == "addnorm" and (c.n == 257 or c.pad or c.d >= 1000)]


@pytest.mark.parametrize("index", REPEAT, ids=[IDS[i] for i in REPEAT])
def test_two_calls_are_bit_identical_and_each_gradient_alone_equals_the_full_call(index):
    case = T.CASES[index]
    t, _, _ = T.reference_of(index)
    a, _ = run_case(case, t)
    b, _ = run_case(case, t, nan_fill=False)
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    for key in ("dx", "dres", "dgamma", "dbeta"):
        if key in a:
            alone, _ = run_case(case, t, want=(key,))
            assert np.array_equal(alone[key], a[key]), key


def test_vec_and_element_routes_agree_on_a_shared_case():
    t = T.inputs_of(T.SHARED_VEC, 977)
    ref = T.reference(T.SHARED_VEC, t)
    bound = T.bounds(T.SHARED_VEC, t, ref)
    a, ra = run_case(T.SHARED_VEC, t)
    b, rb = run_case(T.SHARED_ELEM, t)
    assert ra == [(T.VEC, 16, 1)] * 2 and rb == [(T.ELEM, 16, 0)] * 2
    assert np.array_equal(a["s"], b["s"])            # one rounding of one multiply-add: the same bits on both routes
    for got in (a, b):
        assert T.worst_ratio(got, ref, bound)[0] <= 1.0
    # the two routes add a row in different orders: they differ by the sums' fp32 noise and one rounding of the output
    for key in ("y", "dx", "dres"):
        assert np.abs(a[key] - b[key]).max() <= 2.0 ** -7 * np.abs(a[key]).max()


def test_the_forward_without_statistics_pointers_gives_the_same_y():
    index = next(i for i, c in enumerate(T.CASES) if c.form == "addnorm" and c.dtype == "bf16" and c.n == 257 and c.d == 64)
    case = T.CASES[index]
    t, _, _ = T.reference_of(index)
    full, _ = run_case(case, t)
    dt = torch.bfloat16
    x, res = _matrix(t["x"], case), _matrix(t["residual"], case)
    y = _matrix(None, case)
    draw = torch.tensor([t["draw"]], dtype=torch.int64, device=DEV)
    gamma, beta = _vector(t["gamma"]), _vector(t["beta"])
    rc = L.lib().krs_ln_fwd(L.ptr(x), case.d, L.ptr(res), case.d, L.ptr(gamma), L.ptr(beta), L.BF16,
                            case.n, case.d, case.eps, case.p, t["seed"], L.ptr(draw), L.ptr(y), case.d, None, 0, None, None,
                            L.stream_ptr())
    L.check(rc, "krs_ln_fwd")
    assert y.dtype == dt and np.array_equal(_host(y), full["y"]) and int(draw.item()) == t["draw"]    # draw is only read


def test_refusals_and_no_ops_on_device_pointers():
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV)
    y = torch.full((4, 64), 7.0, dtype=torch.bfloat16, device=DEV)
    lib = L.lib()
    args = lambda n, d, p, yy: (L.ptr(x), 64, None, 0, None, None, L.BF16, n, d, 1e-5, p, 0, None, L.ptr(yy), 64, None, 0, None,
                                None, L.stream_ptr())
    assert lib.krs_ln_fwd(*args(0, 64, 0.0, y)) == 0 and norm_ops.last_route() == (0, 0, 0)
    assert lib.krs_ln_fwd(*args(4, 64, 0.2, y)) == -1 and b"draw" in lib.krs_last_error()
    assert lib.krs_ln_fwd(*args(4, 4097, 0.0, y)) == -2 and b"d <= 4096" in lib.krs_last_error()
    assert lib.krs_ln_fwd(*args(4, 64, 0.0, None)) == -1 and b"no output" in lib.krs_last_error()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full_like(y, 7.0))                 # nothing was written by a refused call or a no-op
    assert lib.krs_ln_fwd(*args(4, 64, 0.0, y)) == 0 and norm_ops.last_route() == (T.VEC, 8, 1)
    torch.cuda.synchronize()
    assert torch.equal(y, torch.zeros_like(y))                     # a zero row: variance 0, y = beta = 0
    kernel, lanes, vec = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.krs_ln_last_route(C.addressof(kernel), C.addressof(lanes), C.addressof(vec)) == T.VEC
    assert (kernel.value, lanes.value, vec.value) == (T.VEC, 8, 1)
