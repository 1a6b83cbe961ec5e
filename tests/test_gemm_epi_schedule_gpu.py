"""The epilogue schedules of gemm_pp64_kernel (krs_gemm_set_option(KRS_GEMM_OPT_EPI_SCHEDULE, 0 | 1 | 2 | 3)) change when
an operand is requested and which workgroup computes a tile -- never a bit.  At the smallest shapes that put the cross
build on the unsplit 64-k ring (14 x 14 tiles of 256 x 256; M = 3500 clamps rows in the last panel, N = 3456 ends on half
a tile, N = 3464 on eight columns; K = 192 is the ring's minimum of three blocks, K = 512 the C3 cross layers'), every
output byte under options 1, 2 and 3 equals option 0's, option 0's equal the two-stage reference schedule
(KRS_GEMM_OPT_PIPELINE = 0), the sentinel rows and columns around C and u stay untouched, the route record names the
schedule, and a second run gives the same bytes."""

import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7FC1          # a bf16 NaN pattern no result takes
MARGIN_ROWS, MARGIN_COLS = 2, 8      # (8 columns = 16 bytes: the window stays on 16 bytes)

# K = 192 is three 64-k blocks, but the planner keeps K < 256 (gplan::kRingMinK) on the 128 x 128 kernels whatever M is: those
# cases run there under every option, name no schedule and must give the same bytes all the same.  K = 256 is the ring's
# shortest main loop (one steady block, then its two tail blocks).
RING_MIN_K = 256
SHAPES = [(m, n, k) for m in (3584, 3500) for n in (3456, 3464) for k in (192, 256, 512)]


class _Framed:
    """An [m, n] bf16 window inside a sentinel-filled allocation: MARGIN_ROWS rows above and below, MARGIN_COLS columns left
    and right of every row (the leading dimension is n + 2 * MARGIN_COLS)."""

    def __init__(self, m, n):
        self.m, self.n, self.ld = m, n, n + 2 * MARGIN_COLS
        self.buf = torch.empty((m + 2 * MARGIN_ROWS, self.ld), dtype=torch.int16, device=DEV)
        self.reset()

    def reset(self):
        self.buf.fill_(SENTINEL)

    @property
    def ptr(self):
        return self.buf.data_ptr() + (MARGIN_ROWS * self.ld + MARGIN_COLS) * 2

    def frame_untouched(self):
        inside = torch.zeros_like(self.buf, dtype=torch.bool)
        inside[MARGIN_ROWS:MARGIN_ROWS + self.m, MARGIN_COLS:MARGIN_COLS + self.n] = True
        return bool((self.buf[~inside] == SENTINEL).all())

    def window_written(self):
        w = self.buf[MARGIN_ROWS:MARGIN_ROWS + self.m, MARGIN_COLS:MARGIN_COLS + self.n]
        return bool((w != SENTINEL).all())


def _set(key, value):
    from keras_rs_amd import _lib as L

    L.check(L.lib().krs_gemm_set_option(key, value), "krs_gemm_set_option")


def _defaults():
    from keras_rs_amd import _lib as L

    L.lib().krs_gemm_set_option(L.GEMM_OPT_PIPELINE, 4)
    L.lib().krs_gemm_set_option(L.GEMM_OPT_EPI_SCHEDULE, -1)


def _rnd(gen, *shape, scale=1.0):
    return ((torch.rand(*shape, device=DEV, generator=gen) - 0.5) * scale).to(torch.bfloat16)


def _gemm(a, bt, c, u, ep):
    """One krs_gemm through the C ABI into the framed outputs; returns (route, schedule) of the launch."""
    from keras_rs_amd import _lib as L
    from keras_rs_amd import dense_ops as D

    m, k = a.shape
    n = bt.shape[0]
    c.reset()
    if u is not None:
        u.reset()
    rc = L.lib().krs_gemm(a.data_ptr(), k, 0, bt.data_ptr(), k, 1, c.ptr, c.ld, m, n, k, L.BF16, L.BF16, C.byref(ep), None, 0,
                          L.stream_ptr())
    L.check(rc, "krs_gemm")
    route, schedule = D.last_gemm_route(), D.last_gemm_schedule()
    torch.cuda.synchronize()
    return route, schedule


def _check_all_schedules(a, bt, make_ep, want_u, build, names_of):
    """Option 0 against pipeline 0, options 1 .. 3 and a second run against option 0: whole allocations, frame included."""
    from keras_rs_amd import _lib as L

    m, n = a.shape[0], bt.shape[0]
    c, u = _Framed(m, n), (_Framed(m, n) if want_u else None)
    ep = make_ep(u)
    ring = a.shape[1] >= RING_MIN_K
    try:
        _set(L.GEMM_OPT_PIPELINE, 0)
        _set(L.GEMM_OPT_EPI_SCHEDULE, 0)
        route, schedule = _gemm(a, bt, c, u, ep)
        assert route["kernel"] in ("mfma", "glds") and route["epilogue"] == build and schedule == frozenset()
        assert c.frame_untouched() and c.window_written(), "C under the reference schedule"
        assert u is None or (u.frame_untouched() and u.window_written()), "u under the reference schedule"
        ref_c, ref_u = c.buf.clone(), (u.buf.clone() if u is not None else None)
        _set(L.GEMM_OPT_PIPELINE, 4)
        for option in (0, 1, 2, 3, 3):           # (the last twice: run to run)
            _set(L.GEMM_OPT_EPI_SCHEDULE, option)
            route, schedule = _gemm(a, bt, c, u, ep)
            assert route == dict(kernel="pp64" if ring else "mfma", splits=1, reduce=None, epilogue=build, ep_vec=True,
                                 thin_width=0, thin_is_a=False), (option, route)
            assert schedule == (names_of(option) if ring else frozenset()), (option, schedule)
            assert torch.equal(c.buf, ref_c), f"C differs under schedule {option} (frame included)"
            assert u is None or torch.equal(u.buf, ref_u), f"u differs under schedule {option} (frame included)"
    finally:
        _defaults()


@pytest.mark.parametrize("m,n,k", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_cross_products_are_byte_equal_under_every_schedule(m, n, k):
    from keras_rs_amd import _lib as L

    gen = torch.Generator(device=DEV).manual_seed(m * 7 + n * 3 + k)
    a, bt = _rnd(gen, m, k), _rnd(gen, n, k, scale=0.2)
    x0, x = _rnd(gen, m, n), _rnd(gen, m, n)
    bias = (torch.rand(n, device=DEV, generator=gen) - 0.5).float()
    for same in (False, True):
        for has_bias in (True, False):
            for act in (L.ACT_NONE, L.ACT_RELU):
                for want_u in (True, False):
                    def make_ep(u, same=same, has_bias=has_bias, act=act):
                        ep = L.GemmEpilogue()
                        ep.x0, ep.x, ep.ldx = x0.data_ptr(), (x0 if same else x).data_ptr(), n
                        ep.act, ep.diag_scale = act, 0.5
                        if has_bias:
                            ep.bias = bias.data_ptr()
                        if u is not None:
                            ep.u_out, ep.ldu = u.ptr, u.ld
                        return ep

                    first = "x_is_x0" if same else "lds_landing"
                    names = {0: frozenset(), 1: frozenset({first}), 2: frozenset({"stagger"}),
                             3: frozenset({first, "stagger"})}
                    _check_all_schedules(a, bt, make_ep, want_u, 1, names.__getitem__)


@pytest.mark.parametrize("m,n,k", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_the_residual_product_is_byte_equal_under_the_stagger(m, n, k):
    from keras_rs_amd import _lib as L

    gen = torch.Generator(device=DEV).manual_seed(m * 5 + n * 11 + k)
    a, bt, r = _rnd(gen, m, k), _rnd(gen, n, k, scale=0.2), _rnd(gen, m, n)

    def make_ep(u):
        ep = L.GemmEpilogue()
        ep.r, ep.ldr, ep.beta = r.data_ptr(), n, 1.0
        return ep

    names = {0: frozenset(), 1: frozenset(), 2: frozenset({"stagger"}), 3: frozenset({"stagger"})}
    _check_all_schedules(a, bt, make_ep, False, 2, names.__getitem__)


@pytest.mark.parametrize("m,n,k", [(3500, 3464, 256), (3584, 3456, 512)], ids=["3500x3464x256", "3584x3456x512"])
def test_the_fused_cross_backward_is_byte_equal_under_the_stagger(m, n, k):
    """krs_gemm_cross_bwd with R and dx0 accumulating (fused epilogue 4) and with the upper layer's u (7): G, dz, dx0 and the
    bias gradient under the staggered tile order against panel order; panel order's G and dz against the two-call form."""
    from keras_rs_amd import _lib as L
    from keras_rs_amd import dense_ops as D

    gen = torch.Generator(device=DEV).manual_seed(m + n + k)
    a, bt = _rnd(gen, m, k), _rnd(gen, n, k, scale=0.2)
    r, x0, u, told, u_up = (_rnd(gen, m, n) for _ in range(5))
    forms = {4: dict(dx0_into=True), 7: dict(u_upper=u_up)}

    def run(form):
        kw = dict(forms[form])
        if kw.pop("dx0_into", False):
            kw["dx0_into"] = told.clone()
        out = D.gemm_cross_bwd(a, bt, r, x0, u, act=L.ACT_RELU, **kw)
        route = D.last_cross_bwd_route()
        torch.cuda.synchronize()
        return out, route

    try:
        for form in forms:
            _set(L.GEMM_OPT_PIPELINE, 0)
            (g0, dz0, _, _), route = run(form)
            assert route == ("two_call", 0)
            _set(L.GEMM_OPT_PIPELINE, 4)
            _set(L.GEMM_OPT_EPI_SCHEDULE, 0)
            ref, route = run(form)
            assert route == ("pp64", form)
            assert torch.equal(ref[0], g0) and torch.equal(ref[1], dz0), form
            for option in (1, 2, 3, 3):
                _set(L.GEMM_OPT_EPI_SCHEDULE, option)
                got, route = run(form)
                assert route == ("pp64", form)
                for name, x, y in zip(("G", "dz", "dx0", "dbias"), got, ref):
                    assert torch.equal(x, y), f"{name} differs under schedule {option} (fused epilogue {form})"
    finally:
        _defaults()
