"""krs_gemm_q8 (K18) on every row of tests/gemm_q8_cases.py, through the C ABI: the kernel each case ran is asserted from
krs_gemm_q8_last_route, and its result is held to the numpy restatement (tests/gemm_q8_restatement.py).

The integer reference of every check is aq.double() @ wq.double().T, computed by torch on the device and never by a kernel
of this library; it is exact because |idot| < 2^31 << 2^53.

  * plain product, fp32, no epilogue: full-range int8 operands (rows of -128 included), random steps with full mantissas, one
    activation row with step 0.  C equals restatement.product BIT FOR BIT -- nothing here is a tolerance -- the step-0 row is
    the canonical quiet NaN and its neighbours are exact.  A second call gives equal bits.
  * epilogue forms, exact (every run with one step-0 activation row: that row is the canonical quiet NaN in C and in u_out
    whatever the epilogue -- ReLU, the ring's cross build included -- and every other row is exact): operands +-1 .. +-4, steps that are powers of two, small-integer bias / x0 / x / R, diag_scale and
    beta from {0.5, 2, -2}: every epilogue step is representable in fp32 -- asserted on the reference -- so C and u_out equal
    the float64 reference bit for bit at fp32 and its one rounding to nearest even at bf16.
  * epilogue forms, real data, all four activations: with z64 = idot * wstep * astep in float64,
        |got - ref| <= gamma(3 + 8) * E + |x0| * act_err [+ half a bf16 ulp],  gamma(n) = n u / (1 - n u), u = 2^-24,
    E = |x0| (|z| + |bias| [+ 1 for sigmoid] + |diag_scale x|) + |x| + |beta R| (without the cross form: |z| + |bias| [+ 1]
    + |beta R|): tests/test_gemm_routes_gpu.py's bound with S replaced by |z| and the product's three roundings (the
    conversion and two multiplies) in place of gamma(k); act_err = 1e-5 for sigmoid and tanh, else 0.
  * padding: every operand with a padded leading dimension or an offset base lives in a wider allocation; input padding holds
    -128, output padding a bit pattern that must be unchanged afterwards.
  * a captured graph of the quantizer and the product replays to equal bits.
"""

import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests import gemm_q8_restatement as RS
from tests.gemm_q8_cases import CASES, FORMS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U32 = 2.0 ** -24
ACT_ERR = 1e-5
PRODUCT_ROUNDINGS, EPILOGUE_OPS = 3, 8
ACT_NAMES = {RS.ACT_NONE: "none", RS.ACT_RELU: "relu", RS.ACT_SIGMOID: "sigmoid", RS.ACT_TANH: "tanh"}
_PATTERN = {torch.bfloat16: (torch.int16, 0x4B3C), torch.float32: (torch.int32, 0x4B3C2D1E)}
_IDS = [c.name for c in CASES]


def _gamma(n):
    return n * U32 / (1.0 - n * U32)


def _gen(case, salt):
    g = torch.Generator(device=DEV)
    g.manual_seed(zlib.crc32(f"{case.name}/{salt}".encode()))
    return g


class _Int8Slab:
    """[rows, cols] int8 at byte offset `off` of a wider allocation, row stride ld >= cols; everything else holds -128."""

    def __init__(self, values, ld, off):
        rows, cols = values.shape
        self.flat = torch.full((off + rows * ld + 16,), -128, dtype=torch.int8, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.flat[off:off + rows * ld].view(rows, ld)[:, :cols] = values
        self.ptr, self.ld = self.flat.data_ptr() + off, ld


class _OutSlab:
    """[rows, cols] of `dtype` at element offset `off` of a wider allocation that holds a bit pattern."""

    def __init__(self, rows, cols, ld, off, dtype):
        self.int_dtype, pattern = _PATTERN[dtype]
        self.flat = torch.empty(off + rows * ld + 8, dtype=dtype, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.flat.view(self.int_dtype).fill_(pattern)
        self.window = self.flat[off:off + rows * ld].view(rows, ld)[:, :cols]
        self.ptr, self.ld, self.pattern = self.flat.data_ptr() + off * self.flat.element_size(), ld, pattern

    def padding_untouched(self):
        bits = self.flat.view(self.int_dtype).clone()
        off = (self.ptr - self.flat.data_ptr()) // self.flat.element_size()
        rows, cols = self.window.shape
        bits[off:off + rows * self.ld].view(rows, self.ld)[:, :cols] = self.pattern
        return bool((bits == self.pattern).all())


_DATA = {}


def _data(case, pattern):
    """{"aq", "wq" int8 on the device, "astep", "wstep" fp32, "idot" int32 [m, n] (torch's float64 product, exact)};
    computed once per case and pattern and left unchanged."""
    key = (case.name, pattern)
    if key not in _DATA:
        g = _gen(case, pattern)
        m, n, k = case.m, case.n, case.k
        if pattern == "full":
            aq = torch.randint(-128, 128, (m, k), generator=g, device=DEV, dtype=torch.int8)
            wq = torch.randint(-128, 128, (n, k), generator=g, device=DEV, dtype=torch.int8)
            aq[0] = -128                                           # a row of -128 against ...
            wq[n // 2] = -128                                      # ... a column of -128: the largest |idot| there is
            if k * 128 * 127 > 2 ** 24 and m > 1 and n > 1:        # K long enough for a sum that fp32 cannot hold:
                aq[1], wq[0] = -128, 127                           # -128 * 127 * (k - 1) + 127 is odd and beyond 2^24,
                aq[1, 7] = 1                                       # so the device's int -> float conversion must round it
            astep = torch.rand(m, generator=g, device=DEV) * 0.1 + 1e-3
            wstep = torch.rand(n, generator=g, device=DEV) * 0.01 + 1e-4
        else:                                                      # "exact": +-1 .. +-4, steps that are powers of two
            def signed(shape):
                mag = torch.randint(1, 5, shape, generator=g, device=DEV)
                return (mag * (torch.randint(0, 2, shape, generator=g, device=DEV) * 2 - 1)).to(torch.int8)

            aq, wq = signed((m, k)), signed((n, k))
            astep = torch.tensor([0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 3, (m,), generator=g, device=DEV)]
            wstep = torch.tensor([0.25, 1.0, 2.0], device=DEV)[torch.randint(0, 3, (n,), generator=g, device=DEV)]
        wide = aq.double() @ wq.double().T
        assert float(wide.abs().max()) < 2.0 ** 31
        _DATA[key] = dict(aq=aq, wq=wq, astep=astep.float().contiguous(), wstep=wstep.float().contiguous(),
                          idot=wide.to(torch.int32))
        assert torch.equal(_DATA[key]["idot"].double(), wide)
    return _DATA[key]


def _launch(case, d, odt, astep=None, form=(), act=RS.ACT_NONE, diag=0.0, beta=1.0, ops=None):
    """One krs_gemm_q8 through the C ABI on padded slabs.  Returns (C slab, u slab or None, route dict)."""
    from keras_rs_amd import _lib as lib
    from keras_rs_amd import dense_ops as D

    lda, ldw, ldc = case.lds()
    a = _Int8Slab(d["aq"], lda, case.a_off)
    w = _Int8Slab(d["wq"], ldw, case.w_off)
    c = _OutSlab(case.m, case.n, ldc, case.c_off, odt)
    astep = d["astep"] if astep is None else astep
    ep, u = None, None
    if form:
        ep = lib.GemmEpilogue()
        ep.act, ep.diag_scale, ep.beta = act, diag, beta
        if "bias" in form:
            ep.bias = ops["bias"].data_ptr()
        if "x0" in form:
            ep.x0, ep.x, ep.ldx = ops["x0"].data_ptr(), ops["x"].data_ptr(), case.n
        if "u" in form:
            u = _OutSlab(case.m, case.n, case.n, 0, odt)
            ep.u_out, ep.ldu = u.ptr, u.ld
        if "r" in form:
            ep.r, ep.ldr = ops["r"].data_ptr(), case.n
    rc = lib.lib().krs_gemm_q8(a.ptr, a.ld, astep.data_ptr(), w.ptr, w.ld, d["wstep"].data_ptr(), c.ptr, c.ld, case.m, case.n,
                               case.k, lib.fdtype(c.flat), C.byref(ep) if ep is not None else None, lib.stream_ptr())
    lib.check(rc, "krs_gemm_q8")
    route = D.last_gemm_q8_route()
    torch.cuda.synchronize()
    assert route["kernel"] == case.kernel and route["k_tail"] == case.k_tail, (case.name, route)
    # the ring's cross build runs exactly where the contract says: bf16 output, x0 without R, vector access everywhere
    cross_build = case.kernel == "ring" and odt == torch.bfloat16 and route["ep_vec"] and "x0" in form and "r" not in form
    assert route["epilogue"] == int(cross_build), (case.name, route)
    assert c.padding_untouched(), "the kernel wrote outside C"
    assert u is None or u.padding_untouched()
    return c, u, route


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_plain_product_equals_the_restatement_bit_for_bit(case):
    d = _data(case, "full")
    astep = d["astep"].clone()
    dead = case.m // 2
    astep[dead] = 0.0                                               # a non-finite activation row, as the quantizer marks it
    if case.k == 3456:                                              # the device rounds a sum that fp32 cannot hold
        odd = int(d["idot"][1, 0])
        assert odd == -128 * 127 * (case.k - 1) + 127 and abs(odd) > 2 ** 24 and float(np.float32(odd)) != float(odd) and dead != 1
    c, _, route = _launch(case, d, torch.float32, astep=astep)
    # the restatement's product from torch's exact integer sums: convert, scale twice, NaN where the step is 0
    want = RS.scale(d["idot"].cpu().numpy(), astep.cpu().numpy(), d["wstep"].cpu().numpy())
    want[dead] = np.nan
    got = c.window.cpu().numpy()
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert (got.view(np.uint32)[dead] == 0x7FC00000).all(), "the step-0 row is not the canonical quiet NaN"
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), (case.name, route, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    if case.m > 1:
        assert np.isfinite(got[[r for r in (dead - 1, dead + 1) if 0 <= r < case.m]]).all()
    again, _, _ = _launch(case, d, torch.float32, astep=astep)
    assert torch.equal(again.window.view(torch.int32), c.window.view(torch.int32)), "two calls differ"


def _ops(case, form, odt, pattern, g):
    """float64 epilogue operands on the device, representable in their dtypes: bias fp32 [n]; x0, x, r of `odt` [m, n]."""
    m, n = case.m, case.n

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=g, device=DEV).double()

    def reals(shape, dtype):
        return ((torch.rand(shape, generator=g, device=DEV) * 2 - 1)).to(dtype).double()

    o = {}
    if "bias" in form:
        o["bias"] = ints((n,), -3, 3) if pattern == "exact" else reals((n,), torch.float32) * 0.5
    if "x0" in form:
        o["x0"] = ints((m, n), -4, 4) if pattern == "exact" else reals((m, n), odt)
        o["x"] = ints((m, n), -3, 3) if pattern == "exact" else reals((m, n), odt)
    if "r" in form:
        o["r"] = ints((m, n), -3, 3) if pattern == "exact" else reals((m, n), odt)
    dev = {k: v.to(torch.float32 if k == "bias" else odt).contiguous() for k, v in o.items()}
    for k in o:
        assert torch.equal(dev[k].double(), o[k])
    return o, dev


def _reference(d, o, form, act, diag, beta):
    """float64 epilogue(z64) on the device.  Returns (C, u or None, steps, bound_c, bound_u): bound_* before the output
    rounding."""
    z = d["idot"].double() * d["wstep"].double()[None, :] * d["astep"].double()[:, None]
    steps, env, v = [z], z.abs(), z
    if "bias" in form:
        v = v + o["bias"]
        env = env + o["bias"].abs()
        steps.append(v)
    if act == RS.ACT_RELU:
        v = v.clamp_min(0.0)
    elif act == RS.ACT_SIGMOID:
        v = torch.sigmoid(v)
        env = env + 1.0
    elif act == RS.ACT_TANH:
        v = torch.tanh(v)
    act_err = ACT_ERR if act in (RS.ACT_SIGMOID, RS.ACT_TANH) else 0.0
    g = _gamma(PRODUCT_ROUNDINGS + EPILOGUE_OPS)
    u, bound_u, lip = None, None, 1.0
    if "x0" in form:
        u, bound_u = v, g * env + act_err
        dx = diag * o["x"]
        inner = v + dx
        prod = o["x0"] * inner
        v = prod + o["x"]
        steps += [dx, inner, prod, v]
        lip = o["x0"].abs()
        env = lip * (env + dx.abs()) + o["x"].abs()
    if "r" in form:
        br = beta * o["r"]
        v = v + br
        steps += [br, v]
        env = env + br.abs()
    return v, (u if "u" in form else None), steps, g * env + lip * act_err, bound_u


# (form, activation, output dtype, diag_scale, beta) every case runs on exact data: bias, both exact activations, the cross
# form with and without u_out, the residual, both output dtypes
_EXACT_RUNS = (("bias", RS.ACT_RELU, torch.float32, 0.0, 1.0), ("cross_u", RS.ACT_NONE, torch.float32, 0.5, 1.0),
               ("cross", RS.ACT_RELU, torch.bfloat16, 2.0, 1.0), ("cross_u", RS.ACT_RELU, torch.bfloat16, 0.5, 1.0),
               ("residual", RS.ACT_NONE, torch.bfloat16, 0.0, -2.0), ("none", RS.ACT_NONE, torch.bfloat16, 0.0, 1.0))
_QUIET_NAN = {torch.float32: 0x7FC00000, torch.bfloat16: 0x7FC0}


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_epilogue_forms_are_exact_on_integer_data(case):
    d = _data(case, "exact")
    # one activation row with step 0 in every run: the non-finite-row rule holds whatever the epilogue (ReLU would turn a NaN
    # into 0), in C and in u_out, on every kernel and on the ring's cross build, and leaves every other row exact
    dead = case.m // 2
    astep = d["astep"].clone()
    astep[dead] = 0.0
    for name, act, odt, diag, beta in _EXACT_RUNS:
        form = FORMS[name]
        o, dev = _ops(case, form, odt, "exact", _gen(case, name))
        ref, ref_u, steps, _, _ = _reference(d, o, form, act, diag, beta)
        for s in steps:                                             # every epilogue step is representable in fp32
            assert torch.equal(s.float().double(), s), (case.name, name)
        c, u, _ = _launch(case, d, odt, astep=astep, form=form or ("none",), act=act, diag=diag, beta=beta, ops=dev)
        idt = _PATTERN[odt][0]
        for got, ref64, what in ((c, ref, "C"), (u, ref_u, "u_out")):
            if got is None:
                continue
            want = ref64.float().to(odt)                            # fp32: exact; bf16: the one rounding to nearest even
            want[dead] = float("nan")
            bits, want_bits = got.window.contiguous().view(idt), want.view(idt)
            assert (bits[dead] == _QUIET_NAN[odt]).all(), (case.name, name, what, "the step-0 row is not the canonical quiet NaN")
            bad = bits != want_bits
            assert not bad.any(), (case.name, name, what, int(bad.sum()), torch.nonzero(bad)[:4].tolist())


# on real data all four activations, each form once per output dtype
_REAL_RUNS = (("bias", RS.ACT_SIGMOID, torch.float32, 0.0, 1.0), ("cross_u", RS.ACT_TANH, torch.float32, 0.5, 1.0),
              ("cross", RS.ACT_RELU, torch.bfloat16, 2.0, 1.0), ("cross_u", RS.ACT_SIGMOID, torch.bfloat16, 0.0, 1.0),
              ("residual", RS.ACT_NONE, torch.float32, 0.0, 0.75), ("bias", RS.ACT_TANH, torch.bfloat16, 0.0, 1.0),
              ("none", RS.ACT_NONE, torch.bfloat16, 0.0, 1.0))


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_epilogue_forms_on_real_data_within_the_float64_bound(case):
    d = _data(case, "full")
    worst = 0.0
    for name, act, odt, diag, beta in _REAL_RUNS:
        form = FORMS[name]
        o, dev = _ops(case, form, odt, "real", _gen(case, name + "/real"))
        ref, ref_u, _, bound_c, bound_u = _reference(d, o, form, act, diag, beta)
        c, u, _ = _launch(case, d, odt, form=form or ("none",), act=act, diag=diag, beta=beta, ops=dev)
        half_ulp = (lambda r: r.abs() * 2.0 ** -8) if odt == torch.bfloat16 else (lambda r: 0.0)
        for got, want, bound, what in ((c, ref, bound_c, "C"), (u, ref_u, bound_u, "u_out")):
            if got is None:
                continue
            err = (got.window.double() - want).abs()
            tol = bound + half_ulp(want)
            ratio = float((err / tol.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (case.name, name, ACT_NAMES[act], what, ratio)
    print(f"{case.name}: worst error / bound = {worst:.3f}")


def test_the_python_op_quantizes_and_multiplies_as_the_restatement_does():
    from keras_rs_amd import dense_ops as D

    rng = np.random.default_rng(18)
    for m, n, k in ((37, 24, 48), (5, 3, 13), (260, 136, 512)):
        x = rng.standard_normal((m, k)).astype(np.float32)
        x[m // 3] *= 50.0
        w = (rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32)
        wq, wstep = RS.quantize_kernel(w)
        z, _, astep = RS.dense(x, wq, wstep)
        got, u = D.gemm_q8(torch.from_numpy(x).to(DEV), torch.from_numpy(wq).to(DEV), torch.from_numpy(wstep).to(DEV))
        assert u is None and got.dtype == torch.float32
        assert (got.cpu().numpy().view(np.uint32) == z.view(np.uint32)).all(), (m, n, k)
        # inside the derived quantization bound of the float product
        err = np.abs(got.cpu().numpy().astype(np.float64) - x.astype(np.float64) @ w.astype(np.float64))
        assert (err <= RS.quantization_bound(x, w, astep, wstep)).all()
    # a non-finite input row comes back as NaNs, the others as before
    x[2, 5] = np.inf
    got2, _ = D.gemm_q8(torch.from_numpy(x).to(DEV), torch.from_numpy(wq).to(DEV), torch.from_numpy(wstep).to(DEV))
    g2 = got2.cpu().numpy()
    assert np.isnan(g2[2]).all() and (np.delete(g2, 2, 0).view(np.uint32) == np.delete(z, 2, 0).view(np.uint32)).all()


@pytest.mark.parametrize("shape", [(300, 264, 256), (192 * 256, 256, 384)], ids=["tile128", "ring"])
def test_a_captured_graph_of_quantizer_and_product_replays_to_equal_bits(shape):
    from keras_rs_amd import dense_ops as D

    m, n, k = shape
    g = torch.Generator(device=DEV)
    g.manual_seed(7)
    x = torch.randn((m, k), generator=g, device=DEV)
    wq = torch.randint(-127, 128, (n, k), generator=g, device=DEV, dtype=torch.int8)
    wstep = torch.rand(n, generator=g, device=DEV) * 0.01 + 1e-4
    bias = torch.randn(n, generator=g, device=DEV)

    def run():
        return D.gemm_q8(x, wq, wstep, bias=bias, act=RS.ACT_RELU)[0]

    eager = run().clone()
    assert D.last_gemm_q8_route()["kernel"] == ("ring" if m >= 192 * 256 else "tile128")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))
    x.mul_(-0.5)                                                    # new inputs in the captured buffers
    want = run().clone()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and not torch.equal(want, eager)
