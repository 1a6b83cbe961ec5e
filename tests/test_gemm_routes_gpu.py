"""krs_gemm on every route of keras_rs_amd/csrc/gemm.hip: the kernel each case ran is asserted from krs_gemm_last_route, and
its result is checked against a float64 reference computed by torch on the device (never by a kernel of this library).

One table drives everything (tests/gemm_route_cases.py; its coverage is checked without a GPU by
tests/test_gemm_routes_host.py).  Per case:

  * exact test on integer data: A and B hold +-1 .. +-4 (no zeros: a dropped or doubled term always changes the sum), the
    epilogue operands small integers, diag_scale and beta come from {0, 0.5, 1, 2, -2}.  Every product, every partial sum in
    any order and every epilogue step is then exactly representable in fp32 -- the test asserts that on the reference -- so
    each route must return the float64 result bit for bit in fp32 and its one round-to-nearest-even in bf16.  All of C and
    all of u_out are compared.  The bf16-only epilogue builds 1 and 2 run a second pattern, B a signed selection matrix with
    32 entries per column, whose results bf16 holds exactly.
  * float64 bound on real-valued data (integers never fill the low mantissa bits), all four activations:
        |got - ref| <= gamma(k + c) * E + |x0| * act_err [+ half a bf16 ulp],   gamma(n) = n u / (1 - n u),  u = 2^-24,
    E = |x0| (S + |bias| [+ 1 for sigmoid] + |diag_scale x|) + |x| + |beta R| the magnitude envelope of the epilogue's
    intermediates over S = sum_k |a| |b| (without the cross form: E = S + |bias| [+ 1] + |beta R|), c = 8 the count of
    epilogue operations (bias add, activation, diag_scale * x, its add, x0 *, + x, beta * R, its add).  It holds for any
    summation order of fp32 sums of (bf16: exact, fp32: once rounded) products, so for every tile shape and split-K.
    act_err is the error of the device functions behind sigmoid (1 / (1 + __expf(-v))) and tanh (tanhf).  The ULP table of
    the HIP math documentation is not among the files a ROCm installation carries, so the term is the project's fp32 bar
    ("fp32 within 1e-5"), used for that term alone; it is 0 for none / ReLU.  No tolerance here was
    tuned to what the kernels return.
  * padding and neighbours: every operand with a padded leading dimension or an offset base pointer lives in a wider
    allocation.  Input padding holds 3 * 2^40 (finite, exact in bf16): a kernel may load it and multiply it by zero, not add
    it.  Output padding holds a bit pattern that must be unchanged afterwards, compared as integers.
  * determinism: split-K and ring cases run twice and must give equal bits.
"""

import ctypes as C
import zlib

import pytest
import torch

from tests.gemm_route_cases import ACT_FORMS, CASES, FORMS, leading_dims

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 3.0 * 2.0 ** 40
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3
ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu", ACT_SIGMOID: "sigmoid", ACT_TANH: "tanh"}
EPILOGUE_OPS = 8
ACT_ERR = 1e-5          # DESIGN.md section 2, "fp32 within 1e-5": stands in for the ULP bounds of __expf / tanhf
U32 = 2.0 ** -24
_PATTERN = {torch.bfloat16: (torch.int16, 0x4B3C), torch.float32: (torch.int32, 0x4B3C2D1E)}


def _dt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def _gamma(n):
    return n * U32 / (1.0 - n * U32)


class _Slab:
    """[rows, cols] of `dtype` at element offset `off` of a wider allocation, row stride ld >= cols.  Inputs: everything
    but the window holds SENTINEL.  Outputs (values = None): the whole allocation holds a bit pattern."""

    def __init__(self, values, rows, cols, ld, off, dtype):
        self.flat = torch.empty(off + rows * ld + 1, dtype=dtype, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.int_dtype, pattern = _PATTERN[dtype]
        if values is None:
            self.flat.view(self.int_dtype).fill_(pattern)
        else:
            self.flat.fill_(SENTINEL)
        self.window = self.flat[off:off + rows * ld].view(rows, ld)[:, :cols]
        if values is not None:
            self.window.copy_(values)           # (float64 -> dtype: the values are representable, asserted by the caller)
            assert torch.equal(self.window.double(), values)
        self.ptr = self.flat.data_ptr() + off * self.flat.element_size()
        self.ld = ld
        self.before = self.flat.clone() if values is None else None

    def padding_untouched(self):
        was, now = self.before.clone(), self.flat.clone()
        for t in (was, now):
            t[self.window_slice()] = 0
        return torch.equal(was.view(self.int_dtype), now.view(self.int_dtype))

    def window_slice(self):
        mask = torch.zeros_like(self.flat, dtype=torch.bool)
        off = (self.ptr - self.flat.data_ptr()) // self.flat.element_size()
        rows, cols = self.window.shape
        mask[off:off + rows * self.ld].view(rows, self.ld)[:, :cols] = True
        return mask


def _signed(shape, lo, hi, g):
    """integers of magnitude lo .. hi with random signs, as float64"""
    mag = torch.randint(lo, hi + 1, shape, generator=g, device=DEV)
    return (mag * (torch.randint(0, 2, shape, generator=g, device=DEV) * 2 - 1)).double()


def _uniform(shape, dtype, g, scale=1.0):
    """uniform reals in (-scale, scale) with the full mantissa of `dtype`, as float64"""
    return ((torch.rand(shape, generator=g, device=DEV, dtype=torch.float32) * 2 - 1) * scale).to(dtype).double()


def _selection(k, n, g):
    """[k, n]: exactly 32 entries of +-1 per column, every k index selected by some column"""
    assert 32 <= k <= 32 * n, "the selection pattern needs 32 <= k <= 32 n"
    perm = torch.randperm(k, generator=g, device=DEV)
    rows = perm[(torch.arange(n, device=DEV)[:, None] * 32 + torch.arange(32, device=DEV)[None, :]) % k]     # [n, 32]
    b = torch.zeros((k, n), dtype=torch.float64, device=DEV)
    b[rows, torch.arange(n, device=DEV)[:, None].expand(n, 32)] = _signed((n, 32), 1, 1, g)
    assert ((b != 0).sum(0) == 32).all() and (b != 0).any(1).all()
    return b


def _operands(case, pattern, g):
    """float64 logical operands: A [m, k], B [k, n], bias [n], x0 / x / r [m, n] (those the epilogue form has)."""
    m, n, k, form = case.m, case.n, case.k, FORMS[case.ep]
    idt, odt = _dt(case.idt), _dt(case.odt)
    o = {}
    if pattern == "real":
        o["a"], o["b"] = _uniform((m, k), idt, g), _uniform((k, n), idt, g)
        if "bias" in form:
            o["bias"] = _uniform((n,), torch.float32, g, 0.5)
        for name in ("x0", "x") if "x0" in form else ():
            o[name] = _uniform((m, n), odt, g)
        if "r" in form:
            o["r"] = _uniform((m, n), odt, g)
        return o
    o["a"] = _signed((m, k), 1, 4, g)
    o["b"] = _selection(k, n, g) if pattern == "select" else _signed((k, n), 1, 4, g)
    if "bias" in form:
        o["bias"] = _signed((n,), 0, 3, g)
    if "x0" in form:
        o["x0"] = _signed((m, n), 1, 1, g) if pattern == "select" else _signed((m, n), 0, 4, g)
        o["x"] = _signed((m, n), 0, 3, g)
    if "r" in form:
        o["r"] = _signed((m, n), 0, 3, g)
    return o


def _reference(case, o, act, diag, beta):
    """float64 epilogue(A . B) as include/krs.h defines it.  Returns (C, u, steps, S, bound_c, bound_u): steps are the
    epilogue's intermediates (for the exactness assertion), S = |A| . |B|, bound_* the real-data bounds of the docstring
    before the output rounding."""
    form = FORMS[case.ep]
    p, s = o["a"] @ o["b"], o["a"].abs() @ o["b"].abs()
    steps = [p]
    env = s.clone()
    v = p
    if "bias" in form:
        v = v + o["bias"]
        env = env + o["bias"].abs()
        steps.append(v)
    if act == ACT_RELU:
        v = v.clamp_min(0.0)
    elif act == ACT_SIGMOID:
        v = torch.sigmoid(v)
        env = env + 1.0
    elif act == ACT_TANH:
        v = torch.tanh(v)
    act_err = ACT_ERR if act in (ACT_SIGMOID, ACT_TANH) else 0.0
    g = _gamma(case.k + EPILOGUE_OPS)
    u, bound_u, lip = None, None, 1.0
    if "x0" in form:
        u = v
        bound_u = g * env + act_err
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
    return v, (u if "u" in form else None), steps, s, g * env + lip * act_err, bound_u


def _launch(case, o, act, diag, beta):
    """One krs_gemm call through the C ABI.  Returns (c_slab, u_slab or None, route record)."""
    from keras_rs_amd import _lib as L
    from keras_rs_amd import dense_ops as D

    m, n, k, form = case.m, case.n, case.k, FORMS[case.ep]
    idt, odt = _dt(case.idt), _dt(case.odt)
    lda, ldb, ldc, ldx, ldu, ldr = leading_dims(case)
    off = case.off
    a_km, b_nk = case.layout == "tn", case.layout == "nt"
    a = _Slab(o["a"].t() if a_km else o["a"], k if a_km else m, m if a_km else k, lda, off.get("a", 0), idt)
    b = _Slab(o["b"].t() if b_nk else o["b"], n if b_nk else k, k if b_nk else n, ldb, off.get("b", 0), idt)
    c = _Slab(None, m, n, ldc, off.get("c", 0), odt)
    keep, u, ep = [a, b, c], None, None
    if case.ep != "null":
        ep = L.GemmEpilogue()
        ep.act, ep.diag_scale, ep.beta = act, diag, beta
        if "bias" in form:
            bias = _Slab(o["bias"][None, :], 1, n, n, off.get("bias", 0), torch.float32)
            ep.bias = bias.ptr
            keep.append(bias)
        if "x0" in form:
            x0 = _Slab(o["x0"], m, n, ldx, off.get("x0", 0), odt)
            x = _Slab(o["x"], m, n, ldx, off.get("x", 0), odt)
            ep.x0, ep.x, ep.ldx = x0.ptr, x.ptr, ldx
            keep += [x0, x]
        if "u" in form:
            u = _Slab(None, m, n, ldu, off.get("u", 0), odt)
            ep.u_out, ep.ldu = u.ptr, ldu
        if "r" in form:
            r = _Slab(o["r"], m, n, ldr, off.get("r", 0), odt)
            ep.r, ep.ldr = r.ptr, ldr
            keep.append(r)
    wsb = int(L.lib().krs_gemm_workspace_bytes(m, n, k, int(a_km))) if case.ws else 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV) if wsb else None
    rc = L.lib().krs_gemm(a.ptr, lda, int(a_km), b.ptr, ldb, int(b_nk), c.ptr, ldc, m, n, k,
                          L.F32 if idt == torch.float32 else L.BF16, L.F32 if odt == torch.float32 else L.BF16,
                          C.byref(ep) if ep is not None else None, L.ptr(ws), wsb, L.stream_ptr())
    L.check(rc, "krs_gemm")
    route = D.last_gemm_route()
    torch.cuda.synchronize()
    del keep
    return c, u, route


def _run(case, pattern, act, twice=False):
    """Operands, the product (under the case's pipeline option), the reference.  Asserts the route and the untouched
    padding; returns (got C, got u, reference tuple)."""
    from keras_rs_amd import _lib as L

    g = torch.Generator(device=DEV)
    g.manual_seed(zlib.crc32(f"{case.name}/{pattern}/{act}".encode()))
    diag, beta = case.diag, case.beta
    if pattern == "select":      # whole numbers only: the results must fit bf16's 8 bits
        diag, beta = (1.0 if abs(diag) == 0.5 else diag), (1.0 if abs(beta) == 0.5 else beta)
    o = _operands(case, pattern, g)
    try:
        L.check(L.lib().krs_gemm_set_option(0, case.pipe), "krs_gemm_set_option")
        c, u, route = _launch(case, o, act, diag, beta)
        if twice:
            c2, u2, route2 = _launch(case, o, act, diag, beta)
    finally:
        L.lib().krs_gemm_set_option(0, 4)
    assert route == case.route, f"{case.name} ran on {route}"
    assert c.padding_untouched(), "C: a store outside [m, n]"
    assert u is None or u.padding_untouched(), "u_out: a store outside [m, n]"
    if twice:
        assert route2 == route
        assert torch.equal(c.flat.view(c.int_dtype), c2.flat.view(c.int_dtype)), "C differs from run to run"
        assert u is None or torch.equal(u.flat.view(u.int_dtype), u2.flat.view(u.int_dtype)), "u differs from run to run"
    return c.window, (u.window if u is not None else None), _reference(case, o, act, diag, beta)


def _bits(t):
    return (t + 0).view(_PATTERN[t.dtype][0])        # (+ 0: a zero compares as +0 whatever its sign)


def _exact_in(t, dtype):
    return torch.equal(t.to(dtype).double(), t)


def _check_exact(case, pattern, act):
    got_c, got_u, (ref_c, ref_u, steps, s, _, _) = _run(case, pattern, act)
    if case.route["kernel"] is None:
        assert got_c.numel() == 0
        return
    # what makes bit equality the right demand: no sum can leave fp32's integers, no epilogue step rounds
    assert s.numel() == 0 or s.max().item() < 2.0 ** 24
    assert all(_exact_in(t, torch.float32) for t in steps)
    odt = _dt(case.odt)
    if pattern == "select":
        assert steps[0].abs().max().item() <= 128          # |A . B| <= 32 * 4
        assert odt == torch.bfloat16 and _exact_in(ref_c, odt) and (ref_u is None or _exact_in(ref_u, odt))
    for name, got, ref in (("C", got_c, ref_c), ("u_out", got_u, ref_u)):
        if ref is None:
            assert got is None
            continue
        exp = ref.float().to(odt)            # float64 -> fp32 is exact here; -> bf16 is the one round-to-nearest-even
        wrong = _bits(got) != _bits(exp)
        assert not wrong.any(), (f"{name}: {int(wrong.sum())} of {wrong.numel()} elements differ, first at "
                                 f"{wrong.nonzero()[0].tolist()}: got {got[wrong][0].item()}, expected {exp[wrong][0].item()}")


def _half_ulp_bf16(x):
    """half a bf16 ulp at magnitude x (x = mant * 2^e, mant in [0.5, 1): ulp = 2^(e - 8))"""
    _, e = torch.frexp(x)
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 9))


def _acts(case):
    return (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH) if case.ep in ACT_FORMS else (ACT_NONE,)


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_route_and_exact_result_on_integer_data(case):
    for act in _acts(case)[:2]:          # none and ReLU: the activations that keep integers
        _check_exact(case, "int", act)


_SELECT = [c for c in CASES if c.route["epilogue"] in (1, 2)]


@pytest.mark.parametrize("case", _SELECT, ids=_ids(_SELECT))
def test_bf16_epilogue_builds_on_a_selection_matrix_whose_results_bf16_holds_exactly(case):
    for act in _acts(case)[:2]:
        _check_exact(case, "select", act)


_REPEATED = {c.name for c in CASES if c.route["splits"] > 1 or c.route["kernel"] in ("pp64", "pp256", "pp256_kstrided")}


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_real_valued_data_within_the_float64_bound(case):
    odt = _dt(case.odt)
    for act in _acts(case):
        got_c, got_u, (ref_c, ref_u, _, _, bound_c, bound_u) = _run(case, "real", act,
                                                                   twice=case.name in _REPEATED and act == ACT_NONE)
        if case.route["kernel"] is None:
            continue
        for name, got, ref, bound in (("C", got_c, ref_c, bound_c), ("u_out", got_u, ref_u, bound_u)):
            if ref is None:
                continue
            if odt == torch.bfloat16:
                bound = bound + _half_ulp_bf16(ref.abs() + bound)
            err = (got.double() - ref).abs()
            assert torch.isfinite(got).all(), name
            share = torch.where(bound > 0, err / bound, (err > 0).double() * float("inf")).max().item()
            # (printed before it is asserted: the figure of the commit message)
            print(f"B4 {case.name} kernel={case.route['kernel']} act={ACT_NAMES[act]} {name} share={share:.4f}")
            assert share <= 1.0, f"{name} act={ACT_NAMES[act]}: largest error is {share:.3f} of its bound"


def test_the_record_is_cleared_by_a_refused_call_and_written_by_the_two_call_cross_backward():
    from keras_rs_amd import _lib as L
    from keras_rs_amd import dense_ops as D
    from tests.gemm_route_cases import R

    g = torch.Generator(device=DEV)
    g.manual_seed(11)
    a, bt = _signed((1032, 2112), 1, 4, g).bfloat16(), _signed((520, 2112), 1, 4, g).bfloat16()
    c, _ = D.gemm(a, bt, b_is_nk=True)
    assert D.last_gemm_route() == R("pp64", splits=4, reduce="vec8", vec=True)
    # the same split product without its workspace is refused before anything is launched: the record says "none"
    out = torch.empty_like(c)
    rc = L.lib().krs_gemm(L.ptr(a), 2112, 0, L.ptr(bt), 2112, 1, L.ptr(out), 520, 1032, 520, 2112, L.BF16, L.BF16, None, None,
                          0, L.stream_ptr())
    assert rc != 0 and D.last_gemm_route() == R(None)
    assert L.lib().krs_gemm_last_route(None) == 0          # (the pointer is optional: the kernel family is also returned)
    # krs_gemm_cross_bwd's two-call form runs krs_gemm's body (one pass over K: no split) and leaves a krs_gemm record; its
    # fused form leaves none of its own (it is not a krs_gemm), so the record still names the product before it
    r, x0, u = (_signed((1032, 520), 0, 3, g).bfloat16() for _ in range(3))
    D.gemm_cross_bwd(a, bt, r, x0, u)
    assert D.last_cross_bwd_route()[0] == "two_call"
    assert D.last_gemm_route() == R("glds", epi=2, vec=True)
    torch.cuda.synchronize()
