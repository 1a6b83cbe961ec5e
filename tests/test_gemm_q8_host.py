"""K18 (krs_gemm_q8, Dense.quantize / FeatureCross.quantize) checked without a GPU: the case table's coverage and every
route through krs_gemm_q8_plan_route, the numpy restatement (tests/gemm_q8_restatement.py) against hand-computed answers,
the derived quantization bound on seeded data, the layers' refusals and state handling with the device calls stubbed, the C
ABI's refusals (which come before any launch, so device pointers may be NULL), and the planner's invariants walked by a
stand-alone program under the sanitizers.  tests/test_gemm_q8_gpu.py holds the kernels to the restatement."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import gemm_q8_restatement as RS
from tests.gemm_q8_cases import BRANCHES, CASES, KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
F32, BF16 = 0, 1
A_BASE, W_BASE, C_BASE, STEP_BASE = 0x100000, 0x4000000, 0x8000000, 0xC000000


def _branch(case):
    """The planner branch a case must reach, worked out here from the contract (include/krs.h, K18), not from the planner."""
    lda, ldw, _ = case.lds()
    for bad, name in ((case.k % 16 != 0 or case.k == 0, "generic:k"), (lda % 16 != 0, "generic:lda"), (ldw % 16 != 0, "generic:ldw"),
                      (case.a_off % 16 != 0, "generic:a_base"), (case.w_off % 16 != 0, "generic:w_base"),
                      (case.m < 256, "tile:small_m"), (case.n < 256, "tile:small_n"), (case.k % 128 != 0, "tile:k_not_pieces"),
                      (case.k < 384, "tile:short_k"),
                      (-(-case.m // 256) * -(-case.n // 256) < 192, "tile:below_fill")):
        if bad:
            return name
    return "ring"


def test_the_case_table_names_every_kernel_and_planner_branch():
    assert {c.kernel for c in CASES} == set(KERNELS)
    assert {c.branch for c in CASES} == set(BRANCHES)
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        assert c.branch == _branch(c), c.name
        assert c.kernel == ("ring" if c.branch == "ring" else c.branch.split(":")[0].replace("tile", "tile128")), c.name
        assert c.k_tail == (c.kernel == "tile128" and c.k % 128 != 0), c.name
    # both epilogue access forms on both MFMA kernels, and a K tail that is no multiple of 32
    for kernel in ("tile128", "ring"):
        vec = {c.n % 8 == 0 and c.lds()[2] % 8 == 0 and c.c_off % 4 == 0 for c in CASES if c.kernel == kernel}
        assert vec == {True, False}, kernel
    assert any(c.kernel == "tile128" and c.k % 32 == 16 for c in CASES)
    assert any(c.k == 16 for c in CASES) and any(c.k == 1 for c in CASES) and any(c.n == 1 for c in CASES)
    assert sum(c.m == 1 for c in CASES) >= 2
    assert any(c.kernel == "ring" and c.k == 384 for c in CASES) and any(c.kernel == "ring" and c.k == 512 for c in CASES)
    # the ring's cross build needs a vector epilogue: a ring case with one, and with padded rows
    assert sum(c.kernel == "ring" and c.n % 8 == 0 and c.lds()[2] % 8 == 0 for c in CASES) >= 2


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_case_takes_the_route_it_names(case):
    from keras_rs_amd import _lib as lib
    from keras_rs_amd import dense_ops as D
    from keras_rs_amd.build import build

    build()
    lda, ldw, ldc = case.lds()
    for odt, esz in ((F32, 4), (BF16, 2)):
        rc, rt = D.plan_gemm_q8_route(A_BASE + case.a_off, lda, STEP_BASE, W_BASE + case.w_off, ldw, STEP_BASE + 0x100000,
                                      C_BASE + case.c_off * esz, ldc, case.m, case.n, case.k, odt)
        assert rc == 0
        ep_vec = case.n % 8 == 0 and ldc % 8 == 0 and (case.c_off * esz) % 16 == 0
        assert rt == dict(kernel=case.kernel, ep_vec=ep_vec, k_tail=case.k_tail, epilogue=0), (case.name, odt)
        # the ring's cross build: bf16 output, x0 without R, vector access everywhere -- and only there
        for form, cross in (("x0", True), ("x0+r", False), ("bias", False)):
            ep = lib.GemmEpilogue()
            ep.bias = STEP_BASE + 0x200000
            if "x0" in form:
                ep.x0, ep.x, ep.ldx = C_BASE + 0x10000000, C_BASE + 0x20000000, case.n
            if "r" in form:
                ep.r, ep.ldr = C_BASE + 0x30000000, case.n
            rc, rt = D.plan_gemm_q8_route(A_BASE + case.a_off, lda, STEP_BASE, W_BASE + case.w_off, ldw, STEP_BASE + 0x100000,
                                          C_BASE + case.c_off * esz, ldc, case.m, case.n, case.k, odt, ep)
            assert rc == 0 and rt["kernel"] == case.kernel
            assert rt["epilogue"] == int(cross and case.kernel == "ring" and odt == BF16 and ep_vec), (case.name, odt, form)
    # the record of the last call is untouched by a plan query
    assert D.last_gemm_q8_route()["kernel"] is None


# ---- the restatement against answers worked out by hand -------------------------------------------------------------------
def test_restatement_on_integer_data_equals_hand_computed_answers():
    # abs-max 127 in every row: step = (127 + 1e-7) / 127 rounds to 1.0f and q = x
    x = np.array([[127, 0, -1], [-127, 2, 0]], np.float32)
    w = np.array([[127, 127, -127], [1, 0, 5], [1, 0, 3]], np.float32)            # Keras layout [K, N]
    aq, astep, bad = RS.quantize(x)
    wq, wstep = RS.quantize_kernel(w)
    assert not bad.any() and (aq == x).all() and (astep == 1).all() and (wq == w.T).all() and (wstep == 1).all()
    want = np.array([[16128, 16129, -16132], [-16127, -16129, 16139]], np.int32)
    assert (RS.idot(aq, wq) == want).all()
    assert RS.product(aq, astep, wq, wstep).tolist() == want.astype(np.float32).tolist()
    # -128 counts like any other value (the quantizer never emits it; a caller may)
    assert RS.idot(np.array([[-128, -128]], np.int8), np.array([[-128, 127]], np.int8)).tolist() == [[16384 - 16256]]
    # steps that are not 1: the two multiplies in the contract's order, each rounded to fp32
    z = RS.scale(want, np.array([0.5, 7.0], np.float32), np.array([0.1, 0.25, 3.0], np.float32))
    assert z[0, 0] == np.float32(np.float32(np.float32(16128.0) * np.float32(0.1)) * np.float32(0.5))
    assert z[1, 2] == np.float32(np.float32(np.float32(16139.0) * np.float32(3.0)) * np.float32(7.0))
    # epilogue: bias, ReLU, the cross form with diag_scale, a residual -- all representable here
    bias = np.array([1.0, -2.0, 0.0], np.float32)
    x0 = np.array([[2.0, 1.0, -1.0], [0.0, 1.0, 3.0]])
    xr = np.array([[1.0, 0.0, 2.0], [4.0, -1.0, 1.0]])
    c, u = RS.epilogue(want.astype(np.float32), astep, bias=bias, act=RS.ACT_RELU, x0=x0, x=xr, diag_scale=0.5)
    assert u.tolist() == [[16129.0, 16127.0, 0.0], [0.0, 0.0, 16139.0]]
    assert c.tolist() == [[2 * 16129.5 + 1, 16127.0, -1.0 + 2.0], [4.0, -0.5 - 1.0, 3 * 16139.5 + 1]]
    c2, _ = RS.epilogue(want.astype(np.float32), astep, r=xr, beta=-2.0)
    assert c2[0].tolist() == [16126.0, 16129.0, -16136.0]
    # bf16 rounding: to nearest, ties to even
    assert RS.to_bf16(np.array([1.0, 1.00390625, 1.01171875, 16129.0], np.float32)).tolist() == [1.0, 1.0, 1.015625, 16128.0]


def test_restatement_rounds_a_dot_product_beyond_2_to_the_24():
    # K = 3456 (the widest layer of the served model): rows of -128 against rows of +-127 and one odd term
    k = 3456
    aq = np.full((2, k), -128, np.int8)
    aq[0, 7] = 1
    wq = np.full((2, k), 127, np.int8)
    wq[1, ::2] = -127
    d = RS.idot(aq, wq)
    assert d[0, 0] == -128 * 127 * (k - 1) + 127 == -56164353 and abs(int(d[0, 0])) > 2 ** 24
    assert d[1, 0] == -128 * 127 * k and d[1, 1] == 0 and d[0, 1] == 16256 + 127     # (index 7: 1 * 127 in place of -128 * 127)
    f = np.float32(d[0, 0])
    assert float(f) != float(d[0, 0]) and float(f) == -56164352.0                  # ulp 4 in [2^25, 2^26): to nearest
    z = RS.scale(d, np.array([1.0, 0.5], np.float32), np.array([1.0, 2.0], np.float32))
    assert z.tolist() == [[-56164352.0, 2.0 * 16383], [-128.0 * 127 * k / 2, 0.0]]
    # a tie: 2^25 + 2 lies half way between 2^25 and 2^25 + 4 and goes to the even significand, 2^25
    assert float(np.int32(2 ** 25 + 2).astype(np.float32)) == 2.0 ** 25 and float(np.int32(2 ** 25 + 6).astype(np.float32)) == 2.0 ** 25 + 8


def test_restatement_marks_nonfinite_rows_with_nans_and_leaves_the_neighbours():
    x = np.array([[1.0, -2.0], [np.nan, 1.0], [3.0, np.inf], [0.0, 0.0]], np.float32)
    aq, astep, bad = RS.quantize(x)
    assert bad.tolist() == [False, True, True, False] and (aq[1:3] == 0).all() and (astep[1:3] == 0).all() and astep[3] > 0
    wq, wstep = RS.quantize_kernel(np.array([[1.0, -1.0], [1.0, 2.0]], np.float32))
    z = RS.product(aq, astep, wq, wstep)
    assert np.isnan(z[1:3]).all() and np.isfinite(z[[0, 3]]).all() and (z[3] == 0).all()
    c, u = RS.epilogue(RS.scale(RS.idot(aq, wq), astep, wstep), astep, bias=np.ones(2, np.float32), act=RS.ACT_RELU,
                       x0=np.ones((4, 2)), x=np.ones((4, 2)))
    assert np.isnan(c[1:3]).all() and np.isnan(u[1:3]).all() and np.isfinite(c[[0, 3]]).all() and np.isfinite(u[[0, 3]]).all()


# ---- the quantization error bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-3, 1.0, 50.0])
@pytest.mark.parametrize("k", [1, 16, 17, 512, 3456])
def test_quantized_products_stay_inside_the_quantization_bound(k, scale):
    """|z_ij - x_i . w_j| <= 1.01 [ (astep_i |w_j|_1 + wstep_j |x_i|_1) / 2 + K astep_i wstep_j / 4 ] (derived in
    gemm_q8_restatement.quantization_bound)."""
    rng = np.random.default_rng(1000 * k + int(scale * 7))
    x = (rng.standard_normal((24, k)) * scale).astype(np.float32)
    w = (rng.standard_normal((k, 40)) / np.sqrt(k)).astype(np.float32)
    wq, wstep = RS.quantize_kernel(w)
    z, _, astep = RS.dense(x, wq, wstep)
    err = np.abs(z.astype(np.float64) - x.astype(np.float64) @ w.astype(np.float64))
    tol = RS.quantization_bound(x, w, astep, wstep)
    assert (tol > 0).all()
    ratio = float((err / tol).max())
    print(f"k={k} scale={scale}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0


# ---- the layers' refusals and state handling, the device calls stubbed ----------------------------------------------------
def _fake_quantize_rows_checked(table, what):
    """quantize_rows_checked on the host: the numpy restatement in place of krs_quantize_rows_q8."""
    import torch

    q, step, bad = RS.quantize(table.detach().float().numpy())
    if bad.any():
        raise ValueError(f"{what}: a table row holds a NaN or an infinity; it cannot be quantized.")
    return torch.from_numpy(q), torch.from_numpy(step)


def _no_device(*a, **k):
    raise AssertionError("quantize() reached the device before refusing")


def test_dense_quantize_refusals_and_state(monkeypatch):
    import torch

    import keras_rs_amd.layers as kl
    from keras_rs_amd.layers import dense as dense_layers

    def built(units=6, d=10, **kw):
        layer = kl.Dense(units, device="cpu", **kw)
        layer.build((None, d))
        return layer

    monkeypatch.setattr(dense_layers, "quantize_rows_checked", _no_device)
    with pytest.raises(ValueError, match="int8"):
        built().quantize("int4")
    with pytest.raises(RuntimeError, match="not built"):
        kl.Dense(4, device="cpu").quantize("int8")
    with pytest.raises(AssertionError, match="reached the device"):      # (and an accepted request does go there)
        built().quantize("int8")
    monkeypatch.setattr(dense_layers, "quantize_rows_checked", _fake_quantize_rows_checked)
    layer = built(activation="relu")
    config, kernel = layer.get_config(), layer.kernel.detach().clone()
    assert [tuple(w.shape) for w in layer.weights] == [(10, 6), (6,)] and set(layer.state_dict()) == {"kernel", "bias"}
    # a kernel with a NaN raises and leaves the layer as it was
    with torch.no_grad():
        layer.kernel[3, 2] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        layer.quantize("int8")
    assert layer.quantization_mode is None and layer.kernel is not None and set(layer.state_dict()) == {"kernel", "bias"}
    with torch.no_grad():
        layer.kernel.copy_(kernel)
    layer.quantize("int8")
    assert layer.quantization_mode == "int8" and layer.kernel is None
    assert [tuple(w.shape) for w in layer.weights] == [(6,)] and layer.weights[0] is layer.bias
    assert layer.bias.dtype == torch.float32 and isinstance(layer.bias, torch.nn.Parameter)
    sd = layer.state_dict()
    assert set(sd) == {"bias", "kernel_q", "kernel_step"}
    assert sd["kernel_q"].dtype == torch.int8 and tuple(sd["kernel_q"].shape) == (6, 10)
    assert sd["kernel_step"].dtype == torch.float32 and tuple(sd["kernel_step"].shape) == (6,)
    wq, wstep = RS.quantize_kernel(kernel.numpy())
    assert (sd["kernel_q"].numpy() == wq).all() and (sd["kernel_step"].numpy() == wstep).all()
    assert layer.get_config() == config
    with pytest.raises(RuntimeError, match="already quantized"):
        layer.quantize("int8")
    # the state loads into a second layer quantized the same way, and only there
    other = built(activation="relu")
    with pytest.raises(RuntimeError):
        other.load_state_dict(sd)
    other.quantize("int8")
    other.load_state_dict(sd)
    assert torch.equal(other.kernel_q, layer.kernel_q) and torch.equal(other.kernel_step, layer.kernel_step)
    # a dtype cast keeps the steps fp32 with their values
    steps = layer.kernel_step.clone()
    layer.bfloat16()
    assert layer.kernel_step.dtype == torch.float32 and torch.equal(layer.kernel_step, steps)
    assert layer.kernel_q.dtype == torch.int8
    # a layer without a bias has no weights left
    nobias = built(use_bias=False)
    nobias.quantize()
    assert nobias.weights == [] and set(nobias.state_dict()) == {"kernel_q", "kernel_step"}
    # an unquantized layer is what it was
    plain = built()
    assert plain.quantization_mode is None and set(plain.state_dict()) == {"kernel", "bias"}


def test_feature_cross_quantize_refusals_and_state(monkeypatch):
    import torch

    import keras_rs_amd.layers as kl
    from keras_rs_amd.layers import dense as dense_layers

    def built(d=12, **kw):
        layer = kl.FeatureCross(device="cpu", **kw)
        layer.build((None, d))
        return layer

    monkeypatch.setattr(dense_layers, "quantize_rows_checked", _no_device)
    with pytest.raises(ValueError, match="int8"):
        built().quantize("fp8")
    with pytest.raises(RuntimeError, match="not built"):
        kl.FeatureCross(device="cpu").quantize("int8")
    monkeypatch.setattr(dense_layers, "quantize_rows_checked", _fake_quantize_rows_checked)
    low = built(projection_dim=4, kernel_regularizer="l2", bias_regularizer="l2")
    config = low.get_config()
    down, kernel = low.down_kernel.detach().clone(), low.kernel.detach().clone()
    assert len(low.losses) == 3
    # an infinity in the SECOND kernel: nothing is touched, the first kernel included
    with torch.no_grad():
        low.kernel[1, 1] = float("inf")
    with pytest.raises(ValueError, match="infinity"):
        low.quantize("int8")
    assert low.quantization_mode is None and low.down_kernel is not None and low.kernel is not None
    assert set(low.state_dict()) == {"down_kernel", "kernel", "bias"}
    with torch.no_grad():
        low.kernel.copy_(kernel)
    low.quantize("int8")
    assert low.down_kernel is None and low.kernel is None and [w is low.bias for w in low.weights] == [True]
    assert len(low.losses) == 1                                           # the bias penalty stays
    sd = low.state_dict()
    assert set(sd) == {"bias", "down_kernel_q", "down_kernel_step", "kernel_q", "kernel_step"}
    assert tuple(sd["down_kernel_q"].shape) == (4, 12) and tuple(sd["kernel_q"].shape) == (12, 4)
    dq, dstep = RS.quantize_kernel(down.numpy())
    kq, kstep = RS.quantize_kernel(kernel.numpy())
    assert (sd["down_kernel_q"].numpy() == dq).all() and (sd["down_kernel_step"].numpy() == dstep).all()
    assert (sd["kernel_q"].numpy() == kq).all() and (sd["kernel_step"].numpy() == kstep).all()
    assert low.get_config() == config
    with pytest.raises(RuntimeError, match="already quantized"):
        low.quantize()
    other = built(projection_dim=4)
    other.quantize()
    other.load_state_dict(sd)
    assert torch.equal(other.kernel_q, low.kernel_q) and torch.equal(other.down_kernel_step, low.down_kernel_step)
    low.bfloat16()
    assert low.kernel_step.dtype == low.down_kernel_step.dtype == torch.float32
    full = built()
    full.quantize()
    assert set(full.state_dict()) == {"bias", "kernel_q", "kernel_step"} and tuple(full.kernel_q.shape) == (12, 12)


def test_gemm_q8_wrapper_refuses_host_tensors_and_misfit_shapes():
    import torch

    from keras_rs_amd import _lib as lib
    from keras_rs_amd import dense_ops as D

    with pytest.raises(lib.KrsError, match="no CPU fallback"):
        D.gemm_q8(torch.zeros((2, 16)), torch.zeros((4, 16), dtype=torch.int8), torch.ones(4))
    with pytest.raises(lib.KrsError, match="no CPU fallback"):
        D.gemm_q8_prequantized(torch.zeros((2, 16), dtype=torch.int8), torch.ones(2), torch.zeros((4, 16), dtype=torch.int8),
                               torch.ones(4))


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------
def test_abi_refusals_without_a_device():
    from keras_rs_amd import _lib as lib
    from keras_rs_amd import dense_ops as D
    from keras_rs_amd.build import build

    build()
    fn = lib.lib().krs_gemm_q8
    fake = 0x100000
    #       aq    lda  astep wq    ldw  wstep c     ldc m   n   k    odt      ep    stream
    call = [fake, 128, fake, fake, 128, fake, fake, 64, 32, 64, 128, lib.F32, None, None]
    AQ, LDA, ASTEP, WQ, LDW, WSTEP, CC, LDC, M, N, K, ODT, EP = range(13)
    ep_x0_only = lib.GemmEpilogue()
    ep_x0_only.x0 = fake
    import ctypes

    for what, changes, status, names in (
            ("negative m", {M: -1}, INVALID, "negative"),
            ("negative n", {N: -1}, INVALID, "negative"),
            ("negative k", {K: -1}, INVALID, "negative"),
            ("lda below k", {LDA: 127}, INVALID, "stride"),
            ("ldw below k", {LDW: 127}, INVALID, "stride"),
            ("ldc below n", {LDC: 63}, INVALID, "stride"),
            ("bad output dtype", {ODT: lib.I8}, INVALID, "out_dtype"),
            ("k above 131072", {K: 131073, LDA: 131073, LDW: 131073}, UNSUPPORTED, "131072"),
            ("k above 131072, checked before the null operands", {K: 1 << 20, LDA: 1 << 20, LDW: 1 << 20, AQ: None}, UNSUPPORTED, "131072"),
            ("m above 2^31 - 1", {M: 2 ** 31}, UNSUPPORTED, "2^31"),
            ("a grid beyond the launch limits", {M: 2 ** 31 - 1, N: 2 ** 31 - 1, LDC: 2 ** 31 - 1, K: 1, LDA: 1, LDW: 1}, UNSUPPORTED, "grid"),
            ("null aq", {AQ: None}, INVALID, "null"),
            ("null astep", {ASTEP: None}, INVALID, "null"),
            ("null wq", {WQ: None}, INVALID, "null"),
            ("null wstep", {WSTEP: None}, INVALID, "null"),
            ("null c", {CC: None}, INVALID, "null"),
            ("x0 without x", {EP: ctypes.byref(ep_x0_only)}, INVALID, "x with x0")):
        args = list(call)
        for pos, value in changes.items():
            args[pos] = value
        assert fn(*args) == status, what
        message = lib.lib().krs_last_error().decode()
        assert message.startswith("krs_gemm_q8"), what
        assert names in message, (what, message)
        assert D.last_gemm_q8_route() == dict(kernel=None, ep_vec=False, k_tail=False, epilogue=0), what
        rt = lib.GemmQ8Route()
        assert lib.lib().krs_gemm_q8_plan_route(*args[:13], ctypes.byref(rt)) == status, what
        assert (rt.kernel, rt.ep_vec, rt.k_tail, rt.epilogue) == (0, 0, 0, 0), what
    # an empty product is a successful no-op that reads nothing, NULL operands included
    for pos in (M, N):
        args = [None if i in (AQ, ASTEP, WQ, WSTEP, CC) else v for i, v in enumerate(call)]
        args[pos] = 0
        assert fn(*args) == 0
        assert D.last_gemm_q8_route()["kernel"] is None
    # k = 131072 itself is accepted by the planner
    rc, rt = D.plan_gemm_q8_route(fake, 131072, fake, fake, 131072, fake, fake, 64, 32, 64, 131072, lib.F32)
    assert rc == 0 and rt["kernel"] == "tile128"


def test_the_planner_header_compiles_without_hip_and_keeps_its_invariants_under_the_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gemm_q8_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "gemm_q8_plan_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "0 failed checks" in run.stdout
