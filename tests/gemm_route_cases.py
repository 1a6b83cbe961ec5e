"""The case table of tests/test_gemm_routes_gpu.py (krs_gemm on every route) and of its coverage check,
tests/test_gemm_routes_host.py.  No torch, no GPU: plain data.

A case fixes one krs_gemm call: operand layout, dtypes, sizes, the padding of every leading dimension, an element
offset of every base pointer, the epilogue form, the pipeline option, whether a workspace is passed -- and the route
record krs_gemm_last_route must report for it.  The expected routes are asserted on the host against the planner
(keras_rs_amd/csrc/gemm_plan.h, tests/test_gemm_routes_host.py) and on the device against what ran, so a dispatch change
shows up as a failing case, not as lost coverage.
"""

from collections import namedtuple

Case = namedtuple("Case", "name layout idt odt m n k ep route pad off pipe ws diag beta")

# epilogue forms -> the operands the krs_gemm_epilogue carries ("null": a NULL epilogue pointer; "plain": an empty struct)
FORMS = {
    "null": (), "plain": (), "bias": ("bias",), "cross": ("bias", "x0"), "cross_u": ("bias", "x0", "u"),
    "res": ("r",), "bias_res": ("bias", "r"), "cross_res": ("bias", "x0", "u", "r"),
}
# (a bias comes with an activation: these forms run once per activation)
ACT_FORMS = ("bias", "cross", "cross_u", "bias_res", "cross_res")


def R(kernel, splits=1, reduce=None, epi=0, vec=False, width=0, thin_is_a=False):
    """An expected route record, in the form dense_ops.last_gemm_route() returns."""
    if kernel is None:
        return dict(kernel=None, splits=0, reduce=None, epilogue=0, ep_vec=False, thin_width=0, thin_is_a=False)
    return dict(kernel=kernel, splits=splits, reduce=reduce, epilogue=epi, ep_vec=vec, thin_width=width,
                thin_is_a=thin_is_a)


def case(name, layout, idt, odt, m, n, k, ep, route, pad=None, off=None, pipe=4, ws=True, diag=0.5, beta=-2.0):
    """pad: extra elements on the leading dimension of a, b, c, x (x0 and x share ldx), u, r; off: element offset of the
    base pointer of a, b, c, bias, x0, x, u, r inside its allocation; diag / beta: diag_scale and beta of the epilogue."""
    assert ep in FORMS and layout in ("nn", "nt", "tn") and idt in ("bf16", "f32") and odt in ("bf16", "f32")
    return Case(name, layout, idt, odt, m, n, k, ep, route, dict(pad or {}), dict(off or {}), pipe, ws, diag, beta)


def leading_dims(c):
    """(lda, ldb, ldc, ldx, ldu, ldr) of a case."""
    p = c.pad
    lda = (c.m if c.layout == "tn" else c.k) + p.get("a", 0)
    ldb = (c.k if c.layout == "nt" else c.n) + p.get("b", 0)
    return lda, ldb, c.n + p.get("c", 0), c.n + p.get("x", 0), c.n + p.get("u", 0), c.n + p.get("r", 0)


def split_geometry(c):
    """(k per split, k of the last split) of a split case, by krs_gemm's rule: ceil(k / splits), rounded up to whole tile
    rows of 128 bytes on the tile kernels."""
    s = c.route["splits"]
    kps = -(-c.k // s)
    if c.route["kernel"] != "thin":
        bk = 64 if c.idt == "bf16" else 32
        kps = -(-kps // bk) * bk
    return kps, c.k - (s - 1) * kps


P8 = dict(a=8, b=16, c=8, x=16, u=8, r=24)       # padded leading dimensions that keep every row on 16 bytes
P3 = dict(a=3, b=5, c=1, x=5, u=2, r=7)          # odd ones, for the scalar paths (ldu < ldx)

CASES = [
    # gemm_mfma_kernel: three layouts, two dtypes, epilogue builds 0 / 1 / 2, vector and scalar stores, split-K by the
    # three reduce kernels, and the smallest MFMA-eligible shapes
    case("mfma-nn-bf16-bias", "nn", "bf16", "bf16", 130, 200, 72, "bias", R("mfma", vec=True), pad=P8),
    case("mfma-nn-bf16-bias-f32out", "nn", "bf16", "f32", 130, 200, 72, "bias", R("mfma", vec=True), pad=P8),
    case("mfma-nt-bf16-k288-cross", "nt", "bf16", "bf16", 520, 264, 288, "cross_u", R("mfma", epi=1, vec=True), pad=P8),
    case("mfma-nt-bf16-k288-cross-f32out", "nt", "bf16", "f32", 520, 264, 288, "cross_u", R("mfma", vec=True), pad=P8),
    case("mfma-nt-bf16-res", "nt", "bf16", "bf16", 300, 136, 200, "res", R("mfma", epi=2, vec=True), pad=P8, beta=0.5),
    case("mfma-nt-bf16-res-f32out", "nt", "bf16", "f32", 300, 136, 200, "res", R("mfma", vec=True), pad=P8, beta=0.5),
    case("mfma-nt-bf16-ragged-n", "nt", "bf16", "bf16", 300, 203, 136, "cross_res", R("mfma"), pad=dict(a=8, b=8,
         c=3, x=5, u=2, r=1)),
    case("mfma-nt-bf16-ragged-n-f32out", "nt", "bf16", "f32", 300, 203, 136, "cross_res", R("mfma"), pad=dict(a=8,
         b=8, c=3, x=5, u=2, r=1)),
    case("mfma-nn-bf16-c-off", "nn", "bf16", "bf16", 130, 200, 72, "bias_res", R("mfma"), off=dict(c=1, r=3), beta=2.0),
    case("mfma-nn-bf16-c-off-f32out", "nn", "bf16", "f32", 130, 200, 72, "bias_res", R("mfma"), off=dict(c=1, r=3),
         beta=2.0),
    case("mfma-tn-bf16-k200", "tn", "bf16", "bf16", 136, 264, 200, "cross", R("mfma", epi=1, vec=True), pad=P8,
         diag=2.0),
    case("mfma-tn-bf16-k200-f32out", "tn", "bf16", "f32", 136, 264, 200, "cross", R("mfma", vec=True), pad=P8,
         diag=2.0),
    case("mfma-tn-bf16-split17", "tn", "bf16", "bf16", 16, 16, 9000, "bias", R("mfma", splits=17, reduce="vec8",
         vec=True)),
    case("mfma-tn-bf16-split17-f32out", "tn", "bf16", "f32", 16, 16, 9000, "bias", R("mfma", splits=17,
         reduce="vec8", vec=True)),
    case("mfma-nn-bf16-split-null", "nn", "bf16", "f32", 130, 200, 4104, "null", R("mfma", splits=4, reduce="vec4",
         vec=True)),
    case("mfma-nn-f32-bias", "nn", "f32", "f32", 130, 200, 72, "bias", R("mfma", vec=True), pad=P8),
    case("mfma-nt-f32-cross", "nt", "f32", "f32", 257, 131, 100, "cross_u", R("mfma"), pad=dict(a=4, b=8, c=5, x=3,
         u=2, r=0)),
    case("mfma-tn-f32-res", "tn", "f32", "f32", 132, 264, 1000, "res", R("mfma", vec=True), pad=P8, beta=1.0),
    case("mfma-tn-f32-split-vec4", "tn", "f32", "f32", 256, 388, 4100, "null", R("mfma", splits=4, reduce="vec4"),
         pad=dict(a=4, b=4, c=4)),
    case("mfma-tn-f32-split-vec8", "tn", "f32", "f32", 256, 384, 4100, "cross_res", R("mfma", splits=4,
         reduce="vec8", vec=True), pad=P8, diag=-2.0, beta=0.5),
    case("mfma-nt-f32-split-scalar", "nt", "f32", "f32", 130, 203, 4100, "bias_res", R("mfma", splits=4,
         reduce="scalar"), pad=dict(a=4, b=4, c=1, r=3)),
    case("mfma-nt-f32-null", "nt", "f32", "f32", 100, 52, 36, "null", R("mfma")),
    # the general split rule asks for 6 slabs where the ring rule (bf16 only) would ask for 5: the query sizes the larger
    case("mfma-nt-f32-split6-query-ws", "nt", "f32", "f32", 2056, 1032, 6144, "null", R("mfma", splits=6,
         reduce="vec4", vec=True)),
    case("mfma-nn-f32-4x4x4", "nn", "f32", "f32", 4, 4, 4, "bias", R("mfma")),
    case("mfma-nt-bf16-8x8x8", "nt", "bf16", "bf16", 8, 8, 8, "bias", R("mfma", vec=True)),
    case("mfma-nt-bf16-8x8x8-f32out", "nt", "bf16", "f32", 8, 8, 8, "bias", R("mfma", vec=True)),
    case("mfma-tn-bf16-8x8x8", "tn", "bf16", "bf16", 8, 8, 8, "bias_res", R("mfma", vec=True)),
    case("mfma-tn-bf16-8x8x8-f32out", "tn", "bf16", "f32", 8, 8, 8, "bias_res", R("mfma", vec=True)),
    # gemm_glds_kernel: K-contiguous operands, K >= 1024 in whole tile rows, too few 256 x 256 tiles for the ring
    case("glds-bf16-bias", "nt", "bf16", "bf16", 300, 136, 1024, "bias", R("glds", vec=True), pad=P8),
    case("glds-bf16-bias-f32out", "nt", "bf16", "f32", 300, 136, 1024, "bias", R("glds", vec=True), pad=P8),
    case("glds-bf16-cross", "nt", "bf16", "bf16", 130, 264, 1088, "cross_u", R("glds", epi=1, vec=True), pad=P8,
         diag=1.0),
    case("glds-bf16-cross-f32out", "nt", "bf16", "f32", 130, 264, 1088, "cross_u", R("glds", vec=True), pad=P8,
         diag=1.0),
    case("glds-bf16-res", "nt", "bf16", "bf16", 300, 136, 1152, "res", R("glds", epi=2, vec=True), pad=P8, beta=2.0),
    case("glds-bf16-res-f32out", "nt", "bf16", "f32", 300, 136, 1152, "res", R("glds", vec=True), pad=P8, beta=2.0),
    case("glds-bf16-ragged-n", "nt", "bf16", "bf16", 300, 203, 1024, "cross_res", R("glds"), pad=dict(a=8, b=8, c=3,
         x=5, u=2, r=1)),
    case("glds-bf16-ragged-n-f32out", "nt", "bf16", "f32", 300, 203, 1024, "cross_res", R("glds"), pad=dict(a=8, b=8,
         c=3, x=5, u=2, r=1)),
    case("glds-f32-bias", "nt", "f32", "f32", 130, 72, 1024, "bias_res", R("glds", vec=True), pad=P8, beta=0.0),
    case("glds-f32-x-off", "nt", "f32", "f32", 260, 136, 1056, "cross_u", R("glds"), pad=dict(x=3, u=2),
         off=dict(x=1, x0=1), diag=0.0),
    # the unsplit rings (192 or more 256 x 256 tiles): gemm_pp64_kernel by default, gemm_pp256_kernel under pipeline 5, the
    # 128 x 128 kernels under pipeline 0
    case("pp64-k256-bias", "nt", "bf16", "bf16", 12288, 4096, 256, "bias", R("pp64", vec=True)),
    case("pp64-k256-bias-f32out", "nt", "bf16", "f32", 12288, 4096, 256, "bias", R("pp64", vec=True)),
    case("pp64-k448-cross-ragged", "nt", "bf16", "bf16", 12296, 4104, 448, "cross_u", R("pp64", epi=1, vec=True),
         pad=P8),
    case("pp64-k448-cross-ragged-f32out", "nt", "bf16", "f32", 12296, 4104, 448, "cross_u", R("pp64", vec=True),
         pad=P8),
    case("pp64-k320-res-ragged", "nt", "bf16", "bf16", 12296, 4104, 320, "res", R("pp64", epi=2, vec=True), pad=P8,
         beta=0.5),
    case("pp64-k320-res-ragged-f32out", "nt", "bf16", "f32", 12296, 4104, 320, "res", R("pp64", vec=True), pad=P8,
         beta=0.5),
    case("pp64-k256-ragged-n", "nt", "bf16", "bf16", 12290, 4099, 256, "cross_res", R("pp64"), pad=dict(a=8, b=8,
         c=1, x=5, u=2, r=3)),
    case("pp64-k256-ragged-n-f32out", "nt", "bf16", "f32", 12290, 4099, 256, "cross_res", R("pp64"), pad=dict(a=8,
         b=8, c=1, x=5, u=2, r=3)),
    case("pp256-k320-pipe5-bias", "nt", "bf16", "bf16", 12288, 4096, 320, "bias_res", R("pp256", vec=True), pipe=5,
         beta=1.0),
    case("pp256-k320-pipe5-bias-f32out", "nt", "bf16", "f32", 12288, 4096, 320, "bias_res", R("pp256", vec=True),
         pipe=5, beta=1.0),
    case("pp256-k256-pipe5-cross-ragged", "nt", "bf16", "bf16", 12296, 4104, 256, "cross_u", R("pp256", epi=1,
         vec=True), pad=P8, pipe=5, diag=-2.0),
    case("pp256-k256-pipe5-cross-ragged-f32out", "nt", "bf16", "f32", 12296, 4104, 256, "cross_u", R("pp256",
         vec=True), pad=P8, pipe=5, diag=-2.0),
    case("pp256-k448-pipe5-res-ragged", "nt", "bf16", "bf16", 12296, 4104, 448, "res", R("pp256", epi=2, vec=True),
         pad=P8, pipe=5),
    case("pp256-k448-pipe5-res-ragged-f32out", "nt", "bf16", "f32", 12296, 4104, 448, "res", R("pp256", vec=True),
         pad=P8, pipe=5),
    case("pp256-k256-pipe5-ragged-n", "nt", "bf16", "bf16", 12290, 4099, 256, "cross_res", R("pp256"), pad=dict(a=8,
         b=8, c=1, x=5, u=2, r=3), pipe=5),
    case("pp256-k256-pipe5-ragged-n-f32out", "nt", "bf16", "f32", 12290, 4099, 256, "cross_res", R("pp256"),
         pad=dict(a=8, b=8, c=1, x=5, u=2, r=3), pipe=5),
    case("ring-shape-pipe0-k256", "nt", "bf16", "bf16", 12296, 4104, 256, "cross_u", R("mfma", epi=1, vec=True),
         pad=P8, pipe=0),
    case("ring-shape-pipe0-k256-f32out", "nt", "bf16", "f32", 12296, 4104, 256, "cross_u", R("mfma", vec=True),
         pad=P8, pipe=0),
    case("ring-shape-pipe0-k1024", "nt", "bf16", "bf16", 12296, 4104, 1024, "res", R("glds", epi=2, vec=True),
         pad=P8, pipe=0),
    # the split ring (fewer than 192 tiles, K >= 2048): K = 32 mod 64 on gemm_pp256_kernel, whole 64-k blocks on
    # gemm_pp64_kernel; the last split is the short one
    case("ring-split-32k-vec8", "nt", "bf16", "bf16", 1032, 520, 2080, "cross_res", R("pp256", splits=4,
         reduce="vec8", vec=True), pad=P8),
    case("ring-split-32k-vec8-f32out", "nt", "bf16", "f32", 1032, 520, 2080, "cross_res", R("pp256", splits=4,
         reduce="vec8", vec=True), pad=P8),
    case("ring-split-64k-vec8", "nt", "bf16", "bf16", 1032, 520, 2112, "bias", R("pp64", splits=4, reduce="vec8",
         vec=True), pad=P8),
    case("ring-split-64k-vec8-f32out", "nt", "bf16", "f32", 1032, 520, 2112, "bias", R("pp64", splits=4,
         reduce="vec8", vec=True), pad=P8),
    case("ring-split-32k-scalar", "nt", "bf16", "bf16", 520, 523, 2080, "bias_res", R("pp256", splits=4,
         reduce="scalar"), pad=dict(a=8, b=8, c=3, r=1), beta=0.5),
    case("ring-split-32k-scalar-f32out", "nt", "bf16", "f32", 520, 523, 2080, "bias_res", R("pp256", splits=4,
         reduce="scalar"), pad=dict(a=8, b=8, c=3, r=1), beta=0.5),
    case("ring-split-64k-scalar", "nt", "bf16", "bf16", 520, 520, 2112, "cross_u", R("pp64", splits=4,
         reduce="scalar"), pad=dict(x=8), off=dict(c=1)),
    case("ring-split-64k-scalar-f32out", "nt", "bf16", "f32", 520, 520, 2112, "cross_u", R("pp64", splits=4,
         reduce="scalar"), pad=dict(x=8), off=dict(c=1)),
    case("ring-split-32k-vec4", "nt", "bf16", "f32", 1032, 516, 2080, "null", R("pp256", splits=4, reduce="vec4"),
         pad=dict(a=8, b=8, c=4)),
    case("ring-split-64k-vec4", "nt", "bf16", "f32", 520, 1028, 2112, "null", R("pp64", splits=4, reduce="vec4")),
    case("ring-split-pipe5", "nt", "bf16", "bf16", 1032, 520, 2112, "bias", R("pp256", splits=4, reduce="vec8",
         vec=True), pipe=5),
    case("ring-split-pipe0", "nt", "bf16", "bf16", 1032, 520, 2112, "bias", R("mfma", splits=4, reduce="vec8",
         vec=True), pipe=0),
    # bf16 weight gradients: gemm_tn_glds_kernel and the K-strided build of gemm_pp256_kernel
    case("tn-glds-unsplit", "tn", "bf16", "bf16", 136, 72, 512, "bias", R("tn_glds", vec=True), pad=P8),
    case("tn-glds-unsplit-f32out", "tn", "bf16", "f32", 136, 72, 512, "bias", R("tn_glds", vec=True), pad=P8),
    case("tn-glds-split-vec4", "tn", "bf16", "f32", 136, 264, 4288, "null", R("tn_glds", splits=4, reduce="vec4"),
         pad=dict(a=8, b=8, c=4)),
    case("tn-glds-split-vec8", "tn", "bf16", "bf16", 136, 264, 4288, "cross_res", R("tn_glds", splits=4,
         reduce="vec8", vec=True), pad=P8),
    case("tn-glds-split-vec8-f32out", "tn", "bf16", "f32", 136, 264, 4288, "cross_res", R("tn_glds", splits=4,
         reduce="vec8", vec=True), pad=P8),
    case("tn-glds-split-scalar", "tn", "bf16", "bf16", 136, 264, 4288, "bias_res", R("tn_glds", splits=4,
         reduce="scalar"), off=dict(c=1)),
    case("tn-glds-split-scalar-f32out", "tn", "bf16", "f32", 136, 264, 4288, "bias_res", R("tn_glds", splits=4,
         reduce="scalar"), off=dict(c=1)),
    case("pp256k-unsplit", "tn", "bf16", "bf16", 264, 520, 512, "cross_u", R("pp256_kstrided", vec=True), pad=P8),
    case("pp256k-unsplit-f32out", "tn", "bf16", "f32", 264, 520, 512, "cross_u", R("pp256_kstrided", vec=True), pad=P8),
    case("pp256k-split-vec4", "tn", "bf16", "f32", 264, 520, 4352, "null", R("pp256_kstrided", splits=8,
         reduce="vec4"), pad=dict(a=8, b=8, c=4)),
    case("pp256k-split-vec8", "tn", "bf16", "bf16", 264, 520, 4352, "bias_res", R("pp256_kstrided", splits=8,
         reduce="vec8", vec=True), pad=P8, beta=2.0),
    case("pp256k-split-vec8-f32out", "tn", "bf16", "f32", 264, 520, 4352, "bias_res", R("pp256_kstrided", splits=8,
         reduce="vec8", vec=True), pad=P8, beta=2.0),
    case("pp256k-split-scalar", "tn", "bf16", "bf16", 264, 520, 4352, "cross_u", R("pp256_kstrided", splits=8,
         reduce="scalar"), pad=dict(c=3, x=5, u=2)),
    case("pp256k-split-scalar-f32out", "tn", "bf16", "f32", 264, 520, 4352, "cross_u", R("pp256_kstrided", splits=8,
         reduce="scalar"), pad=dict(c=3, x=5, u=2)),
    case("pp256k-pipe0-tn-glds", "tn", "bf16", "bf16", 264, 520, 512, "bias", R("tn_glds", vec=True), pipe=0),
    # 9 splits of 576 would leave the last one 64 k, half a ring: the planner skips that count (8 x 640, the last 192)
    case("pp256k-split-short-last", "tn", "bf16", "bf16", 256, 256, 4672, "bias", R("pp256_kstrided", splits=8,
         reduce="vec8", vec=True)),
    # gemm_thin_kernel: widths 1 / 4 / 8 / 16, either operand thin, split and (no workspace passed) unsplit
    case("thin-w1-a-split-bf16", "tn", "bf16", "bf16", 1, 520, 4100, "bias", R("thin", splits=8, reduce="scalar",
         width=1, thin_is_a=True), pad=P3),
    case("thin-w1-a-nows-bf16", "tn", "bf16", "bf16", 1, 300, 1030, "bias", R("thin", width=1, thin_is_a=True),
         pad=P3, ws=False),
    case("thin-w1-b-split-f32", "tn", "f32", "f32", 264, 1, 4100, "bias", R("thin", splits=8, reduce="scalar",
         width=1, thin_is_a=False), pad=P3),
    case("thin-w1-b-nows-f32", "tn", "f32", "f32", 300, 1, 1030, "bias", R("thin", width=1, thin_is_a=False), pad=P3,
         ws=False),
    case("thin-w4-a-split-f32", "tn", "f32", "f32", 3, 520, 4100, "cross_u", R("thin", splits=8, reduce="scalar",
         width=4, thin_is_a=True), pad=P3),
    case("thin-w4-a-nows-f32", "tn", "f32", "f32", 3, 300, 1030, "plain", R("thin", width=4, thin_is_a=True), pad=P3,
         ws=False),
    case("thin-w4-b-split-bf16", "tn", "bf16", "bf16", 264, 3, 4100, "cross_u", R("thin", splits=8, reduce="scalar",
         width=4, thin_is_a=False), pad=P3),
    case("thin-w4-b-nows-bf16", "tn", "bf16", "bf16", 300, 3, 1030, "plain", R("thin", width=4, thin_is_a=False),
         pad=P3, ws=False),
    case("thin-w8-a-split-bf16", "tn", "bf16", "bf16", 7, 520, 4100, "bias_res", R("thin", splits=8, reduce="scalar",
         width=8, thin_is_a=True), pad=P3),
    case("thin-w8-a-nows-bf16", "tn", "bf16", "bf16", 7, 300, 1030, "bias", R("thin", width=8, thin_is_a=True),
         pad=P3, ws=False),
    case("thin-w8-b-split-f32", "tn", "f32", "f32", 264, 7, 4100, "bias_res", R("thin", splits=8, reduce="scalar",
         width=8, thin_is_a=False), pad=P3),
    case("thin-w8-b-nows-f32", "tn", "f32", "f32", 300, 7, 1030, "bias", R("thin", width=8, thin_is_a=False), pad=P3,
         ws=False),
    case("thin-w16-a-split-f32", "tn", "f32", "f32", 13, 520, 4100, "cross_res", R("thin", splits=8, reduce="scalar",
         width=16, thin_is_a=True), pad=P3),
    case("thin-w16-a-nows-f32", "tn", "f32", "f32", 13, 300, 1030, "bias", R("thin", width=16, thin_is_a=True),
         pad=P3, ws=False),
    case("thin-w16-b-split-bf16", "tn", "bf16", "bf16", 264, 13, 4100, "cross_res", R("thin", splits=8,
         reduce="scalar", width=16, thin_is_a=False), pad=P3),
    case("thin-w16-b-split-bf16-f32out", "tn", "bf16", "f32", 264, 13, 4100, "cross_res", R("thin", splits=8,
         reduce="scalar", width=16, thin_is_a=False), pad=P3),
    case("thin-w16-b-nows-bf16", "tn", "bf16", "bf16", 300, 13, 1030, "bias", R("thin", width=16, thin_is_a=False),
         pad=P3, ws=False),
    case("thin-w16-a-off-bf16", "tn", "bf16", "bf16", 16, 520, 2048, "null", R("thin", splits=4, reduce="scalar",
         vec=True, width=16, thin_is_a=True), off=dict(a=1)),
    case("thin-w16-a-off-bf16-f32out", "tn", "bf16", "f32", 16, 520, 2048, "null", R("thin", splits=4,
         reduce="scalar", vec=True, width=16, thin_is_a=True), off=dict(a=1)),
    case("thin-w8-b-off-f32", "tn", "f32", "f32", 300, 8, 1500, "res", R("thin", splits=2, reduce="scalar", vec=True,
         width=8, thin_is_a=False), off=dict(b=1), beta=0.5),
    # gemm_rowdot_kernel (N <= 8) and gemm_smallk_kernel (K <= 16): shapes the planner's tile_eligible refuses
    case("rowdot-nn-bf16-n1", "nn", "bf16", "bf16", 2048, 1, 256, "bias", R("rowdot"), pad=P3),
    case("rowdot-nn-bf16-n1-f32out", "nn", "bf16", "f32", 2048, 1, 256, "bias", R("rowdot"), pad=P3),
    case("rowdot-nt-bf16-k77", "nt", "bf16", "bf16", 1500, 3, 77, "cross_u", R("rowdot"), pad=P3),
    case("rowdot-nt-bf16-k77-f32out", "nt", "bf16", "f32", 1500, 3, 77, "cross_u", R("rowdot"), pad=P3),
    case("rowdot-nt-f32-k77", "nt", "f32", "f32", 1500, 3, 77, "cross_res", R("rowdot"), pad=P3),
    case("rowdot-nn-f32-n5", "nn", "f32", "f32", 1100, 5, 43, "bias_res", R("rowdot"), pad=P3),
    case("rowdot-nt-bf16-a-off", "nt", "bf16", "bf16", 1100, 8, 40, "bias", R("rowdot", vec=True), pad=dict(a=8, b=8,
         c=8), off=dict(a=1)),
    case("rowdot-nt-bf16-a-off-f32out", "nt", "bf16", "f32", 1100, 8, 40, "bias", R("rowdot", vec=True),
         pad=dict(a=8, b=8, c=8), off=dict(a=1)),
    case("rowdot-nt-f32-a-off", "nt", "f32", "f32", 1030, 8, 42, "res", R("rowdot", vec=True), pad=dict(a=2, r=8,
         c=8), off=dict(a=1)),
    case("smallk-nt-bf16-k1", "nt", "bf16", "bf16", 2048, 256, 1, "bias", R("smallk", vec=True), pad=dict(a=3, b=1,
         c=8)),
    case("smallk-nt-bf16-k1-f32out", "nt", "bf16", "f32", 2048, 256, 1, "bias", R("smallk", vec=True), pad=dict(a=3,
         b=1, c=8)),
    case("smallk-nn-f32-k5", "nn", "f32", "f32", 300, 512, 5, "cross_u", R("smallk", vec=True),
         pad=dict(a=3, b=8, c=8, x=16, u=8)),
    case("smallk-nn-bf16-k5-scalar", "nn", "bf16", "bf16", 300, 512, 5, "cross_res", R("smallk"), pad=P3),
    case("smallk-nn-bf16-k5-scalar-f32out", "nn", "bf16", "f32", 300, 512, 5, "cross_res", R("smallk"), pad=P3),
    case("smallk-nt-f32-k16-off", "nt", "f32", "f32", 5000, 16, 16, "bias_res", R("smallk", vec=True), off=dict(a=1),
         beta=1.0),
    case("smallk-k0-bias", "nn", "f32", "f32", 1024, 64, 0, "bias", R("smallk", vec=True)),
    # the small shapes tests/test_dense_ops_gpu.py once labelled gemm_rowdot_kernel / gemm_smallk_kernel / gemm_thin_kernel:
    # tile_eligible takes them first wherever the contiguous axes are whole vectors (the 256 -> 1 unit forward included)
    case("dense1-fwd-nt-bf16-3000x1x256", "nt", "bf16", "bf16", 3000, 1, 256, "bias", R("mfma")),
    case("dense1-fwd-nt-bf16-3000x1x256-f32out", "nt", "bf16", "f32", 3000, 1, 256, "bias", R("mfma")),
    case("dense1-fwd-nt-f32-3000x1x256", "nt", "f32", "f32", 3000, 1, 256, "bias", R("mfma")),
    case("rowdot-nt-bf16-n1-k250", "nt", "bf16", "bf16", 3000, 1, 250, "bias", R("rowdot")),
    case("mfma-nn-bf16-1100x8x40", "nn", "bf16", "bf16", 1100, 8, 40, "bias", R("mfma", vec=True)),
    case("mfma-nt-f32-5000x16x16", "nt", "f32", "f32", 5000, 16, 16, "bias", R("mfma", vec=True)),
    case("mfma-tn-f32-8x300x2048", "tn", "f32", "f32", 8, 300, 2048, "plain", R("mfma", splits=4, reduce="scalar")),
    # gemm_generic_kernel, K = 0 (C = epilogue(0)) and M = 0 (nothing launched)
    case("generic-nn-f32", "nn", "f32", "f32", 5, 7, 9, "cross_res", R("generic"), pad=P3),
    case("generic-nt-bf16", "nt", "bf16", "bf16", 33, 19, 21, "cross_u", R("generic"), pad=P3),
    case("generic-nt-bf16-f32out", "nt", "bf16", "f32", 33, 19, 21, "cross_u", R("generic"), pad=P3),
    case("generic-nt-f32", "nt", "f32", "f32", 33, 19, 21, "bias", R("generic"), pad=P3),
    case("generic-tn-f32", "tn", "f32", "f32", 33, 19, 21, "bias_res", R("generic"), pad=P3),
    case("generic-tn-bf16-1100x8x40", "tn", "bf16", "bf16", 1100, 8, 40, "bias", R("generic"), pad=P3),
    case("generic-tn-bf16-1100x8x40-f32out", "tn", "bf16", "f32", 1100, 8, 40, "bias", R("generic"), pad=P3),
    case("generic-nn-bf16-b-off", "nn", "bf16", "bf16", 130, 200, 72, "res", R("generic", vec=True), pad=dict(c=8,
         r=8), off=dict(b=1), beta=0.5),
    case("generic-nn-bf16-b-off-f32out", "nn", "bf16", "f32", 130, 200, 72, "res", R("generic", vec=True),
         pad=dict(c=8, r=8), off=dict(b=1), beta=0.5),
    case("generic-k0-bias", "nt", "bf16", "bf16", 37, 19, 0, "bias", R("generic"), pad=P3),
    case("generic-k0-bias-f32out", "nt", "bf16", "f32", 37, 19, 0, "bias", R("generic"), pad=P3),
    case("none-m0", "nn", "f32", "f32", 0, 16, 8, "bias", R(None)),
]
