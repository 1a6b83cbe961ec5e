"""K18 (krs_gemm_q8, the int8 form of Dense and FeatureCross) restated in plain numpy -- the reference of
tests/test_gemm_q8_host.py, tests/test_gemm_q8_gpu.py and tests/test_dense_q8_layers_gpu.py.  It shares nothing with the
kernels.

    quantize      K16's quantizer (tests/embed_q8_restatement.py), for activation rows and for the rows of W^T
    idot          sum_e aq[i, e] * wq[j, e] in int64, asserted to fit int32 (K <= 131072)
    z             np.float32(idot) -- round to nearest even, |idot| may exceed 2^24 -- times wstep_j, times astep_i: two
                  np.float32 multiplies, each rounded, the dtype asserted
    epilogue      krs_gemm's, in float64 on z (bias, activation, cross form, residual): the caller bounds or, on
                  representable data, equates
    NaN rows      astep_i == 0 (a non-finite activation row): row i of C and of u is NaN whatever the epilogue
    to_bf16       round to nearest even
"""

import numpy as np

from tests import embed_q8_restatement as Q8
from tests.retrieval_q8_restatement import to_bf16  # noqa: F401  (re-exported)

FLAG_NONFINITE_ROW = Q8.FLAG_NONFINITE_ROW
MAX_K = 131072
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3
quantize = Q8.quantize


def quantize_kernel(w):
    """(wq int8 [N, K], wstep float32 [N]) of a Keras kernel W [K, N]: the rows of W^T through the quantizer."""
    wq, wstep, bad = quantize(np.ascontiguousarray(np.asarray(w, np.float32).T))
    assert not bad.any()
    return wq, wstep


def idot(aq, wq):
    """[M, N] int32 dot products of int8 rows ([M, K] against [N, K]), formed in int64 and asserted to fit."""
    aq, wq = np.asarray(aq), np.asarray(wq)
    assert aq.dtype == np.int8 and wq.dtype == np.int8 and aq.shape[1] == wq.shape[1] <= MAX_K
    wide = aq.astype(np.int64) @ wq.astype(np.int64).T
    assert wide.dtype == np.int64 and np.abs(wide).max(initial=0) < 2 ** 31
    return wide.astype(np.int32)


def scale(idots, astep, wstep):
    """z [M, N] float32 = (float32(idot) * wstep_j) * astep_i, each step rounded to fp32."""
    astep, wstep = np.asarray(astep), np.asarray(wstep)
    assert idots.dtype == np.int32 and astep.dtype == np.float32 and wstep.dtype == np.float32
    f = idots.astype(np.float32)                        # round to nearest even above 2^24
    first = f * wstep[None, :]
    assert f.dtype == np.float32 and first.dtype == np.float32
    z = first * astep[:, None]
    assert z.dtype == np.float32
    return z


def product(aq, astep, wq, wstep):
    """C at fp32 without an epilogue: z, with NaN rows where astep == 0."""
    z = scale(idot(aq, wq), astep, wstep)
    z[np.asarray(astep) == 0] = np.nan
    return z


def activation(v, act):
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    if act == ACT_TANH:
        return np.tanh(v)
    return v


def epilogue(z, astep, bias=None, act=ACT_NONE, x0=None, x=None, diag_scale=0.0, r=None, beta=1.0):
    """(C, u) in float64: krs_gemm's epilogue on v = z; u is act(z + bias) (the cross form's u_out) or None.  Rows with
    astep == 0 are NaN in both."""
    v = np.asarray(z, np.float64)
    if bias is not None:
        v = v + np.asarray(bias, np.float64)[None, :]
    v = activation(v, act)
    u = None
    if x0 is not None:
        u = v.copy()
        x64 = np.asarray(x, np.float64)
        v = np.asarray(x0, np.float64) * (v + float(diag_scale) * x64) + x64
    if r is not None:
        v = v + float(beta) * np.asarray(r, np.float64)
    bad = np.asarray(astep) == 0
    v[bad] = np.nan
    if u is not None:
        u[bad] = np.nan
    return v, u


def dense(x, wq, wstep, bias=None, act=ACT_NONE):
    """A quantized Dense call on float32 rows x [M, K]: (z float32, C float64, astep)."""
    aq, astep, _ = quantize(x)
    z = scale(idot(aq, wq), astep, wstep)
    return z, epilogue(z, astep, bias=bias, act=act)[0], astep


def quantization_bound(x, w, astep, wstep):
    """[M, N] float64: 1.01 * [ (astep_i ||w_j||_1 + wstep_j ||x_i||_1) / 2 + K astep_i wstep_j / 4 ] for x [M, K] and
    the Keras kernel w [K, N].  With the dequantized rows x^ = x - ex and w^ = w - ew, |ex| <= astep / 2 and
    |ew| <= wstep / 2 per element (abs-max scaling never clips): x . w - x^ . w^ = x . ew + ex . w - ex . ew, whose three
    terms are bounded by the three terms above.  The 1 % covers the fp32 roundings of inv, step, the conversion and the
    two multiplies (each about 6e-8 relative)."""
    x64, w64 = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64))
    k = x64.shape[1]
    a, s = np.asarray(astep, np.float64)[:, None], np.asarray(wstep, np.float64)[None, :]
    return 1.01 * (0.5 * (a * w64.sum(axis=0)[None, :] + s * x64.sum(axis=1)[:, None]) + 0.25 * k * a * s)
