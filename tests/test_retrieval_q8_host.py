"""K17 (krs_retrieval_topk_q8, the int8 index of BruteForceRetrieval) checked without a GPU: the numpy restatement
(tests/retrieval_q8_restatement.py) against hand-computed answers, the quantization error bound on seeded normal data,
the layer's quantize() refusals before any device work, the workspace size and the C ABI's refusals (which come before
any launch, so device pointers may be NULL).  tests/test_retrieval_q8_gpu.py holds the kernel to the restatement."""

import numpy as np
import pytest

from tests import retrieval_q8_restatement as RQ

INVALID, UNSUPPORTED = -1, -2


# ---- the restatement on integer data, against answers worked out by hand -------------------------------------------------
def test_restatement_on_integer_data_equals_hand_computed_answers():
    # abs-max 127 in every row: step = (127 + 1e-7) / 127 rounds to 1.0f and q = x
    query = np.array([[127, 0, -1], [-127, 2, 0]], np.float32)
    cand = np.array([[1, 1, 1], [127, 0, 0], [1, 1, 1], [-127, 5, 3], [0, 0, -127]], np.float32)
    cq, cstep = cand.astype(np.int8), np.ones((5,), np.float32)       # (rows 0 and 2 handed in as int8 directly)
    full = [1, 3, 4]
    fq, fstep, bad = RQ.quantize(cand[full])
    assert not bad.any() and (fq == cand[full]).all() and (fstep == np.float32(1.0)).all()
    qq, qstep, _ = RQ.quantize(query)
    assert (qq == query).all() and (qstep == np.float32(1.0)).all()
    want = np.array([[126, 16129, 126, -16132, 127], [-125, -16129, -125, 16139, 0]], np.int32)
    assert (RQ.idot(qq, cq) == want).all()
    r = RQ.restate(query, cq, cstep, 4)
    assert r["scores"].dtype == np.float32 and r["ids"].dtype == np.int32 and r["flag"] == 0
    assert r["ids"].tolist() == [[1, 4, 0, 2], [3, 4, 0, 2]]             # ties (126, -125) go to the lower index
    assert r["scores"].tolist() == [[16129.0, 127.0, 126.0, 126.0], [16139.0, 0.0, -125.0, -125.0]]
    ids = np.array([50, 40, 30, 20, 10], np.int32)
    assert RQ.restate(query, cq, cstep, 2, ids=ids)["ids"].tolist() == [[40, 10], [20, 10]]
    # steps that are not 1: the two multiplies, in the contract's order, each rounded to fp32
    cstep2 = np.array([0.1, 0.25, 3.0, 1.0, 1e-3], np.float32)
    s = RQ.scores(qq, np.array([0.5, 7.0], np.float32), cq, cstep2)
    assert s[0, 0] == np.float32(np.float32(np.float32(126.0) * np.float32(0.1)) * np.float32(0.5))
    assert s[1, 3] == np.float32(np.float32(16139.0) * np.float32(7.0))
    # bf16 rounding: to nearest, ties to even
    got = RQ.to_bf16(np.array([1.0, 1.00390625, 1.01171875, 16129.0, -125.0, 0.0], np.float32))
    assert got.tolist() == [1.0, 1.0, 1.015625, 16128.0, -125.0, 0.0]


def test_restatement_orders_signed_zeros_as_one_value_and_marks_nonfinite_rows():
    # idot < 0 times a zero step is -0.0: it ties with +0.0 and the index decides; the returned zero is +0.0
    qq = np.array([[1, 0]], np.int8)
    cq = np.array([[-5, 0], [3, 0], [0, 0], [-1, 0]], np.int8)
    cstep = np.array([0.0, 0.0, 1.0, 0.0], np.float32)
    s = RQ.scores(qq, np.array([1.0], np.float32), cq, cstep)
    assert np.signbit(s[0, 0]) and not np.signbit(s[0, 1]) and (s == 0).all()
    assert RQ.order(s, 4).tolist() == [[0, 1, 2, 3]]
    query = np.array([[1.0, -2.0], [np.nan, 1.0], [3.0, np.inf], [0.0, 0.0]], np.float32)
    cand = np.array([[1.0, 1.0], [-1.0, -1.0], [2.0, -2.0]], np.float32)
    cq2, cstep2, _ = RQ.quantize(cand)
    r = RQ.restate(query, cq2, cstep2, 2)
    assert r["bad"].tolist() == [False, True, True, False] and r["flag"] == RQ.FLAG_NONFINITE_ROW
    assert (r["qq"][1:3] == 0).all() and (r["qstep"][1:3] == 0).all()
    assert r["ids"][1:].tolist() == [[0, 1]] * 3                        # an all-zero row also scores 0 everywhere
    assert (r["scores"][1:] == 0).all() and not np.signbit(r["scores"]).any()
    assert r["ids"][0].tolist() == [2, 1]                               # 1*2 + (-2)(-2) = 6 > 1 > -1


# ---- the quantization error bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-3, 1.0, 50.0])
@pytest.mark.parametrize("d", [1, 16, 17, 100, 128, 512])
def test_quantized_scores_stay_inside_the_quantization_bound(d, scale):
    """|s_ij - q_i . c_j| <= 1.01 [ (cstep_j |q_i|_1 + qstep_i |c_j|_1) / 2 + d qstep_i cstep_j / 4 ] (derived in
    retrieval_q8_restatement.quantization_bound); measured worst ratio over these cases: 0.78 of the bracket (d = 1 at scale 1e-3), 0.52 for d >= 16."""
    rng = np.random.default_rng(1000 * d + int(scale * 7))
    query = (rng.standard_normal((24, d)) * scale).astype(np.float32)
    cand = (rng.standard_normal((200, d)) * scale).astype(np.float32)
    cq, cstep, bad = RQ.quantize(cand)
    r = RQ.restate(query, cq, cstep, 1)
    assert not bad.any() and not r["bad"].any()
    err = np.abs(r["s"].astype(np.float64) - RQ.exact_scores(query, cand))
    tol = RQ.quantization_bound(query, cand, r["qstep"], cstep)
    assert (tol > 0).all()
    ratio = float((err / tol).max())
    print(f"d={d} scale={scale}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0


# ---- the layer's refusals come before any device work --------------------------------------------------------------------
def _cpu_layer(n=200, d=8, k=5, **kw):
    import keras_rs_amd.layers as kl

    rng = np.random.default_rng(3)
    return kl.BruteForceRetrieval(rng.standard_normal((n, d)).astype(np.float32), k=k, device="cpu", **kw)


def test_layer_refusals_are_raised_before_any_device_call(monkeypatch):
    import torch

    import keras_rs_amd.layers as kl
    from keras_rs_amd.layers import retrieval as retrieval_layers

    def no_device(*a, **k):
        raise AssertionError("quantize() reached the device before refusing")

    monkeypatch.setattr(retrieval_layers, "quantize_rows_checked", no_device)
    with pytest.raises(ValueError, match="int8"):
        _cpu_layer().quantize("int4")
    with pytest.raises(ValueError, match="no candidates"):
        kl.BruteForceRetrieval(k=5, device="cpu").quantize("int8")
    with pytest.raises(ValueError, match="128"):
        _cpu_layer(k=129).quantize("int8")
    with pytest.raises(ValueError, match="512"):
        _cpu_layer(n=20, d=513).quantize()
    # a layer in the quantized state (put together by hand: there is no device here to quantize on)
    layer = _cpu_layer()
    layer.register_buffer("candidate_embeddings_q", torch.zeros((200, 8), dtype=torch.int8))
    layer.register_buffer("candidate_embeddings_step", torch.zeros((200,), dtype=torch.float32))
    layer.candidate_embeddings = None
    layer.quantization_mode = "int8"
    with pytest.raises(ValueError, match="already quantized"):
        layer.quantize("int8")
    with pytest.raises(AssertionError, match="reached the device"):      # (and an accepted request does go there)
        _cpu_layer().quantize("int8")
    # an unquantized layer is what it was: one float weight, no quantization mode, the config without a new key
    plain = _cpu_layer()
    assert plain.quantization_mode is None and [tuple(w.shape) for w in plain.weights] == [(200, 8)]
    assert set(plain.get_config()) == {"name", "trainable", "dtype", "k", "return_scores"}
    assert set(plain.state_dict()) == {"candidate_embeddings"}


# ---- workspace and the C ABI's refusals -----------------------------------------------------------------------------------
def test_workspace_bytes_and_abi_refusals_without_a_device():
    import torch

    from keras_rs_amd import _lib as lib
    from keras_rs_amd import retrieval_ops
    from keras_rs_amd.build import build

    build()
    wsb = retrieval_ops.retrieval_topk_q8_workspace_bytes
    assert wsb(64, 1 << 20, 128, 100) > 0 and wsb(1, 1, 1, 1) > 0 and wsb(8192, 1 << 20, 512, 128) > 0
    assert wsb(0, 1000, 128, 10) == 0
    # the quantized queries ride on top of K8's lists: b rows of d rounded up to 32 bytes, and 4 b bytes
    lists = retrieval_ops.retrieval_topk_workspace_bytes(64, 1 << 20, 128, 100, torch.bfloat16)
    assert wsb(64, 1 << 20, 128, 100) == lists + 64 * 128 + 256
    assert retrieval_ops.Q8_MAX_K == 128 and retrieval_ops.Q8_MAX_D == 512

    fn = lib.lib().krs_retrieval_topk_q8
    #       q     ldq  qdt      cq    ldc  cstep ids   b  n     d    k   out   odt      oids  err   ws    wsb stream
    call = [None, 128, lib.F32, None, 128, None, None, 4, 1000, 128, 10, None, lib.F32, None, None, None, 0, None]
    B, N, D, K, LDQ, LDC, QDT, ODT = 7, 8, 9, 10, 1, 4, 2, 12
    for what, changes, status, names in (
            ("k above 128", {K: 129}, UNSUPPORTED, "128"),
            ("d above 512", {D: 513, LDQ: 513, LDC: 513}, UNSUPPORTED, "512"),
            ("k above n", {K: 11, N: 10}, INVALID, None),
            ("k = 0", {K: 0}, INVALID, None),
            ("k above n and above 128", {K: 200, N: 150}, INVALID, None),
            ("n = 0", {N: 0}, INVALID, None),
            ("d = 0", {D: 0}, INVALID, None),
            ("negative b", {B: -1}, INVALID, None),
            ("more than INT32_MAX candidates", {N: 2 ** 31}, INVALID, None),
            ("ldq below d", {LDQ: 127}, INVALID, None),
            ("ldc below d", {LDC: 127}, INVALID, None),
            ("int8 queries", {QDT: lib.I8}, INVALID, None),
            ("bad output dtype", {ODT: 5}, INVALID, None),
            ("null operands", {}, INVALID, "null")):
        args = list(call)
        for pos, value in changes.items():
            args[pos] = value
        assert fn(*args) == status, what
        message = lib.lib().krs_last_error().decode()
        assert message.startswith("krs_retrieval_topk_q8"), what
        if names:
            assert names in message, (what, message)
    args = list(call)
    args[B] = 0
    assert fn(*args) == 0                                   # an empty batch: nothing is launched, nothing is read
    fake = 0x100000
    args = list(call)
    for pos in (0, 3, 5, 13):
        args[pos] = fake
    assert fn(*args) == -4                                  # KRS_ERR_WORKSPACE: checked before the first launch
