"""K23 (krs_ah_encode, krs_retrieval_ivf_ah, krs_retrieval_rescore, AsymmetricHashingRetrieval) checked without a GPU:
the numpy restatement (tests/retrieval_ah_restatement.py) against hand-computed answers, what the case table covers, the
workspace sizes, the C ABI's refusals (which come before any launch, so device pointers may be NULL), the layer's
argument checks and its config.  tests/test_retrieval_ah_gpu.py holds the kernels to the restatement."""

import numpy as np
import pytest

from tests import retrieval_ah_cases as CASES
from tests import retrieval_ah_restatement as RA

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4


# ---- the restatement, against answers worked out by hand ------------------------------------------------------------------
def _tiny():
    """D = 2, one block of 2 columns.  Centres: 0 = (0, 0), 1 = (1, 0), 2 = (0, 1), 3 = (1, 0) again, the rest far away."""
    codebooks = np.full((1, 16, 2), 8.0, np.float32)
    codebooks[0, :4] = [[0, 0], [1, 0], [0, 1], [1, 0]]
    centroids = np.array([[1, 0], [0, 1]], np.float32)
    #                 0       1       2       3       4
    cand = np.array([[2, 0], [1, 1], [1, 0], [0, 2], [3, 0]], np.float32)
    assign = np.array([0, 1, 0, 1, 0])
    return codebooks, centroids, cand, assign


def test_encoder_ties_go_to_the_lowest_code():
    codebooks, centroids, cand, assign = _tiny()
    # residuals: (1, 0), (1, 0), (0, 0), (0, 1), (2, 0).  (1, 0) is centre 1 and centre 3: the lower code.  (2, 0) is 1
    # away from centres 1 and 3, 4 from centre 0, 5 from centre 2: code 1.
    assert RA.encode(cand, assign, centroids, codebooks).tolist() == [[1], [1], [0], [2], [1]]
    # (0.5, 0) is 0.25 from centre 0 and from centres 1 and 3: the three-way tie goes to code 0
    assert RA.encode(np.array([[1.5, 0]], np.float32), [0], centroids, codebooks).tolist() == [[0]]
    # a padded last block: D = 3, m = 2: the column 3 that does not exist counts as e = 0, c = 0 whatever the codebook holds
    cb = np.zeros((2, 16, 2), np.float32)
    cb[1, :, 1] = 5.0                                                     # (garbage in the padding column)
    cb[1, :, 0] = np.arange(16)
    cb[0] = 8.0
    got = RA.encode(np.array([[0, 0, 7], [0, 0, 7.5]], np.float32), [0, 0], np.zeros((1, 3), np.float32), cb)
    assert got[:, 1].tolist() == [7, 7]                                   # 7.5: 7 and 8 tie, the lower code
    assert RA.decode(got, cb, 3)[:, 2].tolist() == [7.0, 7.0]


def test_nibble_layout():
    assert RA.code_bytes(6, 2) == 4 and RA.code_bytes(16, 2) == 4 and RA.code_bytes(18, 2) == 8
    assert RA.code_bytes(128, 2) == 32 and RA.code_bytes(512, 2) == 128 and RA.code_bytes(100, 8) == 8
    assert RA.code_bytes(32, 8) == 4 and RA.code_bytes(100, 4) == 16
    # block j is nibble j: byte j // 2, the even j in the low four bits; the row is padded with zero nibbles
    assert RA.pack([[1, 2, 3]], 6, 2).tolist() == [[0x21, 0x03, 0, 0]]
    nine = RA.pack([[15, 0, 1, 2, 3, 4, 5, 6, 9]], 18, 2)
    assert nine.tolist() == [[0x0F, 0x21, 0x43, 0x65, 0x09, 0, 0, 0]] and nine.dtype == np.uint8
    assert RA.unpack(nine, 18, 2).tolist() == [[15, 0, 1, 2, 3, 4, 5, 6, 9]]
    rng = np.random.default_rng(1)
    nib = rng.integers(0, 16, size=(7, 13))
    assert (RA.unpack(RA.pack(nib, 100, 8), 100, 8) == nib).all()


def test_restatement_equals_hand_computed_answers():
    codebooks, centroids, cand, assign = _tiny()
    nib = RA.encode(cand, assign, centroids, codebooks)
    # centroid + decode: (2, 0), (1, 1), (1, 0), (0, 2), (2, 0): candidate 4 = (3, 0) is the one the codes get wrong
    assert (RA.decode(nib, codebooks, 2) + centroids[assign]).tolist() == [[2, 0], [1, 1], [1, 0], [0, 2], [2, 0]]
    q = np.array([[1, 1]], np.float32)
    # both leaves score 1: leaf 0 first.  AH scores 2, 2, 1, 2, 2: the tie between candidate 0 (leaf 0) and candidate 1
    # (leaf 1) goes to the lower ORIGINAL index
    scan = RA.restate(q, centroids, codebooks, nib, assign, probes=2, k=3)
    assert scan["leaves"].tolist() == [[0, 1]]
    assert scan["ids"].tolist() == [[0, 1, 3]] and scan["scores"].tolist() == [[2.0, 2.0, 2.0]]
    # the reorder sees the scan's r best only: with r = 3 candidate 4 (exact score 3, the true best) is not among them
    few = RA.restate(q, centroids, codebooks, nib, assign, probes=2, k=2, r=3, rows=cand)
    assert few["merged"].tolist() == [[0, 1, 3]] and few["ids"].tolist() == [[0, 1]]
    assert few["scores"].tolist() == [[2.0, 2.0]]
    # with r = 5 it is, and its exact score puts it first
    ids = np.array([50, 40, 30, 20, 10], np.int32)
    full = RA.restate(q, centroids, codebooks, nib, assign, probes=2, k=2, r=5, rows=cand, ids=ids)
    assert full["index"].tolist() == [[4, 0]] and full["ids"].tolist() == [[10, 50]]
    assert full["scores"].tolist() == [[3.0, 2.0]]
    # one probe: leaf 0 = {0, 2, 4}: fewer than k = 4 -> id -1 (also with ids), score -inf; fewer than r as well
    short = RA.restate(q, centroids, codebooks, nib, assign, probes=1, k=4, ids=ids)
    assert short["ids"].tolist() == [[50, 10, 30, -1]] and short["scores"].tolist() == [[2.0, 2.0, 1.0, -np.inf]]
    short = RA.restate(q, centroids, codebooks, nib, assign, probes=1, k=4, r=5, rows=cand, ids=ids)
    assert short["merged"].tolist() == [[0, 4, 2, -1, -1]] and short["count"].tolist() == [3]
    assert short["ids"].tolist() == [[10, 50, 30, -1]] and short["scores"].tolist() == [[3.0, 2.0, 1.0, -np.inf]]
    # the selection of krs_retrieval_rescore alone: padding and out-of-range entries are skipped, ties by index
    sel = RA.rescore_select(q, cand, [[3, -1, 1, 0, 7]], 4)
    assert sel["ids"].tolist() == [[0, 1, 3, -1]] and sel["scores"].tolist() == [[2.0, 2.0, 2.0, -np.inf]]
    # an fp32 query is rounded to bf16 for the scan only: 1.00390625 (1 + 2^-8) -> 1.0 against decode, not against centroids
    q2 = np.array([[1.00390625, 0]], np.float32)
    s = RA.ah_scores(q2, centroids, RA.decode(nib, codebooks, 2), assign)
    assert s[0, 0] == np.float32(1.0) + np.float32(1.00390625)


# ---- what the case table covers ------------------------------------------------------------------------------------------
def test_case_table_covers_what_the_kernels_can_get_wrong():
    made = [CASES.make(name) for name in CASES.NAMES]
    assert len(set(CASES.NAMES)) == len(CASES.NAMES)
    sizes, tiles, b_seen, flags = set(), set(), set(), set()
    for c in made:
        n, d = c["cand"].shape
        b, leaves, k, r, m = c["query"].shape[0], len(c["sizes"]), c["k"], c["r"], c["m"]
        assert n <= 2000 and b <= 70 and 1 <= k <= min(n, 128) and d <= 512 and m in (2, 4, 8)
        assert r is None or k <= r <= 128
        for name in ("cand", "query", "centroids", "codebooks"):
            assert np.abs(c[name]).max() <= 8 and (c[name] == np.round(c[name])).all()
        assert (np.bincount(c["assignments"], minlength=leaves) == c["sizes"]).all()
        assert c["codebooks"].shape == (RA.blocks_of(d, m), 16, m)
        if d % m:
            flags.add("padded last block")
            assert (c["codebooks"][-1, :, d % m:] == 0).all()
        assert {0, 15} <= set(np.unique(c["nibbles"]).tolist())
        sizes |= set(c["sizes"])
        ref = RA.restate(c["query"], c["centroids"], c["codebooks"], c["nibbles"], c["assignments"], c["probes"], k, r=r,
                         rows=None if r is None else c["cand"], ids=c["ids"])
        probed = np.bincount(ref["leaves"].reshape(-1), minlength=leaves)
        tiles |= set(probed.tolist())
        b_seen.add(b)
        flags |= {f"m={m}", f"d={d}", f"{c['dtype']} queries", "ids" if c["ids"] is not None else "no ids",
                  "reorder" if r is not None else "scan only"}
        if r == k:
            flags.add("r = k")
        if r == 128:
            flags.add("r = 128")
        if k == 1:
            flags.add("k = 1")
        if c["pad"]:
            flags.add("odd stride" if c["pad"] % 8 else "stride")
        if (ref["count"] < k).any():
            flags.add("fewer than k, " + ("reorder" if r is not None else "scan only"))
        if r is not None and ((ref["count"] < r) & (ref["count"] >= k)).any():
            flags.add("fewer than r")
        if any(s == 0 and probed[l] > 0 for l, s in enumerate(c["sizes"])):
            flags.add("empty leaf probed")
        if (probed == 0).any():
            flags.add("unprobed leaf")
        if k <= 8 and any(s >= 400 and probed[l] > 0 for l, s in enumerate(c["sizes"])):
            flags.add("queue cut")
        if ((ref["scores"][:, 1:] == ref["scores"][:, :-1]) & np.isfinite(ref["scores"][:, 1:])).any():
            flags.add("ties")
        if r is not None:
            # the codes matter: somewhere the AH order of the merged list is not the exact order
            exact = RA.restate(c["query"], c["centroids"], c["codebooks"], c["nibbles"], c["assignments"], c["probes"],
                               k, r=k, rows=c["cand"])
            if (exact["index"] != ref["index"]).any():
                flags.add("reorder changes the result")
    assert {0, 1, 127, 128, 129} <= sizes
    assert {0, 1, 32, 33} <= tiles
    assert {1, 33} <= b_seen
    assert flags >= {"m=2", "m=4", "m=8", "d=32", "d=100", "d=512", "padded last block", "bf16 queries", "f32 queries",
                     "ids", "no ids", "reorder", "scan only", "r = k", "r = 128", "k = 1", "stride", "odd stride",
                     "fewer than k, reorder", "fewer than k, scan only", "fewer than r", "empty leaf probed",
                     "unprobed leaf", "queue cut", "ties", "reorder changes the result"}


# ---- workspaces and the C ABI's refusals ----------------------------------------------------------------------------------
def _align(v):
    return (v + 255) // 256 * 256


def test_workspace_bytes_follow_the_documented_formulas():
    import torch

    from keras_rs_amd import retrieval_ops
    from keras_rs_amd.build import build

    build()
    ivf, ah = retrieval_ops.retrieval_ivf_workspace_bytes, retrieval_ops.retrieval_ivf_ah_workspace_bytes
    rescore = retrieval_ops.retrieval_rescore_workspace_bytes
    for b, n, d, leaves, probes, k, r in ((64, 1 << 20, 128, 1024, 8, 100, 128), (8192, 1 << 20, 128, 1024, 32, 10, 100),
                                          (1, 5, 3, 2, 1, 1, 1), (70, 900, 32, 8, 3, 8, 128)):
        for dtype in (torch.bfloat16, torch.float32):
            base = ivf(b, n, d, leaves, probes, r, dtype) + _align(4 * b * probes)
            assert ah(b, n, d, leaves, probes, k, r, 2, True, dtype) == base + _align(4 * b * r) + _align(8 * b * r)
            assert ah(b, n, d, leaves, probes, k, k, 4, False, dtype) == \
                ivf(b, n, d, leaves, probes, k, dtype) + _align(4 * b * probes)
        assert rescore(b, r, k) == _align(8 * b * r)
    assert ah(0, 1000, 128, 10, 2, 10, 10, 2, False, torch.float32) == 0
    assert ah(4, 1000, 128, 10, 2, 10, 20, 2, False, torch.float32) == 0        # r != k without reordering
    assert ah(4, 1000, 128, 10, 2, 10, 9, 2, True, torch.float32) == 0          # r < k
    assert ah(4, 1000, 128, 10, 2, 10, 129, 2, True, torch.float32) == 0        # r above 128
    assert ah(4, 1000, 128, 10, 2, 10, 10, 3, True, torch.float32) == 0         # m
    assert ah(4, 1000, 128, 10, 11, 10, 10, 2, True, torch.float32) == 0        # probes above leaves
    assert rescore(0, 10, 10) == 0 and rescore(4, 129, 10) == 0 and rescore(4, 10, 11) == 0
    assert retrieval_ops.AH_MAX_R == 128 and retrieval_ops.AH_BLOCK_DIMS == (2, 4, 8)
    for d, m in ((6, 2), (128, 2), (100, 8), (100, 4), (512, 2), (32, 8)):
        assert retrieval_ops.ah_code_bytes(d, m) == RA.code_bytes(d, m)
    assert retrieval_ops.ah_code_bytes(513, 2) == 0 and retrieval_ops.ah_code_bytes(64, 3) == 0


def _refusals(fn, prefix, call, table, required, b_pos, ws_pos):
    from keras_rs_amd import _lib as lib

    for what, changes, status, names in table:
        args = list(call)
        for pos, value in changes.items():
            args[pos] = value
        assert fn(*args) == status, what
        message = lib.lib().krs_last_error().decode()
        assert message.startswith(prefix + ":"), (what, message)
        if names:
            assert names in message, (what, message)
    if b_pos is not None:
        args = list(call)
        args[b_pos] = 0
        assert fn(*args) == 0                               # nothing to do: nothing is launched, nothing is read
    fake = 0x100000
    for missing in required:                                # each required pointer on its own
        args = list(call)
        for pos in required:
            args[pos] = None if pos == missing else fake
        assert fn(*args) == INVALID and "null" in lib.lib().krs_last_error().decode(), missing
    if ws_pos is not None:
        args = list(call)
        for pos in required:
            args[pos] = fake
        assert fn(*args) == WORKSPACE                       # checked before the first launch
        args[ws_pos], args[ws_pos + 1] = fake, 1            # a workspace pointer with too few bytes
        assert fn(*args) == WORKSPACE


def test_ivf_ah_refusals_come_before_any_launch():
    from keras_rs_amd import _lib as lib
    from keras_rs_amd.build import build

    build()
    #       q     ldq  cen   ldm  cb    m  codes ldcode offs  ridx  rows  ldr  ids   dtype    b  n     d    leaves probes k   r
    call = [None, 128, None, 128, None, 2, None, 32,    None, None, None, 128, None, lib.F32, 4, 1000, 128, 200,   8,     10, 10,
            None, None, None, None, 0, None]
    LDQ, LDM, M, LDCODE, ROWS, LDR, DT, B, N, D, LEAVES, PROBES, K, R = 1, 3, 5, 7, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20
    fake = 0x100000
    table = (
        ("k above 128", {K: 129, R: 129}, UNSUPPORTED, "128"),
        ("d above 512", {D: 513, LDQ: 513, LDM: 513}, UNSUPPORTED, "512"),
        ("probes above 128", {PROBES: 129}, UNSUPPORTED, "128"),
        ("b * probes above INT32_MAX", {B: 2 ** 28}, UNSUPPORTED, "2^31"),
        ("r above 128", {ROWS: fake, R: 129}, UNSUPPORTED, "r = 129"),
        ("probes above leaves", {PROBES: 9, LEAVES: 8}, INVALID, "probes"),
        ("probes = 0", {PROBES: 0}, INVALID, "probes"),
        ("k above n", {K: 11, R: 11, N: 10}, INVALID, None),
        ("k = 0", {K: 0, R: 0}, INVALID, None),
        ("n = 0", {N: 0}, INVALID, None),
        ("d = 0", {D: 0}, INVALID, None),
        ("leaves = 0", {LEAVES: 0}, INVALID, None),
        ("negative b", {B: -1}, INVALID, None),
        ("more than INT32_MAX candidates", {N: 2 ** 31}, INVALID, None),
        ("m = 3", {M: 3}, INVALID, "dimensions_per_block"),
        ("m = 1", {M: 1}, INVALID, "dimensions_per_block"),
        ("m = 16", {M: 16}, INVALID, "dimensions_per_block"),
        ("r below k with rows", {ROWS: fake, R: 9}, INVALID, "r = 9"),
        ("r above k without rows", {R: 11}, INVALID, "r = 11"),
        ("ldq below d", {LDQ: 127}, INVALID, "stride"),
        ("ldm below d", {LDM: 127}, INVALID, "stride"),
        ("ldr below d", {ROWS: fake, LDR: 127}, INVALID, "stride"),
        ("code stride below the row", {LDCODE: 28}, INVALID, "code row stride"),
        ("code stride not a multiple of 4", {LDCODE: 34}, INVALID, "code row stride"),
        ("int8", {DT: lib.I8}, INVALID, "dtype"),
        ("null operands", {}, INVALID, "null"))
    _refusals(lib.lib().krs_retrieval_ivf_ah, "krs_retrieval_ivf_ah", call, table, (0, 2, 4, 6, 8, 9, 22), B, 24)
    args = list(call)
    for pos in (0, 2, 4, 8, 9, 22):
        args[pos] = fake
    args[6] = fake + 2                                      # codes off a 4-byte boundary
    assert lib.lib().krs_retrieval_ivf_ah(*args) == INVALID and "boundary" in lib.lib().krs_last_error().decode()


def test_rescore_refusals_come_before_any_launch():
    from keras_rs_amd import _lib as lib
    from keras_rs_amd.build import build

    build()
    #       q     ldq  rows  ldr  idx   ldi ids   dtype    b  n     d    r   k   out   oids  ws    wsb stream
    call = [None, 128, None, 128, None, 20, None, lib.F32, 4, 1000, 128, 20, 10, None, None, None, 0, None]
    LDQ, LDR, LDI, DT, B, N, D, R, K = 1, 3, 5, 7, 8, 9, 10, 11, 12
    table = (
        ("r above 128", {R: 129, LDI: 129}, UNSUPPORTED, "128"),
        ("d above 512", {D: 513, LDQ: 513, LDR: 513}, UNSUPPORTED, "512"),
        ("k above r", {K: 21}, INVALID, "k = 21"),
        ("k = 0", {K: 0}, INVALID, None),
        ("r = 0", {R: 0, K: 0}, INVALID, None),
        ("n = 0", {N: 0}, INVALID, None),
        ("d = 0", {D: 0}, INVALID, None),
        ("negative b", {B: -1}, INVALID, None),
        ("more than INT32_MAX candidates", {N: 2 ** 31}, INVALID, None),
        ("ldq below d", {LDQ: 127}, INVALID, "stride"),
        ("ldr below d", {LDR: 127}, INVALID, "stride"),
        ("ldi below r", {LDI: 19}, INVALID, "stride"),
        ("int8", {DT: lib.I8}, INVALID, "dtype"),
        ("null operands", {}, INVALID, "null"))
    _refusals(lib.lib().krs_retrieval_rescore, "krs_retrieval_rescore", call, table, (0, 2, 4, 14), B, 15)


def test_encode_refusals_come_before_any_launch():
    from keras_rs_amd import _lib as lib
    from keras_rs_amd.build import build

    build()
    #       x     ldx  ridx  leaf  cen   ldm  dtype    cb    n     d    leaves m  codes ldcode stream
    call = [None, 128, None, None, None, 128, lib.F32, None, 1000, 128, 200,   2, None, 32,    None]
    LDX, LDM, DT, N, D, LEAVES, M, LDCODE = 1, 5, 6, 8, 9, 10, 11, 13
    table = (
        ("d above 512", {D: 513, LDX: 513, LDM: 513, LDCODE: 132}, UNSUPPORTED, "512"),
        ("negative n", {N: -1}, INVALID, None),
        ("d = 0", {D: 0}, INVALID, None),
        ("leaves = 0", {LEAVES: 0}, INVALID, None),
        ("more than INT32_MAX rows", {N: 2 ** 31}, INVALID, None),
        ("m = 3", {M: 3}, INVALID, "dimensions_per_block"),
        ("ldx below d", {LDX: 127}, INVALID, "stride"),
        ("ldm below d", {LDM: 127}, INVALID, "stride"),
        ("code stride below the row", {LDCODE: 28}, INVALID, "code row stride"),
        ("code stride not a multiple of 4", {LDCODE: 33}, INVALID, "code row stride"),
        ("int8", {DT: lib.I8}, INVALID, "dtype"),
        ("null operands", {}, INVALID, "null"))
    _refusals(lib.lib().krs_ah_encode, "krs_ah_encode", call, table, (0, 3, 4, 7, 12), N, None)
    args = list(call)
    for pos in (0, 3, 4, 7):
        args[pos] = 0x100000
    args[12] = 0x100001                                     # codes off a 4-byte boundary
    assert lib.lib().krs_ah_encode(*args) == INVALID and "boundary" in lib.lib().krs_last_error().decode()


# ---- the layer: argument checks and config --------------------------------------------------------------------------------
def test_layer_argument_checks_and_config():
    import torch

    import keras_rs_amd.layers as kl

    A = kl.AsymmetricHashingRetrieval
    assert issubclass(A, kl.PartitionedRetrieval)
    for bad in ({"k": 0}, {"k": 129}, {"num_leaves": 0}, {"num_leaves_to_search": 129}, {"training_iterations": -1},
                {"seed": "a"}, {"dimensions_per_block": 1}, {"dimensions_per_block": 3}, {"dimensions_per_block": 16},
                {"dimensions_per_block": 2.0}, {"num_reordering_candidates": 129}, {"num_reordering_candidates": 9},
                {"num_reordering_candidates": 20.0}, {"num_reordering_candidates": True}, {"training_sample_size": 15},
                {"training_sample_size": 1e5}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            A(device="cpu", **bad)
    A(k=10, num_reordering_candidates=10, device="cpu")                  # r = k is allowed
    with pytest.raises(NotImplementedError, match="anisotropic_quantization_threshold"):
        A(device="cpu", anisotropic_quantization_threshold=0.2)
    with pytest.raises(ValueError, match="without providing `candidate_embeddings`"):
        A(candidate_ids=np.arange(4), device="cpu")
    with pytest.raises(TypeError):
        A(device="cpu", blocks=3)
    layer = A(k=7, return_scores=False, num_leaves=16, num_leaves_to_search=3, training_iterations=2, seed=11,
              dimensions_per_block=4, num_reordering_candidates=50, training_sample_size=1000, device="cpu", name="ah")
    config = layer.get_config()
    partitioned = kl.PartitionedRetrieval(k=7, return_scores=False, num_leaves=16, num_leaves_to_search=3,
                                          training_iterations=2, seed=11, device="cpu", name="ah").get_config()
    assert config == {**partitioned, "dimensions_per_block": 4, "num_reordering_candidates": 50,
                      "training_sample_size": 1000, "anisotropic_quantization_threshold": None}
    again = A.from_config(config)
    assert again.get_config() == config and again.num_reordering_candidates == 50 and again.probes() == 3
    defaults = A(device="cpu").get_config()
    assert defaults["dimensions_per_block"] == 2 and defaults["num_reordering_candidates"] is None
    assert defaults["training_sample_size"] == 100_000
    # an empty layer: the state holds nothing, a call says what BruteForceRetrieval says
    assert layer.state_dict() == {} and layer.weights == [] and not layer.built
    with pytest.raises(ValueError, match="No candidates: call `update_candidates` before using the layer."):
        layer.call(np.zeros((2, 8), np.float32))
    with pytest.raises(NotImplementedError, match="K17"):
        layer.quantize("int8")
    # candidate and codebook checks come before any device work
    with pytest.raises(ValueError, match="less than the number of candidates to retrieve"):
        A(np.zeros((5, 8), np.float32), k=10, device="cpu")
    with pytest.raises(ValueError, match="512"):
        A(np.zeros((20, 513), np.float32), k=1, device="cpu")
    rows, centroids = np.zeros((20, 8), np.float32), np.zeros((2, 8), np.float32)
    assign = np.arange(20) % 2
    for what, codebooks, kwargs in (("shape", np.zeros((4, 15, 2)), {}), ("shape", np.zeros((4, 16, 3)), {}),
                                    ("shape", np.zeros((64, 2)), {}), ("blocks", np.zeros((3, 16, 2)), {}),
                                    ("dimensions_per_block", np.zeros((4, 16, 2)), {"dimensions_per_block": 4})):
        with pytest.raises(ValueError, match=what):
            A.from_codebooks(rows, centroids, assign, codebooks, k=5, device="cpu", **kwargs)
    # the nibbles of stored code rows, as the layer's training reads them
    packed = torch.from_numpy(RA.pack([[15, 0, 1, 2, 3, 4, 5, 6, 9]], 18, 2))
    assert kl.retrieval.unpack_codes(packed, 9).tolist() == [[15, 0, 1, 2, 3, 4, 5, 6, 9]]
