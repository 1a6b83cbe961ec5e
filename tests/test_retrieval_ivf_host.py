"""K21 (krs_retrieval_ivf, PartitionedRetrieval) checked without a GPU: the numpy restatement
(tests/retrieval_ivf_restatement.py) against hand-computed answers, what the case table covers, the workspace size,
the C ABI's refusals (which come before any launch, so device pointers may be NULL), the layer's argument checks, the
validation of from_partition and the stored layout.  tests/test_retrieval_ivf_gpu.py holds the kernel to the
restatement."""

import numpy as np
import pytest

from tests import retrieval_ivf_cases as CASES
from tests import retrieval_ivf_restatement as RI

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4


# ---- the restatement, against answers worked out by hand ------------------------------------------------------------------
def test_restatement_equals_hand_computed_answers():
    centroids = np.array([[1, 0], [0, 1], [1, 1], [-1, -1]], np.float32)
    #                 0       1       2       3       4       5
    cand = np.array([[2, 0], [0, 3], [1, 1], [2, 0], [5, 5], [0, 2]], np.float32)
    assign = np.array([2, 1, 0, 0, 3, 1])
    query = np.array([[1, 0], [0, 1], [1, 1]], np.float32)
    # centroid scores: q0 -> (1, 0, 1, -1): leaves 0, 2 (the tie goes to the lower leaf); q1 -> (0, 1, 1, -1): leaves 1, 2;
    # q2 -> (1, 1, 2, -2): leaf 2, then leaf 0 before leaf 1
    assert RI.probe(query, centroids, 2).tolist() == [[0, 2], [1, 2], [2, 0]]
    r = RI.restate(query, centroids, cand, assign, probes=2, k=3)
    # q0: pool {0, 2, 3} scores (2, 1, 2): the cross-leaf tie 0 (leaf 2) / 3 (leaf 0) goes to the lower ORIGINAL index
    # q1: pool {0, 1, 5} scores (0, 3, 2);  q2: pool {0, 2, 3} scores (2, 2, 2): index order
    assert r["ids"].tolist() == [[0, 3, 2], [1, 5, 0], [0, 2, 3]]
    assert r["scores"].tolist() == [[2.0, 2.0, 1.0], [3.0, 2.0, 0.0], [2.0, 2.0, 2.0]]
    assert r["leaves"].dtype == np.int32 and r["ids"].dtype == np.int32 and r["scores"].dtype == np.float32
    # candidate 4 (score 5 for q0) sits in leaf 3, which nobody probes: the price of the approximation
    assert 4 not in r["ids"]
    # every leaf probed: the exact answer
    full = RI.restate(query, centroids, cand, assign, probes=4, k=2)
    assert full["ids"].tolist() == [[4, 0], [4, 1], [4, 1]]
    # ids are looked up by ORIGINAL index
    ids = np.array([60, 50, 40, 30, 20, 10], np.int32)
    assert RI.restate(query, centroids, cand, assign, 2, 3, ids=ids)["ids"].tolist() == \
        [[60, 30, 40], [50, 10, 60], [60, 40, 30]]
    # one probe, k = 3: q0 -> leaf 0 = {2, 3}: two candidates, then the padding: id -1 (also with ids), score -inf
    short = RI.restate(query[:1], centroids, cand, assign, probes=1, k=3, ids=ids)
    assert short["ids"].tolist() == [[30, 40, -1]] and short["index"].tolist() == [[3, 2, -1]]
    assert short["scores"].tolist() == [[2.0, 1.0, -np.inf]] and short["count"].tolist() == [2]
    # bf16 outputs: rounded to nearest even, the padding stays -inf
    big = RI.restate(np.array([[257.0, 0]], np.float32), centroids, cand, assign, 1, 3, out_bf16=True)
    assert big["scores"].tolist() == [[512.0, 256.0, -np.inf]]         # 514 -> 512 (tie to even), 257 -> 256
    # -0.0 ranks as +0.0 and comes back as +0.0
    z = RI.restate(np.array([[-1.0, 0]], np.float32), np.array([[-1, 0]], np.float32),
                   np.array([[0, 1], [0, 2]], np.float32), np.array([0, 0]), 1, 2)
    assert z["ids"].tolist() == [[0, 1]] and not np.signbit(z["scores"]).any()


def test_layout_is_a_stable_sort_by_leaf():
    import torch

    from keras_rs_amd.layers import retrieval as RL

    rng = np.random.default_rng(5)
    assign = rng.integers(0, 7, size=300)
    assign[assign == 3] = 4                                             # an empty leaf
    row_index, offsets = RI.layout(assign, 7)
    got_index, got_offsets = RL.partition_layout(torch.as_tensor(assign), 7)
    assert got_index.dtype == torch.int32 and got_offsets.dtype == torch.int32
    assert (got_index.numpy() == row_index).all() and (got_offsets.numpy() == offsets).all()
    assert offsets[0] == 0 and offsets[-1] == 300 and (np.diff(offsets) >= 0).all() and offsets[3] == offsets[4]
    assert sorted(row_index.tolist()) == list(range(300))
    for leaf in range(7):
        seg = row_index[offsets[leaf]:offsets[leaf + 1]]
        assert (assign[seg] == leaf).all() and (np.diff(seg) > 0).all()   # ascending inside every leaf


# ---- what the case table covers ------------------------------------------------------------------------------------------
def test_case_table_covers_what_the_kernel_can_get_wrong():
    made = [CASES.make(name) for name in CASES.NAMES]
    assert len(set(CASES.NAMES)) == len(CASES.NAMES)
    sizes, tiles, b_seen, k_seen = set(), set(), set(), set()
    flags = set()
    for c in made:
        n, d = c["cand"].shape
        b, leaves = c["query"].shape[0], len(c["sizes"])
        assert n <= 2000 and b <= 70 and 1 <= c["k"] <= min(n, 128) and d <= 512
        assert np.abs(c["cand"]).max() <= 8 and np.abs(c["query"]).max() <= 8 and np.abs(c["centroids"]).max() <= 8
        assert (np.bincount(c["assignments"], minlength=leaves) == c["sizes"]).all()
        sizes |= set(c["sizes"])
        r = RI.restate(c["query"], c["centroids"], c["cand"], c["assignments"], c["probes"], c["k"], ids=c["ids"])
        probed = np.bincount(r["leaves"].reshape(-1), minlength=leaves)
        tiles |= set(probed.tolist())
        b_seen.add(b)
        k_seen.add(c["k"])
        if c["probes"] == 1:
            flags.add("one probe")
        if c["probes"] == leaves:
            flags.add("every leaf probed")
        if (r["count"] < c["k"]).any():
            flags.add("short, radix merge" if c["probes"] * c["k"] > 2048 else "short, small merge")
        if c["probes"] * c["k"] > 2048 and (r["count"] >= c["k"]).all():
            flags.add("radix merge")
        # a leaf of >= 400 rows that is scanned with k <= 8: its queue overflows and is cut back
        if c["k"] <= 8 and any(s >= 400 and probed[l] > 0 for l, s in enumerate(c["sizes"])):
            flags.add("queue cut")
        if any(s == 0 and probed[l] > 0 for l, s in enumerate(c["sizes"])):
            flags.add("empty leaf probed")
        flags.add(f"{c['dtype']} d={d}")
        flags.add("ids" if c["ids"] is not None else "no ids")
        if c["pad"]:
            flags.add("stride")
        # ties, the place where the order can go wrong: some returned row repeats a score
        if ((r["scores"][:, 1:] == r["scores"][:, :-1]) & np.isfinite(r["scores"][:, 1:])).any():
            flags.add("ties")
    assert {0, 1, 127, 128, 129} <= sizes
    assert {0, 1, 32, 33} <= tiles and max(tiles) > 64
    assert {1, 33} <= b_seen and {1, 128} <= k_seen
    assert flags >= {"one probe", "every leaf probed", "short, radix merge", "short, small merge", "radix merge",
                     "queue cut", "empty leaf probed", "bf16 d=32", "bf16 d=100", "f32 d=512", "ids", "no ids", "stride",
                     "ties"}
    routing = made[CASES.NAMES.index("routing")]
    r = RI.restate(routing["query"], routing["centroids"], routing["cand"], routing["assignments"], 3, 8)
    assert np.bincount(r["leaves"].reshape(-1), minlength=8).tolist()[:4] == [70, 33, 32, 1]
    assert np.bincount(r["leaves"].reshape(-1), minlength=8)[7] == 0


# ---- workspace and the C ABI's refusals -----------------------------------------------------------------------------------
def _align(v):
    return (v + 255) // 256 * 256


def test_workspace_bytes_follow_the_documented_formula():
    import torch

    from keras_rs_amd import retrieval_ops
    from keras_rs_amd.build import build

    build()
    wsb = retrieval_ops.retrieval_ivf_workspace_bytes
    for b, n, d, leaves, probes, k in ((64, 1 << 20, 128, 1024, 8, 100), (8192, 1 << 20, 128, 1024, 32, 100),
                                       (1, 5, 3, 2, 1, 1), (70, 900, 32, 8, 3, 8), (9, 180, 32, 60, 20, 128)):
        probe = retrieval_ops.retrieval_topk_workspace_bytes(b, leaves, d, probes, torch.bfloat16)
        ints = _align(4 * (leaves + 1))
        sums = _align(4 * ((leaves + 1 + 1023) // 1024 + 1) + 256)
        merge = _align(b * (1 << (k - 1).bit_length()) * 8) if probes * k > 2048 else 0
        want = probe + 2 * _align(4 * b * probes) + 5 * ints + sums + _align(8 * b * probes * k) + merge
        assert wsb(b, n, d, leaves, probes, k, torch.bfloat16) == want, (b, n, d, leaves, probes, k)
    # the pairs dominate: b * probes * k * 8 bytes
    assert 8192 * 32 * 100 * 8 <= wsb(8192, 1 << 20, 128, 1024, 32, 100, torch.bfloat16) < 1.2 * 8192 * 32 * 100 * 8
    assert wsb(0, 1000, 128, 10, 2, 10, torch.float32) == 0
    assert wsb(4, 1000, 128, 10, 11, 10, torch.float32) == 0            # an unsupported shape asks for nothing
    assert retrieval_ops.IVF_MAX_K == 128 and retrieval_ops.IVF_MAX_D == 512 and retrieval_ops.IVF_MAX_PROBES == 128


def test_abi_refusals_come_before_any_launch():
    from keras_rs_amd import _lib as lib
    from keras_rs_amd.build import build

    build()
    fn = lib.lib().krs_retrieval_ivf
    #       q     ldq  cen   ldm  c     ldc  offs  rows  ids   dtype    b  n     d    leaves probes k  out   oids  olvs  ws    wsb stream
    call = [None, 128, None, 128, None, 128, None, None, None, lib.F32, 4, 1000, 128, 200,   8,     10, None, None, None, None, 0, None]
    LDQ, LDM, LDC, DT, B, N, D, LEAVES, PROBES, K = 1, 3, 5, 9, 10, 11, 12, 13, 14, 15
    for what, changes, status, names in (
            ("k above 128", {K: 129}, UNSUPPORTED, "128"),
            ("d above 512", {D: 513, LDQ: 513, LDM: 513, LDC: 513}, UNSUPPORTED, "512"),
            ("probes above 128", {PROBES: 129}, UNSUPPORTED, "128"),
            ("b * probes above INT32_MAX", {B: 2 ** 28, PROBES: 8}, UNSUPPORTED, "2^31"),
            ("probes above leaves", {PROBES: 9, LEAVES: 8}, INVALID, "probes"),
            ("probes above leaves and above 128", {PROBES: 200, LEAVES: 150}, INVALID, "probes"),
            ("probes = 0", {PROBES: 0}, INVALID, "probes"),
            ("k above n", {K: 11, N: 10}, INVALID, None),
            ("k = 0", {K: 0}, INVALID, None),
            ("k above n and above 128", {K: 200, N: 150}, INVALID, None),
            ("n = 0", {N: 0}, INVALID, None),
            ("d = 0", {D: 0}, INVALID, None),
            ("leaves = 0", {LEAVES: 0}, INVALID, None),
            ("negative b", {B: -1}, INVALID, None),
            ("more than INT32_MAX candidates", {N: 2 ** 31}, INVALID, None),
            ("ldq below d", {LDQ: 127}, INVALID, "stride"),
            ("ldm below d", {LDM: 127}, INVALID, "stride"),
            ("ldc below d", {LDC: 127}, INVALID, "stride"),
            ("int8 rows", {DT: lib.I8}, INVALID, "dtype"),
            ("null operands", {}, INVALID, "null")):
        args = list(call)
        for pos, value in changes.items():
            args[pos] = value
        assert fn(*args) == status, what
        message = lib.lib().krs_last_error().decode()
        assert message.startswith("krs_retrieval_ivf"), what
        if names:
            assert names in message, (what, message)
    args = list(call)
    args[B] = 0
    assert fn(*args) == 0                                   # an empty batch: nothing is launched, nothing is read
    fake = 0x100000
    for missing in (0, 2, 4, 6, 7, 17):                     # each required pointer on its own
        args = list(call)
        for pos in (0, 2, 4, 6, 7, 17):
            args[pos] = None if pos == missing else fake
        assert fn(*args) == INVALID and "null" in lib.lib().krs_last_error().decode()
    args = list(call)
    for pos in (0, 2, 4, 6, 7, 17):
        args[pos] = fake
    assert fn(*args) == WORKSPACE                           # checked before the first launch
    args[19], args[20] = fake, 1                            # a workspace pointer with too few bytes
    assert fn(*args) == WORKSPACE


# ---- the layer: argument checks, from_partition, config ------------------------------------------------------------------
def _rows(n=60, d=8, seed=3):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def test_layer_argument_checks():
    import keras_rs_amd.layers as kl

    P = kl.PartitionedRetrieval
    assert issubclass(P, kl.Retrieval)
    for bad in ({"k": 0}, {"k": 129}, {"k": 2.5}, {"num_leaves": 0}, {"num_leaves": 1.5}, {"num_leaves": True},
                {"num_leaves_to_search": 0}, {"num_leaves_to_search": 129}, {"num_leaves": 4, "num_leaves_to_search": 5},
                {"training_iterations": -1}, {"training_iterations": 1.0}, {"seed": "a"}):
        with pytest.raises(ValueError, match=next(iter(bad)) if len(bad) == 1 else "num_leaves_to_search"):
            P(device="cpu", **bad)
    with pytest.raises(ValueError, match="without providing `candidate_embeddings`"):
        P(candidate_ids=np.arange(4), device="cpu")
    with pytest.raises(TypeError):
        P(device="cpu", leaves=3)
    layer = P(k=7, return_scores=False, num_leaves=16, num_leaves_to_search=3, training_iterations=2, seed=11,
              device="cpu", name="ivf")
    config = layer.get_config()
    assert config == {"name": "ivf", "trainable": True, "dtype": "float32", "k": 7, "return_scores": False,
                      "num_leaves": 16, "num_leaves_to_search": 3, "training_iterations": 2, "seed": 11}
    assert P.from_config(config).get_config() == config
    assert P(device="cpu").get_config()["num_leaves"] is None
    # the same messages as BruteForceRetrieval for a layer without candidates and for a wrong query shape
    brute = kl.BruteForceRetrieval(device="cpu")
    for empty in (layer, brute):
        with pytest.raises(ValueError, match="No candidates: call `update_candidates` before using the layer."):
            empty.call(np.zeros((2, 8), np.float32))
    with pytest.raises(NotImplementedError, match="K17"):
        layer.quantize("int8")
    # the defaults of the two leaf counts
    assert P(device="cpu")._leaves_for(10000) == 100 and P(device="cpu")._leaves_for(1) == 1
    with pytest.raises(ValueError, match="more than the number of candidates"):
        P(num_leaves=20, device="cpu")._leaves_for(10)
    # candidate checks come before any device work
    with pytest.raises(ValueError, match="less than the number of candidates to retrieve"):
        P(_rows(5), k=10, device="cpu")
    with pytest.raises(ValueError, match="rank 2"):
        P(np.zeros((5,), np.float32), k=1, device="cpu")
    with pytest.raises(ValueError, match="512"):
        P(np.zeros((20, 513), np.float32), k=1, device="cpu")
    with pytest.raises(ValueError, match="same number of rows"):
        P(_rows(20), candidate_ids=np.arange(19), k=1, device="cpu")


def test_from_partition_validates_and_lays_the_index_out():
    import torch

    import keras_rs_amd.layers as kl

    P = kl.PartitionedRetrieval
    rows, centroids = _rows(60), _rows(5, seed=4)
    assign = np.random.default_rng(6).integers(0, 5, size=60)
    assign[assign == 2] = 1                                             # an empty leaf
    for what, kwargs in (
            ("rank 2", {"centroids": centroids[0]}),
            ("columns", {"centroids": _rows(5, d=7)}),
            ("integers", {"assignments": assign.astype(np.float32)}),
            ("integers", {"assignments": assign[:59]}),
            ("integers", {"assignments": assign.reshape(60, 1)}),
            ("inside", {"assignments": np.where(np.arange(60) == 7, 5, assign)}),
            ("inside", {"assignments": np.where(np.arange(60) == 7, -1, assign)}),
            ("num_leaves", {"num_leaves": 6}),
            ("num_leaves_to_search", {"num_leaves_to_search": 6}),
            ("same number of rows", {"candidate_ids": np.arange(59)}),
            ("fit int32", {"candidate_ids": np.arange(60) + 2 ** 31}),
            ("less than the number of candidates", {"k": 61})):
        args = {"candidate_embeddings": rows, "centroids": centroids, "assignments": assign, "k": 5, "device": "cpu"}
        args.update(kwargs)
        with pytest.raises(ValueError, match=what):
            P.from_partition(**args)
    ids = (np.arange(60) * 2 + 100).astype(np.int64)
    layer = P.from_partition(rows, centroids, assign, candidate_ids=ids, k=5, num_leaves_to_search=2, device="cpu")
    assert layer.num_leaves == 5 and layer.probes() == 2 and layer.built
    row_index, offsets = RI.layout(assign, 5)
    assert (layer.row_index.numpy() == row_index).all() and (layer.leaf_offsets.numpy() == offsets).all()
    assert (layer.candidate_rows.numpy() == rows[row_index]).all()
    assert (layer.centroids.numpy() == centroids).all() and layer.candidate_ids.dtype == torch.int32
    assert (layer.candidate_ids.numpy() == ids).all()                   # ids stay in ORIGINAL order
    assert (layer.assignments.numpy() == assign).all()
    assert set(layer.state_dict()) == {"candidate_rows", "leaf_offsets", "row_index", "centroids", "candidate_ids"}
    assert layer.weights == []
    with pytest.raises(ValueError, match=r"The query must have shape \(batch, 8\)"):
        layer.call(np.zeros((2, 9), np.float32))
    # a saved index restores a fresh layer without training, whatever shapes it had
    fresh = P(k=5, num_leaves_to_search=2, device="cpu")
    fresh.load_state_dict(layer.state_dict())
    for name, saved in layer.state_dict().items():
        assert torch.equal(getattr(fresh, name), saved), name
    assert fresh.built and (fresh.assignments.numpy() == assign).all() and fresh.probes() == 2
    assert P.from_partition(rows, centroids, assign, k=5, device="cpu").probes() == 1      # max(1, 5 // 10)
