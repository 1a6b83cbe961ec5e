"""K16 (int8 row-quantized tables) checked without a GPU: the case table of tests/embed_q8_cases.py is well formed and names
every kernel instantiation the planner can name; the planner (keras_rs_amd/csrc/embed_fwd_q8_plan.h through
krs_embed_bag_fwd_q8_plan_route, which launches nothing) gives every case its expected route and every refusal its status
with an all-zero record; the lookup evaluated in plain fp32 stays inside the bound the GPU test holds the kernels to; the
restated quantizer keeps its three properties; the layers' quantize() refusals come before any device work; and the
planner's invariants are walked by a stand-alone program built with the sanitizers
(tests/host/embed_fwd_q8_plan_check.cpp).  tests/test_embed_q8_gpu.py asserts the same records against what ran."""

import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import embed_q8_restatement as Q
from tests.embed_q8_cases import (BAD, BY_NAME, CASES, ES, GENERIC_DIMS, LARGEST, LPRS, OUTS, R, VEC_DIMS, VOCABS, inputs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1


def _have(pred=lambda c: True, **want):
    def ok(c):
        return all((getattr(c, k) if hasattr(c, k) and k != "route" else c.route[k]) == v for k, v in want.items()) and pred(c)
    return [c for c in CASES if ok(c)]


def _slot_offsets(c):
    return {(col * ES[c.odt]) % 16 for col in c.out_cols}


def test_the_table_is_well_formed_and_covers_every_instantiation():
    assert len({c.name for c in CASES}) == len(CASES) and LARGEST in BY_NAME
    for c in CASES:
        assert set(c.route) == set(R(None)) and c.route["table_dtype"] == "i8", c.name
        assert c.batch in (1, 5, 67) and c.n_feats in (1, 3) and max(t for t, _ in c.feats) <= 1, c.name
        assert c.lead >= 1 and c.gap >= 1 and c.tail >= 1 and c.width > c.n_feats * c.dim, c.name
        assert c.width * c.batch * 4 <= 4 << 20 and c.nnz * c.dim <= 4 << 20, c.name
        assert not c.bad or c.bad == BAD, c.name
    assert 37 <= min(VOCABS) and max(VOCABS) <= 300
    # embed_bag_fwd_q8_vec<OT, LPR, HAS_W>: 2 x 4 x 2 = 16, and both output types of the generic kernel
    missing = [(o, lpr, w) for o, lpr, w in itertools.product(OUTS, LPRS, (False, True))
               if not _have(kernel="vec", odt=o, lpr=lpr, has_w=w)]
    assert missing == []
    assert {c.route["kernel"] for c in CASES} == {"vec", "generic"}
    # the dims of both paths; on the vector path one that leaves lanes idle and one that fills the group
    assert {c.dim for c in _have(kernel="vec")} >= {16, 48, 128, 1024} | {d for ds in VEC_DIMS.values() for d in ds}
    for lpr, dims in VEC_DIMS.items():
        assert all(d % 16 == 0 and (lpr // 2 if lpr > 8 else 0) < d // 16 <= lpr for d in dims) and dims[-1] == 16 * lpr
    for o, csr in itertools.product(OUTS, (False, True)):
        assert {c.dim for c in _have(lambda c: c.csr == csr, kernel="generic", odt=o)} >= set(GENERIC_DIMS), (o, csr)
    for k in ("vec", "generic"):
        got = _have(kernel=k)
        assert {c.batch for c in got} == {1, 5, 67} and {c.n_feats for c in got} == {1, 3}, k
        assert {c.weights for c in got} == {None, "uniform", "mixed"}, k
        assert {(c.id64, bool(c.bad)) for c in got} >= {(False, True), (True, True), (False, False), (True, False)}, k
        assert {c.off64 for c in got if c.csr} == {False, True}, k
        assert [c for c in got if _slot_offsets(c) == {0}] and [c for c in got if _slot_offsets(c) - {0}], k
    assert {h for c in CASES if c.hots for h in c.hots} >= {1, 2, 33}
    for o in OUTS:      # the element-store branch of the pooled kernel, and a pure-gather call, per output type
        assert [c for c in _have(kernel="vec", odt=o) if _slot_offsets(c) - {0}]
        assert _have(kernel="vec", odt=o, hots=(1, 1, 1), weights=None)
    # CSR edges: a first and a last empty bag, one bag of 200 lookups that crosses the id window (8 * LPR ids)
    edges = _have(lambda c: c.name.startswith("csr-edges"))
    assert {c.route["lpr"] for c in edges} == {8, 16}
    for c in edges:
        assert c.lens[0] == 0 and c.lens[-1] == 0 and 200 in c.lens and 200 > 8 * c.route["lpr"]
    # zero denominators on both kernels: mean bags whose weights cancel, sqrtn bags of all-zero weights
    for k in ("vec", "generic"):
        assert _have(lambda c: c.name.startswith("den0"), kernel=k, weights="mixed", hots=(2, 2, 2))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_inputs_of_every_case_are_what_the_case_says(case):
    c, h = case, inputs(case.name)
    ids = h["ids"].astype(np.int64)
    assert h["ids"].dtype == (np.int64 if c.id64 else np.int32) and ids.shape[0] == c.nnz
    assert (h["offsets"] is None) == (not c.csr) and (h["weights"] is None) == (c.weights is None)
    if c.csr:
        assert h["offsets"].dtype == (np.int64 if c.off64 else np.int32) and h["offsets"][-1] == c.nnz
    start, end = Q.RS.bag_bounds(c.n_feats, c.batch, c.hots, h["offsets"])
    vocab = np.repeat(np.array([VOCABS[t] for t, _ in c.feats]).repeat(c.batch), end - start)
    valid = (ids >= 0) & (ids < vocab)
    planted = {"vocab" if v == vocab[i] else int(v) for i, v in enumerate(ids) if not valid[i]}
    assert planted == set(c.bad) and valid.any() and (ids[valid] != 0).all()
    for q, s, v in zip(h["q_tables"], h["steps"], VOCABS):
        assert q.shape == (v, c.dim) and q.dtype == np.int8 and s.shape == (v,) and s.dtype == np.float32
        assert (q[1] == -128).all() and (q[2] == 127).all() and np.isnan(s[0]) and np.isfinite(s[1:]).all()
        assert s[1:].min() < 2e-6 and s[1:].max() > 5.0
        if c.dim >= 16:      # the 16 bytes of a piece all differ; about half of the table's bytes are negative
            assert all(len(set(q[r, :16].tolist())) == 16 for r in range(3, v))
            assert 0.4 <= float((q[3:] < 0).mean()) <= 0.6


@pytest.fixture(scope="module")
def lib():
    from keras_rs_amd import _lib as L
    from keras_rs_amd.build import build

    build()
    return L


def _dt(L, name):
    return L.F32 if name == "f32" else L.BF16


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_planner_gives_every_case_its_expected_route(lib, case):
    from keras_rs_amd import embedding_ops as E

    c = case
    got = E.embed_fwd_q8_plan_route(c.n_feats, 0x200000 if c.csr else None, 0x300000 if c.weights else None, c.nnz, c.batch,
                                    c.dim, 0x100000, _dt(lib, c.odt), c.width)
    assert got == dict(c.route, status=0)


def test_block_counts_at_known_shapes_and_refusals(lib):
    import ctypes as C

    from keras_rs_amd import embedding_ops as E

    ok = dict(n_feats=2, offsets=None, weights=None, nnz=600, batch=100, dim=128, out=0x100000, out_dtype=lib.BF16, out_ld=256)
    # mean 3 -> 10 bags per group, 8 groups per wave: ceil(100 / 80) = 2 waves x 2 features = 4 -> 1 workgroup
    assert E.embed_fwd_q8_plan_route(**ok) == dict(R("vec", "bf16", 8, bpg=10, blocks=1), status=0)
    # the C3 shape: 26 features, batch 16384, one lookup per bag stays on the pooled kernel (there is no gather kernel)
    assert E.embed_fwd_q8_plan_route(**dict(ok, n_feats=26, batch=16384, nnz=26 * 16384)) == dict(
        R("vec", "bf16", 8, bpg=16, blocks=832), status=0)
    assert E.embed_fwd_q8_plan_route(**dict(ok, dim=6)) == dict(R("generic", "bf16", 8, blocks=7), status=0)
    assert E.embed_fwd_q8_plan_route(**dict(ok, dim=1040))["kernel"] == "generic"
    assert E.embed_fwd_q8_plan_route(**dict(ok, dim=1024)) == dict(R("vec", "bf16", 64, bpg=10, blocks=5), status=0)
    assert E.embed_fwd_q8_plan_route(**dict(ok, weights=0x10))["has_w"]
    assert E.embed_fwd_q8_plan_route(**dict(ok, n_feats=0)) == dict(R(None), status=0)
    assert E.embed_fwd_q8_plan_route(**dict(ok, batch=0)) == dict(R(None), status=0)
    INVALID, UNSUPPORTED = -1, -2
    refused = [
        ("int8 output", dict(out_dtype=lib.I8), INVALID), ("bad output dtype", dict(out_dtype=-1), INVALID),
        ("negative batch", dict(batch=-1), INVALID), ("negative features", dict(n_feats=-1), INVALID),
        ("negative nnz", dict(nnz=-1), INVALID), ("dim 0", dict(dim=0), INVALID), ("negative dim", dict(dim=-16), INVALID),
        ("null out", dict(out=None), INVALID),
        ("batch beyond INT_MAX - 128", dict(batch=INT_MAX - 127, nnz=0), UNSUPPORTED),
        ("batch INT_MAX", dict(batch=INT_MAX, n_feats=1, nnz=INT_MAX), UNSUPPORTED),
        # generic kernel at lpr 64: four bags per workgroup, 5 x (2^31 - 200) bags need more than 2^31 - 1 workgroups
        ("grid too large", dict(n_feats=5, batch=INT_MAX - 199, dim=1040, nnz=0), UNSUPPORTED),
    ]
    before = E.embed_fwd_q8_last_route()
    for what, change, status in refused:
        assert E.embed_fwd_q8_plan_route(**dict(ok, **change)) == dict(R(None), status=status), what
        assert lib.lib().krs_last_error(), what
    assert E.embed_fwd_q8_plan_route(**dict(ok, batch=INT_MAX - 128, nnz=0))["status"] == 0
    edge = E.embed_fwd_q8_plan_route(**dict(ok, n_feats=4, batch=INT_MAX - 128, dim=1040, nnz=0))
    assert edge["status"] == 0 and edge["blocks"] == INT_MAX - 128
    assert E.embed_fwd_q8_last_route() == before            # (the query does not touch the record of the last call)
    # the entries' own refusals come before any launch, so they can be made here; each leaves an all-zero record
    fake = 0x100000
    call = [fake, fake, 2, fake, lib.I32, None, lib.I32, None, 600, 100, 128, fake, lib.BF16, 256, None, None]
    for what, pos, value, status in (("bad id type", 4, 2, INVALID), ("bad offset type", 6, -1, INVALID),
                                     ("null ids", 3, None, INVALID), ("null tables", 0, None, INVALID),
                                     ("null feats", 1, None, INVALID), ("bad dtype", 12, lib.I8, INVALID),
                                     ("dim 0", 10, 0, INVALID), ("batch beyond INT_MAX - 128", 9, INT_MAX - 100, UNSUPPORTED)):
        args = list(call)
        args[pos] = value
        assert lib.lib().krs_embed_bag_fwd_q8(*args) == status, what
        assert E.embed_fwd_q8_last_route() == R(None), what
        assert lib.lib().krs_embed_bag_fwd_q8_last_route(None) == 0          # (the pointer is optional)
    args = list(call)
    args[9] = 0
    assert lib.lib().krs_embed_bag_fwd_q8(*args) == 0 and E.embed_fwd_q8_last_route() == R(None)      # an empty call
    qcall = [fake, lib.F32, 10, 16, fake, fake, None, None]
    for what, pos, value, status in (("null table", 0, None, INVALID), ("null q", 4, None, INVALID),
                                     ("null step", 5, None, INVALID), ("int8 source", 1, lib.I8, INVALID),
                                     ("dim 0", 3, 0, INVALID), ("negative vocab", 2, -1, INVALID),
                                     ("more than INT32_MAX rows", 2, INT_MAX + 1, UNSUPPORTED)):
        args = list(qcall)
        args[pos] = value
        assert lib.lib().krs_quantize_rows_q8(*args) == status, what
    args = list(qcall)
    args[2] = 0
    assert lib.lib().krs_quantize_rows_q8(*args) == 0                       # an empty table: nothing is launched
    assert C.sizeof(lib.EmbedFwdRoute()) == 40 and lib.TABLE_DT.itemsize == 32 and lib.I8 == 2 and lib.FLAG_NONFINITE_ROW == 8


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_lookup_evaluated_in_fp32_stays_inside_the_bound(case):
    import torch

    c, h = case, inputs(case.name)
    args = (h["q_tables"], h["steps"], c.feats, c.batch, c.dim, h["ids"])
    kw = dict(hots=c.hots, offsets=h["offsets"], weights=h["weights"])
    ref = Q.restate(*args, **kw)
    out32 = Q.evaluate_fp32(*args, **kw)
    assert ref["bad"] == bool(c.bad)
    assert np.isfinite(ref["out"]).all() and np.isfinite(out32).all()          # step[0] = NaN is never looked up
    if c.odt == "bf16":
        out32 = torch.from_numpy(out32).to(torch.bfloat16).float().numpy()
    zero = ref["den"] == 0
    assert (ref["out"][zero] == 0).all() and (out32[zero] == 0).all()
    if c.name.startswith("den0"):      # mean bags whose weights cancel, sqrtn bags whose weights are all zero
        comb = ref["comb"]
        assert zero[comb == Q.MEAN].any() and zero[comb == Q.SQRTN].any() and not zero[comb == Q.SUM].any()
        assert (~zero)[comb == Q.MEAN].any()
    err, tol = np.abs(out32 - ref["out"]), Q.bound(ref, c.odt == "bf16")
    assert (err[~zero] <= tol[~zero]).all(), float((err[~zero] / np.maximum(tol[~zero], 1e-300)).max())


# ---- the restated quantizer ----------------------------------------------------------------------------------------------

def _quantizer_tables():
    rng = np.random.default_rng(16)
    tables = []
    for dim in (1, 16, 20, 128, 1040):
        x = (rng.standard_normal((67, dim)) * np.logspace(-8, 6, 67)[:, None]).astype(np.float32)
        x[3] = 0
        x[4] = -np.abs(x[4]) - np.float32(1e-3)
        x[5] = np.float32(2) ** -140                     # an fp32 subnormal row
        x[6] = np.finfo(np.float32).max
        tables.append(x)
    return tables


@pytest.mark.parametrize("x", _quantizer_tables(), ids=lambda x: f"d{x.shape[1]}")
def test_the_restated_quantizer_keeps_its_properties(x):
    q, step, bad = Q.quantize(x)
    assert q.dtype == np.int8 and step.dtype == np.float32 and not bad.any()
    assert np.abs(q.astype(np.int32)).max() <= 127
    # max |q| == 127 on every finite row whose abs-max a is not tiny: the largest element maps to 127 a / (a + 1e-7), which
    # rounds to 127 once 127e-7 / (a + 1e-7) < 0.5, i.e. a > 2.53e-5 (2^-15 leaves room for the roundings).  Below that the
    # 1e-7 of the divisor shows: the row's largest |q| is that quotient rounded, 0 for an all-zero row.
    a = np.abs(x).max(axis=1).astype(np.float64)
    top = np.abs(q.astype(np.int32)).max(axis=1)
    big = a >= 2.0 ** -15
    assert big.sum() >= 40 and (top[big] == 127).all()
    small = ~big
    assert small.sum() >= 5 and (np.abs(top[small] - 127 * a[small] / (a[small] + 1e-7)) <= 0.5 + 1e-3).all()
    assert (q[3] == 0).all() and step[3] == np.float32(1e-7) / np.float32(127)
    assert q[4].min() == -127 and (q[4] <= 0).all()          # a row whose largest element is negative
    # |x - q * step| <= step * (0.5 + 2^-14): rint contributes 0.5; the two roundings of x * inv and the mismatch of
    # inv * step from 1 contribute at most 127 * 4 * 2^-24 < 2^-15, doubled
    err = np.abs(x.astype(np.float64) - Q.dequantized(q, step))
    assert (err <= step.astype(np.float64)[:, None] * (0.5 + 2.0 ** -14)).all()


def test_the_restated_quantizer_on_ties_and_nonfinite_rows():
    x = np.zeros((5, 6), np.float32)
    x[0] = [127, 0.5, 1.5, 2.5, -0.5, -1.5]
    x[1] = [1, 2, np.nan, 4, 5, 6]
    x[2] = [3, -1, 2, 0.5, 0, 1]
    x[3] = [1, np.inf, 3, 4, 5, 6]
    x[4] = [-8, 1, 2, 3, 4, 5]
    q, step, bad = Q.quantize(x)
    assert np.float32(127) + np.float32(1e-7) == np.float32(127)              # inv == 1 on the tie row
    assert q[0].tolist() == [127, 0, 2, 2, 0, -2] and step[0] == np.float32(1)
    assert bad.tolist() == [False, True, False, True, False]
    assert (q[[1, 3]] == 0).all() and (step[[1, 3]] == 0).all()
    assert q[2].tolist() == [127, -42, 85, 21, 0, 42] and q[4, 0] == -127 and step[4] > 0


# ---- the layers refuse before any device work ------------------------------------------------------------------------------

def test_every_refusal_of_the_layer_methods_comes_before_any_device_work():
    """On a machine without a GPU any device work raises KrsError (a RuntimeError whose text names the missing GPU or
    library): the refusals below must be the layers' own, raised first."""
    import keras_rs_amd.layers as kl
    from keras_rs_amd import _lib as L

    def own(exc_info):
        assert not isinstance(exc_info.value, L.KrsError), exc_info.value

    for layer in (kl.EmbedReduce(10, 4, device="cpu"), kl.Embedding(10, 4, device="cpu")):
        with pytest.raises(ValueError, match="int8"):
            layer.quantize("int4")
        with pytest.raises(RuntimeError, match="not built") as e:
            layer.quantize("int8")
        own(e)
        layer.build()
        with pytest.raises(ValueError, match="int8"):
            layer.quantize("float8")
        layer.quantization_mode = "int8"           # (as after a first call)
        with pytest.raises(RuntimeError, match="already quantized") as e:
            layer.quantize("int8")
        own(e)
    tc = kl.TableConfig("t", 10, 4, placement="default_device", optimizer="sgd", combiner="sum")
    de = kl.DistributedEmbedding({"a": kl.FeatureConfig("a", tc, (2,), (2, 4))}, device="cpu")
    with pytest.raises(ValueError, match="int8"):
        de.quantize("int4")
    with pytest.raises(RuntimeError, match="not built") as e:
        de.quantize("int8")
    own(e)
    with pytest.raises(RuntimeError, match="not quantized") as e:
        de.get_quantized_tables()
    own(e)
    de.build(None)
    de.quantization_mode = "int8"
    with pytest.raises(RuntimeError, match="already quantized") as e:
        de.quantize("int8")
    own(e)
    with pytest.raises(RuntimeError, match="training=True") as e:
        de({"a": np.zeros(2, np.int32)}, training=True)
    own(e)
    with pytest.raises(RuntimeError, match="cannot be set") as e:
        de.set_embedding_tables({"t": np.zeros((10, 4), np.float32)})
    own(e)


def test_a_dtype_cast_keeps_the_steps_fp32_and_an_empty_table_is_refused():
    """Module.half() / .bfloat16() on a quantized layer: the int8 rows are no floating tensor and stay, the step buffer
    keeps its fp32 bits (the kernel reads fp32; a cast would also round the steps).  Needs no device: the buffers are
    planted as quantize() leaves them.  QuantizedBags refuses a table without rows before it looks at the device: the
    kernels read row 0 and step[0] as the stand-in of an invalid slot."""
    import torch

    import keras_rs_amd.layers as kl
    from keras_rs_amd import _lib as L
    from keras_rs_amd import embedding_ops as E

    layer = kl.EmbedReduce(10, 4, device="cpu")
    layer.build()
    layer.embeddings = None
    layer.register_buffer("embeddings_q", torch.arange(40, dtype=torch.int8).reshape(10, 4))
    layer.register_buffer("embeddings_step", torch.rand(10) + 1e-3)
    layer.quantization_mode = "int8"
    steps = layer.embeddings_step.clone()
    for cast in (layer.half, layer.bfloat16, layer.double, layer.float):
        cast()
        assert layer.embeddings_step.dtype == torch.float32 and torch.equal(layer.embeddings_step, steps)
        assert layer.embeddings_q.dtype == torch.int8
    tc = kl.TableConfig("t", 10, 4, placement="default_device", optimizer="sgd", combiner="sum")
    de = kl.DistributedEmbedding({"a": kl.FeatureConfig("a", tc, (2,), (2, 4))}, device="cpu")
    de.register_buffer("default_device_t_step", steps.clone())
    de.quantization_mode = "int8"
    de.half()
    assert de.default_device_t_step.dtype == torch.float32 and torch.equal(de.default_device_t_step, steps)
    with pytest.raises(L.KrsError, match="at least one row"):
        E.QuantizedBags([torch.zeros((0, 16), dtype=torch.int8)], [torch.zeros(0)], [(0, "sum", 0)])


def test_the_planner_header_compiles_without_hip_and_keeps_its_invariants_under_the_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "embed_fwd_q8_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "embed_fwd_q8_plan_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "0 failed checks" in run.stdout
