"""Coverage of the krs_gemm route table (tests/gemm_route_cases.py), checked without a GPU: the expected route records,
which tests/test_gemm_routes_gpu.py asserts case by case on the device, name every kernel family, build, width, reduce
kernel and pipeline of keras_rs_amd/csrc/gemm.hip.  A case dropped from the table fails here, not silently."""

from tests.gemm_route_cases import ACT_FORMS, CASES, FORMS, leading_dims, split_geometry

TILE_KERNELS = ("mfma", "glds", "pp256", "pp64")


def _have(**want):
    """the cases whose fields / route fields equal `want`"""
    def ok(c):
        return all((getattr(c, k) if hasattr(c, k) else c.route[k]) == v for k, v in want.items())
    return [c for c in CASES if ok(c)]


def test_the_table_is_well_formed():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert set(c.route) == {"kernel", "splits", "reduce", "epilogue", "ep_vec", "thin_width", "thin_is_a"}, c.name
        assert (c.route["splits"] > 1) == (c.route["reduce"] is not None), c.name
        assert all(ld >= ext for ld, ext in zip(leading_dims(c)[2:], (c.n,) * 4)), c.name
        assert set(c.pad) <= set("abcxur") and set(c.off) <= {"a", "b", "c", "bias", "x0", "x", "u", "r"}, c.name
        if "u" in FORMS[c.ep]:       # (a kernel that confused ldu and ldx must read inside x0's allocation)
            assert leading_dims(c)[4] <= leading_dims(c)[3], c.name


def test_every_kernel_family_dtype_and_layout_is_expected_somewhere():
    built = {   # family -> (input dtypes, layouts) it is built for / reachable with
        "generic": (("bf16", "f32"), ("nn", "nt", "tn")),
        "mfma": (("bf16", "f32"), ("nn", "nt", "tn")),
        "glds": (("bf16", "f32"), ("nt",)),
        "tn_glds": (("bf16",), ("tn",)),
        "pp256": (("bf16",), ("nt",)),
        "pp256_kstrided": (("bf16",), ("tn",)),
        "pp64": (("bf16",), ("nt",)),
        "thin": (("bf16", "f32"), ("tn",)),
        "rowdot": (("bf16", "f32"), ("nn", "nt")),
        "smallk": (("bf16", "f32"), ("nn", "nt")),
    }
    missing = [(k, dt, lay) for k, (dts, lays) in built.items() for dt in dts for lay in lays
               if not _have(kernel=k, idt=dt, layout=lay)]
    assert missing == []
    assert {c.route["kernel"] for c in CASES} == set(built) | {None}
    # every bf16 product also with fp32 output (the ABI allows it on every route)
    assert [k for k in built if not _have(kernel=k, idt="bf16", odt="f32")] == []
    # fp32 output from bf16 input with a cross and with a residual epilogue
    assert [c for c in CASES if c.idt == "bf16" and c.odt == "f32" and "x0" in FORMS[c.ep]]
    assert [c for c in CASES if c.idt == "bf16" and c.odt == "f32" and "r" in FORMS[c.ep]]


def test_every_epilogue_build_and_store_path_of_the_tile_kernels():
    missing = [(k, e) for k in TILE_KERNELS for e in (0, 1, 2) if not _have(kernel=k, epilogue=e, splits=1)]
    missing += [(k, "ep_vec", v) for k in TILE_KERNELS for v in (True, False) if not _have(kernel=k, ep_vec=v, splits=1)]
    assert missing == []
    # partial tiles on both edges and an n that is not a multiple of 8, once per tile kernel that accepts such an n
    for k in TILE_KERNELS:
        assert [c for c in _have(kernel=k) if c.n % 8 and c.m % 256 and c.n % 256 and c.m % 128 and c.n % 128], k
    for k in ("tn_glds", "pp256_kstrided"):      # (these need m and n in whole vectors)
        assert [c for c in _have(kernel=k) if c.m % 128 and c.n % 128 and c.m % 256 and c.n % 256], k


def test_every_thin_width_on_both_sides_split_and_unsplit():
    missing = [(w, a, split) for w in (1, 4, 8, 16) for a in (True, False) for split in (True, False)
               if not [c for c in _have(kernel="thin", thin_width=w, thin_is_a=a) if (c.route["splits"] > 1) == split]]
    assert missing == []
    assert all(not c.ws for c in _have(kernel="thin", splits=1))      # the unsplit form: no workspace passed


def test_split_k_reaches_every_reduce_kernel_and_every_split_tile_kernel_with_a_short_last_split():
    def short_last(cases):
        return [c for c in cases if 0 < split_geometry(c)[1] < split_geometry(c)[0]]

    assert [r for r in ("scalar", "vec4", "vec8") if not short_last(_have(reduce=r))] == []
    split = [c for c in CASES if c.route["splits"] > 1]
    for k in ("tn_glds", "pp256_kstrided", "pp256", "pp64", "thin", "mfma"):
        assert short_last([c for c in split if c.route["kernel"] == k]), k
    # the split ring: 32-k blocks (K = 32 mod 64) on gemm_pp256_kernel, 64-k blocks on gemm_pp64_kernel
    assert [c for c in short_last(split) if c.route["kernel"] == "pp256" and c.layout == "nt" and c.k % 64 == 32]
    assert [c for c in short_last(split) if c.route["kernel"] == "pp64" and c.k % 64 == 0]
    # a NULL epilogue on a split product (what gemm_slab_reduce_vec4_kernel requires), and on an unsplit one
    assert all(c.ep == "null" for c in _have(reduce="vec4"))
    assert [c for c in CASES if c.ep == "null" and c.route["splits"] == 1 and c.route["kernel"]]


def test_pipelines_small_eligible_shapes_and_the_empty_products():
    ring = [c for c in CASES if c.layout == "nt" and c.idt == "bf16" and -(-c.m // 256) * -(-c.n // 256) >= 192]
    assert {c.pipe for c in ring} == {0, 4, 5}
    assert {c.route["kernel"] for c in ring if c.pipe == 4} == {"pp64"}
    assert {c.route["kernel"] for c in ring if c.pipe == 5} == {"pp256"}
    assert {c.route["kernel"] for c in ring if c.pipe == 0} <= {"mfma", "glds"}
    assert [c for c in _have(kernel="mfma", idt="f32") if max(c.m, c.n, c.k) <= 4]
    assert [c for c in _have(kernel="mfma", idt="bf16") if max(c.m, c.n, c.k) <= 8]
    assert [c for c in CASES if c.k == 0 and c.m and c.n and c.ep == "bias"]        # C = relu(bias)
    assert [c for c in CASES if c.m == 0 and c.route["kernel"] is None]


def test_the_argument_classes_the_layers_use_are_present():
    for key in "abcxur":                             # every leading dimension padded somewhere ...
        assert [c for c in CASES if c.pad.get(key)], key
    for key in ("a", "b", "c", "x0", "x", "r"):      # ... and every base pointer off 16 bytes somewhere
        assert [c for c in CASES if c.off.get(key)], key
    assert {c.ep for c in CASES} == set(FORMS)
    for v in (0.0, 0.5, 1.0, 2.0, -2.0):
        assert [c for c in CASES if c.diag == v and "x0" in FORMS[c.ep]], ("diag_scale", v)
        assert [c for c in CASES if c.beta == v and "r" in FORMS[c.ep]], ("beta", v)
    assert set(ACT_FORMS) <= set(FORMS)
