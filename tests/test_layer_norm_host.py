"""K22 without a GPU: the restatement against hand-computed rows and torch's own layer norm; the case table's coverage;
the host planner under the sanitizers, and the routes the table claims; the dropout hash; the bounds; the ABI table
and every refusal of the entry points (they come before the first launch, so NULL pointers do); the layers' host
logic."""

import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers, norm_ops
from tests import layer_norm_cases as T
from tests import layer_norm_restatement as R
from tests.test_capi_symbols import _header, header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in T.CASES]


# ---- (a) the restatement --------------------------------------------------------------------------------------------
def test_restatement_on_hand_computed_rows():
    # row (1, 2, 3, 6): mean 3, deviations (-2, -1, 0, 3), variance 14 / 4 = 3.5
    x = np.array([[1.0, 2.0, 3.0, 6.0]])
    f = R.forward(x, eps=0.5)
    assert f["mean"][0] == 3.0 and f["rstd"][0] == 0.5 and np.array_equal(f["y"], [[-1.0, -0.5, 0.0, 1.5]])
    f = R.forward(x - 1.0, np.ones((1, 4)), gamma=np.array([2.0, 0.0, 1.0, -2.0]), beta=np.array([0.0, 7.0, 1.0, 1.0]), eps=0.5)
    assert np.array_equal(f["s"], x) and np.array_equal(f["y"], [[-2.0, 7.0, 1.0, -2.0]])
    # backward by hand: xh = (-1, -.5, 0, 1.5), dy = (1, 0, 0, 0), gamma = 1: g = dy, mean g = .25, mean(g xh) = -.25
    # ds = rstd (g - .25 + .25 xh) = .5 (0.5, -.375, -.25, .125)
    f = R.forward(x, eps=0.5)
    g = R.backward(f["s"], f["mean"], f["rstd"], None, np.array([[1.0, 0.0, 0.0, 0.0]]), np.full((1, 4), 10.0))
    assert np.array_equal(g["dres"], [[10.25, 9.8125, 9.875, 10.0625]]) and np.array_equal(g["dx"], g["dres"])
    assert np.array_equal(g["dgamma"], [-1.0, 0.0, 0.0, 0.0]) and np.array_equal(g["dbeta"], [1.0, 0.0, 0.0, 0.0])
    # the add form: no statistics, dres = dsum, dx = dsum where kept
    a = R.forward(x, np.ones((1, 4)), eps=0.0, norm=False)
    assert set(a) == {"s"} and np.array_equal(a["s"], x + 1.0)
    kept = R.kept(3, 4, 1, 4, 0.5)
    g = R.backward(a["s"], None, None, None, None, np.full((1, 4), 3.0), p=0.5, seed=3, draw=4)
    assert np.array_equal(g["dres"], np.full((1, 4), 3.0)) and np.array_equal(g["dx"], np.where(kept, 6.0, 0.0))


@pytest.mark.parametrize("index", [i for i, c in enumerate(T.CASES) if c.form != "add" and c.n <= 65 and c.d <= 1024][::3])
def test_restatement_agrees_with_torch_layer_norm_in_float64(index):
    case = T.CASES[index]
    t, ref, _ = T.reference_of(index)
    s = torch.from_numpy(ref["s"].copy()).requires_grad_(True)
    w = [None if t[k] is None else torch.from_numpy(t[k].copy()).requires_grad_(True) for k in ("gamma", "beta")]
    y = torch.nn.functional.layer_norm(s, (case.d,), w[0], w[1], float(np.float32(case.eps)))
    assert np.abs(y.detach().numpy() - ref["y"]).max() <= 1e-9 * max(1.0, np.abs(ref["y"]).max())
    wanted = [s] + [v for v in w if v is not None]
    grads = torch.autograd.grad(y, wanted, torch.from_numpy(t["dy"]))
    ds = grads[0].numpy() + (0.0 if t["dsum"] is None else t["dsum"])
    scale = max(1.0, np.abs(ref["dres"]).max())
    assert np.abs(ds - ref["dres"]).max() <= 1e-9 * scale
    assert np.abs(ds * R.keep_factor(t["seed"], t["draw"], case.n, case.d, case.p) - ref["dx"]).max() <= 2e-9 * scale
    rest = list(grads[1:])
    if w[0] is not None:
        assert np.abs(rest.pop(0).numpy() - ref["dgamma"]).max() <= 1e-9 * max(1.0, np.abs(ref["dgamma"]).max())
    if w[1] is not None:
        assert np.abs(rest.pop(0).numpy() - ref["dbeta"]).max() <= 1e-9 * max(1.0, np.abs(ref["dbeta"]).max())


def test_the_table_is_the_stated_matrix():
    assert len(set(IDS)) == len(T.CASES) and all(c.n <= 257 for c in T.CASES)
    for dtype in ("bf16", "fp32"):
        own = [c for c in T.CASES if c.dtype == dtype]
        assert {c.n for c in own} == set(T.ROWS) and {c.d for c in own} == set(T.WIDTHS)
        assert {c.eps for c in own} == set(T.EPS) and {c.p for c in own} == {0.0, 0.2}
        # every route x form x dropout combination (the norm form has no dropout)
        want = {(r, f, p) for r in (T.VEC, T.ELEM) for f in T.FORMS for p in (0.0, 0.2)} - {(r, "norm", 0.2) for r in (1, 2)}
        assert want <= {(c.route, c.form, c.p) for c in own}
        # every kernel build: (route, registers a lane), and every lanes_per_row on both routes
        assert {(c.route, T.per_lane_of(c.d)) for c in own} == {(r, e) for r in (1, 2) for e in (8, 16, 32, 64)}
        assert {(c.route, c.lanes) for c in own} == {(r, l) for r in (1, 2) for l in (8, 16, 32, 64)}
        for form in ("norm", "addnorm"):
            assert {(c.gamma, c.beta) for c in own if c.form == form} == {(g, b) for g in (False, True) for b in (False, True)}
        assert {c.res for c in own if c.form == "addnorm"} == {False, True} == {c.res for c in own if c.form == "add"}
        assert any(c.pad and c.vec for c in own) and any(c.pad and not c.vec and c.d % 8 == 0 for c in own)
        assert any(c.pad and c.d % 2 for c in own) or any(c.pad % 2 for c in own)
        assert {c.special for c in own} == {"", "const", "gamma0"}
        assert any(c.n == 257 and c.d == d for c in own for d in (50, 4096))
    assert all(c.res is False and c.p == 0 for c in T.CASES if c.form == "norm")
    assert all(c.res or c.p > 0 for c in T.CASES if c.form != "norm")


def test_a_constant_row_gives_beta_exactly_and_finite_gradients():
    for index, case in enumerate(T.CASES):
        if case.special != "const":
            continue
        t, ref, _ = T.reference_of(index)
        got = T.rounded(case, t)
        want = np.zeros(case.d) if t["beta"] is None else t["beta"]
        for r, beta in ((ref, want), (got, R.round_to(want, case.dtype))):
            assert np.array_equal(r["s"][0], np.full(case.d, 1.5)) and np.array_equal(r["y"][0], beta)
            assert all(np.isfinite(v).all() for v in r.values())
        assert ref["rstd"][0] == 1.0 / math.sqrt(float(np.float32(case.eps)))


# ---- (b) the planner ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tests/host/ln_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("ln_plan") / "ln_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "ln_plan_check.cpp"),
                    "-o", exe], check=True)

    def ask(args):
        run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
        lines = run.stdout.strip().splitlines()
        assert "0 failed checks" in lines[-1]
        return lines[:-1]

    return ask


def test_the_planner_keeps_its_invariants_over_the_grid_under_the_sanitizers(planner):
    assert planner([]) == []


def test_the_claimed_routes_are_the_planners(planner):
    args = []
    for c in T.CASES:
        args += [c.n, c.d, 1 if c.dtype == "bf16" else 0, c.vec]
    lines = planner(args)
    assert len(lines) == len(T.CASES)
    several = 0
    for c, line in zip(T.CASES, lines):
        status, kernel, lanes, per_lane, vec, rows_per_pass, rows_per_group, groups, ws = map(int, line.split())
        assert (status, kernel, lanes, vec) == (0, c.route, c.lanes, c.vec), c.name
        assert per_lane == T.per_lane_of(c.d) and rows_per_pass == 256 // lanes == rows_per_group
        assert groups == math.ceil(c.n / rows_per_pass) and ws == math.ceil(groups * 2 * c.d * 4 / 256) * 256
        several += c.n == 257 and groups >= 5
    assert several >= 10                        # 257 rows: the weight-gradient partials span several workgroups


def test_the_workspace_formula_and_the_refusals_of_the_planner(planner):
    ask = lambda *a: list(map(int, planner(list(a))[0].split()))
    # 819200 rows of 64: 32 rows a pass, 2048 workgroups of 13 passes (the last ones short)
    assert ask(819200, 64, 1, 1) == [0, T.VEC, 8, 8, 1, 32, 416, 1970, 1970 * 2 * 64 * 4]
    assert ask(65536, 1024, 0, 0) == [0, T.ELEM, 64, 16, 0, 4, 32, 2048, 2048 * 2 * 1024 * 4]
    assert ask(0, 64, 1, 1)[:2] == [0, 0] and ask(0, 64, 1, 1)[-1] == 0
    assert ask(4, 4097, 1, 1)[:2] == [-2, 0] and ask(2 ** 31, 8, 1, 1)[:2] == [-2, 0] and ask(2 ** 31 - 1, 8, 1, 1)[0] == 0
    assert ask(-1, 8, 1, 1)[0] == -1 and ask(4, 0, 1, 1)[0] == -1 and ask(4, 8, 2, 1)[0] == -1


# ---- (c) the dropout hash -------------------------------------------------------------------------------------------
def test_the_hash_is_k19s_with_the_row_as_its_group(planner):
    seed, draw = 0x1234_5678_9ABC_DEF0, (7 << 32) + 5
    h = R.row_hash(seed, draw, 300, 70)
    points = [(0, 0), (5, 39), (257, 1), (299, 69)]
    args = []
    for i, j in points:
        args += ["hash", seed, draw, i, j]
    assert [int(x) for x in planner(args)] == [int(h[i, j]) for i, j in points]
    # written out once more, in plain Python integers
    def mix(x):
        x ^= x >> 16
        x = x * 0x7FEB352D & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ x >> 16
    i, j = points[1]
    base = mix(mix(mix(mix(mix((seed & 0xFFFFFFFF) ^ 0x9E3779B9) ^ (seed >> 32)) ^ (draw & 0xFFFFFFFF)) ^ (draw >> 32)) ^ i)
    assert int(h[i, j]) == mix((base + j) & 0xFFFFFFFF)


def test_the_hash_keeps_its_share_and_draws_are_independent():
    p, n = 0.2, 2 ** 16
    thr = R.drop_threshold(p)
    assert thr == math.floor(float(np.float32(p)) * 2 ** 32)
    pf = thr / 2 ** 32
    for rows, cols in ((2 ** 16, 1), (1024, 64), (16, 4096)):          # one column, a model's width, the widest row
        a, z = R.kept(99, 4, rows, cols, p), R.kept(99, 5, rows, cols, p)
        assert a.size == n
        assert abs(a.mean() - (1 - pf)) <= 5 * math.sqrt(pf * (1 - pf) / n)
        dif = 2 * pf * (1 - pf)
        assert abs((a != z).mean() - dif) <= 5 * math.sqrt(dif * (1 - dif) / n)
    kf = R.keep_factor(99, 4, 64, 64, p)
    assert set(np.unique(kf)) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}


# ---- (d) the bounds -------------------------------------------------------------------------------------------------
def test_c_is_twice_the_smallest_that_holds_the_rounding_restatement():
    worst, worst_s = 0.0, 0.0
    for index, case in enumerate(T.CASES):
        if case.dtype != "bf16":
            continue
        t, ref, _ = T.reference_of(index)
        got, bound = T.rounded(case, t), T.bounds(case, t, ref, c=1.0)
        scaled = {k: v for k, v in ref.items() if k != "s"}
        worst = max(worst, T.worst_ratio(got, scaled, bound)[0])
        worst_s = max(worst_s, T.worst_ratio(got, {"s": ref["s"]}, bound)[0])
    print(f"worst ratio of the rounding restatement at C = 1: {worst:.4f} (header: {T.OBSERVED_MAX}, C = {T.C}); s: {worst_s:.4f}")
    assert worst <= T.OBSERVED_MAX <= T.C / 2 <= 1.01 * T.OBSERVED_MAX
    assert worst_s <= 1.0


def test_fp32_cases_keep_the_standing_tolerance_and_the_restatement_meets_it():
    for index, case in enumerate(T.CASES):
        if case.dtype != "fp32":
            continue
        t, ref, bound = T.reference_of(index)
        assert T.FP32_TOL == 1e-5 and np.array_equal(bound["s"], 1e-5 + 1e-5 * np.abs(ref["s"]))
        if "dgamma" in ref:
            assert np.array_equal(bound["dgamma"], np.full(case.d, 1e-5 + 1e-5 * np.abs(ref["dgamma"]).max()))
        assert T.worst_ratio(T.rounded(case, t), ref, bound)[0] <= 1.0


@pytest.mark.parametrize("defect", ["draw", "no_mean_term", "no_xhat_term", "stats_of_x", "gamma_on_beta", "unscaled_keep"])
def test_the_bounds_would_not_hide_a_defect(defect):
    """Six mistakes a kernel could make, applied to the float64 reference: each leaves the bounds of every case it
    applies to."""
    applied = 0
    for index, case in enumerate(T.CASES):
        t, ref, bound = T.reference_of(index)
        n, d = case.n, case.d
        got = dict(ref)
        if defect == "draw" and case.p > 0 and n * d >= 64:
            bad = T._run(case, {**t, "draw": t["draw"] + 1}, None)
            got = bad
        elif defect in ("no_mean_term", "no_xhat_term") and case.form != "add" and d >= 7 and n >= 7 and not case.special:
            xh = (ref["s"] - ref["mean"][:, None]) * ref["rstd"][:, None]
            g = t["dy"] * (1.0 if t["gamma"] is None else t["gamma"])
            m1, m2 = g.mean(axis=1, keepdims=True), (g * xh).mean(axis=1, keepdims=True)
            ds = ref["rstd"][:, None] * (g - (0 if defect == "no_mean_term" else m1) - (0 if defect == "no_xhat_term" else xh * m2))
            got["dres"] = ds + (0.0 if t["dsum"] is None else t["dsum"])
        elif defect == "stats_of_x" and case.form == "addnorm" and case.res and d >= 7:
            got["mean"] = t["x"].mean(axis=1)
        elif defect == "gamma_on_beta" and case.form != "add" and case.gamma and case.beta and d >= 7 and not case.special:
            got["y"] = t["gamma"] * (ref["y"] - t["beta"]) / np.where(t["gamma"] == 0, 1.0, t["gamma"]) + t["gamma"] * t["beta"]
        elif defect == "unscaled_keep" and case.p > 0 and n * d >= 64:
            got["dx"] = ref["dres"] * R.kept(t["seed"], t["draw"], n, d, case.p)
        else:
            continue
        ratio, where = T.worst_ratio(got, ref, bound)
        assert ratio > 1.0, f"{defect} stays inside the bound of {case.name} (worst ratio {ratio:.3f} at {where})"
        applied += 1
    assert applied >= 10


# ---- (e) the ABI ----------------------------------------------------------------------------------------------------
LN_ENTRIES = ("krs_ln_workspace_bytes", "krs_ln_fwd", "krs_ln_bwd", "krs_ln_last_route")


def test_abi_prototypes_match_the_header():
    declared = header_prototypes(_header())
    for name in LN_ENTRIES:
        assert name in declared and name in L.PROTOTYPES, name
        restype, argtypes = L.PROTOTYPES[name]
        assert (restype, list(argtypes)) == (declared[name][0], list(declared[name][1])), name
    assert len(L.PROTOTYPES["krs_ln_fwd"][1]) == 20 and len(L.PROTOTYPES["krs_ln_bwd"][1]) == 24
    assert hasattr(L.lib(), "krs_ln_fwd") and (norm_ops.VEC, norm_ops.ELEM, norm_ops.MAX_D) == (1, 2, 4096)


def _fwd(**kw):
    a = dict(x=1, ldx=64, residual=None, ldr=0, gamma=None, beta=None, dtype=L.BF16, n=4, d=64, eps=1e-5, p=0.0, seed=0,
             draw=None, y=1, ldy=64, sum=None, lds=0, mean=None, rstd=None)
    a.update(kw)
    rc = L.lib().krs_ln_fwd(*a.values(), None)
    return rc, L.lib().krs_last_error().decode()


def _bwd(**kw):
    a = dict(s=1, lds=64, dy=1, lddy=64, dsum=None, lddsum=0, gamma=None, mean=1, rstd=1, dtype=L.BF16, n=4, d=64, p=0.0,
             seed=0, draw=None, dx=1, lddx=64, dres=None, lddres=0, dgamma=None, dbeta=None, ws=None, ws_bytes=0)
    a.update(kw)
    rc = L.lib().krs_ln_bwd(*a.values(), None)
    return rc, L.lib().krs_last_error().decode()


INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4


def test_status_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "krs.h")).read()
    for name, value in (("KRS_ERR_INVALID", INVALID), ("KRS_ERR_UNSUPPORTED", UNSUPPORTED), ("KRS_ERR_WORKSPACE", WORKSPACE)):
        assert f"{name} = {value}" in text, name


@pytest.mark.parametrize("kw, code, names", [
    (dict(n=-1), INVALID, "n >= 0"), (dict(d=0), INVALID, "d >= 1"), (dict(dtype=2), INVALID, "dtype"),
    (dict(p=1.0), INVALID, "dropout_p"), (dict(p=-0.1), INVALID, "dropout_p"), (dict(eps=-1.0), INVALID, "eps"),
    (dict(ldx=63), INVALID, "stride"), (dict(ldy=10), INVALID, "stride"), (dict(residual=1, ldr=8), INVALID, "stride"),
    (dict(sum=1, lds=63), INVALID, "stride"), (dict(x=None), INVALID, "null x"),
    (dict(y=None), INVALID, "no output"), (dict(y=None, sum=1, lds=64, mean=1), INVALID, "add form"),
    (dict(y=None, sum=1, lds=64, gamma=1), INVALID, "add form"), (dict(p=0.2), INVALID, "draw"),
    (dict(d=4097, ldx=4097, ldy=4097), UNSUPPORTED, "d <= 4096"), (dict(n=2 ** 31), UNSUPPORTED, "n <= 2^31 - 1"),
])
def test_forward_refusals_come_before_any_pointer_is_read(kw, code, names):
    rc, msg = _fwd(**kw)
    assert rc == code and names in msg and "krs_ln_fwd" in msg, (rc, msg)
    assert norm_ops.last_route() == (0, 0, 0)


@pytest.mark.parametrize("kw, code, names", [
    (dict(n=-1), INVALID, "n >= 0"), (dict(d=0), INVALID, "d >= 1"), (dict(dtype=-1), INVALID, "dtype"),
    (dict(p=1.5), INVALID, "dropout_p"), (dict(dx=None), INVALID, "no gradient"), (dict(lds=8), INVALID, "stride"),
    (dict(lddx=63), INVALID, "stride"), (dict(dsum=1, lddsum=1), INVALID, "stride"), (dict(dres=1, lddres=0), INVALID, "stride"),
    (dict(dy=None), INVALID, "no gradient arrives"), (dict(mean=None), INVALID, "needs s, mean and rstd"),
    (dict(s=None), INVALID, "needs s, mean and rstd"), (dict(dy=None, dsum=1, lddsum=64, dgamma=1), INVALID, "need dy"),
    (dict(p=0.2), INVALID, "draw"), (dict(dgamma=1), WORKSPACE, "workspace"),
    (dict(dbeta=1, ws=1, ws_bytes=511), WORKSPACE, "needs 512"),
    (dict(d=5000, lds=5000, lddy=5000, lddx=5000), UNSUPPORTED, "d <= 4096"), (dict(n=2 ** 31), UNSUPPORTED, "n <= 2^31 - 1"),
])
def test_backward_refusals_come_before_any_pointer_is_read(kw, code, names):
    rc, msg = _bwd(**kw)
    assert rc == code and names in msg and "krs_ln_bwd" in msg, (rc, msg)
    assert norm_ops.last_route() == (0, 0, 0)


def test_empty_calls_are_no_ops_and_the_workspace_entry_is_the_planners():
    assert _fwd(n=0, x=None, y=None)[0] == 0 and _bwd(n=0, s=None, dy=None, mean=None, rstd=None)[0] == 0
    assert norm_ops.last_route() == (0, 0, 0)
    ws = L.lib().krs_ln_workspace_bytes
    assert ws(0, 64) == 0 and ws(4, 5000) == 0 and ws(-1, 8) == 0 and ws(4, 64) == 512 and ws(257, 50) == 3840    # 9 workgroups x 2 x 50 x 4


# ---- (f) the Python op's and the layers' host logic -----------------------------------------------------------------
def test_the_op_refuses_what_the_kernel_would():
    x = torch.zeros(2, 3, 8)
    with pytest.raises(L.KrsError, match="no CPU fallback"):
        norm_ops.residual_layer_norm(x, epsilon=1e-5)
    assert not norm_ops.supported(x) and not norm_ops.supported(torch.zeros(2, 8, dtype=torch.float16))


def test_layer_normalization_arguments_config_and_weights():
    ln = layers.LayerNormalization(1e-8, device="cpu")
    ln.build((2, 7, 12))
    assert ln.epsilon == 1e-8 and [tuple(w.shape) for w in ln.weights] == [(12,), (12,)]
    assert ln.weights[0] is ln.gamma and ln.weights[1] is ln.beta and ln.gamma.dtype == ln.beta.dtype == torch.float32
    assert list(ln.state_dict()) == ["gamma", "beta"]
    assert torch.equal(ln.gamma, torch.ones(12)) and torch.equal(ln.beta, torch.zeros(12))
    for kw, names in ((dict(center=False), ["gamma"]), (dict(scale=False), ["beta"]), (dict(center=False, scale=False), [])):
        part = layers.LayerNormalization(device="cpu", **kw)
        part.build((3, 12))
        assert list(part.state_dict()) == names and len(part.weights) == len(names) and part.epsilon == 1e-3
        x = torch.randn(3, 12)
        want = torch.nn.functional.layer_norm(x, (12,), part.gamma, part.beta, 1e-3)
        assert torch.allclose(part(x), want)                        # (off the device: torch's arithmetic, as before)
    init = layers.LayerNormalization(gamma_initializer={"class_name": "Constant", "config": {"value": 2.0}},
                                     beta_initializer="ones", device="cpu")
    init.build((1, 4))
    assert torch.equal(init.gamma, torch.full((4,), 2.0)) and torch.equal(init.beta, torch.ones(4))
    cfg = init.get_config()
    assert layers.LayerNormalization.from_config(cfg).get_config() == cfg
    assert cfg["center"] is True and cfg["scale"] is True and cfg["epsilon"] == 1e-3
    with pytest.raises(TypeError):
        layers.LayerNormalization(1e-5, False)                      # center, scale are keyword-only
    with pytest.raises(NotImplementedError, match="axis"):
        layers.LayerNormalization(axis=1)
    with pytest.raises(NotImplementedError, match="rms_scaling"):
        layers.LayerNormalization(rms_scaling=True)
    assert layers.LayerNormalization(axis=-1, device="cpu").epsilon == 1e-3


def test_transformer_decoder_keeps_its_weights_and_gains_a_switch_and_a_counter():
    from keras_rs_amd.layers import sequence

    assert sequence.FUSE_NORM is True or os.environ.get("KRS_FUSE_NORM") == "0"
    dec = layers.TransformerDecoder(intermediate_dim=20, num_heads=2, dropout=0.1, normalize_first=True, seed=11, device="cpu")
    dec.build((2, 7, 12))
    shapes = [tuple(w.shape) for w in dec.weights]
    assert shapes == [(12, 2, 6), (2, 6)] * 3 + [(2, 6, 12), (12,)] + [(12,), (12,)] + [(12, 20), (20,), (20, 12), (12,)] \
        + [(12,), (12,)]
    assert not any("draw" in k for k in dec.state_dict())
    counter = dec.draw_counter()
    assert counter.dtype == torch.int64 and counter.numel() == 1 and counter is dec.draw_counter()
    assert counter is not dec.self_attention.draw_counter()
    assert sequence._ATTN_RESIDUAL_SEED != sequence._FF_RESIDUAL_SEED
    # off the device the block is the torch composition, as before
    x = torch.randn(2, 7, 12)
    assert isinstance(dec.self_attention_layer_norm, layers.LayerNormalization)
    with pytest.raises(L.KrsError):
        dec(x)
