"""K25 without a GPU: the host planner (csrc/lstm_plan.h, through tests/host/lstm_plan_check.cpp under the sanitizers)
over u = 1 .. 1024 in both dtypes and at its refusals; krs_lstm_reserve_bytes against the planner; the float64
reference against torch.nn.LSTM and on its masked-step rule."""

import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from tests import lstm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST, GENERIC = 1, 2
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tests/host/lstm_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("lstm_plan") / "lstm_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "lstm_plan_check.cpp"),
                    "-o", exe], check=True)

    def ask(tuples):
        run = subprocess.run([exe] + [str(a) for t in tuples for a in t], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        return [line.split(None, 10) for line in run.stdout.splitlines()]

    return ask


@pytest.mark.parametrize("dtype", [L.F32, L.BF16], ids=["fp32", "bf16"])
def test_routes_upad_lds_and_reserve_over_every_u(planner, dtype):
    b, l = 65, 7
    lines = planner([(b, l, u, dtype) for u in range(1, 1025)])
    assert len(lines) == 1024
    build = __import__("keras_rs_amd.build", fromlist=["build"]).build
    build()
    lib = L.lib()
    for u, line in zip(range(1, 1025), lines):
        status, kernel, upad, rows, threads, groups, lds_fwd, lds_bwd, vgprs, reserve = map(int, line[:10])
        assert status == 0 and 0 < lds_fwd <= LDS_LIMIT and 0 < lds_bwd <= LDS_LIMIT, u
        if dtype == L.BF16 and u <= 128:
            want = 32 if u <= 32 else 64 if u <= 64 else 128
            assert (kernel, upad, rows, threads, groups) == (FAST, want, 32, 2 * want, 3), u
            # forward: U as [4 upad][upad] bf16 and two h tiles; backward: two da tiles [32][4 upad] bf16 and 32 ints in
            # LDS, this lane's half row of U (4 upad bf16 / 2) in registers -- at most half of a lane's 512
            assert lds_fwd == (4 * want + 64) * (2 * want + 16) and lds_bwd == 64 * (8 * want + 16) + 128, u
            assert vgprs == want <= 256 and (want < 128 or (lds_fwd, lds_bwd) == (156672, 66688)), u
        else:
            assert (kernel, upad, rows, threads, groups, vgprs) == (GENERIC, 0, 4, 256, 17, 0), u
            assert lds_fwd == 3 * 4 * u * 4 and lds_bwd == 6 * 4 * u * 4 + 16, u
        assert reserve == b * l * u * (16 if dtype == L.BF16 else 20) == lib.krs_lstm_reserve_bytes(b, l, u, dtype), u
    assert lib.krs_lstm_reserve_bytes(0, l, 8, dtype) == 0 and lib.krs_lstm_reserve_bytes(b, 0, 8, dtype) == 0


@pytest.mark.parametrize("args,status,word", [
    ((-1, 7, 8, 1), -1, "b >= 0"), ((3, -1, 8, 1), -1, "l >= 0"), ((3, 7, 0, 0), -1, "u >= 1"),
    ((3, 7, 8, 2), -1, "KRS_F32 or KRS_BF16"), ((3, 7, 1025, 1), -2, "u <= 1024"), ((3, 7, 1025, 0), -2, "u <= 1024"),
    ((3, 1 << 31, 8, 0), -2, "2^31 - 1"), ((1 << 34, 7, 8, 1), -2, "2^31 - 1"), ((0, 7, 8, 1), 0, None), ((3, 0, 8, 0), 0, None)])
def test_refusals_carry_their_messages_and_empty_calls_launch_nothing(planner, args, status, word):
    (line,) = planner([args])
    assert (int(line[0]), int(line[1]), int(line[5])) == (status, 0, 0)
    assert word is None or word in line[10]


@pytest.mark.parametrize("b,l,u,init", [(3, 5, 7, True), (2, 1, 4, False)])
def test_the_reference_agrees_with_torch_lstm_in_float64(b, l, u, init):
    rng = np.random.default_rng(u)
    xz, rk = rng.standard_normal((b, l, 4 * u)), rng.standard_normal((u, 4 * u)) / np.sqrt(u)
    h0, c0 = (rng.standard_normal((b, u)), rng.standard_normal((b, u))) if init else (None, None)
    dhs, dh, dc = rng.standard_normal((b, l, u)), rng.standard_normal((b, u)), rng.standard_normal((b, u))
    ref = R.lstm(xz, rk, None, h0, c0, dhs, dh, dc)
    # torch's gate order is i, f, g, o too; weight_ih = identity makes the input xz itself
    net = torch.nn.LSTM(4 * u, u, batch_first=True, bias=False).double()
    with torch.no_grad():
        net.weight_ih_l0.copy_(torch.eye(4 * u, dtype=torch.float64))
        net.weight_hh_l0.copy_(torch.from_numpy(rk.T.copy()))
    x = torch.from_numpy(xz).requires_grad_(True)
    s0 = [torch.from_numpy(np.zeros((b, u)) if s is None else s)[None].clone().requires_grad_(True) for s in (h0, c0)]
    out, (h, c) = net(x, tuple(s0))
    ((out * torch.from_numpy(dhs)).sum() + (h[0] * torch.from_numpy(dh)).sum() + (c[0] * torch.from_numpy(dc)).sum()).backward()
    got = {"hs": out, "h": h[0], "c": c[0], "dxz": x.grad, "dh0": s0[0].grad[0], "dc0": s0[1].grad[0],
           "drk": net.weight_hh_l0.grad.T}
    for key in R.OUTPUTS:
        assert np.abs(got[key].detach().numpy() - ref[key]).max() <= 1e-12 * max(1.0, np.abs(ref[key]).max()), key


def test_the_masked_step_rule_of_the_reference():
    rng = np.random.default_rng(1)
    b, l, u, keep = 2, 6, 4, [1, 3, 4]
    xz, rk = rng.standard_normal((b, l, 4 * u)), rng.standard_normal((u, 4 * u))
    h0, c0, dhs = rng.standard_normal((b, u)), rng.standard_normal((b, u)), rng.standard_normal((b, l, u))
    valid = np.array([[0, 1, 0, 1, 1, 0], [0, 0, 0, 0, 0, 0]], dtype=np.uint8)
    ref = R.lstm(xz, rk, valid, h0, c0, dhs, None, None)
    # row 0 is its three valid steps run alone: outputs repeated through the padding, zeros before the first valid step
    dense_dhs = np.stack([dhs[0, 1] + dhs[0, 2], dhs[0, 3], dhs[0, 4] + dhs[0, 5]])[None]
    alone = R.lstm(xz[:1, keep], rk, None, h0[:1], c0[:1], dense_dhs, None, None)
    assert not ref["hs"][0, 0].any() and np.allclose(ref["hs"][0, 1:], alone["hs"][0, [0, 0, 1, 2, 2]], atol=1e-14)
    assert np.allclose(ref["dxz"][0, keep], alone["dxz"][0], atol=1e-14) and not ref["dxz"][0, [0, 2, 5]].any()
    assert np.allclose(ref["dh0"][0], alone["dh0"][0], atol=1e-14) and np.allclose(ref["dc0"][0], alone["dc0"][0], atol=1e-14)
    # the all-padding row: zero outputs, both states carried, nothing flows
    assert not ref["hs"][1].any() and np.array_equal(ref["h"][1], h0[1]) and np.array_equal(ref["c"][1], c0[1])
    assert not ref["dxz"][1].any() and not ref["dh0"][1].any()
