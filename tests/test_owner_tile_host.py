"""The layout that K13 - K15 and K19 share (keras_rs_amd/csrc/krs_owner_tile.h), without a GPU: the index arithmetic of
the header -- the swizzled tile image, the accumulator-row rule, the score chain's reads and the gather's -- walked by
tests/host/owner_tile_check.cpp under the sanitizers for every DPAD."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_owner_tile_layout_keeps_its_contract_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tests/host/owner_tile_check.cpp")
    exe = str(tmp_path / "owner_tile_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "owner_tile_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last.endswith(" 0 failed checks") and int(last.split()[0]) > 10000, last
