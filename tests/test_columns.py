"""Host logic of the reduced camera system's columns (tscm_calib_amd/csrc/tscm_columns.h: plan_columns), checked by
tests/native/columns_check.cpp on random problems planned with plan_layout -- 1 to 32 cameras and mono, cameras without views,
cameras whose pose is held -- under held-intrinsics masks (none, all held, DS, UCM, cx_cy, one per camera): the column
classes and the control step's classes of DESIGN 15, the compact numbering and its kernel-argument form, the contiguous
tables and k_solve_nd plans without a mask, monotonicity in the mask (what sizes Abig), and k_solve_reduced's operand map
read on operands tagged with their (row, column).  Built twice: plain, and under AddressSanitizer + UBSan.  No GPU."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "columns_check.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def build(name, flags):
    exe = os.path.join(ROOT, "tmp", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def checker(request):
    if request.param == "plain":
        exe, r = build("columns_check", ["-O2"])
    else:
        exe, r = build("columns_check_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
        if r.returncode != 0 and "asan" in (r.stderr + r.stdout).lower():
            pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout)


def test_header_is_plain_cpp17():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "tscm_calib_amd", "csrc", "tscm_columns.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_problems_every_mask(checker, seed):
    r = run(checker, "random", seed, 400)
    assert r["ok"], r
    # what the sample must have exercised: mono, rigs past the register solver, rigs of k_solve_reduced and of k_solve_nd,
    # cameras without views and with a held pose, blocks with holes, systems without a free column, right-hand side tiles
    assert r["plans"] == 400 * 6 and r["mono"] > 0 and r["big_rigs"] > 0 and r["dense4"] > 0 and r["nd"] > 0, r
    assert r["no_views"] > 0 and r["pose_held"] > 0 and r["holes"] > 0 and r["empty"] > 0 and r["rhs_tiles"] > 0, r
    # a mask never refuses where no mask succeeds (and no mask succeeded on every problem)
    assert r["refused"] == 0, r
