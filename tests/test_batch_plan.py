"""Host plan of the batched mono refinement (tscm_calib_amd/csrc/tscm_batch_plan.h): random batches of 1-300 problems with
0-2,000 views each, 9x6 and 11x8 boards and random masks are planned and checked by tests/native/batch_plan_check.cpp --
every view with corners is exactly one slot of its own problem, chunks tile each problem's slots and never span two
problems, a problem's plan is the same wherever it sits in the batch -- and the refusals come back with their codes.
Built twice: plain, and under AddressSanitizer + UBSan.  No GPU."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "batch_plan_check.cpp")
E_INVALID, E_UNSUPPORTED = -1, -5

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def build(name, flags):
    exe = os.path.join(ROOT, "tmp", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def checker(request):
    if request.param == "plain":
        exe, r = build("batch_plan_check", ["-O2"])
    else:
        exe, r = build("batch_plan_check_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
        if r.returncode != 0 and "asan" in (r.stderr + r.stdout).lower():
            pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout)


def test_header_is_plain_cpp17():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "tscm_calib_amd", "csrc", "tscm_batch_plan.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("seed", [1, 2])
def test_random_batches(checker, seed):
    r = run(checker, "random", seed, 40)
    assert r["ok"], r
    # what the sample must have exercised: problems without corners, problems past 1,000 views, masks, several chunks per problem
    assert r["problems"] > 300 and r["empty"] > 0 and r["big"] > 0 and r["masked"] > 0 and r["multi_chunk"] > 0, r
    assert r["repeated"] > 0, r            # batches with a board seen twice, each refused


def test_refusals(checker):
    r = run(checker, "refusals")
    assert r == {
        "ok": 0, "zero_problems": E_INVALID, "null_problems": E_INVALID,
        "not_mono": E_UNSUPPORTED, "mono_two_cameras": E_INVALID, "rig": E_UNSUPPORTED,
        "board_points_differ": E_UNSUPPORTED, "board_xy_differ": E_UNSUPPORTED,
        "mask_bits": E_INVALID, "masks_ok": 0,
        "loss_kind": E_INVALID, "loss_scale": E_INVALID, "loss_ok": 0,
        "iterations": E_INVALID, "fp32": E_UNSUPPORTED, "exec_flags": E_UNSUPPORTED, "exec_flags_unknown": E_INVALID,
        "repeated_board": E_INVALID, "repeated_board_empty": 0,
    }
