"""The trust-region step of the LM solver (tscm_calib_amd/csrc/tscm_ctrl.h: lm_step), the one copy behind every route of the
library, on the CPU: tests/native/ctrl_step_check.cpp drives it with scripted scalar sequences and compares the control
block and the log entry with Ceres' rules -- iteration 0, accepted steps (radius x 3, its cap, the cubic rule), rejected
and invalid steps, a non-finite cost, the history branch of the step quality and every exit.  Built twice: plain, and under
AddressSanitizer + UBSan.  No GPU."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ctrl_step_check.cpp")
SCENARIOS = ["iteration_zero", "accepted_steps", "rejected_steps", "invalid_steps", "non_finite_cost", "history_branch", "exits"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def build(name, flags):
    exe = os.path.join(ROOT, "tmp", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def checker(request):
    if request.param == "plain":
        exe, r = build("ctrl_step_check", ["-O2"])
    else:
        exe, r = build("ctrl_step_check_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
        if r.returncode != 0 and "asan" in (r.stderr + r.stdout).lower():
            pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_header_is_plain_cpp17():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "tscm_calib_amd", "csrc", "tscm_ctrl.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_scripted_sequences(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    out = json.loads(r.stdout)
    assert r.returncode == 0 and out["ok"] == 1 and out["failures"] == [], (r.returncode, out, r.stderr[-2000:])
    assert out["scenarios"] == SCENARIOS and out["checks"] >= 50, out
