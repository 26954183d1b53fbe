"""The trust-region step of the LM solver (tscm_calib_amd/csrc/tscm_ctrl.h: lm_step), the one copy behind every route of the
library, on the CPU: tests/native/ctrl_step_check.cpp drives it with scripted scalar sequences and compares the control
block and the log entry with Ceres' rules -- iteration 0, accepted steps (radius x 3, its cap, the cubic rule), rejected
and invalid steps, a non-finite cost, the history branch of the step quality and every exit.  Built twice: plain, and under
AddressSanitizer + UBSan.  No GPU."""
import json
import subprocess

import pytest

from tests import native_check as N

SCENARIOS = ["iteration_zero", "accepted_steps", "rejected_steps", "invalid_steps", "non_finite_cost", "history_branch", "exits"]

pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("ctrl_step_check.cpp", "ctrl_step_check")


def test_header_is_plain_cpp17():
    N.assert_plain_cpp17("tscm_ctrl.h")


def test_scripted_sequences(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    out = json.loads(r.stdout)
    assert r.returncode == 0 and out["ok"] == 1 and out["failures"] == [], (r.returncode, out, r.stderr[-2000:])
    assert out["scenarios"] == SCENARIOS and out["checks"] >= 50, out
