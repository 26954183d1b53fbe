"""Host plan of the batched mono refinement (tscm_calib_amd/csrc/tscm_batch_plan.h): random batches of 1-300 problems with
0-2,000 views each, 9x6 and 11x8 boards and random masks are planned and checked by tests/native/batch_plan_check.cpp --
every view with corners is exactly one slot of its own problem, chunks tile each problem's slots and never span two
problems, a problem's plan is the same wherever it sits in the batch -- and the refusals come back with their codes.
Built twice: plain, and under AddressSanitizer + UBSan.  No GPU."""
import pytest

from tests import native_check as N

E_INVALID, E_UNSUPPORTED = -1, -5

pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("batch_plan_check.cpp", "batch_plan_check")


def test_header_is_plain_cpp17():
    N.assert_plain_cpp17("tscm_batch_plan.h")


@pytest.mark.parametrize("seed", [1, 2])
def test_random_batches(checker, seed):
    r = N.run(checker, "random", seed, 40)
    assert r["ok"], r
    # what the sample must have exercised: problems without corners, problems past 1,000 views, masks, several chunks per problem
    assert r["problems"] > 300 and r["empty"] > 0 and r["big"] > 0 and r["masked"] > 0 and r["multi_chunk"] > 0, r
    assert r["repeated"] > 0, r            # batches with a board seen twice, each refused


def test_refusals(checker):
    r = N.run(checker, "refusals")
    assert r == {
        "ok": 0, "zero_problems": E_INVALID, "null_problems": E_INVALID,
        "not_mono": E_UNSUPPORTED, "mono_two_cameras": E_INVALID, "rig": E_UNSUPPORTED,
        "board_points_differ": E_UNSUPPORTED, "board_xy_differ": E_UNSUPPORTED,
        "mask_bits": E_INVALID, "masks_ok": 0,
        "loss_kind": E_INVALID, "loss_scale": E_INVALID, "loss_ok": 0,
        "iterations": E_INVALID, "fp32": E_UNSUPPORTED, "exec_flags": E_UNSUPPORTED, "exec_flags_unknown": E_INVALID,
        "repeated_board": E_INVALID, "repeated_board_empty": 0,
    }
