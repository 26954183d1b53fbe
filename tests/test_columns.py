"""Host logic of the reduced camera system's columns (tscm_calib_amd/csrc/tscm_columns.h: plan_columns), checked by
tests/native/columns_check.cpp on random problems planned with plan_layout -- 1 to 32 cameras and mono, cameras without views,
cameras whose pose is held -- under held-intrinsics masks (none, all held, DS, UCM, cx_cy, one per camera): the column
classes and the control step's classes of DESIGN 15, the compact numbering and its kernel-argument form, the contiguous
tables and k_solve_nd plans without a mask, monotonicity in the mask (what sizes Abig), and k_solve_reduced's operand map
read on operands tagged with their (row, column).  Built twice: plain, and under AddressSanitizer + UBSan.  No GPU."""
import pytest

from tests import native_check as N


pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("columns_check.cpp", "columns_check")


def test_header_is_plain_cpp17():
    N.assert_plain_cpp17("tscm_columns.h")


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_problems_every_mask(checker, seed):
    r = N.run(checker, "random", seed, 400)
    assert r["ok"], r
    # what the sample must have exercised: mono, rigs past the register solver, rigs of k_solve_reduced and of k_solve_nd,
    # cameras without views and with a held pose, blocks with holes, systems without a free column, right-hand side tiles
    assert r["plans"] == 400 * 6 and r["mono"] > 0 and r["big_rigs"] > 0 and r["dense4"] > 0 and r["nd"] > 0, r
    assert r["no_views"] > 0 and r["pose_held"] > 0 and r["holes"] > 0 and r["empty"] > 0 and r["rhs_tiles"] > 0, r
    # a mask never refuses where no mask succeeds (and no mask succeeded on every problem)
    assert r["refused"] == 0, r
