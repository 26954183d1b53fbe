"""Host logic of solver creation (tscm_calib_amd/csrc/tscm_layout.h): the layout plan of one rank's share of a problem --
frame ownership, device view and board order, the Gram kernels' view chunks, the board-major record slots, the camera-pair
blocks of T, the Schur kernels' board chunks, fallback pairs and tile numbering -- checked on random problems for every rank
by tests/native/layout_check.cpp, which re-derives each invariant from the problem, and the refusals at the problem-size
limits, planned on view tables without observations.  Built twice: plain, and under AddressSanitizer + UBSan.  No GPU."""
import pytest

from tests import native_check as N

E_INVALID, E_UNSUPPORTED = -1, -5
TOO_LARGE = "problem too large for 32-bit buffer offsets (more than 3.7 M views or 536 M corners on one GPU)"

pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("layout_check.cpp", "layout_check")


def test_header_is_plain_cpp17():
    N.assert_plain_cpp17("tscm_layout.h")


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_problems_every_rank(checker, seed):
    r = N.run(checker, "random", seed, 250)
    assert r["ok"], r
    # what the sample must have exercised: several worlds, mono and rigs past the register solver, views without corners,
    # boards of more than three views (fallback pairs), full board chunks and Gram chunks of several views
    assert r["worlds"] >= 6 and r["mono"] > 0 and r["big_rigs"] > 0 and r["cams_max"] > 16, r
    assert r["empty_views"] > 0 and r["slow_boards"] > 0 and r["fallback_pairs"] > 0, r
    assert r["full_board_chunks"] > 0 and r["multi_view_chunks"] > 0, r


def test_refusals(checker):
    r = N.run(checker, "refusals")
    expect = {
        "duplicate_view": [E_INVALID, "two views with the same (camera, board)"],
        "duplicate_empty_view": [0, ""],
        "corners_at_limit": [0, ""],
        "corners_above_limit": [E_UNSUPPORTED, TOO_LARGE],
        "corners_2_31": [E_UNSUPPORTED, "more than 2^31 corners"],
        "views_at_limit": [0, ""],
        "views_above_limit": [E_UNSUPPORTED, TOO_LARGE],
        "null_problem": [E_INVALID, "problem is NULL"],
        "zero_points": [E_INVALID, "negative or zero problem dimensions"],
        "negative_boards": [E_INVALID, "negative or zero problem dimensions"],
        "mono_two_cameras": [E_INVALID, "mono problem needs exactly one camera"],
        "null_board_xy": [E_INVALID, "NULL parameter/board array"],
        "null_cam_rt": [E_INVALID, "NULL parameter/board array"],
        "null_obs": [E_INVALID, "NULL view/observation array"],
        "too_many_cameras": [E_UNSUPPORTED, "more than 32 cameras"],
        "camera_out_of_range": [E_INVALID, "view_camera out of range"],
        "board_out_of_range": [E_INVALID, "view_board out of range"],
        "count_above_points": [E_INVALID, "view_count outside [0, n_points]"],
        "negative_offset": [E_INVALID, "negative view_offset"],
        "valid": [0, ""],
    }
    assert r == expect
