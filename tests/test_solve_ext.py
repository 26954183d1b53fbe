"""Host plan of the e-row and solution tiles of k_solve_reduced (tscm_calib_amd/csrc/tscm_columns.h: plan_solve_ext), with
which the camera step of rigs of up to four cameras falls out of the reduced system's factorisation, checked by
tests/native/solve_ext_check.cpp: rigs of 1..4 cameras, every subset of held poses, the six kinds of held-intrinsics masks
of columns_check -- one owner per tile, owners without an entry in solve_map and outside the look-ahead thread's wave, the
recorded wave sums against a recount, "fallback" exactly when the tiles do not fit -- and a plain-C++ emulation of the
blocked step over the planned tiles on Jacobi-scaled SPD systems of 7, 20, 41 and 46 columns against a long double solve:
the new path's forward error is at most twice the back-substitution path's on the same matrix (measured: 1.006 at most).
Built twice: plain, and under AddressSanitizer + UBSan.  No GPU."""
import pytest

from tests import native_check as N


pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("solve_ext_check.cpp", "solve_ext_check")


@pytest.mark.parametrize("seed", [1, 2])
def test_every_tile_has_one_owner_below_the_last_wave(checker, seed):
    r = N.run(checker, "plan", seed, 6)
    assert r["ok"], r
    # 1..4 cameras x every subset of held poses x 6 mask kinds, 6 rounds
    assert r["plans"] == 6 * 6 * (2 + 4 + 8 + 16), r
    # the sample reached the largest system (4 free cameras: 13 panels, the fallback), many panel counts, and planned tiles
    assert r["np_max"] == 13 and r["fallback"] >= 1 and r["np_seen"] >= 10 and r["ext"] > r["plans"] // 2 and r["tiles"] > 0, r


def test_emulated_step_against_long_double(checker):
    r = N.run(checker, "emulate")
    assert r["ok"], r
    assert r["worst_ratio"] <= 2.0, r
