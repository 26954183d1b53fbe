"""The one definition of the chessboard structure recovery (tscm_calib_amd/csrc/tscm_boards_core.h) on the CPU, outside the
library: tests/native/boards_core_check.cpp runs its serial instantiation -- per-seed jobs, overlap resolution, turn -- on
candidate sets it generates itself, with workspaces of exactly the sizes the header states.  Built twice, plain and under
AddressSanitizer + UBSan; both builds print the same checksum over every record and board, and the boards of the sets the
program prints are those of the library's host call.  No GPU."""
import numpy as np
import pytest

from tests import native_check as N
from tscm_calib_amd import corners

pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("boards_core_check.cpp", "boards_core_check")
N_SETS = 120
_seen = {}


def test_header_is_plain_cpp17():
    N.assert_plain_cpp17("tscm_boards_core.h")


def test_serial_instantiation_runs_clean_and_builds_agree(checker):
    out = N.run(checker, N_SETS)
    assert out["n_sets"] == N_SETS and sum(out["status"]) == out["seeds"] > 0
    assert all(c > 0 for c in out["status"]), out["status"]                 # the sets reach every exit of a job
    assert out["boards"] >= out["complete"] >= N_SETS // 2, (out["boards"], out["complete"])     # most grids come out whole
    _seen[checker] = out["checksum"]
    assert len(set(_seen.values())) == 1, _seen                             # plain and sanitised builds: one checksum
    for k, s in enumerate(out["sets"]):                                     # and the library's host call gives these boards
        x, y = np.array(s["x"]), np.array(s["y"])
        v1, v2 = np.array(s["v1"]).reshape(-1, 2), np.array(s["v2"]).reshape(-1, 2)
        lib_boards = corners.chessboards_from_corners_batch([(x, y, v1, v2)], where="host")[0]
        assert len(lib_boards) == len(s["boards"]), k
        for b, q in zip(lib_boards, s["boards"]):
            assert b.shape == (q[0], q[1]) and np.array_equal(b.ravel(), q[2:]), k
