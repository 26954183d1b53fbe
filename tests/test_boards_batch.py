"""The batched chessboard structure recovery on the host (tscm_chessboards_from_corners_batch, where = HOST: the serial
instantiation of tscm_calib_amd/csrc/tscm_boards_core.h) through the C ABI: its final boards against
tscm_chessboards_from_corners -- a different definition in one documented step, the extrapolation without atan2 / cos / sin,
equal in its boards unless a winning proposal holds an exact tie -- on the random candidate sets of tests/test_boards.py,
clutter-heavy sets and rendered views; the properties of the per-seed stages; every refusal; the edge inputs.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc
from tests import boards_cases as B
from tscm_calib_amd import corners, lib, synth


def _same_boards(a, b, where):
    assert len(a) == len(b), (where, [u.shape for u in a], [u.shape for u in b])
    for u, v in zip(a, b):
        assert u.shape == v.shape and np.array_equal(u, v), where


def _both(x, y, v1, v2):
    """(boards of today's function, boards of the new definition on the host, its stages)."""
    old = corners.chessboards_from_corners(x, y, v1, v2)
    new = corners.chessboards_from_corners_batch([(x, y, v1, v2)], where="host")[0]
    st = corners.chessboards_batch_stages([(x, y, v1, v2)], where="host")[0]
    return old, new, st


@pytest.mark.parametrize("seed", B.SEEDS)
def test_same_boards_as_the_sequential_function_on_random_sets(seed):
    x, y, v1, v2, _ = B.random_candidates(seed)
    old, new, st = _both(x, y, v1, v2)
    _same_boards(old, new, f"seed {seed}")
    B.check_stages(x, y, st, new, f"seed {seed}")


@pytest.mark.parametrize("seed", B.HEAVY_SEEDS)
def test_same_boards_with_60_to_120_clutter_points(seed):
    x, y, v1, v2, _ = B.heavy_candidates(seed)
    assert 60 <= len(x) - _[0] * _[1] <= 120
    old, new, st = _both(x, y, v1, v2)
    _same_boards(old, new, f"seed {seed}")
    B.check_stages(x, y, st, new, f"seed {seed}")


@functools.lru_cache(maxsize=None)
def _rendered(view):
    """Oracle candidates of a rendered 9 x 6 view, as tests/test_boards.py takes them.  Never written to."""
    p = synth.make_problem(1, 6, 3, noise_px=0.0, perturb=False)
    img = synth.render_chessboard(p.meta["gt_intr"][0], p.meta["gt_board_rt"][view], 9, 6, 45.0, 1280, 1080, supersample=2)
    d = orc.detect_corners(img)
    keep = d["score"] >= 0.01
    return d["x"][keep], d["y"][keep], d["v1"][keep], d["v2"][keep]


@pytest.mark.parametrize("view", [0, 1, 2])
def test_same_boards_on_rendered_views(view):
    x, y, v1, v2 = _rendered(view)
    old, new, st = _both(x, y, v1, v2)
    assert len(old) == 1 and old[0].shape == (6, 9)
    _same_boards(old, new, f"view {view}")
    B.check_stages(x, y, st, new, f"view {view}")


def test_a_batch_equals_its_images_one_by_one():
    sets = [B.random_candidates(s)[:4] for s in (3, 4, 5)] + [B.edge_sets()[k] for k in B.MIXED]
    batch = corners.chessboards_from_corners_batch(sets, where="host")
    stages = corners.chessboards_batch_stages(sets, where="host")
    assert len(batch) == len(stages) == len(sets)
    for k, s in enumerate(sets):
        _same_boards(corners.chessboards_from_corners_batch([s], where="host")[0], batch[k], f"image {k}")
        one = corners.chessboards_batch_stages([s], where="host")[0]
        for key in ("status", "rows", "cols", "steps", "offset", "cells"):
            assert np.array_equal(one[key], stages[k][key]), (k, key)
        assert np.array_equal(one["energy"].view(np.uint64), stages[k]["energy"].view(np.uint64)), k
        assert not stages[k]["on_device"]


# ------------------------------------------------------------------------------------------------ edge inputs
def test_empty_batch():
    assert corners.chessboards_from_corners_batch([], where="host") == []
    assert corners.chessboards_batch_stages([], where="host") == []


@pytest.mark.parametrize("name", ["n0", "n8"])
def test_fewer_than_nine_candidates_give_nothing(name):
    x, y, v1, v2 = B.edge_sets()[name]
    old, new, st = _both(x, y, v1, v2)
    assert old == new == []
    assert st["n"] == len(x) and not st["status"].any() and st["cells"].shape == (0,)


def test_nine_candidates_at_one_point():
    """Every distance is 0, every energy term 0 / 0: NaN energies are never taken, no board, as today's function."""
    x, y, v1, v2 = B.edge_sets()["n9_one_point"]
    old, new, st = _both(x, y, v1, v2)
    assert old == new == []
    B.check_stages(x, y, st, new)
    assert not np.any(st["status"] == 3)


@pytest.mark.parametrize("name", ["duplicates", "grid_with_candidate_0", "zero_directions", "n12", "n70"])
def test_edge_sets(name):
    """Duplicated candidates tie exactly in every distance, and both definitions take the first; candidate 0 is the empty
    marker in both; a seed without directions sees every candidate at distance 0 in both."""
    x, y, v1, v2 = B.edge_sets()[name]
    old, new, st = _both(x, y, v1, v2)
    _same_boards(old, new, name)
    counts = B.check_stages(x, y, st, new, name)
    if name in ("duplicates", "zero_directions", "n70"):
        assert counts[3] > 0 and len(new) >= 1, (name, counts)                     # the set does reach the growth and the resolution
    if name == "grid_with_candidate_0":
        assert any(0 in st["cells"][st["offset"][i]:st["offset"][i + 1]] for i in np.flatnonzero(st["status"] >= 1)), "no record holds candidate 0"


def test_mixed_batch_of_0_8_12_and_70_candidates():
    sets = [B.edge_sets()[k] for k in B.MIXED]
    new = corners.chessboards_from_corners_batch(sets, where="host")
    stages = corners.chessboards_batch_stages(sets, where="host")
    assert [s["n"] for s in stages] == [0, 8, 12, 70]
    assert new[0] == [] and new[1] == []
    for s, b, st in zip(sets, new, stages):
        _same_boards(corners.chessboards_from_corners(*s), b, st["n"])
        B.check_stages(s[0], s[1], st, b, st["n"])


# ------------------------------------------------------------------------------------------------ refusals
def _call(name, n_images, recs, where, out):
    f = getattr(lib.lib(), name)
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return f(n_images, recs, where, 0, out)


def _record(x, y, v1, v2):
    keep, recs = corners._candidate_records([(x, y, v1, v2)])
    return keep, recs


@pytest.mark.parametrize("name,out_type", [("tscm_chessboards_from_corners_batch", lib.CChessboards), ("tscm_chessboards_batch_stages", lib.CBoardSeedStages)])
def test_refusals(name, out_type):
    x, y, v1, v2 = B.edge_sets()["n12"]
    keep, recs = _record(x, y, v1, v2)
    out = (out_type * 1)()
    assert _call(name, 1, recs, lib.BOARDS_HOST, None) == -1                        # NULL out
    assert _call(name, 1, None, lib.BOARDS_HOST, out) == -1                         # NULL cands
    assert _call(name, -1, recs, lib.BOARDS_HOST, out) == -1                        # negative n_images
    for where in (-1, 2, 7):
        assert _call(name, 1, recs, where, out) == -1, where                        # unknown where
        assert b"where" in lib.lib().tscm_last_error()
    recs[0].n = -3
    assert _call(name, 1, recs, lib.BOARDS_HOST, out) == -1                         # negative count
    recs[0].n = 12
    for field in ("x", "y", "v1", "v2"):                                            # a NULL list
        keep2, r2 = _record(x, y, v1, v2)
        setattr(r2[0], field, C.POINTER(C.c_double)())
        assert _call(name, 1, r2, lib.BOARDS_HOST, out) == -1, field
    for bad in (np.nan, np.inf, -np.inf, 32768.0, -32767.5, 1e300):                 # a coordinate outside the definition
        for which in (0, 1):
            c = [x.copy(), y.copy()]
            c[which][5] = bad
            keep2, r2 = _record(c[0], c[1], v1, v2)
            assert _call(name, 1, r2, lib.BOARDS_HOST, out) == -1, (bad, which)
            assert b"coordinate" in lib.lib().tscm_last_error()
    c = x.copy()
    c[5] = -32767.0                                                                 # the limit itself is served
    keep2, r2 = _record(c, y, v1, v2)
    assert _call(name, 1, r2, lib.BOARDS_HOST, out) == 0
    free = lib.lib().tscm_chessboards_free if out_type is lib.CChessboards else lib.lib().tscm_board_seed_stages_free
    free.restype = None
    free.argtypes = [C.c_void_p]
    free(out)
    assert _call(name, 0, None, lib.BOARDS_HOST, out) == 0                          # an empty batch needs no candidates
    with pytest.raises(ValueError):
        corners.chessboards_from_corners_batch([(x, y, v1, v2)], where="gpu")
    with pytest.raises(ValueError):
        corners.find_chessboards([], 9, 6, recover="fast")


def test_more_than_65535_candidates_are_unsupported_as_today():
    n = 65536
    z = np.zeros(n)
    keep, recs = _record(z, z, np.zeros((n, 2)), np.zeros((n, 2)))
    out = (lib.CChessboards * 1)()
    assert _call("tscm_chessboards_from_corners_batch", 1, recs, lib.BOARDS_HOST, out) == -5


def test_exports_and_abi():
    for name in ("tscm_chessboards_from_corners_batch", "tscm_chessboards_batch_stages", "tscm_board_seed_stages_free", "tscm_chessboards_batch_seconds"):
        assert name in lib.EXPORTS and getattr(lib.lib(), name) is not None
    assert corners.chessboards_batch_seconds() == 0.0 or corners.chessboards_batch_seconds() > 0.0
