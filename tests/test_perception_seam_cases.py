"""What the seam and limit cases of the perception GPU tests are there to reach, asserted on the host restatements alone
(tests/stereo_ref.py, tests/pano_ref.py), so that a change of an input recipe cannot take a case's reach away unnoticed,
with or without a device.  The case tables are those of the GPU test modules, imported and not copied.

The constants the cases are built around live in the kernels and are quoted here, not parsed:
  kCostSegment = 256             tscm_stereo.hip: pixels of a row per k_cost / k_right_winner block
  kPrefetch = 4                  tscm_stereo_kernels.h: steps of a scanline in flight in k_aggregate, 4 scanlines per block
  kPanoTileW x kPanoTileH = 64 x 16, kPanoHaloW x kPanoHaloH = 34 x 10
                                 tscm_pano_kernels.h: the fine tile of k_pano_lapblend / k_pano_collapse and its coarse halo
  kPanoMaxCameras = 16, kPanoMaxLevels = 6
                                 tscm_pano_kernels.h: the ends of the API's ranges; k_pano_overlap keeps 16 x 16 LDS slots"""
import numpy as np
import pytest

from tests import pano_ref as PR
from tests import test_gpu_panorama as gp
from tests import test_gpu_stereo as gst
from tests import test_gpu_sweep_compose as gc
from tests import test_gpu_sweep_visibility as gv

SEGMENT = 256
TILE_W, TILE_H = 64, 16
HALO_W, HALO_H = 34, 10

WIDE = [name for name, c in gst.CASES.items() if c[1] > SEGMENT]
# pano_w, pano_h, levels -> rows, columns of the top level
TOPS = {(96, 48, 4): (3, 6), (128, 64, 5): (2, 4), (64, 64, 6): (1, 1), (64, 32, 3): (4, 8)}


# ------------------------------------------------------------------------------------------------ stereo
def test_the_stereo_table_has_the_seam_shapes():
    shapes = {(c[1], c[2]) for c in gst.CASES.values()}
    assert {(256, 4), (257, 5), (300, 9), (513, 6), (300, 12), (21, 75), (3, 40), (1, 70), (70, 1), (8, 6), (1, 1)} <= shapes
    assert sorted(gst.CASES[name][1] for name in WIDE) == [257, 300, 300, 300, 513]
    assert max(c[1] for name, c in gst.CASES.items() if name not in WIDE) == SEGMENT       # and one case exactly on the boundary
    full = [c for c in gst.CASES.values() if c[1] > SEGMENT and c[3]["num_disparities"] == 256]
    assert full, "no case fills the right[kCostSegment + 256] window: n = 256 and D = 256"
    assert any(c[1] - SEGMENT > 0 and SEGMENT - (c[3].get("min_disparity", 0) + 255) > 0 for c in full)     # r0 > 0 in the second block


@pytest.mark.parametrize("case", WIDE)
def test_the_later_segments_are_mostly_valid(case):
    name, w, h, p = gst.CASES[case]
    ref = gst._reference(name, w, h, tuple(sorted(p.items())))
    valid = ref["disparity"] != 16 * (p.get("min_disparity", 0) - 1)
    assert valid[:, SEGMENT:].mean() >= 0.5


@pytest.mark.parametrize("case", [name for name in WIDE if gst.CASES[name][0] == "noise"])
def test_the_left_right_rule_reads_across_the_segment_seam(case):
    """In every noise case wider than a segment at least half of the pixels of the later segments are valid, and among them
    is one whose kR entry lies in the first segment: x >= 256 > x - d.  (The board is flat at the seam: its winner there is
    k = 0, and what it is for is the next test.)"""
    name, w, h, p = gst.CASES[case]
    assert p["disp12_max_diff"] >= 0
    ref = gst._reference(name, w, h, tuple(sorted(p.items())))
    dmin = p.get("min_disparity", 0)
    valid = ref["disparity"] != 16 * (dmin - 1)
    d = dmin + ref["aggregated"].argmin(axis=-1)                  # the first, i.e. lowest, k: the winner's disparity in pixels
    x = np.broadcast_to(np.arange(w), (h, w))
    later = x >= SEGMENT
    share = valid[later].mean()
    across = valid & later & (x - d < SEGMENT)
    print(f"{case}: {100 * valid.mean():.0f} % valid, {100 * share:.0f} % in columns >= {SEGMENT}, {int(across.sum())} valid pixels read kR across the seam")
    assert share >= 0.5
    assert across.any()


def test_negative_winners_feed_the_second_block_from_the_first():
    """k_right_winner's block at s0 walks the columns from lo = max(0, s0 + dmin).  The columns below s0 hold candidates of
    negative disparity only, so a lower bound that is too high goes unnoticed unless such a candidate wins: with the images
    swapped there are valid pixels x < 256 whose kR entry x - d lies in the second segment."""
    name, w, h, p = gst.CASES["two-segments-negative-disparity"]
    dmin = p["min_disparity"]
    assert name == "noise-swapped" and dmin < 0 and p["disp12_max_diff"] >= 0
    ref = gst._reference(name, w, h, tuple(sorted(p.items())))
    valid = ref["disparity"] != 16 * (dmin - 1)
    d = dmin + ref["aggregated"].argmin(axis=-1)
    x = np.broadcast_to(np.arange(w), (h, w))
    back = valid & (x < SEGMENT) & (x - d >= SEGMENT)
    print(f"negative disparity: {100 * valid.mean():.0f} % valid, {int(back.sum())} valid pixels of the first segment read kR in the second")
    assert valid.mean() >= 0.5 and (d[valid] < 0).mean() >= 0.9
    assert back.sum() >= h                                        # about d = 5 or 12 pixels in each of the h rows


def test_the_board_ties_across_the_segment_seam():
    """kR(y, x2) is the lowest k that minimises S(y, x2 + k, k).  On the board there are x2 of the first segment whose minimum
    is shared by several k, one of them read from a column of the second segment, and x2 of the second segment with a shared
    minimum too: 'lowest k' decides in both blocks of k_right_winner."""
    name, w, h, p = gst.CASES["two-segments-board"]
    assert name == "board" and p.get("min_disparity", 0) == 0 and p["disp12_max_diff"] >= 0
    S = gst._reference(name, w, h, tuple(sorted(p.items())))["aggregated"].astype(np.int64)
    D = S.shape[-1]
    straddling = later = 0
    for x2 in range(SEGMENT - D + 1, w):
        ks = np.arange(min(D, w - x2))
        vals = S[:, x2 + ks, ks]                                   # [h, len(ks)]
        tied = vals == vals.min(axis=1, keepdims=True)
        many = tied.sum(axis=1) >= 2
        if x2 < SEGMENT:
            straddling += int((many & tied[:, x2 + ks >= SEGMENT].any(axis=1)).sum())
        else:
            later += int(many.sum())
    print(f"board: {straddling} kR entries of the first segment tie with a column of the second, {later} ties inside the second")
    assert straddling > 0 and later > 0


def test_the_tall_case_restarts_every_diagonal_three_times():
    """A diagonal of k_aggregate moves one column per row and starts a new path whenever it runs over the image edge, once
    every w rows: h // w restarts at least on every line."""
    _, w, h, _ = gst.CASES["tall-diagonals-wrap-thrice"]
    assert h // w >= 3 and h % 4 != 0
    for name in ("three-columns", "single-column", "one-pixel"):
        assert gst.CASES[name][1] < 4                              # fewer scanlines than a block of k_aggregate holds
    assert gst.CASES["single-row"][2] < 4
    _, w, h, _ = gst.CASES["below-census-window"]
    assert w < 9 and h < 7


# ------------------------------------------------------------------------------------------------ panorama
def _limit_cases(n=None, mode=None):
    return [(i, c) for i, c in enumerate(gp.LIMIT_CASES) if (n is None or c[0] == n) and (mode is None or c[4] == mode)]


def _labels(index, case):
    """label, coverage and the overlap counts of a limit case: they do not depend on the mode, so SEAM gives them cheaply."""
    n, ch, pw, ph = case[:4]
    with_weights = gp._limit_options(index)[1]
    mx, my = gp._limit_tables(n, pw, ph)
    return PR.compose(list(gp._images(n, ch)), list(gp._weights(n)) if with_weights else None, mx, my, PR.SEAM)


def test_the_panorama_table_has_the_limit_shapes():
    assert [c for c in gp.LIMIT_CASES] == [(5, 3, 96, 48, "multiband", 4), (9, 1, 128, 64, "multiband", 5), (16, 1, 64, 64, "multiband", 6),
                                           (16, 1, 64, 64, "multiband", 6), (16, 3, 72, 24, "seam", 0), (16, 3, 72, 24, "feather", 0),
                                           (12, 1, 64, 32, "multiband", 3)]
    deepest = [gp._limit_options(i)[0] for i, c in _limit_cases() if c[5] == 6]
    assert sorted(deepest) == [False, True]                       # wrap_x off and on over the 1 x 1 top
    i, _ = _limit_cases(16, "feather")[0]
    assert gp._limit_options(i)[2], "the 16-camera FEATHER case fills the Gains struct"
    assert len(set(gp.GAINS)) == 16 and min(gp.GAINS) >= 1 and max(gp.GAINS) <= 4095 and gp.GAINS[:3] == (200, 256, 700)


@pytest.mark.parametrize("index,case", _limit_cases(16), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_sixteen_cameras_all_win_all_meet(index, case):
    ref = _labels(index, case)
    assert set(range(16)) <= set(np.unique(ref["label"]).tolist()), np.unique(ref["label"])
    assert ref["coverage"].max() >= 9
    assert ref["count"].shape == (16, 16) and np.all(ref["count"] > 0)
    assert (ref["alpha"][15] > 0).any()                           # bit 15 of the coverage mask


def test_sixteen_cameras_meet_in_the_overlap_case():
    """The inputs of test_overlap_sums_of_sixteen_cameras: 72 x 24 with weight images."""
    mx, my = gp._limit_tables(16, 72, 24)
    for ch in (1, 3):
        ref = PR.compose(list(gp._images(16, ch)), list(gp._weights(16)), mx, my, PR.FEATHER)
        assert np.all(ref["count"] > 0) and np.all(ref["sum"] >= 0)


@pytest.mark.parametrize("case", sorted(set(c for _, c in _limit_cases(mode="multiband"))), ids=lambda c: "%dx%d-L%d" % (c[2], c[3], c[5]))
def test_the_top_level_of_a_limit_pyramid(case):
    pw, ph, levels = case[2], case[3], case[5]
    pyr = PR.pyramid(np.zeros((ph, pw), np.int64), levels, True)
    assert pyr[-1].shape == TOPS[(pw, ph, levels)]
    assert pyr[-1].shape[1] < HALO_W and pyr[-1].shape[0] < HALO_H


def test_twelve_cameras_leave_tiles_without_a_camera():
    """k_pano_lapblend skips a camera whose mask is zero over a whole 64 x 16 tile: the case has such tiles, for cameras that
    win elsewhere."""
    index, case = _limit_cases(12)[0]
    n, _, pw, ph = case[:4]
    lab = _labels(index, case)["label"]
    empty = 0
    for k in range(n):
        tiles = [(lab[y:y + TILE_H, x:x + TILE_W] == k).any() for y in range(0, ph, TILE_H) for x in range(0, pw, TILE_W)]
        assert any(tiles), f"camera {k} wins nowhere"
        empty += tiles.count(False)
    assert empty >= n // 2


# ------------------------------------------------------------------------------------------------ sweep
def test_the_sweep_tables_reach_the_deep_pyramids():
    deep = [c for c in gc.CASES if c[5] == gc.M_ and c[6] >= 4]
    assert sorted((c[0], c[1], c[2], c[4], c[6]) for c in deep) == [(5, 96, 48, 1, 4), (8, 64, 64, 3, 6), (8, 128, 64, 1, 5)]
    assert {c[7] for c in deep} == {False, True}                  # both values of wrap_x
    for c in deep:
        assert PR.pyramid(np.zeros((c[2], c[1]), np.int64), c[6], c[7])[-1].shape == TOPS[(c[1], c[2], c[6])]
    vis = [gv._case(si, ti) for si, ti in gv.CASES]
    assert len(gv.CASES) == len(set(gv.CASES)) == len(set(gv.IDS))
    assert [(c["n"], c["pw"], c["ph"], c["mode"]) for c in vis if c["levels"] == 5] == [(8, 128, 64, gv.M_)]
