"""GPU tests of the hole filling (tscm_stereo_fill, tscm_stereo_fill_stages): the candidates of every direction, their
distances, the filled map and the mask equal the host restatement tests/stereo_fill_ref.py bit for bit (integers, nothing
depends on an order, so there is no tolerance), on sizes around the 64-lane step of the row scan and the prefetch depth of
the column scan; a single valid pixel fills exactly its row, column and diagonals; and on the sphere scene of
tests/test_gpu_sweep.py a knocked-out index map, filled, composes as well as the original one."""
import functools

import numpy as np
import pytest

from tests import stereo_fill_ref as F
from tests import sweep_compose_ref as CR
from tests import test_gpu_sweep as gs
from tests import test_stereo_fill_reference as ref_scene
from tests import test_sweep_compose_reference as compose_scene
from tscm_calib_amd import stereo, sweep

pytestmark = pytest.mark.gpu

INV = -16                                                                     # min_disparity = 0


def _differs(a, b):
    bad = np.argwhere(np.asarray(a) != np.asarray(b))
    return f"{len(bad)} of {np.asarray(a).size} differ, first at {bad[0].tolist() if len(bad) else None}"


def _check(device, d, stages=True, **p):
    """The candidates, the filled map and the mask of the device against the restatement; returns the restatement's stages."""
    ref = F.stages(d, **p)
    if stages:
        got = stereo.fill_stages(d, device=device, **p)
        for stage in ("value", "distance"):
            assert got[stage].dtype == ref[stage].dtype and got[stage].shape == ref[stage].shape, stage
            assert np.array_equal(got[stage], ref[stage]), f"{stage}: {_differs(got[stage], ref[stage])}"
    out, mask = stereo.fill(d, device=device, with_mask=True, **p)
    assert out.dtype == np.int16 and np.array_equal(out, ref["out"]), f"out: {_differs(out, ref['out'])}"
    assert mask.dtype == np.uint8 and np.array_equal(mask, ref["mask"]), f"mask: {_differs(mask, ref['mask'])}"
    return ref


@functools.lru_cache(maxsize=None)
def _random_map(w, h, share=0.3, invalid=INV, seed=0):
    """Values on both sides of zero, none of them the invalid one, `share` of the pixels invalid."""
    rng = np.random.default_rng(100 * w + h + seed)
    d = (16 * rng.integers(-40, 200, size=(h, w)) + 3).astype(np.int16)
    d[rng.random((h, w)) < share] = invalid
    d.setflags(write=False)
    return d


# ------------------------------------------------------------------------------------------------ sizes
SIZES = [(1, 1), (1, 70), (70, 1), (63, 15), (64, 16), (65, 17), (130, 35), (257, 3), (3, 200)]


@pytest.mark.parametrize("wrap_x", [0, 1])
@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_around_the_lane_step_and_the_prefetch_depth(hip_device, w, h, wrap_x):
    _check(hip_device, _random_map(w, h), wrap_x=wrap_x)


@pytest.mark.parametrize("share", [0.9, 0.999])
@pytest.mark.parametrize("w,h", [(130, 35), (257, 3), (3, 200)])
def test_sparse_maps(hip_device, w, h, share):
    d = _random_map(w, h, share)
    for wrap_x in (0, 1):
        _check(hip_device, d, wrap_x=wrap_x)


def test_the_all_valid_and_the_all_invalid_map(hip_device):
    d = _random_map(130, 35, 0.0)
    ref = _check(hip_device, d, wrap_x=1)
    assert np.array_equal(ref["out"], d) and not ref["mask"].any()
    e = np.full((35, 130), INV, dtype=np.int16)
    ref = _check(hip_device, e, wrap_x=1)
    assert np.all(ref["out"] == INV) and np.all(ref["mask"] == 2) and not ref["distance"].any()


# ------------------------------------------------------------------------------------------------ one valid pixel
@pytest.mark.parametrize("wrap_x", [0, 1])
@pytest.mark.parametrize("px,py", [(0, 0), (129, 0), (0, 34), (129, 34), (63, 20), (64, 20), (65, 20), (65, 17)])
def test_a_single_valid_pixel_fills_its_row_column_and_diagonals(hip_device, px, py, wrap_x):
    """The filled set is worked out here, not taken from the restatement: (x, y) is filled iff it is in the pixel's row or
    column, or |x - px| == |y - py|; with wrap_x the last condition holds modulo the width."""
    w, h = 130, 35
    d = np.full((h, w), INV, dtype=np.int16)
    d[py, px] = 777
    out, mask = stereo.fill(d, device=hip_device, with_mask=True, wrap_x=wrap_x)
    yy, xx = np.mgrid[0:h, 0:w]
    dy = np.abs(yy - py)
    if wrap_x:
        diagonal = ((xx - px - dy) % w == 0) | ((xx - px + dy) % w == 0)
    else:
        diagonal = np.abs(xx - px) == dy
    want = (yy == py) | (xx == px) | diagonal
    want[py, px] = False                                                       # the valid pixel itself: mask 0
    assert np.array_equal(mask == 1, want), _differs(mask == 1, want)
    assert mask[py, px] == 0 and np.array_equal(mask == 2, ~want & ((yy != py) | (xx != px)))
    assert np.array_equal(out, np.where(want | ((yy == py) & (xx == px)), 777, INV))
    _check(hip_device, d, wrap_x=wrap_x)


# ------------------------------------------------------------------------------------------------ parameters
@pytest.mark.parametrize("max_distance", [1, 2, 63, 64, 65])
def test_max_distance(hip_device, max_distance):
    for wrap_x in (0, 1):
        _check(hip_device, _random_map(130, 35, 0.999), max_distance=max_distance, wrap_x=wrap_x)
        _check(hip_device, _random_map(257, 3, 0.9), max_distance=max_distance, wrap_x=wrap_x)
        _check(hip_device, _random_map(3, 200, 0.9), max_distance=max_distance, wrap_x=wrap_x)


@pytest.mark.parametrize("paths,min_directions", [(8, 1), (8, 2), (8, 5), (8, 8), (4, 1), (4, 2), (4, 4)])
def test_paths_and_min_directions(hip_device, paths, min_directions):
    masks = [_check(hip_device, _random_map(130, 35, share), paths=paths, min_directions=min_directions, wrap_x=0)["mask"] for share in (0.3, 0.9, 0.99)]
    if min_directions > 1:                                                     # somewhere the rule bites, somewhere it lets a pixel through
        assert any(np.any(m == 2) for m in masks) and any(np.any(m == 1) for m in masks)


@pytest.mark.parametrize("rule", ["lowest", "second_lowest", "median"])
@pytest.mark.parametrize("paths", [4, 8])
def test_rules(hip_device, rule, paths):
    outs = []
    for share in (0.3, 0.9):
        outs.append(_check(hip_device, _random_map(130, 35, share), stages=False, rule=rule, paths=paths, wrap_x=1)["out"])
    assert np.array_equal(outs[0], stereo.fill(_random_map(130, 35, 0.3), device=hip_device, rule=F.RULES[rule], paths=paths, wrap_x=1))


@pytest.mark.parametrize("min_disparity", [-5, 0, 7])
def test_min_disparity_moves_the_invalid_value(hip_device, min_disparity):
    invalid = F.invalid_value(min_disparity)
    d = _random_map(65, 17, 0.3, invalid=invalid, seed=min_disparity).copy()
    d[3, 5], d[3, 6] = -32768 + 16, 32767                                     # the ends of int16 sort as integers
    d[4, 5], d[4, 6] = INV if invalid != INV else 5, invalid
    ref = _check(hip_device, d, min_disparity=min_disparity)
    assert np.any(ref["mask"] == 1) and not np.any(ref["out"] == invalid)


# ------------------------------------------------------------------------------------------------ layout
def test_row_padding_in_and_out(hip_device):
    d = _random_map(130, 35)
    wide = np.full((35, 150), 12345, dtype=np.int16)
    wide[:, :130] = d
    out_wide = np.full((35, 141), -999, dtype=np.int16)
    out = stereo.fill(wide[:, :130], device=hip_device, out=out_wide[:, :130], wrap_x=1)
    assert np.shares_memory(out, out_wide)
    assert np.array_equal(out_wide[:, :130], F.fill(d, wrap_x=1)[0])
    assert np.all(out_wide[:, 130:] == -999) and np.all(wide[:, 130:] == 12345) and np.array_equal(wide[:, :130], d)


def test_in_place_and_without_a_mask(hip_device):
    d = _random_map(130, 35).copy()
    want, _ = F.fill(d)
    wide = np.full((35, 140), 77, dtype=np.int16)
    wide[:, :130] = d
    assert stereo.fill(d, device=hip_device, out=d) is d and np.array_equal(d, want)
    view = wide[:, :130]
    stereo.fill(view, device=hip_device, out=view)
    assert np.array_equal(view, want) and np.all(wide[:, 130:] == 77)
    out, seconds = stereo.fill(_random_map(130, 35), device=hip_device, with_seconds=True)     # mask = NULL in the C call
    assert np.array_equal(out, want) and seconds > 0.0


def test_filter_then_fill_then_fill_again(hip_device):
    """Three levels, two of them 16 apart, 30 % invalid (the maps of tests/test_gpu_stereo_filter.py): the speckle rule
    removes 1392 of the valid pixels, the fill puts a value into every hole, and a second fill finds nothing to do."""
    rng = np.random.default_rng(11)
    d = rng.choice(np.array([160, 176, 400], dtype=np.int16), size=(35, 130))
    d[rng.random((35, 130)) < 0.3] = INV
    filtered = stereo.filter(d, device=hip_device, speckle_window_size=4, speckle_range=1)
    assert np.any((d != INV) & (filtered == INV))
    once, mask = stereo.fill(filtered, device=hip_device, with_mask=True)
    assert np.array_equal(once, F.fill(filtered)[0])
    assert not np.any(once == INV) and np.array_equal(mask == 0, filtered != INV)
    twice, mask2 = stereo.fill(once, device=hip_device, with_mask=True)
    assert np.array_equal(twice, once) and not mask2.any()


# ------------------------------------------------------------------------------------------------ end to end
def test_a_knocked_out_index_map_of_the_sphere_scene_is_restored(hip_device):
    """Sweeper.depth on device-built tables, the holes of ref_scene.sphere_holes set to INVALID, filled with the defaults
    plus wrap_x = 1.  The factor 2 on the CPU reference values is the project's allowance for the unpinned sincos of the
    table kernel, as in tests/test_gpu_sweep.py and tests/test_gpu_sweep_compose.py."""
    intr, T, imgs = gs.sphere_scene()
    pw, ph = gs.SCENE["pano_w"], gs.SCENE["pano_h"]
    inv = sweep.inverse_distances(gs.SCENE["near"], D=gs.SCENE["D"])
    truth = compose_scene.sphere_truth()
    holes = ref_scene.sphere_holes()
    with sweep.Sweeper.from_rig(intr, T, (320, 270), pw, ph, inv, weights=None, device=hip_device, keep_tables=True, paths=gs.SCENE["paths"]) as s:
        idx = s.depth(imgs)
        knocked = idx.copy()
        knocked[holes] = sweep.INVALID
        filled, mask = stereo.fill(knocked, device=hip_device, with_mask=True, wrap_x=1)
        pts, valid = s.points(filled)
        at_filled = s.compose(imgs, filled, mode="feather")
        at_fallback = s.compose(imgs, knocked, mode="feather", fallback_index=0)
    want, want_mask = F.fill(knocked, wrap_x=1)
    assert np.array_equal(filled, want) and np.array_equal(mask, want_mask)                     # (a)
    median = float(np.median(gs.sphere_error(pts, valid & holes)))
    err = ref_scene.error_on(at_filled, truth, holes)
    err_fallback = ref_scene.error_on(at_fallback, truth, holes)
    print(f"sphere, {100 * holes.mean():.1f} % knocked out: {int((filled == sweep.INVALID).sum())} pixels left invalid; on the holes median "
          f"| |P| - R | {median:.2f} mm (CPU reference {ref_scene.SPHERE_FILL_MEDIAN_MM['median']}), FEATHER {err:.2f} filled, "
          f"{err_fallback:.2f} at the fallback (CPU reference {ref_scene.SPHERE_FILL_FEATHER['filled']}, {ref_scene.SPHERE_FILL_FEATHER['fallback']})")
    assert not np.any(filled == sweep.INVALID)                                                  # (b) a condition on the scene
    assert median <= 2.0 * ref_scene.SPHERE_FILL_MEDIAN_MM["median"]                           # (c)
    assert ref_scene.SPHERE_FILL_RATIO < 0.5                                                    # a condition on the scene
    assert err <= 2.0 * ref_scene.SPHERE_FILL_FEATHER["filled"]                                # (d)
    assert err <= 0.5 * err_fallback


def test_pair_depth_takes_a_fill(hip_device):
    """stereo.pair_depth(post=..., fill=...): the map whose points are taken is fill(filter(match)), with wrap_x = 0 and
    the matcher's min_disparity; fill=None gives the bits of the chain without the argument."""
    from tests import test_gpu_stereo_filter as pf
    intr, T, imgs = pf.plane_scene()
    seen = {}

    def chain_on_the_host(left, right, **p):
        disp = stereo.filter(stereo.match(left, right, device=hip_device, **p), device=hip_device, **pf.POST)
        seen["filtered"] = disp
        return F.fill(disp, rule="second_lowest", max_distance=10)[0]

    args = (imgs[0], imgs[1], intr[0], T[0], intr[1], T[1])
    pts_r, valid_r, _ = stereo.pair_depth(*args, device=hip_device, matcher=chain_on_the_host, **pf.SCENE)
    pts, valid, _ = stereo.pair_depth(*args, device=hip_device, post=pf.POST, fill=dict(rule="second_lowest", max_distance=10), **pf.SCENE)
    assert np.array_equal(valid, valid_r) and np.array_equal(pts[valid], pts_r[valid])
    pts_p, valid_p, _ = stereo.pair_depth(*args, device=hip_device, post=pf.POST, **pf.SCENE)
    pts_n, valid_n, _ = stereo.pair_depth(*args, device=hip_device, post=pf.POST, fill=None, **pf.SCENE)
    assert np.array_equal(valid_p, valid_n) and np.array_equal(pts_p[valid_p], pts_n[valid_n])
    assert np.all(valid[valid_p]) and valid.sum() > valid_p.sum() and np.any(seen["filtered"] == INV), "the fill only adds"
    with pytest.raises(TypeError):
        stereo.pair_depth(*args, device=hip_device, fill=dict(min_disparity=0), **pf.SCENE)


def test_the_chains_take_a_fill(hip_device):
    """rig_depth and rig_panorama with fill=...: the map returned is the filled one (wrap_x = 1 by default), the points
    and the frame are taken at it, and fill=None gives the bits of the chain without the argument."""
    intr, T, imgs = gs.sphere_scene()
    pw, ph = gs.SCENE["pano_w"], gs.SCENE["pano_h"]
    kw = dict(near=gs.SCENE["near"], D=gs.SCENE["D"], weights=None, device=hip_device, paths=gs.SCENE["paths"])
    post = dict(speckle_window_size=20, speckle_range=1, median=3)
    raw, _, raw_valid = sweep.rig_depth(imgs, intr, T, pw, ph, post=post, **kw)
    same, _, _ = sweep.rig_depth(imgs, intr, T, pw, ph, post=post, fill=None, **kw)
    assert np.array_equal(raw, same) and np.any(raw == sweep.INVALID)
    idx, pts, valid = sweep.rig_depth(imgs, intr, T, pw, ph, post=post, fill=dict(rule="second_lowest"), **kw)
    assert np.array_equal(idx, F.fill(raw, rule="second_lowest", wrap_x=1)[0])
    assert valid.sum() > raw_valid.sum() and np.all(np.isfinite(pts[valid]))
    flat, _, _ = sweep.rig_depth(imgs, intr, T, pw, ph, post=post, fill=dict(wrap_x=0, max_distance=3), **kw)
    assert np.array_equal(flat, F.fill(raw, wrap_x=0, max_distance=3)[0])
    pano, pidx, cov = sweep.rig_panorama(imgs, intr, T, pw, ph, post=post, fill={}, mode="feather", **kw)
    inv = sweep.inverse_distances(gs.SCENE["near"], D=gs.SCENE["D"])
    with sweep.Sweeper.from_rig(intr, T, (320, 270), pw, ph, inv, weights=None, device=hip_device, keep_tables=True, paths=gs.SCENE["paths"]) as s:
        mx, my = s.mapx, s.mapy
    assert np.array_equal(pidx, F.fill(raw, wrap_x=1)[0])
    host = CR.compose(imgs, None, mx, my, pidx, mode=CR.FEATHER)
    assert np.array_equal(pano[..., None], host["out"]) and np.array_equal(cov, host["coverage"])
    with pytest.raises(TypeError):
        sweep.rig_depth(imgs, intr, T, pw, ph, fill=dict(min_disparity=0), **kw)
