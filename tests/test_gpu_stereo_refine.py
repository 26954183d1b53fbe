"""GPU tests of the edge-aware weighted median (tscm_stereo_refine, tscm_stereo_refine_stages): the refined map, the weight
sums, the participant counts and the first pass equal the host restatement tests/stereo_refine_ref.py bit for bit (integers,
nothing depends on an order, so there is no tolerance), on sizes around the kernel's 32 x 8 tile and its halo; with equal
weights the device gives the masked median of tscm_stereo_filter; and the three chains take the stage behind the fill."""
import functools

import numpy as np
import pytest

from tests import stereo_refine_ref as R
from tests import test_gpu_sweep as gs
from tscm_calib_amd import stereo, sweep

pytestmark = pytest.mark.gpu

STEEP = R.range_weights(4.0)


def _differs(a, b):
    bad = np.argwhere(np.asarray(a) != np.asarray(b))
    return f"{len(bad)} of {np.asarray(a).size} differ, first at {bad[0].tolist() if len(bad) else None}"


def _check(device, d, g, lut=None, **p):
    """One pass of the device, stage values included, against the restatement; returns the restatement's (out, W, count)."""
    ref = R.pass_vectorised(d, g, lut, **p)
    got = stereo.refine_stages(d, g, device=device, weights=lut, **p)
    for name, want in zip(("first_pass", "weight_sum", "count"), ref):
        assert got[name].dtype == want.dtype and got[name].shape == want.shape, name
        assert np.array_equal(got[name], want), f"{name}: {_differs(got[name], want)}"
    out = stereo.refine(d, g, device=device, weights=lut, **p)
    assert out.dtype == np.int16 and np.array_equal(out, ref[0]), f"out: {_differs(out, ref[0])}"
    return ref


@functools.lru_cache(maxsize=None)
def _random_map(w, h, share=0.3, min_disparity=0, seed=0):
    """(map, guide): values on both sides of zero with ties, none of them the invalid one, `share` of the pixels invalid"""
    rng = np.random.default_rng(100 * w + h + seed)
    d = (16 * rng.integers(-40, 40, size=(h, w)) + 3).astype(np.int16)
    d[rng.random((h, w)) < share] = R.invalid_value(min_disparity)
    g = rng.integers(0, 256, size=(h, w)).astype(np.uint8) // 3 * 3           # differences reach into the table's steep start
    g[rng.random((h, w)) < 0.5] //= 32
    d.setflags(write=False)
    g.setflags(write=False)
    return d, g


# ------------------------------------------------------------------------------------------------ sizes
SIZES = [(1, 1), (1, 40), (40, 1), (31, 7), (32, 8), (33, 9), (65, 17), (130, 35)]     # the tile is 32 x 8: W +- 1 and H +- 1 are in


@pytest.mark.parametrize("wrap_x", [0, 1])
@pytest.mark.parametrize("radius", [1, 3, 7])
@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_around_the_tile_and_its_halo(hip_device, w, h, radius, wrap_x):
    d, g = _random_map(w, h)
    for fill_invalid in (0, 1):
        for lut in (STEEP, None):
            out, wsum, count = _check(hip_device, d, g, lut, radius=radius, wrap_x=wrap_x, fill_invalid=fill_invalid)
    assert count.max() <= (2 * radius + 1) ** 2 and wsum.max() <= 255 * (2 * radius + 1) ** 2
    if w >= 31 and h >= 7:
        assert not np.array_equal(out, d), "the pass did something"


@pytest.mark.parametrize("radius", [2, 4, 5, 6])
def test_the_other_radii(hip_device, radius):
    d, g = _random_map(65, 17)
    _check(hip_device, d, g, STEEP, radius=radius, wrap_x=1, fill_invalid=1)


# ------------------------------------------------------------------------------------------------ contents
@pytest.mark.parametrize("share", [0.9, 0.999, 0.0, 1.0])
def test_sparse_dense_and_empty_maps(hip_device, share):
    d, g = _random_map(65, 17, share=share)
    for fill_invalid in (0, 1):
        out, wsum, count = _check(hip_device, d, g, STEEP, radius=3, fill_invalid=fill_invalid)
        if share == 1.0:
            assert np.all(out == -16) and not count.any(), "nothing to take a value from"
        if share == 0.0:
            assert not np.any(out == -16)


def test_a_negative_min_disparity(hip_device):
    d, g = _random_map(65, 17, min_disparity=-5)
    assert np.any(d == -96)
    for fill_invalid in (0, 1):
        out, wsum, _ = _check(hip_device, d, g, STEEP, radius=3, min_disparity=-5, fill_invalid=fill_invalid)
    assert np.array_equal(out == -96, (d == -96) & (wsum == 0)), "with fill_invalid only an invalid pixel whose window carries no weight stays invalid"


def test_the_ends_of_int16(hip_device):
    rng = np.random.default_rng(9)
    d = rng.choice(np.array([-32768, 32767, -32768 + 1, 32766, 0, -16], dtype=np.int16), size=(17, 65))
    g = rng.integers(0, 256, size=(17, 65)).astype(np.uint8)
    for lut in (None, R.range_weights(40.0)):
        out, _, _ = _check(hip_device, d, g, lut, radius=2, fill_invalid=1, wrap_x=1)
        assert np.any(out == -32768) and np.any(out == 32767)


def test_a_table_with_zeros_leaves_pixels_without_weight(hip_device):
    d, g = _random_map(65, 17, share=0.6)
    lut = np.where(np.arange(256) < 2, 9, 0).astype(np.uint8)
    lut[0] = 0                                                                # not even the centre carries weight
    for fill_invalid in (0, 1):
        out, wsum, count = _check(hip_device, d, g, lut, radius=1, fill_invalid=fill_invalid)
        none = (wsum == 0) & (count > 0)
        assert none.any() and np.array_equal(out[none], d[none])


def test_iterations_are_repeated_single_calls(hip_device):
    d, g = _random_map(65, 17)
    p = dict(radius=2, fill_invalid=1, wrap_x=1)
    step = d
    for n in (1, 2, 3):
        step = stereo.refine(step, g, device=hip_device, weights=STEEP, **p)
        got = stereo.refine(d, g, device=hip_device, weights=STEEP, iterations=n, **p)
        assert np.array_equal(got, step), f"{n} iterations: {_differs(got, step)}"
        assert np.array_equal(got, R.refine(d, g, STEEP, iterations=n, **p))
    assert not np.array_equal(step, stereo.refine(d, g, device=hip_device, weights=STEEP, **p))
    stages = stereo.refine_stages(d, g, device=hip_device, weights=STEEP, iterations=3, **p)         # the stage values are the first pass's
    assert np.array_equal(stages["first_pass"], R.refine(d, g, STEEP, **p))


def test_in_place_padded_rows_and_sigma(hip_device):
    d, g = _random_map(130, 35)
    want = R.refine(d, g, STEEP, radius=3)
    own = d.copy()
    assert stereo.refine(own, g, device=hip_device, out=own, sigma=4.0, radius=3) is own and np.array_equal(own, want)
    wide_d, wide_g, wide_o = np.full((35, 140), 77, np.int16), np.full((35, 133), 200, np.uint8), np.full((35, 151), -5, np.int16)
    wide_d[:, :130], wide_g[:, :130] = d, g
    out, seconds = stereo.refine(wide_d[:, :130], wide_g[:, :130], device=hip_device, out=wide_o[:, :130], weights=STEEP, radius=3, with_seconds=True)
    assert np.array_equal(out, want) and np.all(wide_o[:, 130:] == -5) and seconds > 0.0
    view = wide_d[:, :130]
    stereo.refine(view, wide_g[:, :130], device=hip_device, out=view, weights=STEEP, radius=3)
    assert np.array_equal(view, want) and np.all(wide_d[:, 130:] == 77)
    bgr = np.stack([g, g, g], axis=-1)                                        # three equal channels are that grey value
    assert np.array_equal(sweep.bgr_to_gray(bgr), g)
    assert np.array_equal(stereo.refine(d, bgr, device=hip_device, sigma=4.0, radius=3), want)


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("min_disparity", [0, -5])
def test_equal_weights_are_the_filters_median_on_the_device(hip_device, radius, min_disparity):
    d, g = _random_map(130, 35, min_disparity=min_disparity)
    want = stereo.filter(d, device=hip_device, min_disparity=min_disparity, median=2 * radius + 1, speckle_window_size=0)
    got = stereo.refine(d, g, device=hip_device, min_disparity=min_disparity, radius=radius)
    assert np.array_equal(got, want), _differs(got, want)
    assert not np.array_equal(got, d)


# ------------------------------------------------------------------------------------------------ the chains
def test_pair_depth_takes_a_refine(hip_device):
    """stereo.pair_depth(post=..., fill=..., refine=...): the map whose points are taken is refine(fill(filter(match))) with
    the rectified left image as the guide and the matcher's min_disparity; refine=None gives the bits of the chain without
    the argument."""
    from tests import test_gpu_stereo_filter as pf
    intr, T, imgs = pf.plane_scene()
    fill, refine = dict(rule="second_lowest", max_distance=10), dict(radius=2, sigma=12.0, iterations=2)
    seen = {}

    def chain_by_hand(left, right, **p):
        disp = stereo.filter(stereo.match(left, right, device=hip_device, **p), device=hip_device, **pf.POST)
        seen["filled"] = stereo.fill(disp, device=hip_device, **fill)
        seen["refined"] = stereo.refine(seen["filled"], left, device=hip_device, **refine)
        assert np.array_equal(seen["refined"], R.refine(seen["filled"], left, R.range_weights(12.0), radius=2, iterations=2))
        return seen["refined"]

    args = (imgs[0], imgs[1], intr[0], T[0], intr[1], T[1])
    pts_r, valid_r, _ = stereo.pair_depth(*args, device=hip_device, matcher=chain_by_hand, **pf.SCENE)
    pts, valid, _ = stereo.pair_depth(*args, device=hip_device, post=pf.POST, fill=fill, refine=refine, **pf.SCENE)
    assert np.array_equal(valid, valid_r) and np.array_equal(pts[valid], pts_r[valid])
    assert not np.array_equal(seen["refined"], seen["filled"]), "the stage did something"
    pts_p, valid_p, _ = stereo.pair_depth(*args, device=hip_device, post=pf.POST, fill=fill, **pf.SCENE)
    pts_n, valid_n, _ = stereo.pair_depth(*args, device=hip_device, post=pf.POST, fill=fill, refine=None, **pf.SCENE)
    assert np.array_equal(valid_p, valid_n) and np.array_equal(pts_p[valid_p], pts_n[valid_n])
    with pytest.raises(TypeError):
        stereo.pair_depth(*args, device=hip_device, refine=dict(min_disparity=0), **pf.SCENE)


SPHERE_REFINE = dict(radius=2, sigma=25.0)
SPHERE_TRUE_INDEX = 16.0 * (gs.SCENE["D"] - 1) * gs.SCENE["near"] / gs.SPHERE_R          # 158.72: inverse distance 1 / 2500 mm


def sphere_wrong(index16) -> int:
    """pixels further than one hypothesis (16) from the true index of the sphere; an invalid pixel (-16) is one of them"""
    return int((np.abs(np.asarray(index16).astype(np.float64) - SPHERE_TRUE_INDEX) > 16).sum())


def test_the_sweep_chains_take_a_refine(hip_device):
    """rig_depth and rig_panorama with refine=...: the map returned is the refined one (wrap_x = 1 by default), guided by
    the grey frame that Sweeper.compose gives in SEAM mode at the map as it stands; the points and the frame are taken at
    it; refine=None gives the bits of the chain without the argument."""
    intr, T, imgs = gs.sphere_scene()
    pw, ph = gs.SCENE["pano_w"], gs.SCENE["pano_h"]
    kw = dict(near=gs.SCENE["near"], D=gs.SCENE["D"], weights=None, device=hip_device, paths=gs.SCENE["paths"])
    post = dict(speckle_window_size=20, speckle_range=1, median=3)
    filled, _, _ = sweep.rig_depth(imgs, intr, T, pw, ph, post=post, fill={}, **kw)
    same, _, _ = sweep.rig_depth(imgs, intr, T, pw, ph, post=post, fill={}, refine=None, **kw)
    assert np.array_equal(filled, same)
    idx, pts, valid = sweep.rig_depth(imgs, intr, T, pw, ph, post=post, fill={}, refine=SPHERE_REFINE, **kw)
    flat, _, _ = sweep.rig_depth(imgs, intr, T, pw, ph, post=post, fill={}, refine=dict(SPHERE_REFINE, wrap_x=0, fill_invalid=1), **kw)
    pano0, pidx0, cov0 = sweep.rig_panorama(imgs, intr, T, pw, ph, post=post, mode="feather", fallback_index=3, **kw)
    pano1, pidx1, cov1 = sweep.rig_panorama(imgs, intr, T, pw, ph, post=post, mode="feather", fallback_index=3, refine=None, **kw)
    assert np.array_equal(pano0, pano1) and np.array_equal(pidx0, pidx1) and np.array_equal(cov0, cov1)
    pano, pidx, cov = sweep.rig_panorama(imgs, intr, T, pw, ph, post=post, mode="feather", fallback_index=3, refine=SPHERE_REFINE, **kw)
    inv = sweep.inverse_distances(gs.SCENE["near"], D=gs.SCENE["D"])
    with sweep.Sweeper.from_rig(intr, T, (320, 270), pw, ph, inv, weights=None, device=hip_device, paths=gs.SCENE["paths"]) as s:
        guide = s.compose(imgs, index16=filled, mode="seam", fallback_index=0)
        by_hand = stereo.refine(filled, guide, device=hip_device, wrap_x=1, **SPHERE_REFINE)
        by_hand_flat = stereo.refine(filled, guide, device=hip_device, wrap_x=0, fill_invalid=1, **SPHERE_REFINE)
        guide3 = s.compose(imgs, index16=pidx0, mode="seam", fallback_index=3)
        pidx_by_hand = stereo.refine(pidx0, guide3, device=hip_device, wrap_x=1, **SPHERE_REFINE)
        pano_by_hand, cov_by_hand = s.compose(imgs, index16=pidx_by_hand, mode="feather", fallback_index=3, with_coverage=True)
        hand_pts, hand_valid = s.points(by_hand)
    assert np.array_equal(idx, by_hand) and np.array_equal(flat, by_hand_flat)
    assert np.array_equal(idx, R.refine(filled, guide, R.range_weights(SPHERE_REFINE["sigma"]), radius=SPHERE_REFINE["radius"], wrap_x=1))
    assert np.array_equal(valid, hand_valid) and np.array_equal(pts[valid], hand_pts[hand_valid])
    assert np.array_equal(pidx, pidx_by_hand) and np.array_equal(pano, pano_by_hand) and np.array_equal(cov, cov_by_hand)
    assert not np.array_equal(idx, filled) and np.any(pidx0 == sweep.INVALID), "the stage did something; the panorama's map has holes for the fallback"
    # on the sphere the refined map is no further from the true index map than the filled one
    print(f"sphere: pixels beyond +-16 of the true index {SPHERE_TRUE_INDEX:.2f}: filled {sphere_wrong(filled)}, refined {sphere_wrong(idx)}")
    assert sphere_wrong(idx) <= sphere_wrong(filled)
    with pytest.raises(TypeError):
        sweep.rig_depth(imgs, intr, T, pw, ph, refine=dict(min_disparity=0), **kw)
