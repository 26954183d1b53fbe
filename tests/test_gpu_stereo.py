"""GPU tests of the stereo matcher (tscm_stereo_*): every stage and the disparity map equal the host restatement
tests/stereo_ref.py bit for bit (all of it is integer arithmetic), the points agree with an independent two-ray
construction, and stereo.pair_depth runs the chain from two fisheye images of the rig to points on a plane.

Shapes are the smallest at which each path can go wrong.  96 x 48, 67 x 37, 131 x 53, 200 x 20 and 75 x 21 cover the 1..4
disparities per lane of k_aggregate (D = 16..256) inside one row segment.  k_cost and k_right_winner cut a row into segments
of kCostSegment = 256 pixels (tscm_stereo.hip): 256 x 4 is exactly one segment, 257 x 5 gives the second block one column,
300 x 9 with D = 256 fills the 511 right-hand codes of the first block's window and starts the second block's window in
mid-row (r0 = 9 at min_disparity -8), 513 x 6 has three blocks, the last with one column, and a positive min_disparity in
lo = s0 + dmin; the 300 x 12 board ties costs across the seam, and 300 x 9 with the images swapped has its winners at negative
disparity, the only ones for which k_right_winner's lower bound lo decides.  21 x 75 is taller than wide, so every diagonal of k_aggregate
restarts at the image edge three times or more, and 75 rows are no multiple of kPrefetch = 4 (tscm_stereo_kernels.h).  3 x 40
and 1 x 70 leave a vertical or diagonal launch fewer than the 4 scanlines of a block, 70 x 1 does so for the horizontal one,
8 x 6 is below the 9 x 7 census window, so that every tap of every pixel is a replicated border, and 1 x 1 is the least of all."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import lib, maps, stereo, synth
from tests import maps_proj_ref as mref
from tests import stereo_ref as R

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ inputs
def _noise_pair(w, h):
    """The construction of R.shifted_noise_pair at another size: disparity 5 on the top half, 12 on the bottom half."""
    if (w, h) == (96, 48):
        left, right, _ = R.shifted_noise_pair()
        return left, right
    src = np.random.default_rng(7).integers(0, 256, (h, w + 64)).astype(np.uint8)
    d = np.where(np.arange(h) < h // 2, 5, 12)
    return np.stack([src[y, 32 - d[y]:32 - d[y] + w] for y in range(h)]), src[:, 32:32 + w].copy()


def _board_pair(w=96, h=48):
    """Two views of a chessboard a few centimetres apart: large flat regions, where costs tie and 'lowest k' decides."""
    intr = synth.CALIB_INTR[0].copy()
    intr[:4] *= w / synth.IMG_W
    intr[3] = h / 2.0
    views = []
    for tx in (-160.0, -120.0):
        rt = np.array([0.05, -0.1, 0.02, tx, -110.0, 420.0])
        views.append(synth.render_chessboard(intr, rt, 5, 3, 60.0, w, h, supersample=1))
    return views[0], views[1]


@functools.lru_cache(maxsize=None)
def _pair(name, w, h):
    left, right = _board_pair(w, h) if name == "board" else _noise_pair(w, h)
    if name == "noise-swapped":                          # the images trade places: disparity -5 and -12
        left, right = right, left
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=None)
def _reference(name, w, h, key):
    """Stages and disparity of the host restatement, computed once per case."""
    left, right = _pair(name, w, h)
    p = dict(key)
    st = R.stages(left, right, **p)
    q = st["params"]
    st["disparity"] = R.disparity(st["aggregated"], q["min_disparity"], q["uniqueness_ratio"], q["disp12_max_diff"])
    for v in st.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return st


BASE = dict(num_disparities=32, p1=8, p2=32, uniqueness_ratio=10, disp12_max_diff=1, paths=8)
CASES = {
    "noise-4-paths": ("noise", 96, 48, dict(BASE, paths=4)),
    "noise-8-paths": ("noise", 96, 48, BASE),
    "odd-narrower-than-a-tile": ("noise", 67, 37, dict(BASE, num_disparities=16)),
    "two-per-lane": ("noise", 131, 53, dict(BASE, num_disparities=128)),
    "four-per-lane-D-above-width": ("noise", 200, 20, dict(BASE, num_disparities=256)),
    "three-per-lane-last-lane-partial": ("noise", 75, 21, dict(BASE, num_disparities=176, paths=4)),
    "min-disparity-negative": ("noise", 96, 48, dict(BASE, min_disparity=-8)),
    "min-disparity-positive": ("noise", 96, 48, dict(BASE, min_disparity=3)),
    "no-uniqueness": ("noise", 96, 48, dict(BASE, uniqueness_ratio=0)),
    "no-left-right-check": ("noise", 96, 48, dict(BASE, disp12_max_diff=-1)),
    "zero-penalties": ("noise", 96, 48, dict(BASE, p1=0, p2=0)),
    "largest-penalties": ("noise", 96, 48, dict(BASE, p1=255, p2=255)),
    "board-4-paths": ("board", 96, 48, dict(BASE, paths=4)),
    "board-8-paths": ("board", 96, 48, BASE),
    "board-no-checks": ("board", 96, 48, dict(BASE, uniqueness_ratio=0, disp12_max_diff=-1)),
    # rows of more than one kCostSegment = 256 pixel segment
    "exactly-one-segment": ("noise", 256, 4, BASE),
    "second-segment-of-one-pixel": ("noise", 257, 5, dict(BASE, num_disparities=16, paths=4)),
    "two-segments-full-window": ("noise", 300, 9, dict(BASE, num_disparities=256, min_disparity=-8)),
    "three-segments-positive-min": ("noise", 513, 6, dict(BASE, num_disparities=64, min_disparity=3)),
    "two-segments-board": ("board", 300, 12, BASE),
    # winners at negative disparity: the kR entries of the second block are fed from columns below s0, inside lo = s0 + dmin
    "two-segments-negative-disparity": ("noise-swapped", 300, 9, dict(BASE, min_disparity=-24)),
    # taller than wide, fewer than 4 scanlines, below the census window
    "tall-diagonals-wrap-thrice": ("noise", 21, 75, BASE),
    "three-columns": ("noise", 3, 40, dict(BASE, num_disparities=16)),
    "single-column": ("noise", 1, 70, dict(BASE, num_disparities=16)),
    "single-row": ("noise", 70, 1, dict(BASE, num_disparities=16)),
    "below-census-window": ("noise", 8, 6, dict(BASE, num_disparities=16, min_disparity=-4)),
    "one-pixel": ("noise", 1, 1, dict(BASE, num_disparities=16, paths=4)),
}
SEGMENT = 256                    # kCostSegment of tscm_stereo.hip


def _differs(a, b):
    bad = np.argwhere(np.asarray(a) != np.asarray(b))
    return f"{len(bad)} of {np.asarray(a).size} differ, first at {bad[0].tolist() if len(bad) else None}"


@pytest.mark.parametrize("case", list(CASES))
def test_stages_and_disparity_equal_the_reference(hip_device, case):
    name, w, h, p = CASES[case]
    left, right = _pair(name, w, h)
    ref = _reference(name, w, h, tuple(sorted(p.items())))
    got = stereo.stages(left, right, device=hip_device, **p)
    for stage in ("census_left", "census_right", "cost", "aggregated"):
        assert got[stage].dtype == ref[stage].dtype and got[stage].shape == ref[stage].shape
        assert np.array_equal(got[stage], ref[stage]), f"{stage}: {_differs(got[stage], ref[stage])}"
    disp = stereo.match(left, right, device=hip_device, **p)
    assert disp.dtype == np.int16 and np.array_equal(disp, ref["disparity"]), _differs(disp, ref["disparity"])
    if name == "noise" and (w, h) == (96, 48) and p.get("min_disparity", 0) == 0 and p["p2"] == 32:
        assert np.mean(disp != -16) > 0.5                    # the case does exercise the valid branch


def test_row_padding_in_and_out(hip_device):
    w, h, p = 96, 48, BASE
    left, right = _pair("noise", w, h)
    ref = _reference("noise", w, h, tuple(sorted(p.items())))
    wide = [np.full((h, w + 5), 201, dtype=np.uint8) for _ in range(2)]
    wide[0][:, :w], wide[1][:, :w] = left, right
    out = np.full((h, w + 3), -12345, dtype=np.int16)
    got = stereo.match(wide[0][:, :w], wide[1][:, :w], device=hip_device, out=out[:, :w], **p)
    assert got.strides[0] == 2 * (w + 3)
    assert np.array_equal(out[:, :w], ref["disparity"])
    assert np.all(out[:, w:] == -12345), "the padding of the disparity rows keeps the caller's values"
    st = stereo.stages(wide[0][:, :w], wide[1][:, :w], device=hip_device, **p)
    assert np.array_equal(st["aggregated"], ref["aggregated"]) and np.array_equal(st["census_right"], ref["census_right"])


def test_two_segments_without_left_right_check(hip_device):
    """300 x 9 with D = 256: the winner over a row of two segments when k_right_winner does not run and the uniqueness rule is
    off, from contiguous images and from row-padded views into a row-padded output."""
    w, h, p = 300, 9, dict(BASE, num_disparities=256, disp12_max_diff=-1, uniqueness_ratio=0)
    left, right = _pair("noise", w, h)
    ref = _reference("noise", w, h, tuple(sorted(p.items())))
    got = stereo.stages(left, right, device=hip_device, **p)
    for stage in ("census_left", "census_right", "cost", "aggregated"):
        assert got[stage].dtype == ref[stage].dtype and got[stage].shape == ref[stage].shape
        assert np.array_equal(got[stage], ref[stage]), f"{stage}: {_differs(got[stage], ref[stage])}"
    disp = stereo.match(left, right, device=hip_device, **p)
    assert disp.dtype == np.int16 and np.array_equal(disp, ref["disparity"]), _differs(disp, ref["disparity"])
    assert np.all(disp != 16 * (p.get("min_disparity", 0) - 1))          # neither rule runs: no pixel is invalid
    wide = [np.full((h, w + 5), 201, dtype=np.uint8) for _ in range(2)]
    wide[0][:, :w], wide[1][:, :w] = left, right
    out = np.full((h, w + 3), -12345, dtype=np.int16)
    padded = stereo.match(wide[0][:, :w], wide[1][:, :w], device=hip_device, out=out[:, :w], **p)
    assert padded.strides[0] == 2 * (w + 3)
    assert np.array_equal(out[:, :w], ref["disparity"]), _differs(out[:, :w], ref["disparity"])
    assert np.all(out[:, w:] == -12345), "the padding of the disparity rows keeps the caller's values"
    st = stereo.stages(wide[0][:, :w], wide[1][:, :w], device=hip_device, **p)
    for stage in ("census_left", "census_right", "cost", "aggregated"):
        assert np.array_equal(st[stage], ref[stage]), f"{stage}, padded: {_differs(st[stage], ref[stage])}"


def test_two_calls_give_the_same_bits(hip_device):
    left, right = _pair("board", 96, 48)
    a, b = stereo.match(left, right, device=hip_device, **BASE), stereo.match(left, right, device=hip_device, **BASE)
    assert np.array_equal(a, b)
    sa, sb = stereo.stages(left, right, device=hip_device, **BASE), stereo.stages(left, right, device=hip_device, **BASE)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    t = stereo.stage_times()
    assert set(t) == set(stereo.STAGE_NAMES) and t["aggregate"] > 0.0


# ------------------------------------------------------------------------------------------------ points
def _two_ray_points(kind, x, y, d16, fx, fy, cx, cy, B):
    """The point closest to the rays of pixel (x, y) from the origin and of pixel (x - d, y) from (B, 0, 0), in extended
    precision: independent of the closed forms of tscm_stereo_points."""
    ld = np.longdouble
    x, y, d = np.asarray(x, dtype=ld), np.asarray(y, dtype=ld), np.asarray(d16, dtype=ld) / ld(16)
    fx, fy, cx, cy, B = ld(fx), ld(fy), ld(cx), ld(cy), ld(B)

    def direction(col):
        a, b = (col - cx) / fx, (y - cy) / fy
        if kind == "perspective":
            return np.stack([a, b, np.ones_like(a)], axis=-1)
        return np.stack([np.sin(a), np.cos(a) * np.sin(b), np.cos(a) * np.cos(b)], axis=-1)

    # the header forms aL in fp64 and subtracts d / fx from it; the rays here take the same two angles
    aL = ((np.asarray(x, dtype=np.float64) - float(cx)) / float(fx)).astype(ld)
    da = ((np.asarray(d16, dtype=np.float64) / 16.0) / float(fx)).astype(ld)
    if kind == "perspective":
        u, v = direction(x), direction(x - d)
    else:
        b = ((np.asarray(y, dtype=np.float64) - float(cy)) / float(fy)).astype(ld)
        u = np.stack([np.sin(aL), np.cos(aL) * np.sin(b), np.cos(aL) * np.cos(b)], axis=-1)
        v = np.stack([np.sin(aL - da), np.cos(aL - da) * np.sin(b), np.cos(aL - da) * np.cos(b)], axis=-1)
    c = np.zeros(u.shape, dtype=ld)
    c[..., 0] = B
    # minimise |s u - (c + t v)|^2
    uu, vv, uv = (u * u).sum(-1), (v * v).sum(-1), (u * v).sum(-1)
    uc, vc = (u * c).sum(-1), (v * c).sum(-1)
    det = uu * vv - uv * uv
    s = (uc * vv - vc * uv) / det
    t = (uc * uv - vc * uu) / det
    return ((s[..., None] * u + c + t[..., None] * v) / ld(2)).astype(np.float64)


@pytest.mark.parametrize("kind", ["perspective", "longlat"])
def test_points_against_two_rays(hip_device, kind):
    w, h, B = 160, 80, 434.0
    if kind == "longlat":
        desc = maps.MapDesc(synth.CALIB_INTR[0], np.eye(3), w / np.pi, h / (np.pi / 2), w / 2.0, h / 2.0, w, h, projection="longlat")
    else:
        desc = maps.MapDesc(synth.CALIB_INTR[0], np.eye(3), 80.0, 80.0, w / 2.0, h / 2.0, w, h, projection="perspective")
    min_disparity = -2
    invalid = 16 * (min_disparity - 1)
    rng = np.random.default_rng(11)
    # 1 .. 30 px in 1/16 steps, kept 3 px short of the column index: in the long-lat image d = x puts aR at -pi/2, the
    # point into the right camera's centre and its norm at zero, where a relative error says nothing
    xs = np.arange(w)
    disp = np.minimum(rng.integers(16, 16 * 30, (h, w)), np.maximum(16 * (xs - 3), 8)[None, :]).astype(np.int16)
    disp[:, 0] = invalid                                                 # aL = -pi/2: no positive disparity keeps aR inside
    disp[:, 1] = 8                                                       # next to aL = -pi/2, aR half a pixel further out
    disp[:, w - 1] = rng.integers(16, 16 * 30, h)                        # next to aL = +pi/2
    disp[5, 7], disp[6, 9], disp[7, 11], disp[8, 13] = invalid, 0, -16, -5  # the invalid value and non-positive disparities
    pts, valid = stereo.points(disp, desc, B, min_disparity=min_disparity, device=hip_device)
    expect_valid = (disp != invalid) & (disp > 0)
    assert valid.dtype == bool and np.array_equal(valid, expect_valid)
    assert np.all(np.isnan(pts[~valid])) and np.all(np.isfinite(pts[valid]))
    yy, xx = np.mgrid[0:h, 0:w]
    ref = _two_ray_points(kind, xx[valid], yy[valid], disp[valid], desc.fx, desc.fy, desc.cx, desc.cy, B)
    err = np.linalg.norm(pts[valid] - ref, axis=-1) / np.linalg.norm(ref, axis=-1)
    print(f"{kind}: largest relative distance to the two-ray point {err.max():.3e}")
    assert err.max() <= 1e-12
    # the header's closed forms, restated on the host, agree as well
    hp, hv = R.points(disp, desc.fx, desc.fy, desc.cx, desc.cy, B, kind, min_disparity)
    assert np.array_equal(hv, valid)
    assert np.max(np.linalg.norm(pts[valid] - hp[valid], axis=-1) / np.linalg.norm(hp[valid], axis=-1)) <= 1e-12
    # a padded disparity array gives the same points
    wide = np.full((h, w + 3), invalid, dtype=np.int16)
    wide[:, :w] = disp
    p2, v2 = stereo.points(wide[:, :w], desc, B, min_disparity=min_disparity, device=hip_device)
    assert np.array_equal(v2, valid) and np.array_equal(p2[valid], pts[valid])


# ------------------------------------------------------------------------------------------------ end to end
PLANE_N = np.array([0.65, 0.1, 0.75]) / np.linalg.norm([0.65, 0.1, 0.75])   # rig frame, facing the overlap of cameras 0 and 1
PLANE_C = 2500.0                                                          # n . X = c, millimetres
SCENE = dict(width=160, height=80, num_disparities=32, p1=8, p2=32, uniqueness_ratio=10, disp12_max_diff=1, paths=8)
# Median distance of the valid points to the plane, measured with the reference chain on the CPU (maps_proj_ref tables,
# the oracle's remap, stereo_ref matcher and points): 78.93 mm at 2500 mm (74 % of the pixels valid); the plane is seen at
# about 5 pixels of disparity, where one 1/16-pixel step is 31 mm of range.  The device chain differs from it in the fp64 sincos of the table kernel only; a factor 2 covers that.
PLANE_MEDIAN_CPU_MM = 78.93
PLANE_MEDIAN_BOUND_MM = 2.0 * PLANE_MEDIAN_CPU_MM


def _hash_gray(qx, qy):
    key = (qx.astype(np.int64) * 73856093) ^ (qy.astype(np.int64) * 19349663)
    return (synth.splitmix64(key.astype(np.uint64)) >> np.uint64(56)).astype(np.float64)


def render_textured_plane(intr, Twc, width, height, cell=110.0, supersample=2):
    """The ray / plane intersection of synth.render_chessboard for a plane n . X = c of the rig frame, painted with square
    cells of hashed grey; the camera sits at Twc = [R | t] (camera to rig)."""
    Rc, tc = Twc[:, :3], Twc[:, 3]
    e1 = np.cross(PLANE_N, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(PLANE_N, e1)
    offs = (np.arange(supersample) + 0.5) / supersample - 0.5
    acc = np.zeros((height, width))
    jj, ii = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    for oy in offs:
        for ox in offs:
            d = synth.unproject_pixels_np(intr, jj + ox, ii + oy) @ Rc.T          # rays in the rig frame
            den = d @ PLANE_N
            s = (PLANE_C - tc @ PLANE_N) / np.where(np.abs(den) < 1e-12, 1e-12, den)
            P = tc + d * s[..., None]
            g = _hash_gray(np.floor(P @ e1 / cell), np.floor(P @ e2 / cell))
            acc += np.where(s > 0, g, 0.0)
    return np.clip(np.rint(acc / supersample ** 2), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def plane_scene():
    """Cameras 0 and 1 of synth.rig(4) at a quarter of their resolution, and their images of the plane."""
    intr, _ = synth.rig(4)
    intr = intr.copy()
    intr[:, :4] *= 0.25
    T = synth.CALIB_TWC
    imgs = [render_textured_plane(intr[k], T[k], 320, 270) for k in (0, 1)]
    return intr, T, imgs


def plane_distances(pts, valid, Rp, t_a):
    X = pts[valid] @ Rp.T + t_a
    return np.abs(X @ PLANE_N - PLANE_C)


def reference_chain():
    """pair_depth on the CPU: reference tables, the oracle's remap, the host matcher and points."""
    intr, T, imgs = plane_scene()
    p = {k: v for k, v in SCENE.items() if k not in ("width", "height")}
    descs = maps.rectify_pair_descs(intr[0], T[0], intr[1], T[1], "longlat", SCENE["width"], SCENE["height"])
    rect = []
    for img, d in zip(imgs, descs):
        mx, my, _ = mref.build_map_ref(d)
        rect.append(orc.remap(img, mx, my))
    disp = R.match(rect[0], rect[1], **p)
    B = float(np.linalg.norm(T[1][:, 3] - T[0][:, 3]))
    pts, valid = R.points(disp, descs[0].fx, descs[0].fy, descs[0].cx, descs[0].cy, B, "longlat")
    return pts, valid, maps.rectify_pair_rotation(T[0][:, 3], T[1][:, 3]), disp


def test_pair_depth_on_a_textured_plane(hip_device):
    intr, T, imgs = plane_scene()
    seen = {}

    def both_matchers(left, right, **p):
        seen["gpu"] = stereo.match(left, right, device=hip_device, **p)
        seen["ref"] = R.match(left, right, **p)
        return seen["ref"]

    # the chain with the host matcher in place of the device's, on the same rectified images: equal disparity bits
    pts_r, valid_r, _ = stereo.pair_depth(imgs[0], imgs[1], intr[0], T[0], intr[1], T[1], device=hip_device, matcher=both_matchers, **SCENE)
    assert np.array_equal(seen["gpu"], seen["ref"]), _differs(seen["gpu"], seen["ref"])
    pts, valid, Rp = stereo.pair_depth(imgs[0], imgs[1], intr[0], T[0], intr[1], T[1], device=hip_device, **SCENE)
    assert pts.shape == (SCENE["height"], SCENE["width"], 3) and np.array_equal(valid, valid_r)
    assert np.array_equal(pts[valid], pts_r[valid])
    assert np.allclose(Rp, maps.rectify_pair_rotation(T[0][:, 3], T[1][:, 3]), rtol=0, atol=0)
    share = valid.mean()
    median = float(np.median(plane_distances(pts, valid, Rp, T[0][:, 3])))
    print(f"plane at {PLANE_C:.0f} mm: {100 * share:.1f} % of the pixels valid, median distance to the plane {median:.2f} mm "
          f"(reference chain on the CPU {PLANE_MEDIAN_CPU_MM} mm, bound {PLANE_MEDIAN_BOUND_MM} mm)")
    assert valid.any()
    assert median <= PLANE_MEDIAN_BOUND_MM
