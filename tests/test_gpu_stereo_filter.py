"""GPU tests of the disparity post-filter (tscm_stereo_filter, tscm_stereo_filter_stages): labels, sizes, the despeckled
map and the final map equal the host restatement tests/stereo_filter_ref.py bit for bit (integers and order-independent
reductions only, so there is no tolerance), on shapes chosen to break raster-scan labelling, single-pass seam merging,
16-bit or per-tile counters and 16-bit differences; and stereo.pair_depth(post=...) removes outliers of a plane scene."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import maps, stereo, synth
from tests import maps_proj_ref as mref
from tests import stereo_filter_ref as F
from tests import stereo_ref as R

pytestmark = pytest.mark.gpu

INV = -16                                                                     # min_disparity = 0
TILE_W, TILE_H = 64, 16                                                       # the kernels' tile


def _differs(a, b):
    bad = np.argwhere(np.asarray(a) != np.asarray(b))
    return f"{len(bad)} of {np.asarray(a).size} differ, first at {bad[0].tolist() if len(bad) else None}"


def _check(device, d, **p):
    """Every stage and the final map of the device against the restatement; returns the restatement's stages."""
    ref = F.stages(d, **p)
    got = stereo.filter_stages(d, device=device, **p)
    for stage in ("label", "size", "despeckled"):
        assert got[stage].dtype == ref[stage].dtype and got[stage].shape == ref[stage].shape, stage
        assert np.array_equal(got[stage], ref[stage]), f"{stage}: {_differs(got[stage], ref[stage])}"
    out = stereo.filter(d, device=device, **p)
    assert out.dtype == np.int16 and np.array_equal(out, ref["out"]), f"out: {_differs(out, ref['out'])}"
    return ref


@functools.lru_cache(maxsize=None)
def _random_map(w, h, invalid=INV):
    """Three levels, two of them 16 apart (joined at speckle_range >= 1), 30 % invalid."""
    rng = np.random.default_rng(100 * w + h)
    d = rng.choice(np.array([160, 176, 400], dtype=np.int16), size=(h, w))
    d[rng.random((h, w)) < 0.3] = invalid
    d.setflags(write=False)
    return d


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("w,h", [(1, 1), (1, 70), (70, 1), (63, 15), (64, 16), (65, 17), (130, 35)])
def test_sizes_below_a_tile_and_tile_remainders(hip_device, w, h):
    d = _random_map(w, h)
    ref = _check(hip_device, d, speckle_window_size=4, speckle_range=1)
    if w * h > 900:
        assert np.any((d != INV) & (ref["out"] == INV)) and np.any(ref["out"] != INV)    # the rule removes some and keeps some
    _check(hip_device, d, speckle_window_size=0, speckle_range=0)


# ------------------------------------------------------------------------------------------------ shapes
def _u_shape():
    """Two arms in tile columns 0 and 1, joined only along row 33, the middle row of the tiles of tile row 2."""
    w, h = 130, 35
    d = np.full((h, w), INV, dtype=np.int16)
    d[0:34, 10] = 320
    d[0:34, 100] = 320
    d[33, 10:101] = 320
    return d, 10, 34 + 34 + 89


def _spiral(w=200, h=72):
    """A one-pixel-wide rectangular spiral from (0, 0) inwards, one pixel of gap between its turns."""
    d = np.full((h, w), INV, dtype=np.int16)
    x = y = k = 0
    d[0, 0] = 320
    steps = ((1, 0), (0, 1), (-1, 0), (0, -1))

    def free(px, py):
        return 0 <= px < w and 0 <= py < h and d[py, px] == INV

    while True:
        for _ in range(2):
            dx, dy = steps[k]
            ahead_painted = 0 <= x + 2 * dx < w and 0 <= y + 2 * dy < h and d[y + 2 * dy, x + 2 * dx] != INV
            if free(x + dx, y + dy) and not ahead_painted:
                break
            k = (k + 1) % 4
        else:
            return d, 0, int((d != INV).sum())
        x, y = x + dx, y + dy
        d[y, x] = 320


def _serpentine(w=192, h=64):
    d = np.full((h, w), INV, dtype=np.int16)
    d[0::2] = 320
    for j, y in enumerate(range(1, h - 1, 2)):
        d[y, w - 1 if j % 2 == 0 else 0] = 320
    return d, 0, (h // 2) * w + (h // 2 - 1)


@pytest.mark.parametrize("shape", ["u", "spiral", "serpentine"])
def test_one_component_through_many_tiles(hip_device, shape):
    d, first, count = dict(u=_u_shape, spiral=_spiral, serpentine=_serpentine)[shape]()
    assert int(np.flatnonzero(d.ravel() != INV)[0]) == first and int((d != INV).sum()) == count
    if shape == "spiral":
        assert count > 200 * 72 // 3                                          # it does wind through the whole map
    ref = _check(hip_device, d, speckle_window_size=count, speckle_range=0)   # exactly the window: everything goes
    assert np.all(ref["label"][d != INV] == first) and np.all(ref["size"][d != INV] == count)
    assert np.all(ref["out"] == INV)
    ref = _check(hip_device, d, speckle_window_size=count - 1, speckle_range=0, median=3)
    assert np.array_equal(ref["despeckled"], d)


def test_checkerboard_of_isolated_pixels(hip_device):
    w, h = 128, 32
    yy, xx = np.mgrid[0:h, 0:w]
    on = (xx + yy) % 2 == 0
    d = np.where(on, 320, INV).astype(np.int16)
    ref = _check(hip_device, d, speckle_window_size=0, speckle_range=255)
    assert np.array_equal(ref["label"][on], (yy * w + xx)[on]) and np.all(ref["size"][on] == 1)
    ref = _check(hip_device, d, speckle_window_size=1, speckle_range=255, median=5)
    assert np.all(ref["out"] == INV)


def test_component_larger_than_65535_pixels(hip_device):
    w, h = 320, 256
    d = np.full((h, w), 320, dtype=np.int16)
    d[128, 160] = INV
    ref = _check(hip_device, d, speckle_window_size=81918, speckle_range=0)
    assert np.all(ref["size"][d != INV] == 81919) and ref["size"][128, 160] == 0 and np.all(ref["label"][d != INV] == 0)
    assert np.array_equal(ref["out"], d)
    ref = _check(hip_device, d, speckle_window_size=81919, speckle_range=0)
    assert np.all(ref["out"] == INV)


# ------------------------------------------------------------------------------------------------ thresholds
def _threshold_map(speckle_range, lo, hi):
    """Pairs and runs across the tile borders x = 63 | 64 and y = 15 | 16 of a 130 x 35 map, values from lo upwards and
    the far pair (lo, hi), whose difference does not fit 16 bits."""
    thr = 16 * speckle_range
    inv = -32768                                                              # min_disparity = -2047
    d = np.full((35, 130), inv, dtype=np.int16)
    d[2, 63], d[2, 64] = lo, lo + thr                                         # on the threshold: one component of 2
    d[4, 63], d[4, 64] = lo, lo + thr + 1                                     # one past it: two of 1
    d[6, 63], d[6, 64] = lo, hi                                               # 65504 apart at the int16 extremes
    d[15, 20], d[16, 20] = hi - thr, hi                                       # the same across a horizontal border
    d[15, 24], d[16, 24] = hi - thr - 1, hi
    d[15, 28], d[16, 28] = hi, lo
    d[10, 61:66] = lo + 5                                                     # a run of 5 across x = 63 | 64
    d[12, 60:66] = lo + 5                                                     # a run of 6
    d[13:18, 100] = hi - 7                                                    # a column of 5 across y = 15 | 16
    d[13:19, 104] = hi - 7                                                    # a column of 6
    return d


@pytest.mark.parametrize("speckle_range", [0, 255])
def test_window_and_range_on_and_past_the_threshold(hip_device, speckle_range):
    lo, hi = -32752, 32752                                                    # 16 * -2047 and 16 * 2047: what the matcher can emit
    d = _threshold_map(speckle_range, lo, hi)
    ref = _check(hip_device, d, min_disparity=-2047, speckle_window_size=5, speckle_range=speckle_range, median=3)
    w = 130
    assert ref["label"][2, 64] == 2 * w + 63 and ref["size"][2, 63] == 2
    assert ref["label"][4, 64] == 4 * w + 64 and ref["size"][4, 63] == 1
    assert ref["label"][6, 64] == 6 * w + 64, "the difference of the extremes is 65504, not its 16-bit remainder"
    assert ref["label"][16, 20] == 15 * w + 20 and ref["label"][16, 24] == 16 * w + 24 and ref["label"][16, 28] == 16 * w + 28
    inv = -32768
    assert np.all(ref["despeckled"][10, 61:66] == inv) and np.all(ref["despeckled"][12, 60:66] == lo + 5)     # 5 goes, 6 stays
    assert np.all(ref["despeckled"][13:18, 100] == inv) and np.all(ref["despeckled"][13:19, 104] == hi - 7)


def test_negative_min_disparity_and_an_all_invalid_map(hip_device):
    d = _random_map(65, 17, invalid=-96).copy()
    d[d == 160] = -16                                                         # a valid value under min_disparity = -5
    ref = _check(hip_device, d, min_disparity=-5, speckle_window_size=3, speckle_range=1, median=3)
    assert np.any(ref["out"] == -16) and np.any((d == -16) & (ref["out"] == -96))
    none = np.full((35, 130), -96, dtype=np.int16)
    ref = _check(hip_device, none, min_disparity=-5, speckle_window_size=3, speckle_range=1, median=5)
    assert np.all(ref["label"] == -1) and np.all(ref["size"] == 0) and np.all(ref["out"] == -96)


# ------------------------------------------------------------------------------------------------ median
def removed_neighbour_across_a_tile_corner(d, st):
    """Is there a kept pixel within two pixels of a tile corner whose 5 x 5 window holds a pixel of another tile that the
    speckle rule removed?"""
    h, w = d.shape
    removed = (d != INV) & (st["despeckled"] == INV)
    for y, x in np.argwhere(st["despeckled"] != INV):
        near = (x % TILE_W in (0, 1, TILE_W - 2, TILE_W - 1)) and (y % TILE_H in (0, 1, TILE_H - 2, TILE_H - 1))
        if not near or x < 2 or y < 2 or x >= w - 2 or y >= h - 2:
            continue
        for qy in range(y - 2, y + 3):
            for qx in range(x - 2, x + 3):
                if removed[qy, qx] and qy // TILE_H != y // TILE_H and qx // TILE_W != x // TILE_W:
                    return True
    return False


@pytest.mark.parametrize("w,h", [(65, 17), (130, 35)])
@pytest.mark.parametrize("median", [3, 5])
@pytest.mark.parametrize("window", [0, 4])
def test_masked_median(hip_device, w, h, median, window):
    d = _random_map(w, h)
    ref = _check(hip_device, d, speckle_window_size=window, speckle_range=1, median=median)
    assert np.any(ref["out"] != ref["despeckled"]), "the median changes something"
    assert np.array_equal(ref["out"] == INV, ref["despeckled"] == INV), "no hole is filled and no pixel dropped"
    if window and (w, h) == (130, 35):
        assert removed_neighbour_across_a_tile_corner(d, ref)


# ------------------------------------------------------------------------------------------------ padding, in place
def test_row_padding_in_place_and_repeatability(hip_device):
    w, h = 130, 35
    d = _random_map(w, h)
    p = dict(speckle_window_size=4, speckle_range=1, median=3)
    ref = F.stages(d, **p)
    wide_in = np.full((h, w + 5), 777, dtype=np.int16)
    wide_in[:, :w] = d
    wide_out = np.full((h, w + 3), -12345, dtype=np.int16)
    got = stereo.filter(wide_in[:, :w], device=hip_device, out=wide_out[:, :w], **p)
    assert got.strides[0] == 2 * (w + 3)
    assert np.array_equal(wide_out[:, :w], ref["out"]), _differs(wide_out[:, :w], ref["out"])
    assert np.all(wide_out[:, w:] == -12345), "the padding of the output rows keeps the caller's values"
    assert np.all(wide_in[:, w:] == 777) and np.array_equal(wide_in[:, :w], d), "the input is not written"
    st = stereo.filter_stages(wide_in[:, :w], device=hip_device, **p)
    assert np.array_equal(st["label"], ref["label"]) and np.array_equal(st["despeckled"], ref["despeckled"])
    # in place: out is the padded input view itself
    view = wide_in[:, :w]
    same = stereo.filter(view, device=hip_device, out=view, **p)
    assert same is view and np.array_equal(wide_in[:, :w], ref["out"]) and np.all(wide_in[:, w:] == 777)
    # two calls on the same input give the same bits
    a, b = stereo.filter_stages(d, device=hip_device, **p), stereo.filter_stages(d, device=hip_device, **p)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    out, sec = stereo.filter(d, device=hip_device, with_seconds=True, **p)
    assert np.array_equal(out, stereo.filter(d, device=hip_device, **p)) and sec > 0.0


# ------------------------------------------------------------------------------------------------ matcher output
BASE = dict(num_disparities=32, p1=8, p2=32, uniqueness_ratio=10, disp12_max_diff=1, paths=8)


def _board_pair(w=96, h=48):
    """The chessboard pair of the matcher's tests: large flat regions and their islands of wrong matches."""
    intr = synth.CALIB_INTR[0].copy()
    intr[:4] *= w / synth.IMG_W
    intr[3] = h / 2.0
    views = []
    for tx in (-160.0, -120.0):
        rt = np.array([0.05, -0.1, 0.02, tx, -110.0, 420.0])
        views.append(synth.render_chessboard(intr, rt, 5, 3, 60.0, w, h, supersample=1))
    return views[0], views[1]


def test_filter_of_a_real_matcher_output(hip_device):
    left, right = _board_pair()
    disp = stereo.match(left, right, device=hip_device, **BASE)
    assert np.array_equal(disp, R.match(left, right, **BASE))
    # with the default parameters (window 100, range 2) this 96 x 48 map has components on both sides of the rule
    _, size = F.components(disp, 0, 2)
    assert np.any((size > 0) & (size <= 100)) and np.any(size > 100)
    ref = _check(hip_device, disp)
    assert np.any((disp != INV) & (ref["out"] == INV)) and np.any(ref["out"] != INV)
    _check(hip_device, disp, median=5)


# ------------------------------------------------------------------------------------------------ end to end
PLANE_N = np.array([0.65, 0.1, 0.75]) / np.linalg.norm([0.65, 0.1, 0.75])     # rig frame, facing the overlap of cameras 0 and 1
PLANE_C = 2500.0                                                              # n . X = c, millimetres
SCENE = dict(width=160, height=80, num_disparities=32, p1=8, p2=32, uniqueness_ratio=10, disp12_max_diff=1, paths=8)
POST = dict(speckle_window_size=100, speckle_range=2)
OUTLIER_MM = 1000.0


def _hash_gray(qx, qy):
    key = (qx.astype(np.int64) * 73856093) ^ (qy.astype(np.int64) * 19349663)
    return (synth.splitmix64(key.astype(np.uint64)) >> np.uint64(56)).astype(np.float64)


def _render_textured_plane(intr, Twc, width, height, cell=110.0, supersample=2):
    """The plane n . X = c of the rig frame, painted with square cells of hashed grey, seen from Twc = [R | t]."""
    Rc, tc = Twc[:, :3], Twc[:, 3]
    e1 = np.cross(PLANE_N, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(PLANE_N, e1)
    offs = (np.arange(supersample) + 0.5) / supersample - 0.5
    acc = np.zeros((height, width))
    jj, ii = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    for oy in offs:
        for ox in offs:
            rays = synth.unproject_pixels_np(intr, jj + ox, ii + oy) @ Rc.T
            den = rays @ PLANE_N
            s = (PLANE_C - tc @ PLANE_N) / np.where(np.abs(den) < 1e-12, 1e-12, den)
            P = tc + rays * s[..., None]
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
    return intr, T, [_render_textured_plane(intr[k], T[k], 320, 270) for k in (0, 1)]


def outliers(pts, valid, Rp, t_a):
    """Valid points farther than OUTLIER_MM from the plane."""
    X = pts[valid] @ Rp.T + t_a
    return int(np.sum(np.abs(X @ PLANE_N - PLANE_C) > OUTLIER_MM))


@functools.lru_cache(maxsize=None)
def reference_chain():
    """pair_depth on the CPU: reference tables, the oracle's remap, the host matcher, the host filter and host points.
    -> (outliers without the filter, outliers with it, filtered disparity)."""
    intr, T, imgs = plane_scene()
    p = {k: v for k, v in SCENE.items() if k not in ("width", "height")}
    descs = maps.rectify_pair_descs(intr[0], T[0], intr[1], T[1], "longlat", SCENE["width"], SCENE["height"])
    rect = []
    for img, d in zip(imgs, descs):
        mx, my, _ = mref.build_map_ref(d)
        rect.append(orc.remap(img, mx, my))
    disp = R.match(rect[0], rect[1], **p)
    B = float(np.linalg.norm(T[1][:, 3] - T[0][:, 3]))
    Rp = maps.rectify_pair_rotation(T[0][:, 3], T[1][:, 3])
    counts = []
    for dmap in (disp, F.filter(disp, **POST)):
        pts, valid = R.points(dmap, descs[0].fx, descs[0].fy, descs[0].cx, descs[0].cy, B, "longlat")
        counts.append(outliers(pts, valid, Rp, T[0][:, 3]))
    return counts[0], counts[1], F.filter(disp, **POST)


# Measured with reference_chain() on the CPU, POST = window 100, range 2, on the 160 x 80 long-lat pair:
# valid points farther than 1 m from the plane without the filter / with it.
OUTLIERS_CPU_UNFILTERED = 386
OUTLIERS_CPU_FILTERED = 250


def test_pair_depth_with_the_post_filter(hip_device):
    intr, T, imgs = plane_scene()
    seen = {}

    def host_matcher_and_filter(left, right, **p):
        seen["gpu"] = stereo.filter(stereo.match(left, right, device=hip_device, **p), device=hip_device, **POST)
        seen["ref"] = F.filter(R.match(left, right, **p), **POST)
        return seen["ref"]

    # the chain with the host matcher + host filter on the same rectified images: equal disparity bits
    pts_r, valid_r, Rp = stereo.pair_depth(imgs[0], imgs[1], intr[0], T[0], intr[1], T[1], device=hip_device, matcher=host_matcher_and_filter, **SCENE)
    assert np.array_equal(seen["gpu"], seen["ref"]), _differs(seen["gpu"], seen["ref"])
    pts, valid, _ = stereo.pair_depth(imgs[0], imgs[1], intr[0], T[0], intr[1], T[1], device=hip_device, post=POST, **SCENE)
    assert np.array_equal(valid, valid_r) and np.array_equal(pts[valid], pts_r[valid])
    pts_u, valid_u, _ = stereo.pair_depth(imgs[0], imgs[1], intr[0], T[0], intr[1], T[1], device=hip_device, **SCENE)
    assert np.all(valid_u[valid]) and valid.sum() < valid_u.sum(), "the filter only removes"
    unfiltered_cpu, filtered_cpu, _ = reference_chain()
    assert (unfiltered_cpu, filtered_cpu) == (OUTLIERS_CPU_UNFILTERED, OUTLIERS_CPU_FILTERED), "the figures recorded in DESIGN"
    got_u, got_f = outliers(pts_u, valid_u, Rp, T[0][:, 3]), outliers(pts, valid, Rp, T[0][:, 3])
    print(f"plane at {PLANE_C:.0f} mm, valid points farther than {OUTLIER_MM:.0f} mm from it: {got_u} without the filter, {got_f} with "
          f"{POST} (reference chain on the CPU: {unfiltered_cpu}, {filtered_cpu}); {valid_u.sum()} -> {valid.sum()} valid points")
    assert got_f == filtered_cpu
    assert filtered_cpu < unfiltered_cpu
