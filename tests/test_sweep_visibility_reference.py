"""CPU tests of the per-camera visibility at the swept depth: the properties of the definition on the host restatement
tests/sweep_visibility_ref.py with hand-made records and tables (the occlusion threshold, the dilation and the grid edge, the
mirrored ranks, untested pixels, the guard state, tolerance = 255 and a constant map against sweep_compose_ref.compose), the
exports, defaults and the NULL-handle refusal of the C ABI, and the reference figures of the occluder scene that
tests/test_gpu_sweep_visibility.py uses."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import maps_proj_ref as mref
from tests import sweep_compose_ref as CR
from tests import sweep_ref
from tests import sweep_visibility_ref as V
from tests import test_gpu_sweep as scene
from tscm_calib_amd import lib, sweep, synth

SIZE = (16, 12)          # width, height of the hand-made source images
D = 16


def _one_camera(entries, **params):
    """entries: (ix, iy, alpha, index16) per panorama pixel of a one-row panorama, one camera"""
    e = np.array(entries, dtype=np.int64).reshape(-1, 4)
    ix, iy, a, idx = (e[:, k][None, None] for k in range(4))
    return V.from_records(ix, iy, a, idx[0].astype(np.int16), D, SIZE, **{**V.DEFAULTS, **params})


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("r,t", [(0, 0), (3, 2), (2, 11)])
def test_two_pixels_in_one_cell_at_the_threshold(r, t):
    """Ranks r and r + t + 1 in one cell: the farther one is occluded; r and r + t: it is not.  One camera, so the occluded
    pixel is in the guard state 4 and keeps its source."""
    res = _one_camera([(5, 5, 200, 16 * r), (6, 6, 200, 16 * (r + t + 1))], cell_shift=2, tolerance=t)
    assert res["visible"][0, 0].tolist() == [0, 1] and res["state"][0].tolist() == [4, 2] and res["use"][0, 0].tolist() == [1, 1]
    assert res["depth_buffer"][0, 1, 1] == r + t + 2 and res["depth_buffer"].sum() == r + t + 2
    res = _one_camera([(5, 5, 200, 16 * r), (6, 6, 200, 16 * (r + t))], cell_shift=2, tolerance=t)
    assert res["visible"][0, 0].tolist() == [1, 1] and res["state"][0].tolist() == [2, 2]
    # cell_shift = 0: the two records lie in cells of their own
    res = _one_camera([(5, 5, 200, 16 * r), (6, 6, 200, 16 * (r + t + 1))], cell_shift=0, tolerance=t)
    assert res["visible"][0, 0].tolist() == [1, 1] and res["cell"][0, 0].tolist() == [5 * 16 + 5, 6 * 16 + 6]


def test_the_nearest_pixel_of_a_cell_is_visible_without_dilation():
    rng = np.random.default_rng(3)
    n, ph, pw = 3, 6, 40
    ix, iy = rng.integers(-3, SIZE[0] + 3, (n, ph, pw)), rng.integers(-3, SIZE[1] + 3, (n, ph, pw))
    a = rng.integers(0, 3, (n, ph, pw)) * 100
    idx = rng.integers(-16, 16 * D, (ph, pw)).astype(np.int16)
    for high in (0, 1):
        res = V.from_records(ix, iy, a, idx, D, SIZE, cell_shift=1, tolerance=0, dilate=0, near_is_high=high)
        z = np.minimum(D - 1, (idx.astype(np.int64) + 8) >> 4)
        rank1 = (z if high else D - 1 - z) + 1
        for k in range(n):
            on = res["cell"][k] >= 0
            top = res["depth_buffer"][k].ravel()[res["cell"][k][on]]
            assert np.array_equal(res["visible"][k][on], rank1[on] == top)       # tolerance 0: exactly the nearest ones
            assert set(np.unique(res["cell"][k][on & (res["visible"][k] > 0)])) == set(np.unique(res["cell"][k][on]))
        assert (res["state"] == 3).any()


def test_dilate_reaches_the_neighbour_cell_and_not_across_the_grid_edge():
    """16 x 12 pixels in 4 x 4 cells: a 4 x 3 grid.  The occluder sits in cell (1, 1)."""
    near, far = 16 * 9, 16 * 2
    res = _one_camera([(9, 5, 200, far), (5, 5, 200, near)], cell_shift=2, dilate=0)
    assert res["visible"][0, 0].tolist() == [1, 1]                             # cell (2, 1): a neighbour, not read
    res = _one_camera([(9, 5, 200, far), (5, 5, 200, near)], cell_shift=2, dilate=1)
    assert res["visible"][0, 0].tolist() == [0, 1]
    res = _one_camera([(13, 5, 200, far), (5, 5, 200, near)], cell_shift=2, dilate=1)
    assert res["visible"][0, 0].tolist() == [1, 1]                             # cell (3, 1): two cells away
    res = _one_camera([(13, 5, 200, far), (5, 5, 200, near)], cell_shift=2, dilate=2)
    assert res["visible"][0, 0].tolist() == [0, 1]
    # no wrap over the grid edge: an occluder in the last column does not reach the first, nor the row above through it
    res = _one_camera([(1, 5, 200, far), (14, 5, 200, near), (14, 1, 200, near)], cell_shift=2, dilate=2)
    assert res["visible"][0, 0].tolist() == [1, 1, 1]
    # records outside the image are clamped into the border cells
    res = _one_camera([(-7, -9, 200, far), (2, 1, 200, near), (40, 30, 200, near)], cell_shift=2, dilate=0)
    assert res["cell"][0, 0].tolist() == [0, 0, 2 * 4 + 3] and res["visible"][0, 0].tolist() == [0, 1, 1]


def test_near_is_high_0_mirrors_the_ranks():
    lo, hi = 16 * 3, 16 * 12
    a = _one_camera([(5, 5, 200, lo), (6, 6, 200, hi)], near_is_high=1)
    b = _one_camera([(5, 5, 200, lo), (6, 6, 200, hi)], near_is_high=0)
    assert a["visible"][0, 0].tolist() == [0, 1] and b["visible"][0, 0].tolist() == [1, 0]
    assert a["depth_buffer"][0, 1, 1] == 13 and b["depth_buffer"][0, 1, 1] == D - 1 - 3 + 1
    # mirroring the map mirrors the result
    c = _one_camera([(5, 5, 200, 16 * (D - 1) - lo), (6, 6, 200, 16 * (D - 1) - hi)], near_is_high=0)
    assert np.array_equal(c["visible"], a["visible"]) and np.array_equal(c["depth_buffer"], a["depth_buffer"])


def test_an_untested_pixel_does_not_occlude_and_alpha_0_neither():
    res = _one_camera([(5, 5, 200, 16 * 2), (6, 6, 200, -16), (6, 5, 0, 16 * 14)])
    assert res["visible"][0, 0].tolist() == [1, 0, 0] and res["state"][0].tolist() == [2, 0, 1]
    assert res["use"][0, 0].tolist() == [1, 1, 0] and res["cell"][0, 0].tolist() == [5, -1, -1]
    assert res["depth_buffer"].max() == 3 and res["hypothesis"][0].tolist() == [2, 0, 14]


def test_states_and_use_with_two_cameras():
    """Pixel 0 is far and lies behind pixel 1 in camera 0 only (state 3: camera 0 leaves), behind it in both cameras in the
    second run (state 4: both stay)."""
    idx = np.array([[16 * 2, 16 * 12]], dtype=np.int16)
    a = np.full((2, 1, 2), 180)
    iy = np.full((2, 1, 2), 5)
    res = V.from_records(np.array([[[5, 6]], [[1, 9]]]), iy, a, idx, D, SIZE, **V.DEFAULTS)
    assert res["state"][0].tolist() == [3, 2] and res["use"][:, 0, 0].tolist() == [0, 1] and res["use"][:, 0, 1].tolist() == [1, 1]
    res = V.from_records(np.array([[[5, 6]], [[9, 9]]]), iy, a, idx, D, SIZE, **V.DEFAULTS)
    assert res["state"][0].tolist() == [4, 2] and res["use"][:, 0, 0].tolist() == [1, 1] and res["visible"][:, 0, 0].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ against the composer
def _small(n=3, pw=16, ph=8, w=24, h=20, ch=1, seed=0):
    rng = np.random.default_rng(seed)
    mx = rng.uniform(-3.0, w + 2.0, (n, D, ph, pw)).astype(np.float32)
    my = rng.uniform(-3.0, h + 2.0, (n, D, ph, pw)).astype(np.float32)
    imgs = [rng.integers(0, 256, (h, w) if ch == 1 else (h, w, 3)).astype(np.uint8) for _ in range(n)]
    wgt = [None if k == 1 else rng.integers(0, 256, (h, w)).astype(np.uint8) for k in range(n)]
    idx = rng.integers(-16, 16 * D + 40, (ph, pw)).astype(np.int16)
    return imgs, wgt, mx, my, idx


@pytest.mark.parametrize("mode", [CR.SEAM, CR.FEATHER, CR.MULTIBAND])
@pytest.mark.parametrize("ch", [1, 3])
def test_tolerance_255_and_a_constant_map_reproduce_the_composer(mode, ch):
    imgs, wgt, mx, my, idx = _small(ch=ch)
    kw = dict(mode=mode, levels=2, wrap=True, gains=[300, 256, 200], fallback_index=4)
    for index16, vp in ((idx, dict(tolerance=255, cell_shift=1, dilate=1)), (np.full(idx.shape, 16 * 7 + 3, np.int16), dict(tolerance=0, cell_shift=1, dilate=0))):
        got, want = V.compose(imgs, wgt, mx, my, index16, vp, **kw), CR.compose(imgs, wgt, mx, my, index16, **kw)
        assert set(np.unique(got["state"]).tolist()) <= {0, 1, 2}
        for name in ("out", "sampled", "alpha", "label", "coverage", "hypothesis"):
            assert np.array_equal(got[name], want[name]), name
    # and without them the same frame changes, or the two cases above prove nothing
    got = V.compose(imgs, wgt, mx, my, idx, dict(tolerance=0, cell_shift=1, dilate=0), **kw)
    assert (got["state"] == 3).sum() >= 10 and (got["state"] == 4).any()
    assert not np.array_equal(got["out"], CR.compose(imgs, wgt, mx, my, idx, **kw)["out"])


def test_the_guard_state_keeps_the_alphas_and_the_pixel():
    imgs, wgt, mx, my, idx = _small()
    vp = dict(tolerance=0, cell_shift=1, dilate=0)
    got, plain = V.compose(imgs, wgt, mx, my, idx, vp, mode=CR.FEATHER), CR.compose(imgs, wgt, mx, my, idx, mode=CR.FEATHER)
    for st in (0, 1, 2, 4):
        at = got["state"] == st
        assert at.any() and np.array_equal(got["alpha"][:, at], plain["alpha"][:, at]) and np.array_equal(got["out"][at], plain["out"][at]), st
    at = got["state"] == 3
    assert np.all(got["coverage"][at] >= 1) and np.all(got["coverage"][at] < plain["coverage"][at])
    vis = V.visibility(wgt, mx, my, idx, (24, 20), **vp)
    assert np.array_equal(vis["use"][:, at], vis["visible"][:, at])


def test_records_are_packed_as_the_prepare_kernel_packs_them():
    m = np.array([-1.0, -0.02, -0.015625, 0.0, 0.984375, 0.99, 5.5, 1e6, -1e6], dtype=np.float32)
    ix, _ = V.record_positions(m, m)
    assert ix.tolist() == [-1, -1, 0, 0, 1, 1, 5, 32767, -32768]             # rint(32 x) >> 5 (ties to even), saturated


# ------------------------------------------------------------------------------------------------ the occluder scene
# The scene of tests/test_gpu_sweep.py (the textured sphere of 2500 mm around the rig, SCENE) with a ball of BALL_R mm centred
# at BALL_C in the rig frame: 1150 mm from the rig origin at longitude 135 degrees, in the overlap of cameras 1 and 2, so that
# its front is hypothesis 29 of the 32 (near = 800 mm) and the sphere behind it hypothesis 10.  (At longitude 45 degrees, the
# first placement, camera 0 sees the ball too; it sits at the rig origin, has no parallax and carries every SEAM label there,
# so SEAM had nothing to gain: 10.18 without and 10.45 with visibility, FEATHER 17.33 and 9.93.)  Every camera image is the
# nearer ray hit; the truth is the equirect view from the rig origin; the index map is the true one (the nearest hypothesis of
# the true range at every pixel centre), so that matching does not enter.  Mean absolute error against the truth over the
# pixels in state 3 (VISIBILITY below), by the restatements on the reference tables alone:
#   python -c "from tests import test_sweep_visibility_reference as t; print(t.ball_figures())"
BALL_C = np.array([1150.0 * np.sin(0.75 * np.pi), 0.0, 1150.0 * np.cos(0.75 * np.pi)])
BALL_R = 300.0
VISIBILITY = dict(cell_shift=2, tolerance=2, dilate=1, near_is_high=1)
BALL_FIGURES = {"plain": (25.30, 21.24), "visible": (11.33, 10.78)}          # (SEAM, FEATHER)
BALL_STATE3 = 350


def _ball_hit(origin, d):
    """distance along the unit rays d from origin to the ball's front, inf where they miss"""
    oc = origin - BALL_C
    b = d @ oc
    disc = b * b - (oc @ oc - BALL_R ** 2)
    s = -b - np.sqrt(np.maximum(disc, 0.0))
    return np.where((disc > 0) & (s > 0), s, np.inf)


def _shade(origin, d):
    """grey value and range of the nearer hit along the unit rays d: the sphere's hashed cells in longitude / latitude
    about the rig origin, the ball's (half as wide, another hash) about its centre"""
    b = d @ origin
    s_far = -b + np.sqrt(b * b - (origin @ origin - scene.SPHERE_R ** 2))
    s_ball = _ball_hit(origin, d)
    hit = np.isfinite(s_ball)
    P = origin + d * np.where(hit, s_ball, s_far)[..., None]
    Q = np.where(hit[..., None], (P - BALL_C) / BALL_R, P / scene.SPHERE_R)
    lon, lat = np.arctan2(Q[..., 0], Q[..., 2]), np.arcsin(np.clip(Q[..., 1], -1.0, 1.0))
    cell = np.where(hit, 0.3, 0.1)
    return scene._hash_gray(np.floor(lon / cell) + np.where(hit, 977, 0), np.floor(lat / cell)), np.where(hit, s_ball, s_far)


def _panorama_rays(lon, lat):
    return np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)], axis=-1)


def render_camera(intr, Twc, width, height, supersample=2):
    Rc, tc = Twc[:, :3], Twc[:, 3]
    offs = (np.arange(supersample) + 0.5) / supersample - 0.5
    acc = np.zeros((height, width))
    jj, ii = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    for oy in offs:
        for ox in offs:
            d = synth.unproject_pixels_np(intr, jj + ox, ii + oy) @ Rc.T
            ok = np.all(np.isfinite(d), axis=-1)
            acc += np.where(ok, _shade(tc, np.where(ok[..., None], d, 0.0))[0], 0.0)
    return np.clip(np.rint(acc / supersample ** 2), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def ball_scene():
    """(intr, Twc, images, truth, index16): the rig of scene.sphere_scene, its images of the two spheres, the view from the
    rig origin and the true index map"""
    intr, T, _ = scene.sphere_scene()
    pw, ph, Dn, near = scene.SCENE["pano_w"], scene.SCENE["pano_h"], scene.SCENE["D"], scene.SCENE["near"]
    imgs = [render_camera(intr[k], T[k], 320, 270) for k in range(4)]
    zero = np.zeros(3)
    truth = CR.equirect_truth(lambda lon, lat: _shade(zero, _panorama_rays(lon, lat))[0], pw, ph, 4)
    jj, ii = np.meshgrid(np.arange(pw, dtype=np.float64), np.arange(ph, dtype=np.float64))
    rng = _shade(zero, _panorama_rays((jj - pw / 2.0) / (pw / (2 * np.pi)), (ii - ph / 2.0) / (ph / np.pi)))[1]
    idx = (16 * np.clip(np.rint((Dn - 1) * near / rng), 0, Dn - 1)).astype(np.int16)
    return intr, T, imgs, truth, idx


@functools.lru_cache(maxsize=None)
def ball_tables():
    intr, T, _ = scene.sphere_scene()
    pw, ph = scene.SCENE["pano_w"], scene.SCENE["pano_h"]
    inv = sweep.inverse_distances(scene.SCENE["near"], D=scene.SCENE["D"])
    descs = [mref.Desc(intr[k], T[k][:, :3].T, pw / (2 * np.pi), ph / np.pi, pw / 2.0, ph / 2.0, pw, ph, mref.EQUIRECT, check_w2=1) for k in range(4)]
    mx, my, _ = sweep_ref.build_sweep_maps_ref(descs, T[:, :, 3], inv)
    return mx, my


def state3_error(pano, truth, state) -> float:
    at = np.asarray(state) == 3
    return float(np.mean(np.abs(np.asarray(pano).astype(np.int64).reshape(truth.shape)[at] - truth.astype(np.int64)[at])))


def ball_figures() -> dict:
    _, _, imgs, truth, idx = ball_scene()
    mx, my = ball_tables()
    out = dict(plain=[], visible=[])
    for mode in (CR.SEAM, CR.FEATHER):
        vis = V.compose(imgs, None, mx, my, idx, VISIBILITY, mode=mode)
        out["visible"].append(state3_error(vis["out"], truth, vis["state"]))
        out["plain"].append(state3_error(CR.compose(imgs, None, mx, my, idx, mode=mode)["out"], truth, vis["state"]))
    out["state3"] = int((vis["state"] == 3).sum())
    out["states"] = np.bincount(vis["state"].ravel(), minlength=5).tolist()
    return out


def test_the_occluder_scene_gives_the_committed_figures():
    fig = ball_figures()
    print(fig)
    _, _, _, truth, idx = ball_scene()
    assert set(np.unique(idx).tolist()) >= {160, 16 * 29} and (idx >= 0).all()
    assert fig["state3"] == BALL_STATE3 and BALL_STATE3 >= 50
    for name in ("plain", "visible"):
        for got, want in zip(fig[name], BALL_FIGURES[name]):
            assert abs(got - want) < 0.005, (name, got, want)
    # what the pass is for: at the pixels where it takes cameras away the frame is nearer to the truth, in both blends; a
    # condition on the scene, not a tolerance
    for plain, vis in zip(BALL_FIGURES["plain"], BALL_FIGURES["visible"]):
        assert vis < 0.7 * plain


# ------------------------------------------------------------------------------------------------ C ABI
NAMES = ("tscm_sweep_visibility_default_params", "tscm_sweep_visibility", "tscm_sweep_visibility_stages", "tscm_sweep_compose_visible",
         "tscm_sweep_compose_visible_stages")


def test_the_new_symbols_are_exported():
    L = lib.lib()
    for name in NAMES:
        assert name in lib.EXPORTS
        assert hasattr(L, name)
    assert L.tscm_abi_version() == 6


def test_default_params():
    p = sweep.visibility_params()
    assert (p.struct_size, p.cell_shift, p.tolerance, p.dilate, p.near_is_high) == (C.sizeof(lib.CSweepVisibilityParams), 2, 2, 0, 1)
    assert C.sizeof(lib.CSweepVisibilityParams) == 20
    q = sweep.visibility_params(cell_shift=0, tolerance=9, dilate=2, near_is_high=0)
    assert (q.cell_shift, q.tolerance, q.dilate, q.near_is_high) == (0, 9, 2, 0)
    assert V.DEFAULTS == dict(cell_shift=2, tolerance=2, dilate=0, near_is_high=1)
    with pytest.raises(AttributeError):
        sweep.visibility_params(struct_size=4)
    with pytest.raises(AttributeError):
        sweep.visibility_params(radius=1)


def test_a_null_handle_is_refused_before_any_device_is_touched():
    L = lib.lib()
    p, vp = sweep.compose_params(), sweep.visibility_params()
    out = np.zeros(16, np.uint8)
    o = out.ctypes.data_as(C.POINTER(C.c_ubyte))
    assert L.tscm_sweep_visibility(None, None, 4, C.byref(vp), o, o, None) == -1 and b"s is NULL" in L.tscm_last_error()
    assert L.tscm_sweep_visibility_stages(None, None, 4, C.byref(vp), None, None, None, None, o, o) == -1 and b"s is NULL" in L.tscm_last_error()
    assert L.tscm_sweep_compose_visible(None, None, 4, 1, None, 4, C.byref(p), C.byref(vp), None, o, 4, None, None) == -1 and b"s is NULL" in L.tscm_last_error()
    assert L.tscm_sweep_compose_visible_stages(None, None, 4, 1, None, 4, C.byref(p), C.byref(vp), None, None, None, None, None, None, None, None, o, o) == -1
    assert b"s is NULL" in L.tscm_last_error()
    assert not out.any()
