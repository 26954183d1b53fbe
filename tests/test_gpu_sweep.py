"""GPU tests of the sphere sweep (tscm_sweep_*, tscm_build_sweep_maps): every stage output and the index map equal the host
restatement tests/sweep_ref.py bit for bit (all of it is integer arithmetic); the sweep tables and the points are held to
the bounds the remap tables and the stereo points carry.  Shapes are the smallest at which each path can go wrong: a 72 x 24
panorama (no multiple of the 64 x 16 tile, two tiles per row and column), 64 x 32, 5 x 3 (below the census window), 2..4 and
8 cameras, D = 16, 80, 144, 256 (1, 2 partly filled, 3 and 4 hypotheses per lane of the aggregation)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import maps_proj_ref as mref
from tests import sweep_ref as R
from tscm_calib_amd import lib, maps, sweep, synth

pytestmark = pytest.mark.gpu

SRC_W, SRC_H = 48, 40


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _tables(n, D, pw, ph):
    """The tables of tests/test_gpu_panorama.py for n x D planes: random sample positions, a fifth outside the image, a
    tenth (-1, -1), a tenth exactly on integer coordinates; every camera also gets a band of columns it does not see at any
    hypothesis, and the last column is seen by nobody, so that |V| takes every value 0..n."""
    rng = np.random.default_rng(1000 * n + 10 * D + pw)
    shape = (n, D, ph, pw)
    mx = rng.uniform(-0.5, SRC_W - 0.5, shape).astype(np.float32)
    my = rng.uniform(-0.5, SRC_H - 0.5, shape).astype(np.float32)
    pick = rng.uniform(size=shape)
    far = pick < 0.2
    mx[far] = rng.uniform(-40.0, SRC_W + 40.0, far.sum()).astype(np.float32)
    my[far] = rng.uniform(-40.0, SRC_H + 40.0, far.sum()).astype(np.float32)
    hole = (pick >= 0.2) & (pick < 0.3)
    mx[hole], my[hole] = -1.0, -1.0
    whole = (pick >= 0.3) & (pick < 0.4)
    mx[whole], my[whole] = np.rint(mx[whole]), np.rint(my[whole])
    for k in range(n):
        lo = (k * pw) // (n + 1)
        mx[k, :, :, lo:lo + max(pw // 6, 1)], my[k, :, :, lo:lo + max(pw // 6, 1)] = -1.0, -1.0
    mx[:, :, :, pw - 1], my[:, :, :, pw - 1] = -1.0, -1.0
    mx[:, :, 0, 0], my[:, :, 0, 0] = 20.0, 20.0                      # and one pixel that everybody sees
    mx.setflags(write=False)
    my.setflags(write=False)
    return mx, my


@functools.lru_cache(maxsize=None)
def _images(n, seed=0):
    rng = np.random.default_rng(7 + seed)
    out = tuple(rng.integers(0, 256, (SRC_H, SRC_W)).astype(np.uint8) for _ in range(n))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _weights(n):
    rng = np.random.default_rng(99)
    out = []
    for k in range(n):
        wgt = rng.integers(0, 256, (SRC_H, SRC_W)).astype(np.uint8)
        wgt[:, :8] = 0                                   # a_k = 0 where the image itself is not: v_k != 0 without coverage
        out.append(None if k == 1 else wgt)              # a NULL entry among weight images
    return tuple(out)


# n, pw, ph, D, paths, wrap_x, weight images, uniqueness_ratio, p1, p2: the options rotate through the shapes
CASES = [
    (2, 72, 24, 16, 8, True, False, 10, 8, 32),
    (3, 64, 32, 80, 4, False, True, 0, 0, 0),
    (4, 72, 24, 144, 8, True, True, 10, 255, 255),
    (8, 72, 24, 16, 4, False, False, 0, 8, 32),
    (2, 64, 32, 256, 8, False, False, 10, 8, 32),
    (4, 72, 24, 80, 4, True, False, 0, 0, 0),
    (3, 72, 24, 16, 8, False, True, 10, 8, 32),
    (2, 5, 3, 16, 8, True, True, 10, 8, 32),
    (3, 5, 3, 80, 4, False, False, 0, 255, 255),
    (4, 64, 32, 16, 4, True, True, 0, 8, 32),
]


def _params(case):
    n, pw, ph, D, paths, wrap, with_weights, ratio, p1, p2 = case
    return dict(paths=paths, wrap_x=wrap, uniqueness_ratio=ratio, p1=p1, p2=p2)


@functools.lru_cache(maxsize=None)
def _reference(case, seed=0):
    n, pw, ph, D = case[:4]
    mx, my = _tables(n, D, pw, ph)
    return R.stages(list(_images(n, seed)), list(_weights(n)) if case[6] else None, mx, my, **_params(case))


def _sweeper(case, device):
    n, pw, ph, D = case[:4]
    mx, my = _tables(n, D, pw, ph)
    p = _params(case)
    p["wrap_x"] = int(p["wrap_x"])
    return sweep.Sweeper.from_tables(mx, my, (SRC_W, SRC_H), weights=list(_weights(n)) if case[6] else None, device=device, **p)


@pytest.mark.parametrize("case", CASES, ids=["n%d-%dx%d-D%d-p%d-w%d-m%d-u%d-%d-%d" % c for c in CASES])
def test_stages_and_index_map_equal_the_restatement(hip_device, case):
    n = case[0]
    ref = _reference(case)
    with _sweeper(case, hip_device) as s:
        st = s.stages(_images(n))
        idx = s.depth(_images(n))
    for name in ("sampled", "alpha", "census", "cost", "aggregated"):
        assert np.array_equal(st[name], ref[name]), name
    assert np.array_equal(idx, ref["index16"])
    seen = set(np.unique((ref["alpha"] > 0).sum(axis=0)).tolist())
    if case[1] > 5:
        assert seen == set(range(n + 1)), seen                       # |V| takes every value
        assert (idx == sweep.INVALID).any() and (idx >= 0).any()
    assert (ref["cost"] == 64).any() and (ref["cost"] < 64).any()


def test_row_padding_in_and_out(hip_device):
    case = CASES[0]
    n, pw, ph = case[:3]
    ref = _reference(case)
    wide = [np.full((SRC_H, SRC_W + 5), 77, np.uint8) for _ in range(n)]
    views = []
    for buf, img in zip(wide, _images(n)):
        buf[:, :SRC_W] = img
        views.append(buf[:, :SRC_W])
    canvas = np.full((ph, pw + 3), 12345, np.int16)
    with _sweeper(case, hip_device) as s:
        s.depth(views, out=canvas[:, :pw])
    assert np.array_equal(canvas[:, :pw], ref["index16"])
    assert np.all(canvas[:, pw:] == 12345)


def test_a_handle_is_reusable_and_repeatable(hip_device):
    case = CASES[6]
    n = case[0]
    first, second = _images(n, 0), _images(n, 1)
    with _sweeper(case, hip_device) as s:
        a1 = s.depth(first)
        b = s.depth(second)
        a2 = s.depth(first)
        t = s.stage_times()
    assert np.array_equal(a1, a2)
    assert np.array_equal(a1, _reference(case, 0)["index16"]) and np.array_equal(b, _reference(case, 1)["index16"])
    assert not np.array_equal(a1, b)
    assert np.all(t > 0)


def test_a_handle_without_a_frame(hip_device):
    with _sweeper(CASES[0], hip_device) as s:
        assert s._handle is not None
    assert s._handle is None


def test_refusals_that_need_a_handle(hip_device):
    """stride, out_stride, a NULL image, a NULL index16: TSCM_E_INVALID with a text that names the argument."""
    L = lib.lib()
    case = CASES[0]
    n, pw, ph = case[:3]
    imgs = _images(n)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in imgs])
    out = np.zeros((ph, pw), np.int16)
    o = out.ctypes.data_as(C.POINTER(C.c_short))
    with _sweeper(case, hip_device) as s:
        h = s._handle
        assert L.tscm_sweep_depth(h, ptrs, SRC_W - 1, o, pw, None) == -1 and b"stride" in L.tscm_last_error()
        assert L.tscm_sweep_depth(h, ptrs, SRC_W, o, pw - 1, None) == -1 and b"out_stride" in L.tscm_last_error()
        assert L.tscm_sweep_depth(h, ptrs, SRC_W, None, pw, None) == -1 and b"index16" in L.tscm_last_error()
        assert L.tscm_sweep_depth(h, None, SRC_W, o, pw, None) == -1 and b"images" in L.tscm_last_error()
        holed = (C.c_void_p * n)(imgs[0].ctypes.data, None)
        assert L.tscm_sweep_depth(h, holed, SRC_W, o, pw, None) == -1 and b"images[1]" in L.tscm_last_error()
        assert L.tscm_sweep_stages(h, ptrs, SRC_W - 1, None, None, None, None, None) == -1 and b"stride" in L.tscm_last_error()
    assert np.all(out == 0)


# ------------------------------------------------------------------------------------------------ tables
def _rig_descs(kind, w=40, h=20):
    intr, T = synth.CALIB_INTR, synth.CALIB_TWC
    fx = w / (2 * np.pi)
    fy = h / np.pi if kind in (mref.EQUIRECT, mref.LONGLAT) else fx
    descs = [maps.MapDesc(intr[k], T[k][:, :3].T.copy(), fx, fy, w / 2.0, h / 2.0, w, h, check_w2=1, projection=kind) for k in range(4)]
    return descs, T[:, :, 3].copy()


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("kind", [mref.LONGLAT, mref.CYLINDRICAL, mref.STEREOGRAPHIC, mref.EQUIRECT])
def test_sweep_tables_against_the_numpy_reference(hip_device, kind, exact):
    """The comparison of tests/test_gpu_map_projections.py for the tables that are not pinholes: every element within 1
    float32 ulp of the reference value.  The inv = 0 planes equal tscm_build_maps_ex on the same descriptors bit for bit,
    and with all centres at the origin the D planes of a camera are equal."""
    descs, centers = _rig_descs(kind)
    inv = np.array([0.0, 1.0 / 5000.0, 1.0 / 1500.0, 1.0 / 600.0])
    rx, ry, near = R.build_sweep_maps_ref(descs, centers, inv)
    gx, gy, sec = maps.build_sweep_maps(descs, centers, inv, device=hip_device, exact=exact)
    assert sec > 0 and gx.shape == (4, 4, 20, 40)
    assert not near.any()                      # no element of these tables sits on the w2 boundary
    for g, r in ((gx, rx), (gy, ry)):
        assert np.all(np.isfinite(r))
        d = np.abs(g.astype(np.float64) - r.astype(np.float64))
        worst = np.max(d / np.spacing(np.abs(r)).astype(np.float64))
        print(f"{mref.NAMES[kind]} exact {exact}: {int((g != r).sum())} of {g.size} elements differ, worst {worst:.2f} ulp")
        assert np.all(d <= np.spacing(np.abs(r)))
    assert (gx == -1.0).any() and (gx > 0).any()
    for k, d in enumerate(descs):
        d.out_offset = k * 800
    px, py, _ = maps.build_maps(descs, 4 * 800, hip_device, exact=exact)
    assert np.array_equal(gx[:, 0].ravel().view(np.uint32), px.view(np.uint32)) and np.array_equal(gy[:, 0].ravel().view(np.uint32), py.view(np.uint32))
    for d in descs:
        d.out_offset = 0
    zx, zy, _ = maps.build_sweep_maps(descs, np.zeros((4, 3)), inv, device=hip_device, exact=exact)
    for z in range(1, 4):
        assert np.array_equal(zx[:, z].view(np.uint32), zx[:, 0].view(np.uint32)) and np.array_equal(zy[:, z].view(np.uint32), zy[:, 0].view(np.uint32))
    assert np.array_equal(zx[:, 0].view(np.uint32), gx[:, 0].view(np.uint32))
    assert not np.array_equal(gx[1, 3], gx[1, 0])


# ------------------------------------------------------------------------------------------------ points
@pytest.mark.parametrize("kind", [mref.LONGLAT, mref.CYLINDRICAL, mref.STEREOGRAPHIC, mref.EQUIRECT])
def test_points_against_the_restatement(hip_device, kind):
    w, h, D = 37, 19, 16
    fx = w / (2 * np.pi) if kind != mref.STEREOGRAPHIC else w / 3.0
    desc = maps.MapDesc(synth.CALIB_INTR[0], np.eye(3), fx, h / np.pi if kind != mref.STEREOGRAPHIC else fx, w / 2.0, h / 2.0, w, h, projection=kind)
    rng = np.random.default_rng(kind)
    inv = np.concatenate([[0.0], np.cumsum(rng.uniform(1e-4, 5e-4, D - 1))])          # unequal steps, index 0 = infinity
    idx = rng.integers(0, 16 * (D - 1) + 9, (h, w)).astype(np.int16)
    idx[rng.uniform(size=(h, w)) < 0.1] = sweep.INVALID
    idx[0, :4] = [0, 16 * (D - 1), 16 * (D - 1) + 8, 1]
    rp, rv = R.points(idx, desc, inv)
    wide = np.full((h, w + 3), 999, np.int16)
    wide[:, :w] = idx
    for arr in (idx, wide[:, :w]):                                   # a padded index map gives the same points
        gp, gv = sweep.points(arr, desc, inv, device=hip_device)
        assert np.array_equal(gv, rv)
        assert np.isnan(gp[~gv]).all()
        err = np.linalg.norm(gp[gv] - rp[gv], axis=-1) / np.linalg.norm(rp[gv], axis=-1)
        print(f"{mref.NAMES[kind]}: largest relative distance to the restatement {err.max():.3e}")
        assert err.max() <= 1e-12
    assert not rv[0, 0] and rv[0, 1] and rv[0, 2] and rv[0, 3] and (~rv).sum() > 20


# ------------------------------------------------------------------------------------------------ end to end
SPHERE_R = 2500.0
SCENE = dict(pano_w=160, pano_h=80, D=32, near=800.0, paths=8)
# Measured with the reference chain on the CPU (reference_chain below: numpy fp64 tables with the centre term, the oracle's
# remap, the host census / aggregation / winner and points): the median of | |P| - 2500 mm | over the valid pixels and their
# share.  One hypothesis step at 2500 mm spans 2500^2 / (800 * 31) = 252 mm of range; the scene is usable only if the
# reference chain stays below that.  The device chain differs from it in the fp64 sincos of the table kernel only; a factor 2
# covers that, as for the plane of tests/test_gpu_stereo.py.
SPHERE_MEDIAN_CPU_MM = 20.0          # index 160 = 16 x 10 exactly: 24800 / 10 = 2480 mm; more than half of the pixels land there
SPHERE_VALID_SHARE_CPU = 0.996
SPHERE_STEP_MM = SPHERE_R ** 2 / (SCENE["near"] * (SCENE["D"] - 1))


def _hash_gray(qx, qy):
    key = (qx.astype(np.int64) * 73856093) ^ (qy.astype(np.int64) * 19349663)
    return (synth.splitmix64(key.astype(np.uint64)) >> np.uint64(56)).astype(np.float64)


def render_textured_sphere(intr, Twc, width, height, cell=0.1, supersample=2):
    """The hashed grey cells of render_textured_plane (tests/test_gpu_stereo.py) in longitude / latitude on the sphere
    |X| = SPHERE_R of the rig frame, by a ray / sphere intersection from the camera centre; the camera sits at
    Twc = [R | t] (camera to rig), inside the sphere.  cell: radians."""
    Rc, tc = Twc[:, :3], Twc[:, 3]
    offs = (np.arange(supersample) + 0.5) / supersample - 0.5
    acc = np.zeros((height, width))
    jj, ii = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    for oy in offs:
        for ox in offs:
            d = synth.unproject_pixels_np(intr, jj + ox, ii + oy) @ Rc.T          # unit rays in the rig frame
            ok = np.all(np.isfinite(d), axis=-1)
            d = np.where(ok[..., None], d, 0.0)
            b = d @ tc
            s = -b + np.sqrt(b * b - (tc @ tc - SPHERE_R ** 2))                     # the root in front of the camera
            P = tc + d * s[..., None]
            lon, lat = np.arctan2(P[..., 0], P[..., 2]), np.arcsin(np.clip(P[..., 1] / SPHERE_R, -1.0, 1.0))
            acc += np.where(ok, _hash_gray(np.floor(lon / cell), np.floor(lat / cell)), 0.0)
    return np.clip(np.rint(acc / supersample ** 2), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def sphere_scene():
    """Cameras 0..3 of synth.rig(4) at a quarter of their resolution, and their images of the sphere."""
    intr, _ = synth.rig(4)
    intr = intr.copy()
    intr[:, :4] *= 0.25
    T = synth.CALIB_TWC
    imgs = [render_textured_sphere(intr[k], T[k], 320, 270) for k in range(4)]
    return intr, T, imgs


def sphere_error(pts, valid):
    return np.abs(np.linalg.norm(pts[valid], axis=-1) - SPHERE_R)


def reference_chain():
    """rig_depth on the CPU: reference tables with the centre term, the oracle's remap, the host sweep and points."""
    intr, T, imgs = sphere_scene()
    pw, ph = SCENE["pano_w"], SCENE["pano_h"]
    inv = sweep.inverse_distances(SCENE["near"], D=SCENE["D"])
    descs = [mref.Desc(intr[k], T[k][:, :3].T, pw / (2 * np.pi), ph / np.pi, pw / 2.0, ph / 2.0, pw, ph, mref.EQUIRECT, check_w2=1) for k in range(4)]
    mx, my, _ = R.build_sweep_maps_ref(descs, T[:, :, 3], inv)
    idx = R.stages(imgs, None, mx, my, paths=SCENE["paths"], wrap_x=True)["index16"]
    pts, valid = R.points(idx, descs[0], inv)
    return float(np.median(sphere_error(pts, valid))), float(valid.mean())


def test_rig_depth_on_a_textured_sphere(hip_device):
    intr, T, imgs = sphere_scene()
    inv = sweep.inverse_distances(SCENE["near"], D=SCENE["D"])
    with sweep.Sweeper.from_rig(intr, T, (320, 270), SCENE["pano_w"], SCENE["pano_h"], inv, weights=None, device=hip_device, keep_tables=True,
                                paths=SCENE["paths"]) as s:
        idx = s.depth(imgs)
        pts, valid = s.points(idx)
        host = R.stages(imgs, None, s.mapx, s.mapy, paths=SCENE["paths"], wrap_x=True)["index16"]
    # the device-built tables are an input to both sides, so the sincos of the table kernel does not enter
    assert np.array_equal(idx, host)
    share = valid.mean()
    median = float(np.median(sphere_error(pts, valid)))
    print(f"sphere at {SPHERE_R:.0f} mm: {100 * share:.1f} % of the pixels valid, median | |P| - R | {median:.2f} mm (reference chain on the CPU "
          f"{SPHERE_MEDIAN_CPU_MM} mm at {SPHERE_VALID_SHARE_CPU} valid, bound {2.0 * SPHERE_MEDIAN_CPU_MM} mm, one hypothesis step {SPHERE_STEP_MM:.0f} mm)")
    assert SPHERE_MEDIAN_CPU_MM < SPHERE_STEP_MM               # a condition on the scene, not a tolerance
    assert valid.any()
    assert median <= 2.0 * SPHERE_MEDIAN_CPU_MM
