"""GPU tests of the projection kinds of the remap tables (tscm_build_maps_ex: long-lat, cylindrical, stereographic,
equirect) and of tscm_rectify_points against the fp64 numpy reference of tests/maps_proj_ref.py, through the C ABI.
Every test prints its figures before it asserts (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as orc
from tests import maps_proj_ref as ref
from tscm_calib_amd import api, lib, maps, synth

pytestmark = pytest.mark.gpu
NEW_KINDS = [k for k in ref.KINDS if k != ref.PERSPECTIVE]


def _bits(a):
    return a.view(np.uint32)


def _random_batch(seed):
    """The shapes of test_random_table_geometries (widths 1..70, heights 1..9, row padding 0..5, unaligned offsets, 3..40
    tables in one launch), with a random rotation and a random kind per table, PERSPECTIVE among them."""
    rng = np.random.default_rng(7000 + seed)
    descs, off = [], int(rng.integers(0, 7))
    n = int(rng.integers(3, 41))
    kinds = [int(k) for k in rng.integers(0, 5, n)]
    kinds[int(rng.integers(0, n))] = ref.PERSPECTIVE
    kinds[(kinds.index(ref.PERSPECTIVE) + 1) % n] = NEW_KINDS[seed % 4]
    for kind in kinds:
        w, h = int(rng.integers(1, 71)), int(rng.integers(1, 10))
        stride = w + int(rng.integers(0, 6))
        intr = synth.CALIB_INTR[int(rng.integers(0, len(synth.CALIB_INTR)))].copy()
        if rng.integers(0, 2):
            intr[7:] = rng.uniform(-0.3, 0.3, 2)
        f = float(rng.uniform(150.0, 400.0)) if kind in (ref.PERSPECTIVE, ref.STEREOGRAPHIC) else float(rng.uniform(20.0, 400.0))
        descs.append(maps.MapDesc(intr, ref.rotation(rng), f, f * float(rng.uniform(0.9, 1.1)), w / 2.0, h / 2.0, w, h,
                                  offset_x=float(rng.integers(0, 2)) * 1280.0, out_offset=off, out_stride=stride,
                                  check_w2=int(rng.integers(0, 2)), projection=kind))
        off += stride * h + int(rng.integers(0, 5))
    return descs, off


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("seed", range(6))
def test_every_kind_against_the_numpy_reference(hip_device, seed, exact):
    """Every element within 1 float32 ulp of the reference value; gaps and padding untouched."""
    descs, n = _random_batch(seed)
    rx, ry, written, near = ref.build_maps_ref(descs, n)
    gx, gy, sec = maps.build_maps(descs, n, hip_device, exact=exact)
    assert sec > 0
    assert not near.any()                      # no element of these tables sits on the w2 boundary
    assert np.all(gx[~written] == 0.0) and np.all(gy[~written] == 0.0)
    for g, r in ((gx, rx), (gy, ry)):
        assert np.all(np.isfinite(r))
        d = np.abs(g.astype(np.float64) - r.astype(np.float64))
        worst = np.max(d / np.spacing(np.abs(r)).astype(np.float64))
        print(f"seed {seed} exact {exact}: {int((g != r).sum())} of {int(written.sum())} elements differ, worst {worst:.2f} ulp")
        assert np.all(d <= np.spacing(np.abs(r)))


@pytest.mark.parametrize("seed", range(3))
def test_perspective_maps_of_a_mixed_batch_keep_their_bits(hip_device, seed):
    descs, n = _random_batch(seed)
    gx, gy, _ = maps.build_maps(descs, n, hip_device, exact=True)
    pin = [d for d in descs if d.projection == ref.PERSPECTIVE]
    assert pin and len(pin) < len(descs)
    ax, ay, _ = maps.build_maps(pin, n, hip_device, exact=True)         # tscm_build_maps, alone
    ox, oy = orc.build_maps(pin, n)
    for d in pin:
        idx = (d.out_offset + np.arange(d.height)[:, None] * d.out_stride + np.arange(d.width)[None, :]).ravel()
        assert np.array_equal(_bits(gx[idx]), _bits(ax[idx])) and np.array_equal(_bits(gy[idx]), _bits(ay[idx]))
        assert np.array_equal(_bits(gx[idx]), _bits(ox[idx])) and np.array_equal(_bits(gy[idx]), _bits(oy[idx]))


@pytest.mark.parametrize("exact", [True, False])
def test_all_perspective_ex_call_is_tscm_build_maps(hip_device, exact):
    descs, n = _random_batch(1)
    for d in descs:
        d.projection = 0
    bx, by, _ = maps.build_maps(descs, n, hip_device, exact=exact)
    fp = C.POINTER(C.c_float)
    arr = maps._c_descs(descs)
    for kinds in (None, (C.c_int * len(descs))()):
        gx, gy = np.zeros(n, np.float32), np.zeros(n, np.float32)
        lib.check(lib.lib().tscm_build_maps_ex(arr, kinds, len(descs), hip_device, int(exact), gx.ctypes.data_as(fp), gy.ctypes.data_as(fp), n, None))
        assert np.array_equal(_bits(gx), _bits(bx)) and np.array_equal(_bits(gy), _bits(by))
    assert (bx != 0).any()


@pytest.mark.parametrize("kind", [ref.LONGLAT, ref.EQUIRECT])
def test_w2_rule_on_wide_tables(hip_device, kind):
    """A 360 x 180 degree table (80 x 40, 4.5 degrees per element) of camera 1 with a rotation: rays behind the camera are
    (-1, -1) exactly where the reference says, except where the reference's |Z + w2 d1| < 1e-9 d1 (at most 0.5 %)."""
    rng = np.random.default_rng(5)
    d = maps.MapDesc(synth.CALIB_INTR[1], ref.rotation(rng), 80 / (2 * np.pi), 40 / np.pi, 40.0, 20.0, 80, 40, check_w2=1, projection=kind)
    rx, ry, near = ref.build_map_ref(d)
    assert near.mean() <= 0.005
    for exact in (True, False):
        gx, gy, _ = maps.build_maps([d], 80 * 40, hip_device, exact=exact)
        gx, gy = gx.reshape(40, 80), gy.reshape(40, 80)
        behind_g, behind_r = (gx == -1.0) & (gy == -1.0), (rx == -1.0) & (ry == -1.0)
        assert 0.1 < behind_r.mean() < 0.9
        assert np.array_equal(behind_g[~near], behind_r[~near])


def _points_desc(kind, rng):
    """An output image of `kind` for camera 0, rotated, with the w2 rule at w2 = -0.2 (rays beyond 78 degrees fail), so that
    pixels of all three classes -- valid, outside the model's domain, failing w2 -- occur inside the 1280 x 1080 image."""
    d = ref.round_trip_desc(kind, synth.CALIB_INTR[0], ref._small(ref.rotation(rng)))
    return maps.MapDesc(d.intr, d.R, d.fx, d.fy, d.cx, d.cy, d.width, d.height, check_w2=1, w2=-0.2, projection=kind)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_rectify_points_against_the_reference(hip_device, kind):
    """500 pixels over the image and its surroundings: valid equal to the reference's, coordinates within 64 x the
    reference's own round-trip error (floor 1e-10 px)."""
    rng = np.random.default_rng(900 + kind)
    d = _points_desc(kind, rng)
    px = np.stack([rng.uniform(-40.0, synth.IMG_W + 40.0, 500), rng.uniform(-40.0, synth.IMG_H + 40.0, 500)], axis=1)
    rxy, rok = ref.rectify_points_ref(d, px)
    c = ref.unproject_ref(d.intr, px)
    outside, fails = ~np.all(np.isfinite(c), axis=1), np.zeros(500, bool)
    fails[~outside] = c[~outside, 2] <= -d.w2
    assert outside.sum() >= 5 and fails.sum() >= 5 and rok.sum() >= 100
    gxy, gok = maps.rectify_points(d, px, hip_device)
    assert np.array_equal(gok, rok)
    assert np.all(np.isnan(gxy[~gok]))
    err = float(np.max(np.abs(gxy[gok] - rxy[rok])))
    print(f"rectify_points {ref.NAMES[kind]}: max |device - reference| {err:.3e} px, tolerance {ref.point_tolerance(kind):.3e} px, "
          f"reference round trip {ref.round_trip_error(kind):.3e} px")
    assert err <= ref.point_tolerance(kind)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_round_trip_through_the_device(hip_device, kind):
    """Output grid -> (fp64 reference) source pixels -> tscm_rectify_points returns the grid."""
    rng = np.random.default_rng(40 + kind)
    r = ref.round_trip_desc(kind, synth.CALIB_INTR[2], ref._small(ref.rotation(rng)))
    d = maps.MapDesc(r.intr, r.R, r.fx, r.fy, r.cx, r.cy, r.width, r.height, projection=kind)
    _, grid, src, ok = ref.round_trip(r, step=9)
    assert ok.all()
    gxy, gok = maps.rectify_points(d, src, hip_device)
    assert gok.all()
    err = float(np.max(np.abs(gxy - grid)))
    print(f"device round trip {ref.NAMES[kind]}: {err:.3e} px, tolerance {ref.point_tolerance(kind):.3e} px")
    assert err <= ref.point_tolerance(kind)


def test_epipolar_rows_on_the_device(hip_device):
    Pw, _, _ = ref.pair_points()
    T = synth.CALIB_TWC
    px = [api.project(synth.CALIB_INTR[k], (Pw - T[k][:, 3]) @ T[k][:, :3], device=hip_device) for k in (0, 1)]
    rows = {}
    for name in ("longlat", "cylindrical"):
        da, db = maps.rectify_pair_descs(synth.CALIB_INTR[0], T[0], synth.CALIB_INTR[1], T[1], name)
        (xa, oka), (xb, okb) = maps.rectify_points(da, px[0], hip_device), maps.rectify_points(db, px[1], hip_device)
        assert oka.all() and okb.all()
        rows[name] = float(np.max(np.abs(xa[:, 1] - xb[:, 1])))
    print(f"row difference of the pair: longlat {rows['longlat']:.3e} px, cylindrical {rows['cylindrical']:.3e} px")
    assert rows["longlat"] <= ref.point_tolerance(ref.LONGLAT)
    assert rows["cylindrical"] > 1.0


def test_longlat_table_applied_to_an_image(hip_device):
    p = synth.make_problem(1, 4, 3, noise_px=0.0, perturb=False)
    intr = p.meta["gt_intr"][0].copy()
    intr[[0, 1, 2, 3]] *= 0.25                                           # the 1280 x 1080 camera at 320 x 270
    img = synth.render_chessboard(intr, p.meta["gt_board_rt"][0], 9, 6, 45.0, 320, 270, supersample=1)
    d = maps.MapDesc(intr, np.eye(3), 160 / np.pi, 80 / (np.pi / 2), 80.0, 40.0, 160, 80, projection="longlat")
    mx, my, _ = maps.build_maps([d], 160 * 80, hip_device)
    mx, my = mx.reshape(80, 160), my.reshape(80, 160)
    out = maps.remap(img, mx, my, device=hip_device)
    assert out.shape == (80, 160) and np.array_equal(out, orc.remap(img, mx, my))
    assert out.std() > 5
