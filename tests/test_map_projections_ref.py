"""CPU tests of the projection kinds of the remap tables (tscm.h TSCM_PROJ_*): the numpy reference of
tests/maps_proj_ref.py on its own, in fp64, the refusals of tscm_build_maps_ex / tscm_rectify_points that need no device,
and the example host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import maps_proj_ref as ref
from tscm_calib_amd import lib, maps, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KINDS = [k for k in ref.KINDS if k != ref.PERSPECTIVE]


@pytest.mark.parametrize("kind", ref.KINDS)
def test_ray_is_a_positive_multiple_of_a_unit_vector(kind):
    a, b = np.meshgrid(np.linspace(-1.5, 1.5, 31), np.linspace(-1.2, 1.2, 25))
    r = ref.ray(kind, a, b)
    n = np.linalg.norm(r, axis=-1)
    assert np.all(np.isfinite(r)) and np.all(n > 0)
    if kind in (ref.LONGLAT, ref.STEREOGRAPHIC, ref.EQUIRECT):
        assert np.max(np.abs(n - 1.0)) < 4e-16
    # the inverse recovers (a, b): the ray's direction carries them, its length does not matter
    for s in (1.0, 3.7):
        a2, b2, ok = ref.inverse_ray(kind, s * r)
        assert ok.all() and np.max(np.abs(a2 - a)) < 1e-14 and np.max(np.abs(b2 - b)) < 1e-14


@pytest.mark.parametrize("kind", ref.KINDS)
def test_centre_pixel_and_first_order_agreement_with_the_pinhole(kind):
    assert np.array_equal(ref.ray(kind, 0.0, 0.0), [0.0, 0.0, 1.0])
    h = 1e-6                                       # central differences: error h^2 ~ 1e-12
    Ja = (ref.ray(kind, h, 0.0) - ref.ray(kind, -h, 0.0)) / (2 * h)
    Jb = (ref.ray(kind, 0.0, h) - ref.ray(kind, 0.0, -h)) / (2 * h)
    assert np.max(np.abs(Ja - [1.0, 0.0, 0.0])) < 1e-10 and np.max(np.abs(Jb - [0.0, 1.0, 0.0])) < 1e-10


@pytest.mark.parametrize("kind", ref.KINDS)
def test_round_trip_of_the_reference(kind):
    """rectify_points_ref(project_ref(ray(i, j))) == (j, i) on a grid inside the kind's domain.  The largest error is the
    yardstick of the device tolerances (maps_proj_ref.point_tolerance): measured 1.1e-12 px or less for every kind."""
    err = ref.round_trip_error(kind)
    print(f"round trip {ref.NAMES[kind]}: {err:.3e} px")
    assert err < 1e-9
    assert ref.point_tolerance(kind) == max(64 * err, 1e-10)


def _pair(kind, **kw):
    return maps.rectify_pair_descs(synth.CALIB_INTR[0], synth.CALIB_TWC[0], synth.CALIB_INTR[1], synth.CALIB_TWC[1], ref.NAMES[kind], **kw)


def test_epipolar_rows_of_a_pair():
    """A scene point lies on the same row of both rectified images with LONGLAT and PERSPECTIVE, not with CYLINDRICAL."""
    _, pa, pb = ref.pair_points()
    assert pa.shape == (200, 2)
    for kind, kw in ((ref.LONGLAT, {}), (ref.PERSPECTIVE, dict(width=400, height=400, fov_x=np.pi / 2, fov_y=np.pi / 2))):
        da, db = _pair(kind, **kw)
        (xa, oka), (xb, okb) = ref.rectify_points_ref(da, pa), ref.rectify_points_ref(db, pb)
        assert oka.all() and okb.all()
        # rows agree identically in exact arithmetic; what is left is fp64 round-off of the two chains (~1e-11 px)
        assert np.max(np.abs(xa[:, 1] - xb[:, 1])) < 1e-8, ref.NAMES[kind]
        assert np.max(np.abs(xa[:, 0] - xb[:, 0])) > 1.0            # disparity: the columns do differ
    da, db = _pair(ref.CYLINDRICAL)
    (xa, oka), (xb, okb) = ref.rectify_points_ref(da, pa), ref.rectify_points_ref(db, pb)
    assert oka.all() and okb.all() and np.max(np.abs(xa[:, 1] - xb[:, 1])) > 1.0


def test_pair_and_panorama_descriptors():
    da, db = _pair(ref.LONGLAT, width=628, height=314)
    assert (da.projection, da.check_w2, da.offset_x, da.width, da.height) == (lib.PROJ_LONGLAT, 1, 0.0, 628, 314)
    assert da.fx == pytest.approx(628 / np.pi) and da.fy == pytest.approx(314 / (np.pi / 2)) and (da.cx, da.cy) == (314.0, 157.0)
    Rp = maps.rectify_pair_rotation(synth.CALIB_TWC[0][:, 3], synth.CALIB_TWC[1][:, 3])
    assert np.allclose(db.R, synth.CALIB_TWC[1][:, :3].T @ Rp, atol=0, rtol=0)
    with pytest.raises(ValueError):
        _pair(ref.PERSPECTIVE)                       # a pinhole cannot span 180 degrees
    with pytest.raises(ValueError):
        maps.MapDesc(synth.CALIB_INTR[0], np.eye(3), 1.0, 1.0, 0.0, 0.0, 4, 4, projection="fisheye")
    pano = maps.panorama_descs(synth.CALIB_INTR, synth.CALIB_TWC, 720, 360)
    assert len(pano) == 4 and all(d.projection == lib.PROJ_EQUIRECT and d.check_w2 == 1 for d in pano)
    assert pano[2].fx == pytest.approx(720 / (2 * np.pi)) and pano[2].fy == pytest.approx(360 / np.pi)
    # every rig-frame direction is seen (passes the w2 rule) by at least one of the four cameras
    seen = np.zeros((360, 720), dtype=bool)
    for d in pano:
        mx, _, _ = ref.build_map_ref(d)
        seen |= mx != -1.0
    assert seen[60:300].all()                        # 30 degrees about the poles aside: the rig looks at the horizon
    assert maps.undistort_desc(synth.CALIB_INTR[0], 1.0, 1.0, 0.0, 0.0, 4, 4).projection == 0


def _cdesc(**kw):
    d = maps.undistort_desc(synth.CALIB_INTR[0], 100.0, 100.0, 8.0, 8.0, 16, 16, **kw)
    return maps._c_descs([d, d, d])


def test_refusals_that_need_no_device():
    L = lib.lib()
    fp = C.POINTER(C.c_float)
    mx, my = np.zeros(3 * 256, np.float32), np.zeros(3 * 256, np.float32)
    arr = _cdesc()
    for bad in (5, -1, 99):
        kinds = (C.c_int * 3)(0, 1, bad)
        assert L.tscm_build_maps_ex(arr, kinds, 3, 0, 1, mx.ctypes.data_as(fp), my.ctypes.data_as(fp), mx.size, None) == -1
        assert b"map 2" in L.tscm_last_error() and b"projection" in L.tscm_last_error()
        px, out, valid = np.zeros((2, 2)), np.zeros((2, 2)), np.zeros(2, np.uint8)
        assert L.tscm_rectify_points(arr, bad, lib.dptr(px), 2, 0, lib.dptr(out), valid.ctypes.data_as(C.POINTER(C.c_ubyte))) == -1
        assert b"map 0" in L.tscm_last_error() and b"projection" in L.tscm_last_error()
    px, out, valid = np.zeros((2, 2)), np.zeros((2, 2)), np.zeros(2, np.uint8)
    vp = valid.ctypes.data_as(C.POINTER(C.c_ubyte))
    assert L.tscm_rectify_points(arr, 1, lib.dptr(px), -1, 0, lib.dptr(out), vp) == -1
    assert L.tscm_rectify_points(arr, 1, lib.dptr(px), 0, 0, lib.dptr(out), vp) == 0
    assert L.tscm_rectify_points(arr, 1, None, 0, 0, None, None) == 0
    # the refusals of tscm_build_maps hold for the _ex entry point
    arr[1].out_stride = 8
    assert L.tscm_build_maps_ex(arr, (C.c_int * 3)(1, 1, 1), 3, 0, 1, mx.ctypes.data_as(fp), my.ctypes.data_as(fp), mx.size, None) == -1
    assert b"map 1" in L.tscm_last_error()


def test_no_device_means_no_device():
    L = lib.lib()
    if L.tscm_device_count() > 0:
        pytest.skip("a HIP device is present")
    fp = C.POINTER(C.c_float)
    mx, my = np.zeros(3 * 256, np.float32), np.zeros(3 * 256, np.float32)
    arr = _cdesc()
    for kinds in (None, (C.c_int * 3)(0, 0, 0), (C.c_int * 3)(0, 1, 4)):
        assert L.tscm_build_maps_ex(arr, kinds, 3, 0, 1, mx.ctypes.data_as(fp), my.ctypes.data_as(fp), mx.size, None) == -2
    px, out, valid = np.zeros((2, 2)), np.zeros((2, 2)), np.zeros(2, np.uint8)
    assert L.tscm_rectify_points(arr, 1, lib.dptr(px), 2, 0, lib.dptr(out), valid.ctypes.data_as(C.POINTER(C.c_ubyte))) == -2
    d = maps.undistort_desc(synth.CALIB_INTR[0], 100.0, 100.0, 8.0, 8.0, 16, 16, projection="longlat")
    with pytest.raises(lib.TscmError) as e:
        maps.build_maps([d])
    assert e.value.code == -2
    with pytest.raises(lib.TscmError) as e:
        maps.rectify_points(d, px)
    assert e.value.code == -2


def test_rectify_pair_demo_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "tscm_calib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "rectify_pair_demo.cpp"), "-L", csrc, "-ltscm_hip", "-Wl,-rpath," + csrc,
                           "-o", str(tmp_path / "a.out")])
