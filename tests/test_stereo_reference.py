"""CPU tests of the stereo matcher's definition (include/tscm/tscm.h, tscm_stereo_*): the host restatement
tests/stereo_ref.py on hand-worked cases and on the synthetic-shift pair, and the argument refusals of the C ABI, which
return before a device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tscm_calib_amd import lib, stereo
from tests import stereo_ref as R


def test_census_codes_on_ramps():
    ramp = np.tile(np.arange(9, dtype=np.uint8), (7, 1))                      # img(y, x) = x
    code = R.census(ramp)
    # centre pixel: every row reads 1 1 1 1 (c) 0 0 0 0, the centre row without its own bit
    expect = int("111100000" * 3 + "11110000" + "111100000" * 3, 2)
    assert int(code[3, 4]) == expect and expect < 2 ** 62
    assert int(code[0, 0]) == 0                                               # nothing is below the minimum
    # top right corner: clamping repeats column 8 and row 0, so dx < 0 is below the centre and dx >= 0 is not
    assert int(code[0, 8]) == expect
    vert = np.tile((10 * np.arange(7, dtype=np.uint8))[:, None], (1, 9))      # img(y, x) = 10 y
    assert int(R.census(vert)[3, 4]) == int("1" * 27 + "0" * 35, 2)
    # the first neighbour scanned (dy = -3, dx = -4) is the most significant of the 62 bits
    one = np.full((7, 9), 9, dtype=np.uint8)
    one[0, 0] = 0
    assert int(R.census(one)[3, 4]) == 1 << 61


def test_cost_is_64_outside_the_image():
    rng = np.random.default_rng(3)
    left, right = rng.integers(0, 256, (5, 12)).astype(np.uint8), rng.integers(0, 256, (5, 12)).astype(np.uint8)
    cl, cr = R.census(left), R.census(right)
    Cv = R.cost_volume(cl, cr, -3, 16)
    for x in range(12):
        for k in range(16):
            xr = x - (-3 + k)
            if 0 <= xr < 12:
                assert all(int(Cv[y, x, k]) == bin(int(cl[y, x]) ^ int(cr[y, xr])).count("1") for y in range(5))
                assert Cv[:, x, k].max() <= 62
            else:
                assert np.all(Cv[:, x, k] == 64)


def test_single_path_recurrence_by_hand():
    Cv = np.full((1, 4, 16), 10, dtype=np.uint8)
    Cv[0, 0, 3] = 0
    Cv[0, 1, 5] = 0
    Cv[0, 2, 5], Cv[0, 2, 15] = 1, 0
    Cv[0, 3, :] = 3
    L = R.aggregate_direction(Cv, 1, 0, 2, 5)
    assert L[0, 0].tolist() == Cv[0, 0].tolist()                              # the path starts here
    l1 = [15] * 16
    l1[2], l1[3], l1[4], l1[5] = 12, 10, 12, 5                                # m = 0: min(10, 0 + 2, 0 + 5) beside k = 3
    assert L[0, 1].tolist() == l1
    l2 = [15] * 16
    l2[4], l2[5], l2[6], l2[15] = 12, 1, 12, 5                                # m = 5; k = 15 has no k + 1 term
    assert L[0, 2].tolist() == l2
    l3 = [8] * 16
    l3[4], l3[5], l3[6], l3[15] = 5, 3, 5, 7                                  # m = 1
    assert L[0, 3].tolist() == l3
    # the opposite direction on the mirrored volume is the mirror image
    assert np.array_equal(R.aggregate_direction(Cv[:, ::-1], -1, 0, 2, 5)[:, ::-1], L)


def test_subpixel_floor_division_with_negative_numerator():
    S = np.full((1, 1, 16), 100, dtype=np.uint16)
    S[0, 0, 4], S[0, 0, 5], S[0, 0, 6] = 11, 10, 30
    # den = 11 + 30 - 20 = 21, numerator (11 - 30) * 16 + 21 = -283, floor(-283 / 42) = -7 (truncation would give -6)
    assert R.disparity(S, 0, 0, -1)[0, 0] == 16 * 5 - 7
    assert R.disparity(S, -8, 0, -1)[0, 0] == 16 * (5 - 8) - 7
    S[0, 0, 4], S[0, 0, 6] = 30, 11
    assert R.disparity(S, 0, 0, -1)[0, 0] == 16 * 5 + (19 * 16 + 21) // 42
    tie = np.full((1, 1, 16), 7, dtype=np.uint16)                             # all equal: the lowest k, no parabola at k = 0
    assert R.disparity(tie, 2, 0, -1)[0, 0] == 32
    assert R.disparity(tie, 2, 10, -1)[0, 0] == 16                            # and not unique: 7 * 90 < 7 * 100


@pytest.mark.parametrize("paths", [4, 8])
def test_synthetic_shift_pair(paths):
    left, right, d = R.shifted_noise_pair()
    disp = R.match(left, right, num_disparities=32, p1=8, p2=32, uniqueness_ratio=10, disp12_max_diff=1, paths=paths).astype(np.int32)
    rows = np.array([y for y in range(4, 44) if not 20 <= y < 28])            # without the 8 rows around the seam
    inner = disp[rows, 36:92]
    assert np.all(inner != 16 * (0 - 1)), "every interior pixel is valid"
    assert np.all(np.abs(inner - 16 * d[rows][:, None]) <= 16)


def _images(w=24, h=10, stride=None):
    stride = stride or w
    a = np.zeros((h, stride), dtype=np.uint8)
    return a, a.copy()


def _call_match(left, right, w, h, stride, params, disp_stride=None, disp=True):
    ub = C.POINTER(C.c_ubyte)
    disp_stride = w if disp_stride is None else disp_stride
    out = np.zeros((max(h, 1), max(disp_stride, 1)), dtype=np.int16)
    rc = lib.lib().tscm_stereo_match(None if left is None else left.ctypes.data_as(ub), None if right is None else right.ctypes.data_as(ub), w, h, stride,
                                     None if params is None else C.byref(params), 0, out.ctypes.data_as(C.POINTER(C.c_short)) if disp else None, disp_stride, None)
    return rc, lib.lib().tscm_last_error().decode()


def test_default_params():
    p = stereo.params()
    assert p.struct_size == C.sizeof(lib.CStereoParams) == 32
    assert (p.min_disparity, p.num_disparities, p.p1, p.p2, p.paths, p.uniqueness_ratio, p.disp12_max_diff) == (0, 128, 8, 32, 8, 10, 1)
    assert (p.min_disparity, p.num_disparities, p.p1, p.p2, p.paths, p.uniqueness_ratio, p.disp12_max_diff) == tuple(
        R.DEFAULTS[k] for k in ("min_disparity", "num_disparities", "p1", "p2", "paths", "uniqueness_ratio", "disp12_max_diff"))


@pytest.mark.parametrize("field,value,word", [
    ("num_disparities", 24, "num_disparities"), ("num_disparities", 0, "num_disparities"), ("num_disparities", 272, "num_disparities"),
    ("paths", 5, "paths"), ("paths", 16, "paths"), ("p1", 40, "p1"), ("p2", 256, "p2"), ("p1", -1, "p1"),
    ("struct_size", 28, "struct_size"), ("struct_size", 36, "struct_size"), ("uniqueness_ratio", 100, "uniqueness_ratio"),
    ("min_disparity", 2000, "min_disparity"),
])
def test_match_refuses_bad_params_before_any_device(field, value, word):
    left, right = _images()
    p = stereo.params()
    setattr(p, field, value)
    rc, text = _call_match(left, right, 24, 10, 24, p)
    assert rc == -1 and word in text, text
    ub = C.POINTER(C.c_ubyte)
    assert lib.lib().tscm_stereo_stages(left.ctypes.data_as(ub), right.ctypes.data_as(ub), 24, 10, 24, C.byref(p), 0, None, None, None, None) == -1
    assert word in lib.lib().tscm_last_error().decode()


def test_match_refuses_bad_geometry_before_any_device():
    left, right = _images()
    p = stereo.params()
    for args, word in ((dict(left=None), "left"), (dict(right=None), "right"), (dict(stride=23), "stride"), (dict(disp_stride=23), "disp_stride"),
                       (dict(disp=False), "disparity"), (dict(params=None), "params")):
        kw = dict(left=left, right=right, w=24, h=10, stride=24, params=p)
        kw.update(args)
        rc, text = _call_match(**kw)
        assert rc == -1 and word in text, (args, text)
    # an empty image is not an error and needs no device
    assert _call_match(left, right, 0, 10, 24, p)[0] == 0
    assert _call_match(left, right, 24, 0, 24, p)[0] == 0
    # the Python layer raises the same refusals
    with pytest.raises(lib.TscmError) as e:
        stereo.match(left, right, paths=6)
    assert e.value.code == -1 and "paths" in str(e.value)
    with pytest.raises(TypeError):
        stereo.match(left, right, no_such_parameter=1)


def test_points_refusals_before_any_device():
    disp = np.zeros((4, 6), dtype=np.int16)
    pts, valid = np.zeros((4, 6, 3)), np.zeros((4, 6), dtype=np.uint8)
    m = lib.CMapDesc()
    m.fx = m.fy = 100.0
    sp, ub = C.POINTER(C.c_short), C.POINTER(C.c_ubyte)
    f = lib.lib().tscm_stereo_points
    for kind in (lib.PROJ_CYLINDRICAL, lib.PROJ_STEREOGRAPHIC, lib.PROJ_EQUIRECT, 7, -1):
        assert f(disp.ctypes.data_as(sp), 6, 4, 6, 0, C.byref(m), kind, 1.0, 0, lib.dptr(pts), valid.ctypes.data_as(ub)) == -1
        assert "projection" in lib.lib().tscm_last_error().decode()
    assert f(disp.ctypes.data_as(sp), 6, 4, 5, 0, C.byref(m), lib.PROJ_LONGLAT, 1.0, 0, lib.dptr(pts), valid.ctypes.data_as(ub)) == -1
    assert "disp_stride" in lib.lib().tscm_last_error().decode()
    assert f(None, 6, 4, 6, 0, C.byref(m), lib.PROJ_LONGLAT, 1.0, 0, lib.dptr(pts), valid.ctypes.data_as(ub)) == -1
    assert "disparity" in lib.lib().tscm_last_error().decode()
    assert f(disp.ctypes.data_as(sp), 6, 4, 6, 0, None, lib.PROJ_LONGLAT, 1.0, 0, lib.dptr(pts), valid.ctypes.data_as(ub)) == -1
    assert "left_map" in lib.lib().tscm_last_error().decode()
    assert f(disp.ctypes.data_as(sp), 0, 4, 6, 0, C.byref(m), lib.PROJ_LONGLAT, 1.0, 0, lib.dptr(pts), valid.ctypes.data_as(ub)) == 0


def test_stereo_pair_demo_compiles_and_links(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "tscm_calib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "examples", "stereo_pair_demo.cpp"), "-L", csrc, "-ltscm_hip", "-Wl,-rpath," + csrc,
                           "-o", str(tmp_path / "stereo_pair_demo")])


def test_out_of_range_device_is_no_device_and_arguments_come_first():
    """What tests/test_device_selection.py asks of every entry point with a device index, for the stereo entry points."""
    L = lib.lib()
    left, right = _images()
    p = stereo.params(num_disparities=16)
    ub, sp = C.POINTER(C.c_ubyte), C.POINTER(C.c_short)
    lp, rp = left.ctypes.data_as(ub), right.ctypes.data_as(ub)
    disp = np.zeros((10, 24), dtype=np.int16)
    pts, valid = np.zeros((10, 24, 3)), np.zeros((10, 24), dtype=np.uint8)
    m = lib.CMapDesc()
    m.fx = m.fy = 10.0
    n = L.tscm_device_count()
    for dv in (n, -1):
        assert L.tscm_stereo_match(lp, rp, 24, 10, 24, C.byref(p), dv, disp.ctypes.data_as(sp), 24, None) == -2
        assert L.tscm_last_error()
        assert L.tscm_stereo_stages(lp, rp, 24, 10, 24, C.byref(p), dv, None, None, None, None) == -2
        assert L.tscm_stereo_points(disp.ctypes.data_as(sp), 24, 10, 24, 0, C.byref(m), lib.PROJ_LONGLAT, 1.0, dv, lib.dptr(pts), valid.ctypes.data_as(ub)) == -2
    assert L.tscm_stereo_match(None, rp, 24, 10, 24, C.byref(p), n, disp.ctypes.data_as(sp), 24, None) == -1
    assert L.tscm_stereo_stages(lp, None, 24, 10, 24, C.byref(p), n, None, None, None, None) == -1
    assert L.tscm_stereo_points(disp.ctypes.data_as(sp), 24, 10, 24, 0, C.byref(m), lib.PROJ_LONGLAT, 1.0, n, None, valid.ctypes.data_as(ub)) == -1
