"""CPU tests of the composer at the swept depth: the properties of the definition on the host restatement
tests/sweep_compose_ref.py (the rounding and the clamp of the hypothesis index, the fallback, a constant map against
pano_ref.compose), the reference figures of the sphere scene that tests/test_gpu_sweep_compose.py uses, and the exports,
defaults and the refusal of the C ABI that is decided before any device is touched."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import maps_proj_ref as mref
from tests import pano_ref
from tests import sweep_compose_ref as CR
from tests import sweep_ref
from tests import test_gpu_sweep as scene
from tscm_calib_amd import lib, sweep


# ------------------------------------------------------------------------------------------------ hypothesis index
def test_the_index_rounds_to_the_nearest_hypothesis_both_ways():
    """(index16 + 8) >> 4: 16 z - 8 is the first value of z, 16 z + 7 the last; 16 z + 8 belongs to z + 1."""
    D = 32
    for z in (1, 5, 30):
        idx = np.array([[16 * z - 9, 16 * z - 8, 16 * z, 16 * z + 7, 16 * z + 8]], dtype=np.int16)
        assert CR.hypothesis(idx, D).tolist() == [[z - 1, z, z, z, z + 1]]
    assert CR.hypothesis(np.array([[0, 7, 8]], dtype=np.int16), D).tolist() == [[0, 0, 1]]


def test_the_index_is_clamped_at_the_last_hypothesis():
    D = 16
    idx = np.array([[16 * (D - 1) - 8, 16 * (D - 1) + 8, 16 * D, 16 * D + 40, 32767]], dtype=np.int16)
    assert CR.hypothesis(idx, D).tolist() == [[D - 1] * 5]
    assert CR.hypothesis(np.array([[32767]], dtype=np.int16), 256).tolist() == [[255]]          # no overflow of the + 8


@pytest.mark.parametrize("fallback", [0, 3, 15])
def test_negative_entries_take_the_fallback(fallback):
    idx = np.array([[-16, -1, -32768, 0, 48]], dtype=np.int16)
    assert CR.hypothesis(idx, 16, fallback).tolist() == [[fallback, fallback, fallback, 0, 3]]


def test_the_gather_takes_each_pixel_from_its_own_plane():
    maps = np.arange(2 * 3 * 2 * 4, dtype=np.float32).reshape(2, 3, 2, 4)
    z = np.array([[0, 1, 2, 0], [2, 2, 1, 0]])
    g = CR.gather(maps, z)
    for k in range(2):
        for i in range(2):
            for j in range(4):
                assert g[k, i, j] == maps[k, z[i, j], i, j]


# ------------------------------------------------------------------------------------------------ against pano_ref
def _small(n=3, D=16, pw=16, ph=8, w=24, h=20, ch=1, seed=0):
    rng = np.random.default_rng(seed)
    mx = rng.uniform(-3.0, w + 2.0, (n, D, ph, pw)).astype(np.float32)
    my = rng.uniform(-3.0, h + 2.0, (n, D, ph, pw)).astype(np.float32)
    imgs = [rng.integers(0, 256, (h, w) if ch == 1 else (h, w, 3)).astype(np.uint8) for _ in range(n)]
    wgt = [None if k == 1 else rng.integers(0, 256, (h, w)).astype(np.uint8) for k in range(n)]
    return imgs, wgt, mx, my


@pytest.mark.parametrize("mode", [CR.SEAM, CR.FEATHER, CR.MULTIBAND])
@pytest.mark.parametrize("ch", [1, 3])
def test_a_constant_map_reproduces_the_panorama_on_that_table(mode, ch):
    imgs, wgt, mx, my = _small(ch=ch)
    for z0 in (0, 7, 15):
        got = CR.compose(imgs, wgt, mx, my, np.full((8, 16), 16 * z0, np.int16), mode=mode, levels=2, wrap=True, gains=[300, 256, 200])
        want = pano_ref.compose(imgs, wgt, mx[:, z0], my[:, z0], mode=mode, levels=2, wrap=True, gains=[300, 256, 200])
        for name in ("out", "sampled", "alpha", "label", "coverage"):
            assert np.array_equal(got[name], want[name]), name
        assert np.all(got["hypothesis"] == z0)
    # an all-invalid map with fallback 0 is the table at index 0: today's panorama when inv_distance[0] = 0
    got = CR.compose(imgs, wgt, mx, my, np.full((8, 16), sweep.INVALID, np.int16), mode=mode, levels=2, fallback_index=0)
    assert np.array_equal(got["out"], pano_ref.compose(imgs, wgt, mx[:, 0], my[:, 0], mode=mode, levels=2)["out"])


def test_a_mixed_map_takes_each_pixel_from_its_own_table():
    """SEAM and FEATHER are per pixel, so the output at a pixel with hypothesis z is the output of the panorama on table z."""
    imgs, wgt, mx, my = _small()
    rng = np.random.default_rng(5)
    idx = rng.integers(-16, 16 * 16 + 40, (8, 16)).astype(np.int16)
    z = CR.hypothesis(idx, 16, 4)
    assert (idx < 0).any() and (idx > 16 * 16).any()
    for mode in (CR.SEAM, CR.FEATHER):
        got = CR.compose(imgs, wgt, mx, my, idx, mode=mode, fallback_index=4)
        for z0 in np.unique(z):
            want = pano_ref.compose(imgs, wgt, mx[:, z0], my[:, z0], mode=mode)
            assert np.array_equal(got["out"][z == z0], want["out"][z == z0])
            assert np.array_equal(got["coverage"][z == z0], want["coverage"][z == z0])


# ------------------------------------------------------------------------------------------------ the sphere scene
# Mean absolute error of the composed 160 x 80 panorama of the scene of tests/test_gpu_sweep.py against
# the same texture seen from the rig origin, 4 x 4 supersampled (sweep_compose_ref.equirect_truth), by the restatements alone:
#   python -c "from tests import test_sweep_compose_reference as t; print(t.sphere_table())"
# Rows: composed at infinity (all invalid, fallback 0), at the swept index map of the reference chain, at the true
# hypothesis (index 10 everywhere: 24800 / 10 = 2480 mm); columns SEAM, FEATHER, MULTIBAND with 3 levels.
SPHERE_TABLE = {
    "infinity": (26.24, 48.11, 27.29),
    "swept": (12.07, 11.76, 15.45),
    "truth": (12.06, 11.60, 15.44),
}
# What the issue that asked for the composer measured with its own render of the texture; the render's sampling pattern is
# not part of the definition, and 4 x 4 against 16 x 16 positions per pixel alone moves the FEATHER figure from 11.76 to
# 10.71, so the two tables are held together to one grey level.  The GPU test takes its bound from this row's 11.4.
ISSUE_TABLE = {
    "infinity": (25.98, 47.77, 27.03),
    "swept": (11.73, 11.37, 15.13),
    "truth": (11.72, 11.21, 15.12),
}
SPHERE_FEATHER_CPU = 11.4             # the reference value the GPU test doubles
SPHERE_RATIO_CPU = 0.24               # FEATHER at the swept map over FEATHER at infinity
LEVELS = 3


def sphere_shade(lon, lat, cell=0.1):
    return scene._hash_gray(np.floor(lon / cell), np.floor(lat / cell))


@functools.lru_cache(maxsize=None)
def sphere_truth():
    t = CR.equirect_truth(sphere_shade, scene.SCENE["pano_w"], scene.SCENE["pano_h"], 4)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def sphere_reference():
    """The reference tables of the scene (numpy fp64 with the centre term) and the index map of the host sweep on them."""
    intr, T, imgs = scene.sphere_scene()
    pw, ph = scene.SCENE["pano_w"], scene.SCENE["pano_h"]
    inv = sweep.inverse_distances(scene.SCENE["near"], D=scene.SCENE["D"])
    descs = [mref.Desc(intr[k], T[k][:, :3].T, pw / (2 * np.pi), ph / np.pi, pw / 2.0, ph / 2.0, pw, ph, mref.EQUIRECT, check_w2=1) for k in range(4)]
    mx, my, _ = sweep_ref.build_sweep_maps_ref(descs, T[:, :, 3], inv)
    idx = sweep_ref.stages(imgs, None, mx, my, paths=scene.SCENE["paths"], wrap_x=True)["index16"]
    return mx, my, idx


def sphere_errors(imgs, mx, my, index16) -> tuple:
    """(SEAM, FEATHER, MULTIBAND) error of the restatement on the given tables and index map, and the smallest coverage"""
    out, cov = [], 255
    for mode in (CR.SEAM, CR.FEATHER, CR.MULTIBAND):
        res = CR.compose(imgs, None, mx, my, index16, mode=mode, levels=LEVELS, wrap=True, fallback_index=0)
        out.append(CR.mean_abs_error(res["out"], sphere_truth()))
        cov = min(cov, int(res["coverage"].min()))
    return tuple(out), cov


def sphere_table() -> dict:
    _, _, imgs = scene.sphere_scene()
    mx, my, idx = sphere_reference()
    shape = idx.shape
    rows = dict(infinity=np.full(shape, sweep.INVALID, np.int16), swept=idx, truth=np.full(shape, 160, np.int16))
    return {name: sphere_errors(imgs, mx, my, m) for name, m in rows.items()}


def test_the_sphere_scene_gives_the_committed_figures():
    table = sphere_table()
    _, _, idx = sphere_reference()
    assert abs(float((idx >= 0).mean()) - scene.SPHERE_VALID_SHARE_CPU) < 5e-4
    for name, (errs, cov) in table.items():
        print(name, ["%.2f" % e for e in errs], "smallest coverage", cov)
        assert cov >= 2                                            # every pixel is seen by at least two cameras
        for got, want, issue in zip(errs, SPHERE_TABLE[name], ISSUE_TABLE[name]):
            assert abs(got - want) < 0.005
            assert abs(got - issue) < 1.0
    swept, inf = table["swept"][0], table["infinity"][0]
    assert abs(swept[1] / inf[1] - SPHERE_RATIO_CPU) < 0.005 and SPHERE_RATIO_CPU < 0.5
    assert abs(swept[1] - SPHERE_FEATHER_CPU) < 0.5                # the GPU test's reference value, to half a grey level
    # the nearest hypothesis is as good as the true one: no interpolation between hypotheses is needed
    for a, b in zip(swept, table["truth"][0]):
        assert abs(a - b) < 0.2


# ------------------------------------------------------------------------------------------------ C ABI
def test_the_new_symbols_are_exported():
    L = lib.lib()
    for name in ("tscm_sweep_compose_default_params", "tscm_sweep_compose", "tscm_sweep_compose_stages"):
        assert name in lib.EXPORTS
        assert hasattr(L, name)
    assert L.tscm_abi_version() == 6


def test_default_params():
    p = sweep.compose_params()
    assert (p.struct_size, p.mode, p.levels, p.wrap_x, p.fallback_index) == (C.sizeof(lib.CSweepComposeParams), lib.PANO_MULTIBAND, 4, 1, 0)
    assert sweep.compose_params(mode="seam", fallback_index=3).mode == lib.PANO_SEAM
    with pytest.raises(ValueError):
        sweep.compose_params(mode="average")
    with pytest.raises(AttributeError):
        sweep.compose_params(struct_size=4)


def test_a_null_handle_is_refused_before_any_device_is_touched():
    L = lib.lib()
    p = sweep.compose_params()
    out = np.zeros(16, np.uint8)
    o = out.ctypes.data_as(C.POINTER(C.c_ubyte))
    assert L.tscm_sweep_compose(None, None, 4, 1, None, 4, C.byref(p), None, o, 4, None, None) == -1
    assert b"s is NULL" in L.tscm_last_error()
    assert L.tscm_sweep_compose_stages(None, None, 4, 1, None, 4, C.byref(p), None, None, None, None, None, None, None, None) == -1
    assert b"s is NULL" in L.tscm_last_error()
    assert not out.any()


def test_bgr_to_gray_is_the_composers_luminance():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    assert np.array_equal(sweep.bgr_to_gray(img), pano_ref.luminance(img).astype(np.uint8))
    assert sweep.bgr_to_gray(img[..., 0]) is not None and sweep.bgr_to_gray(img[..., 0]).shape == (5, 7)
