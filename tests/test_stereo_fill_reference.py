"""CPU tests of the hole filling's definition (include/tscm/tscm.h, tscm_stereo_fill*): the host restatement
tests/stereo_fill_ref.py on hand-worked maps, its two independently written candidate searches against each other, the
reference figures of the sphere scene that tests/test_gpu_stereo_fill.py uses, and the exports, defaults and refusals of
the C ABI that are decided before any device is touched."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import maps_proj_ref as mref
from tests import stereo_fill_ref as F
from tests import sweep_compose_ref as CR
from tests import sweep_ref
from tests import test_gpu_sweep as scene
from tests import test_sweep_compose_reference as compose_scene
from tscm_calib_amd import lib, stereo, sweep, synth

INV = -16                                                                     # min_disparity = 0


def _holes(h, w, fill=INV):
    return np.full((h, w), fill, dtype=np.int16)


def _both(d, **p):
    """The restatement by the walk and by the scan, which must agree; returns the walk's stages."""
    a, b = F.stages(d, walk=True, **p), F.stages(d, **p)
    for k in ("value", "distance", "out", "mask"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    return a


# ------------------------------------------------------------------------------------------------ the two restatements
@pytest.mark.parametrize("seed", range(6))
def test_walk_equals_scan(seed):
    rng = np.random.default_rng(seed)
    shapes = [(1, 1), (1, 9), (9, 1), (7, 12), (12, 7), (5, 5)]
    h, w = shapes[seed]
    for share in (0.3, 0.9, 0.999):
        d = (16 * rng.integers(-40, 200, size=(h, w)) + 3).astype(np.int16)
        d[rng.random((h, w)) < share] = INV
        for wrap_x in (0, 1):
            for max_distance in (0, 1, 3):
                for paths in (4, 8):
                    s = _both(d, wrap_x=wrap_x, max_distance=max_distance, paths=paths, rule=seed % 3, min_directions=1 + seed % 4)
                    assert s["value"].shape == (paths, h, w) and s["value"].dtype == np.int16 and s["distance"].dtype == np.int16
                    assert np.all(s["value"][s["distance"] == 0] == INV)
                    assert np.array_equal(s["mask"] == 0, d != INV) and np.array_equal(s["out"][d != INV], d[d != INV])


# ------------------------------------------------------------------------------------------------ rules
def _star(values):
    """An 11 x 11 map, all invalid but one pixel in each direction from the centre (5, 5): values[r] at distance r + 1 for
    direction r of F.DIRECTIONS; None leaves the direction empty."""
    d = _holes(11, 11)
    for r, v in enumerate(values):
        if v is not None:
            dx, dy = F.DIRECTIONS[r]
            d[5 + (r % 5 + 1) * dy, 5 + (r % 5 + 1) * dx] = v
    return d


def test_each_rule_on_eight_candidates():
    values = [70, 10, 50, 30, 80, 20, 60, 40]
    s = {rule: _both(_star(values), rule=rule) for rule in F.RULES}
    assert s["lowest"]["value"][:, 5, 5].tolist() == values
    assert s["lowest"]["distance"][:, 5, 5].tolist() == [1, 2, 3, 4, 5, 1, 2, 3]
    assert s["lowest"]["out"][5, 5] == 10 and s["second_lowest"]["out"][5, 5] == 20
    assert s["median"]["out"][5, 5] == 40                                     # index (8 - 1) >> 1 = 3 of 10 20 30 40 50 60 70 80
    assert all(x["mask"][5, 5] == 1 for x in s.values())


@pytest.mark.parametrize("values,lowest,second,median", [
    ([None, None, 90, None, None, None, None, None], 90, 90, 90),            # n = 1: min(1, n - 1) = 0
    ([None, 50, None, None, None, None, 20, None], 20, 50, 20),              # n = 2: median index 0
    ([None, 50, None, 70, None, None, 20, None], 20, 50, 50),                # n = 3
])
def test_each_rule_on_few_candidates(values, lowest, second, median):
    d = _star(values)
    assert _both(d, rule=F.LOWEST)["out"][5, 5] == lowest
    assert _both(d, rule=F.SECOND_LOWEST)["out"][5, 5] == second
    assert _both(d, rule=F.MEDIAN)["out"][5, 5] == median


def test_the_ends_of_int16_sort_as_integers():
    d = _star([None, 32767, None, -32768 + 16, None, None, 0, None])
    assert _both(d, rule=F.LOWEST)["out"][5, 5] == -32768 + 16
    assert _both(d, rule=F.MEDIAN)["out"][5, 5] == 0
    d = _star([None, 32767, None, -32768 + 16, None, None, None, None])
    assert _both(d, rule=F.SECOND_LOWEST)["out"][5, 5] == 32767


# ------------------------------------------------------------------------------------------------ parameters
def test_max_distance_at_t_and_below():
    d = _holes(1, 9)
    d[0, 6] = 320                                                             # t = 4 from column 2, looking along +x
    assert _both(d, max_distance=4)["out"][0, 2] == 320
    far = _both(d, max_distance=3)
    assert far["out"][0, 2] == INV and far["mask"][0, 2] == 2 and far["out"][0, 3] == 320
    assert _both(d, max_distance=0)["out"][0, 0] == 320                       # 0: no limit


def test_min_directions_at_n_and_above():
    d = _star([None, 50, None, 70, None, None, 20, None])                     # n = 3 at the centre
    assert _both(d, min_directions=3)["mask"][5, 5] == 1
    s = _both(d, min_directions=4)
    assert s["mask"][5, 5] == 2 and s["out"][5, 5] == INV


def test_four_paths_ignore_the_diagonals():
    d = _star([None, None, None, None, 10, 20, 30, 40])
    s = _both(d, paths=4)
    assert s["mask"][5, 5] == 2 and s["value"].shape[0] == 4
    assert _both(d, paths=8)["out"][5, 5] == 20                               # the median of four
    d[5, 9] = 90
    assert _both(d, paths=4)["out"][5, 5] == 90


def test_a_hole_across_the_seam_is_filled_from_the_other_side_only_with_wrap_x():
    d = _holes(1, 10)
    d[0, 3] = 111
    d[0, 6] = 222
    flat, wrapped = _both(d, wrap_x=0), _both(d, wrap_x=1)
    # column 9: looking along +x leaves the map, or meets column 3 after 4 steps; along -x column 6
    assert flat["value"][0, 0, 9] == INV and wrapped["value"][0, 0, 9] == 111 and wrapped["distance"][0, 0, 9] == 4
    assert flat["out"][0, 9] == 222 and wrapped["out"][0, 9] == 111           # the median of two is the lower
    assert flat["out"][0, 0] == 111 and wrapped["value"][1, 0, 0] == 222 and wrapped["distance"][1, 0, 0] == 4
    # a diagonal continues over the seam
    e = _holes(3, 5)
    e[2, 0] = 55
    assert _both(e, wrap_x=0)["mask"][0, 3] == 2
    s = _both(e, wrap_x=1)
    assert s["out"][0, 3] == 55 and s["distance"][4, 0, 3] == 2


def test_a_wrapped_horizontal_walk_never_returns_the_pixel_itself():
    one = np.array([[320]], dtype=np.int16)
    s = _both(one, wrap_x=1)
    assert not s["distance"].any() and s["out"][0, 0] == 320
    s = _both(_holes(1, 1), wrap_x=1)
    assert s["mask"][0, 0] == 2
    col = _holes(3, 1)                                                        # w = 1: a wrapped diagonal is the column
    col[2, 0] = 7
    s = _both(col, wrap_x=1)
    assert s["distance"][:, 0, 0].tolist() == [0, 0, 2, 0, 2, 0, 0, 2] and not _both(col, wrap_x=0)["distance"][4:].any()
    d = _holes(1, 8)
    d[0, 5] = 320                                                             # the only valid pixel of its row
    s = _both(d, wrap_x=1)
    assert s["distance"][0, 0].tolist() == [5, 4, 3, 2, 1, 0, 7, 6] and s["distance"][1, 0].tolist() == [3, 4, 5, 6, 7, 0, 1, 2]
    assert np.all(s["out"] == 320) and s["mask"][0].tolist() == [1, 1, 1, 1, 1, 0, 1, 1]


def test_the_all_valid_and_the_all_invalid_map():
    rng = np.random.default_rng(3)
    d = (16 * rng.integers(0, 50, size=(6, 9))).astype(np.int16)
    s = _both(d, wrap_x=1)
    assert np.array_equal(s["out"], d) and not s["mask"].any()
    s = _both(_holes(6, 9), wrap_x=1)
    assert np.all(s["out"] == INV) and np.all(s["mask"] == 2)
    assert F.stages(np.zeros((0, 5), np.int16))["out"].shape == (0, 5) and F.stages(np.zeros((4, 0), np.int16))["value"].shape == (8, 4, 0)


def test_min_disparity_moves_the_invalid_value():
    d = _holes(1, 4, fill=F.invalid_value(7))
    d[0, 1] = INV                                                             # -16 is a value here
    assert _both(d, min_disparity=7)["out"][0].tolist() == [INV] * 4


# ------------------------------------------------------------------------------------------------ the sphere scene
# Measured with this file's sphere_fill_figures(): the reference tables and the host sweep of
# tests/test_sweep_compose_reference.py (index map 99.6 % valid), the holes below, the restatement with the defaults plus
# wrap_x = 1, then sweep_ref.points and the FEATHER composition of tests/sweep_compose_ref.py against sphere_truth().
SPHERE_HOLE_SHARE = 0.337
SPHERE_FILL_MEDIAN_MM = dict(median=20.0, second_lowest=11.4, lowest=27.4, original=20.0)   # median | |P| - 2500 | on the holes
SPHERE_FILL_FEATHER = dict(filled=14.51, original=14.70, fallback=48.75)                    # FEATHER error on the holes, grey levels
SPHERE_FILL_FEATHER_FRAME = dict(filled=11.68, original=11.76, fallback=23.24)              # the same over the whole frame
SPHERE_FILL_RATIO = 0.30                                                                    # filled / fallback on the holes


@functools.lru_cache(maxsize=None)
def sphere_holes() -> np.ndarray:
    """bool [80, 160]: scattered pixels, a block across the seam, a block in the middle and the first six rows."""
    ph, pw = scene.SCENE["pano_h"], scene.SCENE["pano_w"]
    yy, xx = np.mgrid[0:ph, 0:pw]
    holes = (synth.splitmix64((yy * 160 + xx).astype(np.uint64)) >> np.uint64(56)) < np.uint64(51)
    holes[10:30, 150:160] = True
    holes[10:30, 0:12] = True
    holes[50:70, 60:100] = True
    holes[0:6] = True
    holes.setflags(write=False)
    return holes


def error_on(pano, truth, where) -> float:
    return float(np.abs(np.asarray(pano).astype(np.int64).reshape(truth.shape) - truth.astype(np.int64))[where].mean())


def sphere_fill_figures() -> dict:
    intr, T, imgs = scene.sphere_scene()
    mx, my, idx = compose_scene.sphere_reference()
    truth, holes = compose_scene.sphere_truth(), sphere_holes()
    ph, pw = idx.shape
    inv = sweep.inverse_distances(scene.SCENE["near"], D=scene.SCENE["D"])
    desc = mref.Desc(intr[0], T[0][:, :3].T, pw / (2 * np.pi), ph / np.pi, pw / 2.0, ph / 2.0, pw, ph, mref.EQUIRECT, check_w2=1)
    knocked = idx.copy()
    knocked[holes] = sweep.INVALID

    def median_mm(m):
        pts, valid = sweep_ref.points(m, desc, inv)
        return float(np.median(scene.sphere_error(pts, valid & holes)))

    def feather(m):
        out = CR.compose(imgs, None, mx, my, m, mode=CR.FEATHER, wrap=True, fallback_index=0)["out"]
        return error_on(out, truth, holes), error_on(out, truth, np.ones_like(holes))

    maps = dict(original=idx, fallback=knocked)
    left = {}
    for rule in F.RULES:
        maps[rule], mask = F.fill(knocked, rule=rule, wrap_x=1)
        left[rule] = int((mask == 2).sum())
    return dict(share=float(holes.mean()), left=left, median_mm={k: median_mm(m) for k, m in maps.items() if k != "fallback"},
                feather={k: feather(maps[k]) for k in ("median", "original", "fallback")})


def test_the_sphere_scene_gives_the_committed_fill_figures():
    fig = sphere_fill_figures()
    print(fig)
    assert abs(fig["share"] - SPHERE_HOLE_SHARE) < 5e-4
    assert fig["left"] == dict(lowest=0, second_lowest=0, median=0)            # no invalid pixel is left: a condition on the scene
    for k, want in SPHERE_FILL_MEDIAN_MM.items():
        assert abs(fig["median_mm"][k] - want) < 0.05, k
    for k, name in (("median", "filled"), ("original", "original"), ("fallback", "fallback")):
        assert abs(fig["feather"][k][0] - SPHERE_FILL_FEATHER[name]) < 0.01, name
        assert abs(fig["feather"][k][1] - SPHERE_FILL_FEATHER_FRAME[name]) < 0.01, name
    ratio = fig["feather"]["median"][0] / fig["feather"]["fallback"][0]
    assert abs(ratio - SPHERE_FILL_RATIO) < 0.005 and SPHERE_FILL_RATIO < 0.5
    # the filled map composes as well as the one the holes were cut from
    assert abs(fig["feather"]["median"][0] - fig["feather"]["original"][0]) < 0.5


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_new_symbols_are_exported():
    L = lib.lib()
    for name in ("tscm_stereo_fill_default_params", "tscm_stereo_fill", "tscm_stereo_fill_stages"):
        assert name in lib.EXPORTS
        assert hasattr(L, name)
    assert L.tscm_abi_version() == 6


def test_fill_default_params():
    p = stereo.fill_params()
    names = ("min_disparity", "rule", "paths", "max_distance", "min_directions", "wrap_x")
    assert p.struct_size == C.sizeof(lib.CStereoFillParams) == 28
    assert tuple(getattr(p, k) for k in names) == (0, lib.FILL_MEDIAN, 8, 0, 1, 0) == tuple(F.DEFAULTS[k] for k in names)
    assert (lib.FILL_LOWEST, lib.FILL_SECOND_LOWEST, lib.FILL_MEDIAN) == (F.LOWEST, F.SECOND_LOWEST, F.MEDIAN) == (0, 1, 2)
    assert [stereo.fill_params(rule=r).rule for r in ("lowest", "second_lowest", "median")] == [0, 1, 2]
    with pytest.raises(ValueError):
        stereo.fill_params(rule="mean")


def _call_fill(disp=True, w=24, h=10, disp_stride=24, params="default", out=True, out_stride=24, stages=False, **fields):
    sp = C.POINTER(C.c_short)
    a = np.zeros((10, 24), dtype=np.int16)
    o = np.zeros((10, 24), dtype=np.int16)
    p = stereo.fill_params() if params == "default" else params
    for k, v in fields.items():
        setattr(p, k, v)
    pp = None if p is None else C.byref(p)
    L = lib.lib()
    if stages:
        rc = L.tscm_stereo_fill_stages(a.ctypes.data_as(sp) if disp else None, w, h, disp_stride, pp, 0, None, None)
    else:
        rc = L.tscm_stereo_fill(a.ctypes.data_as(sp) if disp else None, w, h, disp_stride, pp, 0, o.ctypes.data_as(sp) if out else None, out_stride, None, None)
    return rc, L.tscm_last_error().decode()


@pytest.mark.parametrize("args,word", [
    (dict(disp=False), "disparity"), (dict(params=None), "params"), (dict(out=False), "out"),
    (dict(disp_stride=23), "disp_stride"), (dict(out_stride=23), "out_stride"),
    (dict(struct_size=24), "struct_size"), (dict(struct_size=32), "struct_size"),
    (dict(rule=-1), "rule"), (dict(rule=3), "rule"),
    (dict(paths=0), "paths"), (dict(paths=5), "paths"), (dict(paths=16), "paths"),
    (dict(min_directions=0), "min_directions"), (dict(min_directions=9), "min_directions"), (dict(paths=4, min_directions=5), "min_directions"),
    (dict(max_distance=-1), "max_distance"), (dict(max_distance=32768), "max_distance"),
    (dict(wrap_x=2), "wrap_x"), (dict(wrap_x=-1), "wrap_x"),
    (dict(min_disparity=-2048), "min_disparity"), (dict(min_disparity=2032), "min_disparity"),
    (dict(w=32768, disp_stride=32768, out_stride=32768), "width"), (dict(h=32768), "height"),
])
def test_fill_refuses_bad_arguments_before_any_device(args, word):
    rc, text = _call_fill(**args)
    assert rc == -1 and word in text, text
    if "out" not in args and "out_stride" not in args:                        # the stages entry point has no `out`
        rc, text = _call_fill(stages=True, **args)
        assert rc == -1 and word in text, text


def test_fill_accepts_the_edges_of_its_ranges_and_empty_images():
    for fields in (dict(min_disparity=-2047), dict(min_disparity=2031), dict(max_distance=32767), dict(min_directions=8), dict(paths=4, min_directions=4),
                   dict(wrap_x=1), dict(rule=0)):
        assert _call_fill(w=0, **fields)[0] == 0, fields
        assert _call_fill(h=0, stages=True, **fields)[0] == 0, fields


def test_python_layer_raises_the_same_refusals():
    d = np.zeros((4, 6), dtype=np.int16)
    with pytest.raises(lib.TscmError) as e:
        stereo.fill(d, paths=6)
    assert e.value.code == -1 and "paths" in str(e.value)
    with pytest.raises(lib.TscmError) as e:
        stereo.fill_stages(d, max_distance=40000)
    assert e.value.code == -1 and "max_distance" in str(e.value)
    with pytest.raises(TypeError):
        stereo.fill(d, no_such_parameter=1)
    with pytest.raises(ValueError):
        stereo.fill(d.astype(np.int32))
    with pytest.raises(ValueError):
        stereo.fill(d, out=np.zeros((4, 7), dtype=np.int16))
    with pytest.raises(TypeError):                                            # pair_depth: min_disparity is the matcher's
        stereo.pair_depth(np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8), np.ones(9), np.eye(3, 4), np.ones(9), np.eye(3, 4),
                          matcher=lambda a, b, **p: np.zeros(a.shape, np.int16), fill=dict(min_disparity=1), width=16, height=8)
    with pytest.raises(TypeError):                                            # the sweep chains: it is 0
        sweep.rig_depth([np.zeros((8, 8), np.uint8)], None, None, fill=dict(min_disparity=0))
    with pytest.raises(TypeError):
        sweep.rig_panorama([np.zeros((8, 8), np.uint8)], None, None, fill=dict(min_disparity=0))


def test_out_of_range_device_is_no_device_and_arguments_come_first():
    """What tests/test_device_selection.py asks of every entry point with a device index."""
    L = lib.lib()
    sp = C.POINTER(C.c_short)
    d, o = np.zeros((10, 24), dtype=np.int16), np.zeros((10, 24), dtype=np.int16)
    p = stereo.fill_params()
    n = L.tscm_device_count()
    for dv in (n, -1):
        assert L.tscm_stereo_fill(d.ctypes.data_as(sp), 24, 10, 24, C.byref(p), dv, o.ctypes.data_as(sp), 24, None, None) == -2
        assert L.tscm_last_error()
        assert L.tscm_stereo_fill_stages(d.ctypes.data_as(sp), 24, 10, 24, C.byref(p), dv, None, None) == -2
    assert L.tscm_stereo_fill(None, 24, 10, 24, C.byref(p), n, o.ctypes.data_as(sp), 24, None, None) == -1
    assert L.tscm_stereo_fill_stages(d.ctypes.data_as(sp), 24, 10, 23, C.byref(p), n, None, None) == -1
