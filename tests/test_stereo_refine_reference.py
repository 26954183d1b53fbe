"""The definition of tscm_stereo_refine (include/tscm/tscm.h) on the host: the two restatements of tests/stereo_refine_ref.py
against each other, the consequences the header states (the masked median of tscm_stereo_filter with equal weights, fixed
points, passes, the seam), the step-edge scene that shows what the guide buys, and what the library answers without a
device: the weight table, the defaults and every refusal."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import stereo_filter_ref as FR
from tests import stereo_refine_ref as R
from tscm_calib_amd import lib, stereo, sweep


def random_map(rng, h, w, holes=0.3, min_disparity=0, lo=-40, hi=200):
    d = (16 * rng.integers(lo, hi, size=(h, w)) + rng.integers(0, 16, size=(h, w))).astype(np.int16)
    d[d == R.invalid_value(min_disparity)] += 1
    d[rng.random((h, w)) < holes] = R.invalid_value(min_disparity)
    return d


def random_guide(rng, h, w):
    return rng.integers(0, 256, size=(h, w)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the two restatements
@pytest.mark.parametrize("seed", range(6))
def test_sort_equals_candidate_scan(seed):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(1, 12)), int(rng.integers(1, 14))
    d = random_map(rng, h, w, holes=(0.3, 0.9, 0.0)[seed % 3], min_disparity=(0, -5)[seed % 2], lo=-3, hi=4)     # few levels: many ties
    g = (random_guide(rng, h, w) // 32 * 32).astype(np.uint8)
    lut = (R.range_weights(20.0), None, np.where(np.arange(256) < 40, 7, 0).astype(np.uint8))[seed % 3]
    for radius in (1, 2, 3):
        for wrap in (0, 1):
            for fill in (0, 1):
                p = dict(min_disparity=(0, -5)[seed % 2], radius=radius, wrap_x=wrap, fill_invalid=fill)
                a, b = R.pass_literal(d, g, lut, **p), R.pass_vectorised(d, g, lut, **p)
                for x, y, name in zip(a, b, ("out", "weight_sum", "count")):
                    assert np.array_equal(x, y), (name, p)
    assert np.array_equal(R.refine_literal(d, g, lut, radius=2, iterations=3), R.refine(d, g, lut, radius=2, iterations=3))


# ------------------------------------------------------------------------------------------------ consequences
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("min_disparity", [0, -5])
def test_equal_weights_are_the_masked_median_of_the_filter(radius, min_disparity):
    rng = np.random.default_rng(10 * radius + min_disparity + 5)
    d = random_map(rng, 23, 31, min_disparity=min_disparity)
    g = random_guide(rng, 23, 31)
    want = FR.masked_median(d, min_disparity, 2 * radius + 1)
    for lut in (None, np.full(256, 1, np.uint8), np.full(256, 200, np.uint8)):
        assert np.array_equal(R.refine(d, g, lut, radius=radius, min_disparity=min_disparity), want)
        assert np.array_equal(R.refine_literal(d, g, lut, radius=radius, min_disparity=min_disparity), want)


def test_a_delta_table_keeps_two_regions_apart():
    """Table 255, 0, 0, ...: only pixels of exactly the centre's grey value carry weight, so on a two-level guide no value
    crosses from one region into the other."""
    rng = np.random.default_rng(3)
    h, w = 20, 30
    g = np.where(np.arange(w)[None, :] + (np.arange(h)[:, None] % 3) < 14, 60, 180).astype(np.uint8) + np.zeros((h, w), np.uint8)
    d = np.where(g == 60, 16 * rng.integers(10, 20, size=(h, w)), 16 * rng.integers(100, 110, size=(h, w))).astype(np.int16)
    d[rng.random((h, w)) < 0.2] = -16
    for fill in (0, 1):
        out = R.refine(d, g, R.range_weights(0.0), radius=3, fill_invalid=fill)
        for level, other in ((60, 180), (180, 60)):
            mine = set(d[(g == level) & (d != -16)].tolist()) | {-16}
            assert set(out[g == level].tolist()) <= mine
            assert not set(out[g == level].tolist()) & (set(d[(g == other) & (d != -16)].tolist()) - mine)


def test_a_zero_weight_sum_keeps_the_input():
    rng = np.random.default_rng(4)
    d, g = random_map(rng, 9, 11), random_guide(rng, 9, 11)
    lut = np.zeros(256, np.uint8)
    for fill in (0, 1):
        out, wsum, count = R.pass_vectorised(d, g, lut, radius=2, fill_invalid=fill)
        assert np.array_equal(out, d) and not wsum.any() and count.any()


def test_a_constant_map_is_a_fixed_point():
    rng = np.random.default_rng(5)
    g = random_guide(rng, 8, 9)
    for value in (16 * 7 + 3, -32768, 32767):
        d = np.full((8, 9), value, dtype=np.int16)
        for lut in (None, R.range_weights(4.0), R.range_weights(0.0)):
            assert np.array_equal(R.refine(d, g, lut, radius=3, iterations=2, wrap_x=1), d)


def test_iterations_are_single_passes_one_after_the_other():
    rng = np.random.default_rng(6)
    d, g, lut = random_map(rng, 12, 17), random_guide(rng, 12, 17), R.range_weights(30.0)
    step = d
    for n in (1, 2, 3):
        step = R.refine(step, g, lut, radius=2, fill_invalid=1)
        assert np.array_equal(R.refine(d, g, lut, radius=2, fill_invalid=1, iterations=n), step)
    assert not np.array_equal(step, R.refine(d, g, lut, radius=2, fill_invalid=1))


def test_wrap_x_commutes_with_a_roll_along_x():
    rng = np.random.default_rng(7)
    d, g, lut = random_map(rng, 10, 19), random_guide(rng, 10, 19), R.range_weights(25.0)
    for shift in (1, 7, 18):
        a = R.refine(np.roll(d, shift, axis=1), np.roll(g, shift, axis=1), lut, radius=3, wrap_x=1, fill_invalid=1)
        assert np.array_equal(a, np.roll(R.refine(d, g, lut, radius=3, wrap_x=1, fill_invalid=1), shift, axis=1))
    assert not np.array_equal(R.refine(d, g, lut, radius=3, wrap_x=1, fill_invalid=1), R.refine(d, g, lut, radius=3, wrap_x=0, fill_invalid=1))


@pytest.mark.parametrize("w", [1, 3])
def test_a_window_wider_than_the_map_counts_once_per_offset(w):
    h = 4
    d = (16 * np.arange(1, h * w + 1)).reshape(h, w).astype(np.int16)
    g = np.zeros((h, w), np.uint8)
    for f in (R.pass_literal, R.pass_vectorised):
        out, wsum, count = f(d, g, None, radius=2, wrap_x=1)
        rows = np.array([min(y + 2, h - 1) - max(y - 2, 0) + 1 for y in range(h)])
        assert np.array_equal(count, np.repeat(5 * rows[:, None], w, axis=1))           # 5 offsets per row, whatever the width
        assert np.array_equal(wsum, 255 * count.astype(np.int32))
    if w == 3:            # row 0 sees rows 0..2: columns x-2 .. x+2 name x+1, x+2 twice each (mod 3) and x once
        x = 0
        values = sorted([int(d[y, (x + dx) % 3]) for y in range(3) for dx in range(-2, 3)])
        assert out[0, x] == values[(len(values) - 1) >> 1]


def test_the_ends_of_int16_order_as_integers():
    d = np.array([[-32768, 32767, -32768, 32767, 0]], dtype=np.int16)
    g = np.zeros((1, 5), np.uint8)
    for f in (R.refine_literal, R.refine):
        assert f(d, g, None, radius=1).tolist() == [[-32768, -32768, 32767, 0, 0]]
        assert f(d, g, None, radius=2).tolist() == [[-32768, -32768, 0, 0, 0]]


# ------------------------------------------------------------------------------------------------ what the guide buys
def step_edge_scene(seed=0, h=32, w=48):
    """A foreground / background step whose position in the map is jittered by up to +-3 px per row around the edge of the
    guide, 10 % outliers, 10 % holes; the guide has two grey levels 120 apart with +-6 noise."""
    rng = np.random.default_rng(seed)
    edge = w // 2
    truth = np.where(np.arange(w)[None, :] < edge, 16 * 40, 16 * 10) + np.zeros((h, 1), np.int64)
    g = (np.where(np.arange(w)[None, :] < edge, 190, 70) + rng.integers(-6, 7, size=(h, w))).astype(np.uint8)
    jitter = rng.integers(-3, 4, size=h)
    d = np.where(np.arange(w)[None, :] < edge + jitter[:, None], 16 * 40, 16 * 10).astype(np.int16)
    outlier = rng.random((h, w)) < 0.10
    d[outlier] = (16 * rng.integers(0, 64, size=int(outlier.sum()))).astype(np.int16)
    d[rng.random((h, w)) < 0.10] = -16
    return d, g, truth.astype(np.int16)


def wrong(d, truth):
    return int(((d != -16) & (d != truth)).sum())


def test_on_a_step_edge_the_guided_median_beats_the_unguided_one_which_beats_the_input():
    d, g, truth = step_edge_scene()
    guided = R.refine(d, g, R.range_weights(10.0), radius=3)
    unguided = R.refine(d, g, None, radius=3)
    print("wrong valid pixels: input %d, unguided %d, guided %d" % (wrong(d, truth), wrong(unguided, truth), wrong(guided, truth)))
    assert wrong(guided, truth) < wrong(unguided, truth) < wrong(d, truth)
    assert np.array_equal(guided == -16, d == -16)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_new_symbols_are_exported():
    L = lib.lib()
    for name in ("tscm_stereo_refine_default_params", "tscm_stereo_refine_weights", "tscm_stereo_refine", "tscm_stereo_refine_stages"):
        assert name in lib.EXPORTS
        assert hasattr(L, name)
    assert L.tscm_abi_version() == 6


def test_refine_default_params():
    p = stereo.refine_params()
    names = ("min_disparity", "radius", "iterations", "fill_invalid", "wrap_x")
    assert p.struct_size == C.sizeof(lib.CStereoRefineParams) == 24
    assert tuple(getattr(p, k) for k in names) == (0, 3, 1, 0, 0) == tuple(R.DEFAULTS[k] for k in names)
    assert stereo.refine_params(radius=7, wrap_x=1).radius == 7


@pytest.mark.parametrize("sigma", [0.5, 4.0, 10.0, 50.0, math.inf])
def test_the_weight_table_follows_the_formula(sigma):
    t = stereo.range_weights(sigma)
    assert t.dtype == np.uint8 and t.shape == (256,) and t[0] == 255
    assert np.all(np.diff(t.astype(np.int64)) <= 0)
    assert np.max(np.abs(t.astype(np.int64) - R.range_weights(sigma).astype(np.int64))) <= 1          # a last ulp of exp may move a rounding
    if math.isinf(sigma):
        assert np.all(t == 255)


@pytest.mark.parametrize("sigma", [0.0, -1.0, -math.inf, math.nan])
def test_a_sigma_that_is_not_positive_gives_the_delta_table(sigma):
    want = [255] + [0] * 255
    assert stereo.range_weights(sigma).tolist() == want == R.range_weights(sigma).tolist()


def _call_refine(disp=True, guide=True, w=24, h=10, disp_stride=24, guide_stride=24, params="default", out=True, out_stride=24, stages=False, **fields):
    sp, ub = C.POINTER(C.c_short), C.POINTER(C.c_ubyte)
    a, g, o = np.zeros((10, 24), dtype=np.int16), np.zeros((10, 24), dtype=np.uint8), np.zeros((10, 24), dtype=np.int16)
    p = stereo.refine_params() if params == "default" else params
    for k, v in fields.items():
        setattr(p, k, v)
    pp = None if p is None else C.byref(p)
    L = lib.lib()
    da, ga = a.ctypes.data_as(sp) if disp else None, g.ctypes.data_as(ub) if guide else None
    if stages:
        rc = L.tscm_stereo_refine_stages(da, w, h, disp_stride, ga, guide_stride, None, pp, 0, None, None, None)
    else:
        rc = L.tscm_stereo_refine(da, w, h, disp_stride, ga, guide_stride, None, pp, 0, o.ctypes.data_as(sp) if out else None, out_stride, None)
    return rc, L.tscm_last_error().decode()


@pytest.mark.parametrize("args,word", [
    (dict(disp=False), "disparity"), (dict(guide=False), "guide"), (dict(params=None), "params"), (dict(out=False), "out"),
    (dict(disp_stride=23), "disp_stride"), (dict(guide_stride=23), "guide_stride"), (dict(out_stride=23), "out_stride"),
    (dict(struct_size=20), "struct_size"), (dict(struct_size=28), "struct_size"),
    (dict(radius=0), "radius"), (dict(radius=8), "radius"), (dict(radius=-1), "radius"),
    (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"),
    (dict(fill_invalid=2), "fill_invalid"), (dict(fill_invalid=-1), "fill_invalid"),
    (dict(wrap_x=2), "wrap_x"), (dict(wrap_x=-1), "wrap_x"),
    (dict(min_disparity=-2048), "min_disparity"), (dict(min_disparity=2032), "min_disparity"),
    (dict(w=65536, h=32768, disp_stride=65536, guide_stride=65536, out_stride=65536), "INT_MAX"),
])
def test_refine_refuses_bad_arguments_before_any_device(args, word):
    rc, text = _call_refine(**args)
    assert rc == -1 and word in text, text
    if "out" not in args and "out_stride" not in args:                        # the stages entry point has no `out`
        rc, text = _call_refine(stages=True, **args)
        assert rc == -1 and word in text, text


def test_refine_accepts_the_edges_of_its_ranges_and_empty_maps():
    for fields in (dict(min_disparity=-2047), dict(min_disparity=2031), dict(radius=1), dict(radius=7), dict(iterations=8), dict(fill_invalid=1), dict(wrap_x=1)):
        assert _call_refine(w=0, **fields)[0] == 0, fields
        assert _call_refine(h=0, stages=True, **fields)[0] == 0, fields
    d, g = np.zeros((5, 0), np.int16), np.zeros((5, 0), np.uint8)
    assert stereo.refine(d, g).shape == (5, 0) and stereo.refine_stages(d, g)["count"].shape == (5, 0)


def test_python_layer_raises_the_same_refusals():
    d, g = np.zeros((4, 6), dtype=np.int16), np.zeros((4, 6), dtype=np.uint8)
    with pytest.raises(lib.TscmError) as e:
        stereo.refine(d, g, radius=9)
    assert e.value.code == -1 and "radius" in str(e.value)
    with pytest.raises(lib.TscmError) as e:
        stereo.refine_stages(d, g, iterations=0)
    assert e.value.code == -1 and "iterations" in str(e.value)
    with pytest.raises(TypeError):
        stereo.refine(d, g, no_such_parameter=1)
    with pytest.raises(TypeError):                                            # one table, named one way
        stereo.refine(d, g, sigma=4.0, weights=np.full(256, 255, np.uint8))
    with pytest.raises(ValueError):
        stereo.refine(d, g, weights=np.zeros(255, np.uint8))
    with pytest.raises(ValueError):
        stereo.refine(d, g[:, :5])
    with pytest.raises(ValueError):
        stereo.refine(d.astype(np.int32), g)
    with pytest.raises(ValueError):
        stereo.refine(d, g, out=np.zeros((4, 7), dtype=np.int16))
    with pytest.raises(TypeError):                                            # pair_depth: min_disparity is the matcher's
        stereo.pair_depth(np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8), np.ones(9), np.eye(3, 4), np.ones(9), np.eye(3, 4),
                          matcher=lambda a, b, **p: np.zeros(a.shape, np.int16), refine=dict(min_disparity=1), width=16, height=8)
    with pytest.raises(TypeError):                                            # the sweep chains: it is 0
        sweep.rig_depth([np.zeros((8, 8), np.uint8)], None, None, refine=dict(min_disparity=0))
    with pytest.raises(TypeError):
        sweep.rig_panorama([np.zeros((8, 8), np.uint8)], None, None, refine=dict(min_disparity=0))


def test_out_of_range_device_is_no_device_and_arguments_come_first():
    """What tests/test_device_selection.py asks of every entry point with a device index."""
    L = lib.lib()
    sp, ub = C.POINTER(C.c_short), C.POINTER(C.c_ubyte)
    d, g, o = np.zeros((10, 24), dtype=np.int16), np.zeros((10, 24), dtype=np.uint8), np.zeros((10, 24), dtype=np.int16)
    p = stereo.refine_params()
    n = L.tscm_device_count()
    for dv in (n, -1):
        assert L.tscm_stereo_refine(d.ctypes.data_as(sp), 24, 10, 24, g.ctypes.data_as(ub), 24, None, C.byref(p), dv, o.ctypes.data_as(sp), 24, None) == -2
        assert L.tscm_last_error()
        assert L.tscm_stereo_refine_stages(d.ctypes.data_as(sp), 24, 10, 24, g.ctypes.data_as(ub), 24, None, C.byref(p), dv, None, None, None) == -2
    assert L.tscm_stereo_refine(None, 24, 10, 24, g.ctypes.data_as(ub), 24, None, C.byref(p), n, o.ctypes.data_as(sp), 24, None) == -1
    assert L.tscm_stereo_refine_stages(d.ctypes.data_as(sp), 24, 10, 24, g.ctypes.data_as(ub), 23, None, C.byref(p), n, None, None, None) == -1
