"""CPU tests of the disparity post-filter's definition (include/tscm/tscm.h, tscm_stereo_filter*): the host restatement
tests/stereo_filter_ref.py on hand-worked maps, its two independently written component labellings against each other,
and the argument refusals of the C ABI, which return before a device is touched."""
import ctypes as C

import numpy as np
import pytest

from tscm_calib_amd import lib, stereo
from tests import stereo_filter_ref as F

INV = -16                                                                     # min_disparity = 0


def _map(rows):
    return np.array(rows, dtype=np.int16)


# ------------------------------------------------------------------------------------------------ components by hand
def test_step_of_exactly_the_range_merges_and_one_more_does_not():
    # range 2: the threshold is 32.  Left block 100, right block 132 (step 32) or 133 (step 33)
    for right, merged in ((132, True), (133, False)):
        d = _map([[100, 100, right, right], [100, 100, right, right]])
        for f in (F.components, F.components_bfs):
            label, size = f(d, 0, 2)
            if merged:
                assert np.all(label == 0) and np.all(size == 8)
            else:
                assert label.tolist() == [[0, 0, 2, 2], [0, 0, 2, 2]] and np.all(size == 4)


def test_a_ramp_merges_end_to_end():
    d = _map([[16 * k for k in range(1, 7)]])                                 # steps of 16 with range 1: ends 80 apart
    for f in (F.components, F.components_bfs):
        label, size = f(d, 0, 1)
        assert np.all(label == 0) and np.all(size == 6)
    label, size = F.components(d, 0, 0)                                       # range 0: only equal values join
    assert label.tolist() == [[0, 1, 2, 3, 4, 5]] and np.all(size == 1)


def test_component_of_exactly_the_window_goes_and_one_more_stays():
    d = _map([[50, 50, 50, INV, 90, 90],
              [INV, INV, INV, INV, 90, 90],
              [INV, INV, INV, INV, INV, INV]])
    st = F.stages(d, speckle_window_size=3, speckle_range=0)
    assert st["size"].tolist() == [[3, 3, 3, 0, 4, 4], [0, 0, 0, 0, 4, 4], [0] * 6]
    assert st["label"].tolist() == [[0, 0, 0, -1, 4, 4], [-1, -1, -1, -1, 4, 4], [-1] * 6]
    assert st["despeckled"].tolist() == [[INV, INV, INV, INV, 90, 90], [INV, INV, INV, INV, 90, 90], [INV] * 6]
    assert np.array_equal(st["out"], st["despeckled"])                        # median 0
    # the same map with window 4 loses both, with window 2 keeps both, with window 0 the rule is off
    assert np.all(F.filter(d, speckle_window_size=4, speckle_range=0) == INV)
    assert np.array_equal(F.filter(d, speckle_window_size=2, speckle_range=0), d)
    assert np.array_equal(F.filter(d, speckle_window_size=0, speckle_range=0), d)


def test_diagonal_contact_is_not_connected():
    d = _map([[40, INV, INV],
              [INV, 40, INV],
              [INV, INV, 40]])
    for f in (F.components, F.components_bfs):
        label, size = f(d, 0, 2)
        assert label.tolist() == [[0, -1, -1], [-1, 4, -1], [-1, -1, 8]]
        assert size.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    # and two valid neighbours that differ by more than the range do not connect through each other
    d = _map([[40, 200], [200, 40]])
    assert F.components(d, 0, 2)[0].tolist() == [[0, 1], [2, 3]]


def test_negative_min_disparity_moves_the_invalid_value():
    assert F.invalid_value(-5) == -96
    d = _map([[-96, -16, -16], [-96, -96, -16], [-16, -96, -96]])
    st = F.stages(d, min_disparity=-5, speckle_window_size=1, speckle_range=2)
    assert st["label"].tolist() == [[-1, 1, 1], [-1, -1, 1], [6, -1, -1]]
    assert st["size"].tolist() == [[0, 3, 3], [0, 0, 3], [1, 0, 0]]
    # -16 is a valid value here: the component of three stays, the single pixel goes to -96
    assert st["out"].tolist() == [[-96, -16, -16], [-96, -96, -16], [-96, -96, -96]]
    # with min_disparity 0 the same numbers read the other way round: -16 is the invalid value and -96 a disparity
    st0 = F.stages(d, min_disparity=0, speckle_window_size=0)
    assert st0["label"].tolist() == [[0, -1, -1], [0, 0, -1], [-1, 0, 0]] and int(st0["size"].max()) == 5


# ------------------------------------------------------------------------------------------------ masked median by hand
def test_masked_median_counts_only_valid_entries():
    # centre (1, 1) with 1, 2 and 4 valid entries in its 3 x 3 window
    one = _map([[INV, INV, INV], [INV, 70, INV], [INV, INV, INV]])
    assert F.masked_median(one, 0, 3)[1, 1] == 70
    two = _map([[INV, INV, INV], [INV, 70, 30], [INV, INV, INV]])
    out = F.masked_median(two, 0, 3)
    assert out[1, 1] == 30 and out[1, 2] == 30                                # n = 2: index 0, the lower element
    four = _map([[90, INV, INV], [INV, 70, 30], [INV, 10, INV]])
    assert F.masked_median(four, 0, 3)[1, 1] == 30                            # sorted 10 30 70 90, index 1
    full = _map([[9, 8, 7], [6, 5, 4], [3, 2, 1]])
    assert F.masked_median(full, 0, 3)[1, 1] == 5
    assert F.masked_median(full, 0, 5)[1, 1] == 5                             # the 5 x 5 window cut to the image: the same 9


def test_masked_median_at_a_corner_uses_the_window_inside_the_image():
    d = _map([[80, 20, 1, 1], [40, 60, 1, 1], [1, 1, 1, 1]])
    # corner (0, 0), 3 x 3: the 4 pixels 80 20 40 60 -> sorted 20 40 60 80, index 1; replicated borders would give 60 or 80
    assert F.masked_median(d, 0, 3)[0, 0] == 40
    # 5 x 5 at the corner covers rows 0..2, columns 0..2: 80 20 1 40 60 1 1 1 1 -> sorted 1 1 1 1 1 20 ..., index 4
    assert F.masked_median(d, 0, 5)[0, 0] == 1
    # 5 x 5 at (1, 1) covers the whole image: five more ones, 12 entries, index 5
    assert F.masked_median(d, 0, 5)[1, 1] == 1
    # left edge (1, 0), 3 x 3: rows 0..2, columns 0..1: 80 20 40 60 1 1 -> sorted 1 1 20 40 60 80, index 2
    assert F.masked_median(d, 0, 3)[1, 0] == 20
    # bottom right corner, 3 x 3: all ones
    assert F.masked_median(d, 0, 3)[2, 3] == 1


def test_invalid_centre_stays_invalid():
    d = _map([[50, 50, 50], [50, INV, 50], [50, 50, 50]])
    for m in (3, 5):
        out = F.masked_median(d, 0, m)
        assert out[1, 1] == INV and np.all(np.delete(out.ravel(), 4) == 50)
    # the median sees the map after the speckle rule: the removed pixel no longer counts in its neighbour's window
    d = _map([[10, INV, 30, 30, 30, 30]])
    st = F.stages(d, speckle_window_size=1, speckle_range=0, median=3)
    assert st["despeckled"].tolist() == [[INV, INV, 30, 30, 30, 30]] and st["out"].tolist() == [[INV, INV, 30, 30, 30, 30]]


def test_identity_with_both_stages_off():
    rng = np.random.default_rng(5)
    d = rng.integers(-200, 2000, (11, 13)).astype(np.int16)
    d[rng.random(d.shape) < 0.3] = INV
    assert np.array_equal(F.filter(d, speckle_window_size=0, median=0), d)
    assert F.filter(d, speckle_window_size=0, median=0) is not d


# ------------------------------------------------------------------------------------------------ two labellings
def _random_map(rng, w, h, invalid=INV, share=0.3, levels=(160, 176, 400)):
    d = rng.choice(np.array(levels, dtype=np.int16), size=(h, w))
    d[rng.random((h, w)) < share] = invalid
    return d


@pytest.mark.parametrize("seed", range(20))
def test_union_find_equals_flood_fill(seed):
    rng = np.random.default_rng(1000 + seed)
    d = _random_map(rng, 40, 24)
    speckle_range = seed % 3                                                  # 0: equal values only; 1: 160 ~ 176; 2: the same
    la, sa = F.components(d, 0, speckle_range)
    lb, sb = F.components_bfs(d, 0, speckle_range)
    assert la.dtype == lb.dtype == np.int32 and np.array_equal(la, lb) and np.array_equal(sa, sb)
    valid = d != INV
    assert np.all(la[~valid] == -1) and np.all(sa[~valid] == 0)
    assert np.all(la[valid] <= np.arange(d.size).reshape(d.shape)[valid])     # a label is the smallest index of its component
    roots = np.unique(la[valid])
    assert sa.ravel()[roots].sum() == valid.sum()                             # the sizes partition the valid pixels
    if seed == 1:
        assert len(roots) > 20 and sa.max() > 20                              # small and large components both occur


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def _call_filter(disp=True, w=24, h=10, disp_stride=24, params="default", out=True, out_stride=24, stages=False, **fields):
    sp, ip = C.POINTER(C.c_short), C.POINTER(C.c_int)
    a = np.zeros((10, 24), dtype=np.int16)
    o = np.zeros((10, 24), dtype=np.int16)
    p = stereo.filter_params() if params == "default" else params
    for k, v in fields.items():
        setattr(p, k, v)
    pp = None if p is None else C.byref(p)
    L = lib.lib()
    if stages:
        rc = L.tscm_stereo_filter_stages(a.ctypes.data_as(sp) if disp else None, w, h, disp_stride, pp, 0, None, None, None)
    else:
        rc = L.tscm_stereo_filter(a.ctypes.data_as(sp) if disp else None, w, h, disp_stride, pp, 0, o.ctypes.data_as(sp) if out else None, out_stride, None)
    return rc, L.tscm_last_error().decode()


def test_filter_default_params():
    p = stereo.filter_params()
    assert p.struct_size == C.sizeof(lib.CStereoFilterParams) == 20
    assert (p.min_disparity, p.speckle_window_size, p.speckle_range, p.median) == (0, 100, 2, 0)
    assert (p.min_disparity, p.speckle_window_size, p.speckle_range, p.median) == tuple(
        F.DEFAULTS[k] for k in ("min_disparity", "speckle_window_size", "speckle_range", "median"))


@pytest.mark.parametrize("args,word", [
    (dict(disp=False), "disparity"), (dict(params=None), "params"), (dict(out=False), "out"),
    (dict(disp_stride=23), "disp_stride"), (dict(out_stride=23), "out_stride"),
    (dict(struct_size=16), "struct_size"), (dict(struct_size=24), "struct_size"),
    (dict(speckle_window_size=-1), "speckle_window_size"),
    (dict(speckle_range=-1), "speckle_range"), (dict(speckle_range=256), "speckle_range"),
    (dict(median=1), "median"), (dict(median=4), "median"), (dict(median=7), "median"), (dict(median=-3), "median"),
    (dict(min_disparity=-2048), "min_disparity"), (dict(min_disparity=2032), "min_disparity"),
    (dict(w=65536, h=32768, disp_stride=65536, out_stride=65536), "width * height"),
])
def test_filter_refuses_bad_arguments_before_any_device(args, word):
    rc, text = _call_filter(**args)
    assert rc == -1 and word in text, text
    if "out" not in args and "out_stride" not in args:                        # the stages entry point has no `out`
        rc, text = _call_filter(stages=True, **args)
        assert rc == -1 and word in text, text


def test_filter_accepts_the_edges_of_its_ranges_and_empty_images():
    # what the matcher accepts at its smallest num_disparities: -2047 .. 2031; an empty image needs no device
    for fields in (dict(min_disparity=-2047), dict(min_disparity=2031), dict(speckle_range=255), dict(speckle_range=0), dict(median=5),
                   dict(speckle_window_size=0)):
        assert _call_filter(w=0, **fields)[0] == 0, fields
        assert _call_filter(h=0, stages=True, **fields)[0] == 0, fields


def test_python_layer_raises_the_same_refusals():
    d = np.zeros((4, 6), dtype=np.int16)
    with pytest.raises(lib.TscmError) as e:
        stereo.filter(d, median=4)
    assert e.value.code == -1 and "median" in str(e.value)
    with pytest.raises(lib.TscmError) as e:
        stereo.filter_stages(d, speckle_range=300)
    assert e.value.code == -1 and "speckle_range" in str(e.value)
    with pytest.raises(TypeError):
        stereo.filter(d, no_such_parameter=1)
    with pytest.raises(ValueError):
        stereo.filter(d.astype(np.int32))
    with pytest.raises(ValueError):
        stereo.filter(d, out=np.zeros((4, 7), dtype=np.int16))
    with pytest.raises(TypeError):                                            # pair_depth: min_disparity is the matcher's
        stereo.pair_depth(np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8), np.ones(9), np.eye(3, 4), np.ones(9), np.eye(3, 4),
                          matcher=lambda a, b, **p: np.zeros(a.shape, np.int16), post=dict(min_disparity=1), width=16, height=8)


def test_out_of_range_device_is_no_device_and_arguments_come_first():
    """What tests/test_device_selection.py asks of every entry point with a device index."""
    L = lib.lib()
    sp = C.POINTER(C.c_short)
    d, o = np.zeros((10, 24), dtype=np.int16), np.zeros((10, 24), dtype=np.int16)
    p = stereo.filter_params()
    n = L.tscm_device_count()
    for dv in (n, -1):
        assert L.tscm_stereo_filter(d.ctypes.data_as(sp), 24, 10, 24, C.byref(p), dv, o.ctypes.data_as(sp), 24, None) == -2
        assert L.tscm_last_error()
        assert L.tscm_stereo_filter_stages(d.ctypes.data_as(sp), 24, 10, 24, C.byref(p), dv, None, None, None) == -2
    assert L.tscm_stereo_filter(None, 24, 10, 24, C.byref(p), n, o.ctypes.data_as(sp), 24, None) == -1
    assert L.tscm_stereo_filter_stages(d.ctypes.data_as(sp), 24, 10, 23, C.byref(p), n, None, None, None) == -1
