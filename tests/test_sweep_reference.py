"""CPU tests of the sphere sweep: the properties of the definition on the host restatement tests/sweep_ref.py (pair cost and
its rounding, the meaning of C == 64, the rule of the uncovered winner, the wrap of the census window, the points, the centre
term of the tables), and the refusals and defaults of the C ABI, which are decided before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from tests import maps_proj_ref as mref
from tests import stereo_ref
from tests import sweep_ref as R
from tscm_calib_amd import lib, maps, sweep, synth


# ------------------------------------------------------------------------------------------------ cost, winner
def _agreeing_pair(z_star, D=16, ph=12, pw=20):
    """Two cameras showing the same 48 x 40 noise image; camera 1's tables are camera 0's shifted by 3 (z - z_star) px."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 48)).astype(np.uint8)
    i, j = np.meshgrid(np.arange(ph), np.arange(pw), indexing="ij")
    mx = np.zeros((2, D, ph, pw), np.float32)
    my = np.zeros((2, D, ph, pw), np.float32)
    for z in range(D):
        mx[0, z], my[0, z] = j + 10.25, i + 9.5
        mx[1, z], my[1, z] = j + 10.25 + 3 * (z - z_star), i + 9.5
    return [img, img], mx, my


@pytest.mark.parametrize("z_star", [0, 5, 15])
def test_cameras_that_agree_at_one_hypothesis_win_there(z_star):
    images, mx, my = _agreeing_pair(z_star)
    st = R.stages(images, None, mx, my, wrap_x=False, uniqueness_ratio=10)
    assert np.all(st["cost"][..., z_star] == 0)
    others = np.delete(st["cost"], z_star, axis=-1)
    assert np.median(others[others < 64]) > 20                 # shifted noise: about half of the 62 bits differ
    assert (others == 64).any()                                # the far shifts leave camera 1's image: one camera left
    assert np.all(np.abs(st["index16"].astype(int) - 16 * z_star) <= 8)
    if z_star in (0, 15):                                      # no parabola term at the ends
        assert np.all(st["index16"] == 16 * z_star)


def _codes(*bit_counts):
    return np.array([(1 << b) - 1 for b in bit_counts], dtype=np.uint64)


def test_the_pair_mean_rounds_both_ways():
    """Three cameras: codes with 0, 1, 2 low bits set give distances 1, 2, 1 = 4 -> (4 + 1) / 3 = 1 (4/3 rounds down);
    0, 1, 3 bits give 1, 3, 2 = 6 -> 2 (exact); 0, 2, 3 give 2, 3, 1 = 6; 0, 1, 4 give 1, 4, 3 = 8 -> 3 (8/3 rounds up)."""
    cen = np.stack([_codes(0, 0, 0, 0), _codes(1, 1, 2, 1), _codes(2, 3, 3, 4)]).reshape(3, 1, 1, 4)
    a = np.full((3, 1, 1, 4), 9, np.uint8)
    assert R.cost_volume(cen, a)[0, :, 0].tolist() == [1, 2, 2, 3]
    # two of the three: the third camera's code does not enter
    a[2] = 0
    assert R.cost_volume(cen, a)[0, :, 0].tolist() == [1, 1, 2, 1]


@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_cost_64_means_fewer_than_two_cameras(n):
    rng = np.random.default_rng(n)
    cen = rng.integers(0, 1 << 62, (n, 2, 6, 7), dtype=np.uint64)
    cen[0, 0], cen[1, 0] = 0, (1 << 62) - 1                    # the largest distance a pair can have
    a = rng.integers(0, 3, (n, 2, 6, 7)).astype(np.uint8)      # a third of the entries 0
    a[:, 0, 0, 0] = 0                                          # nobody
    a[:, 0, 0, 1] = 0
    a[n - 1, 0, 0, 1] = 200                                    # one camera
    a[:, 0, 0, 2] = 0
    a[:2, 0, 0, 2] = 1                                         # cameras 0 and 1 alone: 62
    Cv = R.cost_volume(cen, a)
    cnt = np.moveaxis((a > 0).sum(axis=0), 0, -1)
    assert Cv[0, 0, 0] == 64 and Cv[0, 1, 0] == 64 and Cv[0, 2, 0] == 62
    assert np.all(Cv[cnt < 2] == 64) and np.all(Cv[cnt >= 2] <= 62)
    assert (cnt >= 2).any() and (cnt == 1).any()


def test_the_multiply_shift_division_of_the_kernel_is_exact():
    """k_sweep_cost divides by P = 1, 3, ..., 28 with M = ceil(2^16 / P): (x M) >> 16 == x / P for every x it can meet."""
    for cnt in range(2, 9):
        P = cnt * (cnt - 1) // 2
        M = (65536 + P - 1) // P
        x = np.arange(0, 62 * P + (P >> 1) + 1, dtype=np.int64)
        assert np.array_equal((x * M) >> 16, x // P)
        assert int(x[-1]) * M < 2 ** 32


def test_a_winner_nobody_sees_is_invalid():
    """p1 = p2 = 0 and ratio 0: S = paths * C, so a pixel whose every hypothesis has C = 64 wins at index 0 by the matcher's
    rules; the sweep's extra rule makes it invalid."""
    images, mx, my = _agreeing_pair(5)
    mx = mx.copy()
    mx[:, :, :, 7:10] = -1.0                                   # three columns no camera sees, at any hypothesis
    my = my.copy()
    my[:, :, :, 7:10] = -1.0
    st = R.stages(images, None, mx, my, wrap_x=False, uniqueness_ratio=0, p1=0, p2=0, paths=4)
    assert np.all(st["cost"][:, 7:10] == 64)
    assert np.all(stereo_ref.disparity(st["aggregated"], 0, 0, -1)[:, 7:10] == 0)       # without the rule: index 0
    assert np.all(st["index16"][:, 7:10] == R.INVALID)
    assert np.all(st["index16"][:, :7] >= 0) and np.all(st["index16"][:, 10:] >= 0)
    # the rule looks at C(k*), not at the other hypotheses: C = 64 beside a covered winner changes nothing
    S = np.array([[[10, 3, 50, 60]]], dtype=np.uint16)
    Cv = np.array([[[64, 2, 64, 64]]], dtype=np.uint8)
    assert R.index_map(S, Cv, 0)[0, 0] == stereo_ref.disparity(S, 0, 0, -1)[0, 0] != R.INVALID
    Cv[0, 0, 1] = 64
    assert R.index_map(S, Cv, 0)[0, 0] == R.INVALID


def test_wrapped_and_clamped_census_differ_only_at_the_column_ends():
    rng = np.random.default_rng(11)
    plane = rng.integers(0, 256, (9, 21)).astype(np.uint8)
    wrapped, clamped = R.census(plane, True), R.census(plane, False)
    assert wrapped.shape == clamped.shape == plane.shape
    assert np.array_equal(wrapped[:, 4:-4], clamped[:, 4:-4])
    assert not np.array_equal(wrapped[:, :4], clamped[:, :4]) and not np.array_equal(wrapped[:, -4:], clamped[:, -4:])
    # the wrap is a rotation of the columns: rotate by 8, take the clamped census away from the ends, rotate back
    rolled = np.roll(stereo_ref.census(np.roll(plane, 8, axis=1)), -8, axis=1)
    assert np.array_equal(wrapped[:, :4], rolled[:, :4])
    rolled = np.roll(stereo_ref.census(np.roll(plane, -8, axis=1)), 8, axis=1)
    assert np.array_equal(wrapped[:, -4:], rolled[:, -4:])
    # a panorama narrower than the window
    tiny = rng.integers(0, 256, (3, 5)).astype(np.uint8)
    assert R.census(tiny, True).shape == (3, 5)


# ------------------------------------------------------------------------------------------------ points
def _pano_desc(kind=mref.EQUIRECT, w=8, h=4):
    return mref.Desc(synth.CALIB_INTR[0], np.eye(3), w / (2 * np.pi), h / np.pi, w / 2.0, h / 2.0, w, h, kind)


def test_points_interpolate_between_unequal_steps():
    d = _pano_desc()
    inv = np.array([0.0, 0.001, 0.004, 0.005])
    idx = np.array([[16 + 8, 32 + 4, 16 * 3, 16 * 3 + 8, 0, 8, R.INVALID, 16]] * 4, dtype=np.int16)
    P, ok = R.points(idx, d, inv)
    dist = np.linalg.norm(P, axis=-1)
    expect = [0.0025, 0.00425, 0.005, 0.0055]                  # s = D - 1 and beyond: the last step carries on
    assert np.allclose(1.0 / dist[:, :4], np.array(expect)[None], rtol=1e-14)
    assert ok[:, :4].all() and ok[:, 5].all() and ok[:, 7].all()
    assert np.allclose(1.0 / dist[:, 5], 0.0005, rtol=1e-14)
    assert not ok[:, 4].any() and np.isnan(P[:, 4]).all()      # inv = 0: infinity
    assert not ok[:, 6].any() and np.isnan(P[:, 6]).all()      # an invalid pixel
    # the direction is the panorama's ray
    i, j = np.meshgrid(np.arange(4), np.arange(8), indexing="ij")
    r = mref.ray(mref.EQUIRECT, (j - d.cx) / d.fx, (i - d.cy) / d.fy)
    assert np.allclose(P[ok] / dist[ok][:, None], r[ok], atol=1e-15)


# ------------------------------------------------------------------------------------------------ tables
def _rig_descs(kind, w=40, h=20):
    intr, T = synth.CALIB_INTR, synth.CALIB_TWC
    fx = w / (2 * np.pi)
    fy = h / np.pi if kind in (mref.EQUIRECT, mref.LONGLAT) else fx
    return [mref.Desc(intr[k], T[k][:, :3].T, fx, fy, w / 2.0, h / 2.0, w, h, kind, check_w2=1) for k in range(4)], T[:, :, 3]


@pytest.mark.parametrize("kind", [mref.LONGLAT, mref.CYLINDRICAL, mref.STEREOGRAPHIC, mref.EQUIRECT])
def test_tables_at_infinity_are_the_plain_tables(kind):
    descs, centers = _rig_descs(kind)
    mx, my, _ = R.build_sweep_maps_ref(descs, centers, [0.0, 1e-3])
    for k, d in enumerate(descs):
        rx, ry, _ = mref.build_map_ref(d)
        assert np.array_equal(mx[k, 0].view(np.uint32), rx.view(np.uint32)) and np.array_equal(my[k, 0].view(np.uint32), ry.view(np.uint32))
    assert not np.array_equal(mx[1, 1], mx[1, 0])              # camera 1 is off the origin: the centre term moves its table


@pytest.mark.parametrize("kind", [mref.LONGLAT, mref.CYLINDRICAL, mref.STEREOGRAPHIC, mref.EQUIRECT])
def test_a_table_entry_is_the_projection_of_the_point(kind):
    descs, centers = _rig_descs(kind)
    inv = np.array([1.0 / 8000, 1.0 / 2000, 1.0 / 700, 1.0 / 400])
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(200):
        k, z, i, j = int(rng.integers(0, 4)), int(rng.integers(0, 4)), int(rng.integers(0, 20)), int(rng.integers(0, 40))
        d = descs[k]
        u, v, _, _ = R.source_pixels(d, centers[k], inv[z], i, j)
        point = mref.ray(kind, (j - d.cx) / d.fx, (i - d.cy) / d.fy) / inv[z]           # in the rig frame
        pu, pv, _, _ = mref.project_ref(d.intr, np.asarray(d.R) @ (point - centers[k]))
        worst = max(worst, abs(u - pu), abs(v - pv))
    assert worst < 1e-9, worst


# ------------------------------------------------------------------------------------------------ interface
def test_default_params():
    p = sweep.params()
    assert (p.struct_size, p.num_hypotheses, p.p1, p.p2, p.paths, p.uniqueness_ratio, p.wrap_x) == (C.sizeof(lib.CSweepParams), 64, 8, 32, 8, 10, 1)
    assert C.sizeof(lib.CSweepParams) == 28
    assert sweep.params(num_hypotheses=32, wrap_x=0).num_hypotheses == 32
    with pytest.raises(AttributeError):
        sweep.params(min_disparity=1)
    inv = sweep.inverse_distances(800.0, D=32)
    assert inv[0] == 0.0 and inv[-1] == 1.0 / 800.0 and np.allclose(np.diff(inv), inv[1]) and inv.size == 32
    assert sweep.inverse_distances(500.0, 4000.0, 16)[0] == 1.0 / 4000.0


def _create(n=2, w=48, h=40, pw=8, ph=4, device=0, mapx="ok", mapy="ok", out="ok", params="ok", **over):
    L = lib.lib()
    p = sweep.params(**{k: v for k, v in over.items() if k != "struct_size"})
    if "struct_size" in over:
        p.struct_size = over["struct_size"]
    D = max(int(p.num_hypotheses), 1)
    tab = np.zeros(max(n, 1) * min(D, 256) * pw * ph if pw > 0 and ph > 0 else 1, np.float32)
    fp = C.POINTER(C.c_float)
    hdl = C.c_void_p()
    rc = L.tscm_sweep_create(n, w, h, None, tab.ctypes.data_as(fp) if mapx == "ok" else None, tab.ctypes.data_as(fp) if mapy == "ok" else None, pw, ph,
                             C.byref(p) if params == "ok" else None, device, C.byref(hdl) if out == "ok" else None)
    assert hdl.value is None
    return rc, L.tscm_last_error()


@pytest.mark.parametrize("kw,text", [
    (dict(struct_size=24), b"struct_size"), (dict(num_hypotheses=0), b"num_hypotheses"), (dict(num_hypotheses=24), b"num_hypotheses"),
    (dict(num_hypotheses=272), b"num_hypotheses"), (dict(p1=-1), b"p1"), (dict(p1=40, p2=32), b"p1"), (dict(p2=256), b"p2"),
    (dict(paths=5), b"paths"), (dict(uniqueness_ratio=100), b"uniqueness_ratio"), (dict(uniqueness_ratio=-1), b"uniqueness_ratio"),
    (dict(n=1), b"n_cameras"), (dict(n=9), b"n_cameras"), (dict(w=0), b"width"), (dict(h=32768), b"height"), (dict(pw=0), b"pano_w"),
    (dict(ph=-3), b"pano_h"), (dict(mapx=None), b"mapx"), (dict(mapy=None), b"mapy"), (dict(out=None), b"out"), (dict(params=None), b"params"),
])
def test_create_refuses_before_a_device_is_touched(kw, text):
    rc, msg = _create(**kw)
    assert rc == -1 and text in msg, (rc, msg)


def test_create_asks_for_the_device_after_the_arguments():
    rc, msg = _create(device=10 ** 6)
    assert rc == -2, (rc, msg)
    rc, msg = _create(device=10 ** 6, paths=6)
    assert rc == -1 and b"paths" in msg


def test_frame_calls_refuse_a_null_handle():
    L = lib.lib()
    assert L.tscm_sweep_depth(None, None, 0, None, 0, None) == -1 and b"s is NULL" in L.tscm_last_error()
    assert L.tscm_sweep_stages(None, None, 0, None, None, None, None, None) == -1 and b"s is NULL" in L.tscm_last_error()
    assert L.tscm_sweep_stage_times(None) == -1 and b"seconds" in L.tscm_last_error()
    L.tscm_sweep_destroy(None)


def _points_call(idx="ok", desc="ok", inv="ok", pts="ok", valid="ok", w=8, h=4, stride=8, D=4, kind=lib.PROJ_EQUIRECT, device=0, inv_values=None):
    L = lib.lib()
    index = np.zeros((4, 8), np.int16)
    d = maps._c_descs([maps.MapDesc(synth.CALIB_INTR[0], np.eye(3), 1.0, 1.0, 4.0, 2.0, 8, 4, projection=4)])
    iv = np.array([0.0, 1.0, 2.0, 3.0] if inv_values is None else inv_values, dtype=np.float64)
    P, ok = np.zeros((4, 8, 3)), np.zeros((4, 8), np.uint8)
    rc = L.tscm_sweep_points(index.ctypes.data_as(C.POINTER(C.c_short)) if idx == "ok" else None, w, h, stride, d if desc == "ok" else None, kind,
                             lib.dptr(iv) if inv == "ok" else None, D, device, lib.dptr(P) if pts == "ok" else None,
                             ok.ctypes.data_as(C.POINTER(C.c_ubyte)) if valid == "ok" else None)
    return rc, L.tscm_last_error()


@pytest.mark.parametrize("kw,code,text", [
    (dict(idx=None), -1, b"index16"), (dict(desc=None), -1, b"pano_map"), (dict(inv=None), -1, b"inv_distance"), (dict(pts=None), -1, b"points"),
    (dict(valid=None), -1, b"valid"), (dict(stride=7), -1, b"stride"), (dict(w=-1), -1, b"pano_w"), (dict(D=1), -1, b"D "),
    (dict(kind=7), -1, b"projection"), (dict(kind=lib.PROJ_PERSPECTIVE), -5, b"PERSPECTIVE"), (dict(inv_values=[0.0, np.nan, 2.0, 3.0]), -1, b"inv_distance[1]"),
    (dict(device=10 ** 6), -2, b""),
])
def test_points_refusals(kw, code, text):
    rc, msg = _points_call(**kw)
    assert rc == code and text in msg, (rc, msg)


def _tables_call(n=2, D=3, maps_="ok", proj="ok", centers="ok", inv="ok", mapx="ok", mapy="ok", n_elems=None, kinds=None, inv_values=None, edit=None, device=0):
    L = lib.lib()
    descs = [maps.MapDesc(synth.CALIB_INTR[k], np.eye(3), 2.0, 2.0, 4.0, 2.0, 8, 4, projection=4) for k in range(max(n, 1))]
    if edit:
        edit(descs)
    arr = maps._c_descs(descs)
    kinds = (C.c_int * len(descs))(*(kinds or [lib.PROJ_EQUIRECT] * len(descs)))
    cen = np.zeros((len(descs), 3))
    iv = np.array([0.0, 0.001, 0.002][:max(D, 1)] if inv_values is None else inv_values, dtype=np.float64)
    total = len(descs) * max(D, 1) * 32
    mx, my = np.zeros(total, np.float32), np.zeros(total, np.float32)
    fp = C.POINTER(C.c_float)
    rc = L.tscm_build_sweep_maps(arr if maps_ == "ok" else None, kinds if proj == "ok" else None, n, lib.dptr(cen) if centers == "ok" else None,
                                 lib.dptr(iv) if inv == "ok" else None, D, device, 1, mx.ctypes.data_as(fp) if mapx == "ok" else None,
                                 my.ctypes.data_as(fp) if mapy == "ok" else None, total if n_elems is None else n_elems, None)
    assert not mx.any() and not my.any()
    return rc, L.tscm_last_error()


def _set(index, **fields):
    def edit(descs):
        for k, v in fields.items():
            setattr(descs[index], k, v)
    return edit


@pytest.mark.parametrize("kw,code,text", [
    (dict(maps_=None), -1, b"maps"), (dict(proj=None), -1, b"projection"), (dict(centers=None), -1, b"centers"), (dict(inv=None), -1, b"inv_distance"),
    (dict(mapx=None), -1, b"mapx"), (dict(mapy=None), -1, b"mapy"), (dict(n=0), -1, b"n_cameras"), (dict(D=0), -1, b"D "),
    (dict(edit=_set(1, width=9, out_stride=9)), -1, b"maps[1]"), (dict(edit=_set(1, height=5)), -1, b"maps[1]"),
    (dict(edit=_set(0, out_stride=12)), -1, b"out_stride"), (dict(edit=_set(1, out_offset=32)), -1, b"out_offset"),
    (dict(n_elems=2 * 3 * 32 - 1), -1, b"n_elems"), (dict(inv_values=[-0.001, 0.0, 0.001]), -1, b"inv_distance[0]"),
    (dict(inv_values=[0.0, np.inf, 1.0]), -1, b"inv_distance[1]"), (dict(inv_values=[0.0, 0.002, 0.002]), -1, b"inv_distance[2]"),
    (dict(inv_values=[0.0, 0.002, 0.001]), -1, b"inv_distance[2]"), (dict(kinds=[4, 9]), -1, b"projection[1]"),
    (dict(kinds=[4, lib.PROJ_PERSPECTIVE]), -5, b"PERSPECTIVE"), (dict(device=10 ** 6), -2, b""),
])
def test_sweep_tables_refusals(kw, code, text):
    rc, msg = _tables_call(**kw)
    assert rc == code and text in msg, (rc, msg)
