"""The perception half of include/tscm/tscm_calib.hpp run on the GPU: rectify_pair_maps, stereo_match / _filter / _points,
Panorama, exposure_gains, Sweep and sweep_points called by tests/native/mirror_perception.cpp, and the five demos of
examples/ run as a user runs them, on PGM / PPM files and a YAML.  Each C++ result equals, bit for bit, what the ctypes
wrappers of tscm_calib_amd give on the same inputs (the other GPU tests pin those wrappers to the host restatements); where
the header does fp64 arithmetic of its own before the first kernel -- the pair rotation, R_cam^T R_pair, the baseline -- its
dumped value goes to both sides and is itself held to a bound that follows from the arithmetic.

Scenes: the textured plane of tests/test_gpu_stereo.py (two cameras) and the textured sphere of tests/test_gpu_sweep.py (four),
320 x 270 sources, 160 x 80 outputs, D = 32 hypotheses from 800 mm, 8 paths.  The inverse distances are the demos'
z / ((D - 1) near), which need not be the bits of np.linspace.

The driver and every demo are built with one set of flags (no -O option, as the build tests of the demos do), so that their
host fp64 arithmetic is the same.  Every child is a fresh process started by _run_child, one at a time; after a child that
ended on a signal, with status 134, 137 or 139, or in the timeout, no further child is started."""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as orc
from tests import gains_ref as G
from tests import stereo_ref
from tests import sweep_ref
from tests.test_gpu_stereo import SCENE as PAIR_SCENE, plane_scene
from tests.test_gpu_sweep import SCENE as SWEEP_SCENE, sphere_scene
from tscm_calib_amd import calib_io, lib, maps, panorama, stereo, sweep

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tscm_calib_amd", "csrc")
CXX = ["g++", "-std=c++11", "-Wall", "-Werror"]
SRC_W, SRC_H = 320, 270
W, H = 160, 80
D, NEAR, PATHS = SWEEP_SCENE["D"], SWEEP_SCENE["near"], SWEEP_SCENE["paths"]
assert (PAIR_SCENE["width"], PAIR_SCENE["height"], SWEEP_SCENE["pano_w"], SWEEP_SCENE["pano_h"]) == (W, H, W, H)
EPS = 2.0 ** -52
PI = float(np.pi)


# ------------------------------------------------------------------------------------------------ children
_abnormal = []            # the first child that ended abnormally


def _run_child(args, cwd):
    """One fresh child process; fails without starting it once an earlier child ended abnormally."""
    if _abnormal:
        pytest.fail("not started: an earlier child ended abnormally (" + _abnormal[0] + ")")
    name = os.path.basename(str(args[0]))
    try:
        r = subprocess.run([str(a) for a in args], cwd=str(cwd), capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _abnormal.append(f"{name}: no end within 120 s")
        pytest.fail(_abnormal[0])
    if r.returncode < 0 or r.returncode in (134, 137, 139):
        _abnormal.append(f"{name}: status {r.returncode}, stderr {r.stderr[-500:]!r}")
        pytest.fail(_abnormal[0])
    return r


@pytest.fixture(scope="module")
def bin_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("mirror_bin")


_built = {}


def _exe(bin_dir, src):
    """examples/<name>.cpp or tests/native/<name>.cpp -> the program, built once per module."""
    if src not in _built:
        out = str(bin_dir / os.path.splitext(os.path.basename(src))[0])
        r = subprocess.run([*CXX, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L", CSRC, "-ltscm_hip", "-Wl,-rpath," + CSRC, "-o", out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        _built[src] = out
    return _built[src]


# ------------------------------------------------------------------------------------------------ the driver's files
_TYPES = [np.uint8, np.int16, np.uint16, np.int32, np.int64, np.float32, np.float64]


def _write_bag(path, records):
    with open(path, "wb") as f:
        f.write(np.array([0x4D435354, 1, len(records)], np.int32).tobytes())
        for name, a in records.items():
            a = np.ascontiguousarray(a)
            code = [np.dtype(t) for t in _TYPES].index(a.dtype)
            f.write(np.array([len(name), code, a.ndim, *a.shape], np.int32).tobytes())
            f.write(name.encode())
            f.write(a.tobytes())


def _read_bag(path):
    raw = open(path, "rb").read()
    head = np.frombuffer(raw, np.int32, 3)
    assert head[0] == 0x4D435354 and head[1] == 1
    pos, out = 12, {}
    for _ in range(int(head[2])):
        n, code, ndim = (int(v) for v in np.frombuffer(raw, np.int32, 3, pos))
        dims = [int(v) for v in np.frombuffer(raw, np.int32, ndim, pos + 12)]
        pos += 12 + 4 * ndim
        name = raw[pos:pos + n].decode()
        pos += n
        count = int(np.prod(dims, dtype=np.int64))
        out[name] = np.frombuffer(raw, _TYPES[code], count, pos).reshape(dims)
        pos += count * np.dtype(_TYPES[code]).itemsize
    assert pos == len(raw)
    return out


def _drive(bin_dir, task, records, expect=0):
    exe = _exe(bin_dir, "tests/native/mirror_perception.cpp")
    tag = f"{task}_{len(os.listdir(str(bin_dir)))}"
    src, dst = str(bin_dir / (tag + "_in.bin")), str(bin_dir / (tag + "_out.bin"))
    _write_bag(src, records)
    r = _run_child([exe, task, src, dst], bin_dir)
    assert r.returncode == expect, (r.returncode, r.stderr[-2000:])
    return _read_bag(dst) if expect == 0 else r.stderr


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False, f"{a.dtype} {a.shape} against {b.dtype} {b.shape}"
    bad = np.argwhere(a != b)
    return len(bad) == 0, f"{len(bad)} of {a.size} differ, first at {bad[0].tolist() if len(bad) else None}"


def _assert_same(a, b, what=""):
    ok, text = _same(a, b)
    assert ok, f"{what}: {text}"


def _assert_same_points(got, got_valid, ref, ref_valid, what):
    """NaN at the same places, the same bits elsewhere, the same valid flags."""
    assert np.array_equal(got_valid.astype(bool), ref_valid), what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.all(np.isnan(got[~ref_valid])) and np.array_equal(got[ref_valid], ref[ref_valid]), what


# ------------------------------------------------------------------------------------------------ inputs
@pytest.fixture(scope="module")
def calib(bin_dir):
    """The quarter-resolution calibration of the two scenes as a YAML file, and the values read back from it: what the
    demos read and what the driver and the Python route are given."""
    intr, T, _ = sphere_scene()
    assert np.array_equal(plane_scene()[0], intr) and np.array_equal(plane_scene()[1], T)
    path = str(bin_dir / "calib.yaml")
    calib_io.write_calib_yaml(path, intr, T[:, :, :3], T[:, :, 3])
    intr, Twc = calib_io.read_calib_yaml(path)
    assert intr.shape == (4, 9) and Twc.shape == (4, 3, 4)
    return path, intr, Twc


def _colour(g):
    return np.stack([g, 255 - g, g // 2 + 60], -1).astype(np.uint8)


def _write_pnm(path, img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P5" if img.ndim == 2 else b"P6", img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def _read_pnm(path):
    """A binary PGM / PPM: uint8 [h, w] or [h, w, 3]; a 16-bit PGM (big-endian) as int64 [h, w]."""
    raw = open(path, "rb").read()
    pos, tok = 0, []
    while len(tok) < 4:                                # magic, width, height, maxval, then one whitespace byte
        while raw[pos:pos + 1].isspace():
            pos += 1
        end = pos
        while end < len(raw) and not raw[end:end + 1].isspace():
            end += 1
        tok.append(raw[pos:end])
        pos = end
    body = raw[pos + 1:]
    w, h, maxval, ch = int(tok[1]), int(tok[2]), int(tok[3]), 3 if tok[0] == b"P6" else 1
    assert tok[0] in (b"P5", b"P6") and maxval in (255, 65535)
    assert len(body) == w * h * ch * (2 if maxval == 65535 else 1), (path, len(body))
    if maxval == 65535:
        return np.frombuffer(body, ">u2").reshape(h, w).astype(np.int64)
    a = np.frombuffer(body, np.uint8)
    return a.reshape(h, w) if ch == 1 else a.reshape(h, w, 3)


# ================================================================================================ pair
STEREO = dict(min_disparity=0, num_disparities=PAIR_SCENE["num_disparities"], p1=8, p2=32, paths=8, uniqueness_ratio=10, disp12_max_diff=1)
FILTER = dict(speckle_window_size=40, speckle_range=2, median=3)
# kind, whether the driver goes on to match / filter / points (rows are epipolar lines in these two kinds only), fov_x, fov_y;
# the long-lat and perspective spans are those of rectify_pair_demo
PAIR_CASES = [(lib.PROJ_LONGLAT, 1, PI, PI / 2), (lib.PROJ_PERSPECTIVE, 1, PI / 2, PI / 2), (lib.PROJ_CYLINDRICAL, 0, PI, PI / 2),
              (lib.PROJ_STEREOGRAPHIC, 0, PI, PI / 2), (lib.PROJ_EQUIRECT, 0, PI, PI / 2)]
PAIR_IDS = ["longlat", "perspective", "cylindrical", "stereographic", "equirect"]


def _pair_records(calib, cases):
    _, intr, Twc = calib
    imgs = plane_scene()[2]
    return dict(intr=intr[:2], Twc=Twc[:2].reshape(2, 12), img_a=imgs[0], img_b=imgs[1], size=np.array([W, H], np.int32),
                cases=np.array([c[:2] for c in cases], np.int32).reshape(-1, 2), fov=np.array([c[2:] for c in cases], np.float64).reshape(-1, 2),
                stereo=np.array([STEREO[k] for k in stereo.PARAM_NAMES], np.int32),
                filter=np.array([FILTER[k] for k in ("speckle_window_size", "speckle_range", "median")], np.int32))


@pytest.fixture(scope="module")
def pair(hip_device, bin_dir, calib):
    return _drive(bin_dir, "pair", _pair_records(calib, PAIR_CASES))


def _desc_of(row, kind):
    """A MapDesc from the 30 dumped values of a tscm_map_desc."""
    return maps.MapDesc(row[:9].copy(), row[9:18].reshape(3, 3).copy(), row[18], row[19], row[20], row[21], int(row[24]), int(row[25]), offset_x=row[22],
                        offset_y=row[23], out_offset=int(row[28]), out_stride=int(row[26]), check_w2=int(row[27]), w2=row[29], projection=kind)


def test_pair_rotation_and_baseline(pair, calib):
    _, _, Twc = calib
    ref = maps.rectify_pair_rotation(Twc[0][:, 3], Twc[1][:, 3])
    diff = float(np.abs(pair["rotation"] - ref).max())
    print(f"rectify_pair_rotation: largest |C++ - Python| {diff:.3e}")
    # three normalisations of vectors of norm <= 1, the same operations in the same order
    assert diff <= 4 * EPS
    assert np.abs(ref.T @ ref - np.eye(3)).max() < 1e-14
    # the baseline is a square root of a sum of three squares on both sides: 2 ulp cover any order of the sum
    B = float(np.linalg.norm(Twc[1][:, 3] - Twc[0][:, 3]))
    assert B > 100 and abs(float(pair["baseline"][0]) - B) <= 2 * EPS * B


@pytest.mark.parametrize("case", range(len(PAIR_CASES)), ids=PAIR_IDS)
def test_pair_descriptors(pair, calib, case):
    _, intr, Twc = calib
    kind, _, fov_x, fov_y = PAIR_CASES[case]
    ref = maps.rectify_pair_descs(intr[0], Twc[0], intr[1], Twc[1], kind, W, H, fov_x, fov_y)
    worst = 0.0
    for k in range(2):
        got = _desc_of(pair[f"desc_{case}"][k], kind)
        # the same expressions on both sides (the stereographic forms differ by powers of two only): equal bits
        for name in ("fx", "fy", "cx", "cy", "width", "height", "out_stride", "check_w2", "w2", "offset_x", "offset_y", "out_offset"):
            assert getattr(got, name) == getattr(ref[k], name), (k, name, getattr(got, name), getattr(ref[k], name))
        assert np.array_equal(got.intr, intr[k])
        assert got.check_w2 == 1 and got.w2 == 0.42399 and got.out_stride == W and got.fx > 0 and got.fy > 0
        # a sum of three products of entries <= 1; numpy's matmul may order or fuse it differently
        worst = max(worst, float(np.abs(got.R - ref[k].R).max()))
        assert np.abs(got.R - ref[k].R).max() <= 4 * EPS
    print(f"{PAIR_IDS[case]}: largest |R_cpp - R_python| of the two descriptors {worst:.3e}")


@pytest.mark.parametrize("kind, fov_x, fov_y", [(lib.PROJ_PERSPECTIVE, PI, PI / 2), (lib.PROJ_CYLINDRICAL, PI, PI)], ids=["perspective-x", "cylindrical-y"])
def test_a_tangent_axis_of_180_degrees_is_refused(hip_device, bin_dir, calib, kind, fov_x, fov_y):
    _, intr, Twc = calib
    text = _drive(bin_dir, "pair", _pair_records(calib, [(kind, 0, fov_x, fov_y)]), expect=3)
    assert "tangent axis" in text
    with pytest.raises(ValueError, match="tangent axis"):
        maps.rectify_pair_descs(intr[0], Twc[0], intr[1], Twc[1], kind, W, H, fov_x, fov_y)


@pytest.mark.parametrize("case", [0, 1], ids=PAIR_IDS[:2])
def test_pair_tables_equal_build_maps_on_the_dumped_descriptors(hip_device, pair, case):
    kind = PAIR_CASES[case][0]
    for k in range(2):
        d = _desc_of(pair[f"desc_{case}"][k], kind)
        mx, my, _ = maps.build_maps([d], device=hip_device)
        _assert_same(pair[f"mapx_{case}"][k].ravel().view(np.uint32), mx.view(np.uint32), f"mapx of camera {k}")
        _assert_same(pair[f"mapy_{case}"][k].ravel().view(np.uint32), my.view(np.uint32), f"mapy of camera {k}")
    inside = (pair[f"mapx_{case}"] >= 0) & (pair[f"mapx_{case}"] <= SRC_W - 1) & (pair[f"mapy_{case}"] >= 0) & (pair[f"mapy_{case}"] <= SRC_H - 1)
    assert inside.mean() > 0.3 and not np.array_equal(pair[f"mapx_{case}"][0], pair[f"mapx_{case}"][1])


@pytest.mark.parametrize("case", range(len(PAIR_CASES)), ids=PAIR_IDS)
def test_pair_rectified_images_equal_the_oracle_remap(pair, case):
    imgs = plane_scene()[2]
    for k in range(2):
        _assert_same(pair[f"rect_{case}"][k], orc.remap(imgs[k], pair[f"mapx_{case}"][k], pair[f"mapy_{case}"][k]), f"camera {k}")
    assert pair[f"rect_{case}"].std() > 10


@pytest.mark.parametrize("case", [0, 1], ids=PAIR_IDS[:2])
def test_pair_disparity_filter_and_points(hip_device, pair, case):
    kind = PAIR_CASES[case][0]
    left, right = pair[f"rect_{case}"]
    disp = pair[f"disparity_{case}"]
    _assert_same(disp, stereo.match(left, right, device=hip_device, **STEREO), "disparity")
    if kind == lib.PROJ_LONGLAT:
        _assert_same(disp, stereo_ref.match(left, right, **{k: v for k, v in STEREO.items() if k != "min_disparity"}), "disparity against the host matcher")
    filtered = pair[f"filtered_{case}"]
    _assert_same(filtered, stereo.filter(disp, device=hip_device, min_disparity=0, **FILTER), "filtered")
    assert not np.array_equal(filtered, disp)                     # the filter did something
    d0 = _desc_of(pair[f"desc_{case}"][0], kind)
    B = float(pair["baseline"][0])
    for dmap, sfx in ((disp, ""), (filtered, "_f")):
        pts, valid = stereo.points(dmap, d0, B, min_disparity=0, device=hip_device)
        _assert_same_points(pair[f"points{sfx}_{case}"], pair[f"valid{sfx}_{case}"], pts, valid, f"points{sfx}")
        assert set(np.unique(pair[f"valid{sfx}_{case}"]).tolist()) <= {0, 1}
        share = valid.mean()
        print(f"{PAIR_IDS[case]} points{sfx}: {100 * share:.1f} % valid")
        assert share > 0.5 if (kind == lib.PROJ_LONGLAT and not sfx) else valid.any()      # not a comparison of empty maps


# ================================================================================================ panorama
SEAM, FEATHER, MULTIBAND = lib.PANO_SEAM, lib.PANO_FEATHER, lib.PANO_MULTIBAND
MODE_NAMES = {SEAM: "seam", FEATHER: "feather", MULTIBAND: "multiband"}
# mode, levels, channels, with the weight images, projection; 6 and 7 are what panorama_demo runs on PPM and PGM input
PANO_CONFIGS = [(SEAM, 4, 1, 1, lib.PROJ_EQUIRECT), (SEAM, 4, 3, 1, lib.PROJ_EQUIRECT), (FEATHER, 4, 1, 1, lib.PROJ_EQUIRECT),
                (FEATHER, 4, 3, 1, lib.PROJ_EQUIRECT), (MULTIBAND, 4, 1, 1, lib.PROJ_EQUIRECT), (MULTIBAND, 4, 3, 1, lib.PROJ_EQUIRECT),
                (MULTIBAND, 4, 3, 0, lib.PROJ_EQUIRECT), (MULTIBAND, 4, 1, 0, lib.PROJ_EQUIRECT), (SEAM, 4, 1, 0, lib.PROJ_CYLINDRICAL)]
PANO_IDS = ["%s-c%d-%s-%s" % (MODE_NAMES[m], c, "weights" if wgt else "plain", "cyl" if p == lib.PROJ_CYLINDRICAL else "eq") for m, _, c, wgt, p in PANO_CONFIGS]
DEMO_PPM, DEMO_PGM = 6, 7
PAD = 7


@functools.lru_cache(maxsize=None)
def _pano_frame():
    """The sphere's frame with camera 1 at 0.8 x its exposure, so that the gains are not all 1."""
    grey = list(sphere_scene()[2])
    grey[1] = ((grey[1].astype(np.int64) * 4 + 2) // 5).astype(np.uint8)
    return np.stack(grey), np.stack([_colour(g) for g in grey])


@pytest.fixture(scope="module")
def pano_weights(hip_device, calib):
    """Radial masks per camera, one NULL entry among them."""
    _, intr, _ = calib
    return [None if k == 1 else panorama.radial_weights(intr[k], SRC_W, SRC_H, device=hip_device) for k in range(4)]


@pytest.fixture(scope="module")
def pano(hip_device, bin_dir, calib, pano_weights):
    _, intr, Twc = calib
    grey, colour = _pano_frame()
    rec = dict(intr=intr, Twc=Twc.reshape(4, 12), gray=grey, color=colour, pano=np.array([W, H], np.int32), pad=np.array([PAD], np.int32),
               weights=np.stack([np.zeros((SRC_H, SRC_W), np.uint8) if x is None else x for x in pano_weights]),
               weight_on=np.array([x is not None for x in pano_weights], np.int32), configs=np.array(PANO_CONFIGS, np.int32))
    return _drive(bin_dir, "panorama", rec)


@pytest.mark.parametrize("m", range(len(PANO_CONFIGS)), ids=PANO_IDS)
def test_panorama_overlap_gains_and_bytes(hip_device, pano, calib, pano_weights, m):
    _, intr, Twc = calib
    mode, levels, ch, with_weights, proj = PANO_CONFIGS[m]
    grey, colour = _pano_frame()
    images = list(grey if ch == 1 else colour)
    gains = pano[f"gains_{m}"]
    with panorama.Composer(intr, Twc, (SRC_W, SRC_H), (W, H), channels=ch, mode=MODE_NAMES[mode], levels=levels, weights=pano_weights if with_weights else None,
                           projection=proj, device=hip_device) as c:
        count, total = c.overlap(images)
        plain, with_gains = c.compose(images), c.compose(images, gains=gains)
    for sfx in ("", "_p"):                                         # rows of width * channels bytes, and padded rows
        _assert_same(pano[f"count{sfx}_{m}"], count, "count" + sfx)
        _assert_same(pano[f"sum{sfx}_{m}"], total, "sum" + sfx)
        _assert_same(pano[f"out{sfx}_{m}"].reshape(plain.shape), plain, "out" + sfx)
        _assert_same(pano[f"out{sfx}g_{m}" if sfx else f"out_g_{m}"].reshape(plain.shape), with_gains, "out with gains" + sfx)
    assert np.all(np.diag(count) > 0) and np.triu(count, 1).sum() > 0 and (plain > 0).mean() > 0.5
    assert not np.array_equal(plain, with_gains)
    # exposure_gains: round(256 g) of the exact rational solution of the documented system, from the same integers
    x = G.exact_q8(count.tolist(), total.tolist())
    dist = [G.half_distance(v) for v in x]
    print(f"{PANO_IDS[m]}: gains {gains.tolist()}, exact 256 g {[round(float(v), 4) for v in x]}, smallest distance to a half-integer {float(min(dist)):.3e}")
    # a condition on the scene, not a tolerance: no camera is left out of the comparison
    assert min(dist) >= G.NEAR_HALF
    assert gains.tolist() == [G.rounded_q8(v) for v in x]
    # the dark camera stands apart: raised in grey; lowered in colour, whose luminance is led by the inverted channel 255 - g
    assert gains.dtype == np.uint16 and len(set(gains.tolist())) > 1 and gains[1] == (gains.max() if ch == 1 else gains.min())
    _assert_same(gains, panorama.exposure_gains(count, total), "the Python route's gains")


# ================================================================================================ sweep
SWEEP_CONFIGS = [(SEAM, 4, 1), (SEAM, 4, 3), (MULTIBAND, 4, 1), (MULTIBAND, 4, 3)]
SWEEP_IDS = ["%s-c%d" % (MODE_NAMES[m], c) for m, _, c in SWEEP_CONFIGS]
SWEEP_GAINS = np.array([256, 300, 230, 270], np.uint16)


def _inv():
    """sweep_depth_demo's hypotheses: uniform in inverse distance, index 0 = infinity."""
    return np.arange(D, dtype=np.float64) / (float(D - 1) * NEAR)


@functools.lru_cache(maxsize=None)
def _sweep_frame():
    grey = sphere_scene()[2]
    return np.stack(grey), np.stack([_colour(g) for g in grey])


@pytest.fixture(scope="module")
def swept(hip_device, bin_dir, calib):
    _, intr, Twc = calib
    grey, colour = _sweep_frame()
    assert _inv()[0] == 0.0 and np.all(np.diff(_inv()) > 0)
    rec = dict(intr=intr, Twc=Twc.reshape(4, 12), gray=grey, color=colour, pano=np.array([W, H], np.int32), pad=np.array([PAD], np.int32), inv=_inv(),
               params=np.array([D, 8, 32, PATHS, 10, 1], np.int32), gains=SWEEP_GAINS, configs=np.array(SWEEP_CONFIGS, np.int32))
    return _drive(bin_dir, "sweep", rec)


@pytest.fixture(scope="module")
def swept_python(hip_device, calib):
    """The Python route on the same inputs, computed once: index map, host restatement, points, and per compose config the
    panorama at the swept depth (the handle's own map, the map passed, with gains) and at infinity."""
    _, intr, Twc = calib
    grey, colour = _sweep_frame()
    res = {}
    with sweep.Sweeper.from_rig(intr, Twc, (SRC_W, SRC_H), W, H, _inv(), weights=None, device=hip_device, keep_tables=True, paths=PATHS) as s:
        idx = s.depth(list(grey))
        res["index"] = idx
        res["host"] = sweep_ref.stages(list(grey), None, s.mapx, s.mapy, paths=PATHS, wrap_x=True)["index16"]
        res["points"], res["valid"] = s.points(idx)
        nothing = np.full((H, W), sweep.INVALID, np.int16)
        for m, (mode, levels, ch) in enumerate(SWEEP_CONFIGS):
            images = list(grey if ch == 1 else colour)
            kw = dict(mode=MODE_NAMES[mode], levels=levels)
            res["null", m] = s.compose(images, **kw)
            res["explicit", m], res["coverage", m] = s.compose(images, index16=idx, with_coverage=True, **kw)
            res["invalid", m] = s.compose(images, index16=nothing, **kw)
            res["padg", m], res["coverage_p", m] = s.compose(images, index16=idx, gains=SWEEP_GAINS, with_coverage=True, **kw)
    for m, (mode, levels, ch) in enumerate(SWEEP_CONFIGS):
        with panorama.Composer(intr, Twc, (SRC_W, SRC_H), (W, H), channels=ch, mode=MODE_NAMES[mode], levels=levels, weights=None, device=hip_device) as c:
            res["pano", m] = c.compose(list(grey if ch == 1 else colour))
    return res


def test_sweep_depth_and_points(swept, swept_python):
    ref = swept_python
    _assert_same(swept["index"], ref["index"], "depth")
    _assert_same(swept["index_p"], ref["index"], "depth from padded rows")
    _assert_same(swept["index"], ref["host"], "depth against the host restatement on the Python route's tables")
    _assert_same_points(swept["points"], swept["valid"], ref["points"], ref["valid"], "points")
    share_idx, share_pts = float((swept["index"] >= 0).mean()), float(swept["valid"].astype(bool).mean())
    print(f"sweep: {100 * share_idx:.1f} % of the index map valid, {100 * share_pts:.1f} % of the points")
    assert share_idx > 0.5 and share_pts > 0.5                     # not a comparison of empty maps


@pytest.mark.parametrize("m", range(len(SWEEP_CONFIGS)), ids=SWEEP_IDS)
def test_sweep_compose(swept, swept_python, m):
    ref = swept_python
    shape = ref["null", m].shape
    got = {k: swept[f"{k}_{m}"].reshape(shape) for k in ("null", "explicit", "covered", "invalid", "padg", "pano")}
    # index16 = NULL is the map the last depth() left on the device, also after composes with other maps
    _assert_same(got["null"], got["explicit"], "NULL against the map passed")
    _assert_same(got["covered"], got["explicit"], "with a coverage vector")
    _assert_same(got["null"], ref["null", m], "NULL against Sweeper.compose")
    _assert_same(got["explicit"], ref["explicit", m], "explicit against Sweeper.compose")
    _assert_same(swept[f"coverage_{m}"], ref["coverage", m], "coverage")
    _assert_same(got["padg"], ref["padg", m], "padded rows with gains")
    _assert_same(swept[f"coverage_p_{m}"], ref["coverage_p", m], "coverage of the padded call")
    # tscm.h: inv_distance[0] = 0, an all-invalid map and fallback_index = 0 give the panorama at infinity
    _assert_same(got["invalid"], got["pano"], "Sweep::compose of an all-invalid map against Panorama::compose")
    _assert_same(got["invalid"], ref["invalid", m], "all-invalid against Sweeper.compose")
    _assert_same(got["pano"], ref["pano", m], "Panorama::compose against Composer.compose")
    assert not np.array_equal(got["explicit"], got["invalid"]) and not np.array_equal(got["explicit"], got["padg"])
    assert (got["explicit"] > 0).mean() > 0.5 and swept[f"coverage_{m}"].max() >= 2


# ================================================================================================ the demos
def _demo(bin_dir, name, args, cwd):
    r = _run_child([_exe(bin_dir, f"examples/{name}.cpp"), *args], cwd)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    return r.stdout


@pytest.mark.parametrize("case", [0, 1], ids=PAIR_IDS[:2])
def test_rectify_pair_demo(bin_dir, calib, pair, tmp_path, case):
    imgs = plane_scene()[2]
    _write_pnm(str(tmp_path / "a.pgm"), imgs[0])
    _write_pnm(str(tmp_path / "b.pgm"), imgs[1])
    extra = [] if PAIR_CASES[case][0] == lib.PROJ_LONGLAT else [PAIR_CASES[case][0]]          # long-lat is the demo's default
    out = _demo(bin_dir, "rectify_pair_demo", [calib[0], 0, 1, "a.pgm", "b.pgm", "out_a.pgm", "out_b.pgm", W, H, *extra], tmp_path)
    assert out.count("% of the table inside the image") == 2
    for k, name in enumerate(("out_a.pgm", "out_b.pgm")):
        _assert_same(_read_pnm(str(tmp_path / name)), pair[f"rect_{case}"][k], name)


@pytest.mark.parametrize("post", [False, True], ids=["raw", "speckle-median"])
def test_stereo_pair_demo(bin_dir, calib, pair, tmp_path, post):
    imgs = plane_scene()[2]
    _write_pnm(str(tmp_path / "a.pgm"), imgs[0])
    _write_pnm(str(tmp_path / "b.pgm"), imgs[1])
    opts = ["--speckle", "%d,%d" % (FILTER["speckle_window_size"], FILTER["speckle_range"]), "--median", FILTER["median"]] if post else []
    _demo(bin_dir, "stereo_pair_demo", [*opts, calib[0], 0, 1, "a.pgm", "b.pgm", "disparity.pgm", "points.txt", W, H, STEREO["num_disparities"], STEREO["paths"]],
          tmp_path)
    sfx = "_f" if post else ""
    disp, pts, valid = pair["filtered_0" if post else "disparity_0"], pair[f"points{sfx}_0"], pair[f"valid{sfx}_0"].astype(bool)
    # the demo's rule: disparity in pixels, rounded, saturated at 255, 0 where there is no point
    shown = np.where(valid, np.clip((disp.astype(np.int64) + 8) // 16, 0, 255), 0).astype(np.uint8)
    _assert_same(_read_pnm(str(tmp_path / "disparity.pgm")), shown, "disparity.pgm")
    rows = np.loadtxt(str(tmp_path / "points.txt"), ndmin=2)
    assert rows.shape == (int(valid.sum()), 5) and valid.sum() > 0
    yy, xx = np.nonzero(valid)                                    # row-major, the order of the file
    assert np.array_equal(rows[:, 0], xx) and np.array_equal(rows[:, 1], yy)
    # 9 significant digits: half a unit of the ninth digit is at most 5e-9 of the value
    assert np.all(np.abs(rows[:, 2:] - pts[valid]) <= 5e-9 * np.abs(pts[valid]))


@pytest.mark.parametrize("with_gains", [False, True], ids=["no-gains", "gains"])
def test_panorama_demo(bin_dir, calib, pano, tmp_path, with_gains):
    _, colour = _pano_frame()
    names = [f"cam{k}.ppm" for k in range(4)]
    for name, img in zip(names, colour):
        _write_pnm(str(tmp_path / name), img)
    out = _demo(bin_dir, "panorama_demo", [calib[0], *names, "--size", W, H, *([] if with_gains else ["--no-gains"])], tmp_path)
    m = DEMO_PPM
    assert PANO_CONFIGS[m] == (MULTIBAND, 4, 3, 0, lib.PROJ_EQUIRECT)        # the demo's defaults, no weight images
    _assert_same(_read_pnm(str(tmp_path / "panorama.ppm")), pano[f"out_g_{m}" if with_gains else f"out_{m}"], "panorama.ppm")
    printed = out.split("gains", 1)[1].split(", kernels")[0].split()
    gains = pano[f"gains_{m}"] if with_gains else np.full(4, 256)
    assert printed == ["%.3f" % (g / 256.0) for g in gains], (printed, gains)


def test_panorama_demo_on_grey_input(bin_dir, calib, pano, tmp_path):
    grey, _ = _pano_frame()
    names = [f"cam{k}.pgm" for k in range(4)]
    for name, img in zip(names, grey):
        _write_pnm(str(tmp_path / name), img)
    _demo(bin_dir, "panorama_demo", [calib[0], *names, "--size", W, H], tmp_path)
    assert PANO_CONFIGS[DEMO_PGM] == (MULTIBAND, 4, 1, 0, lib.PROJ_EQUIRECT)
    _assert_same(_read_pnm(str(tmp_path / "panorama.pgm")), pano[f"out_g_{DEMO_PGM}"][..., 0], "panorama.pgm")


def test_sweep_depth_demo(bin_dir, calib, swept, tmp_path):
    grey, _ = _sweep_frame()
    names = [f"cam{k}.pgm" for k in range(4)]
    for name, img in zip(names, grey):
        _write_pnm(str(tmp_path / name), img)
    _demo(bin_dir, "sweep_depth_demo", [calib[0], *names, "--size", W, H, "--near", "%g" % NEAR, "--hypotheses", D, "--paths", PATHS], tmp_path)
    # 16-bit big-endian, 16 x index + 16, so 0 = invalid
    _assert_same(_read_pnm(str(tmp_path / "sweep_index.pgm")) - 16, swept["index"].astype(np.int64), "sweep_index.pgm")
    ply = open(str(tmp_path / "sweep_points.ply")).read().split("end_header\n")
    n_valid = int(swept["valid"].astype(bool).sum())
    assert f"element vertex {n_valid}\n" in ply[0] and len(ply[1].splitlines()) == n_valid


def test_sweep_panorama_demo_on_ppm_input(hip_device, bin_dir, calib, tmp_path):
    _, intr, Twc = calib
    _, colour = _sweep_frame()
    names = [f"cam{k}.ppm" for k in range(4)]
    for name, img in zip(names, colour):
        _write_pnm(str(tmp_path / name), img)
    _demo(bin_dir, "sweep_panorama_demo", [calib[0], *names, "--size", W, H, "--near", "%g" % NEAR, "--hypotheses", D, "--paths", PATHS], tmp_path)
    # the Python route: depth on the composer's grey values of the three bytes in file order, the frame blended in colour
    with sweep.Sweeper.from_rig(intr, Twc, (SRC_W, SRC_H), W, H, _inv(), weights=None, device=hip_device, paths=PATHS) as s:
        idx = s.depth([sweep.bgr_to_gray(x) for x in colour])
        ref = s.compose(list(colour), mode="multiband", levels=4)
    assert (idx >= 0).mean() > 0.5
    _assert_same(_read_pnm(str(tmp_path / "sweep_panorama.ppm")), ref, "sweep_panorama.ppm")
