"""Hole filling through include/tscm/tscm_calib.hpp on the GPU: tscm::stereo_fill called by tests/native/mirror_fill.cpp equals
stereo.fill bit for bit, and stereo_pair_demo, sweep_depth_demo and sweep_panorama_demo with --fill write the bytes that the
Python route gives on the same inputs.  Built and run the way tests/test_gpu_cpp_mirror.py does, whose scenes, files and
child-process rule (one fresh child at a time, none after an abnormal end) are used here."""
import numpy as np
import pytest

from tests import test_gpu_cpp_mirror as M
from tests.test_gpu_cpp_mirror import bin_dir, calib  # noqa: F401  (fixtures)
from tests.test_gpu_stereo import plane_scene
from tscm_calib_amd import lib, stereo, sweep

pytestmark = pytest.mark.gpu

W, H = M.W, M.H
FILL_NAMES = ("min_disparity", "rule", "paths", "max_distance", "min_directions", "wrap_x")
DEMO_FILL = dict(rule="second_lowest", max_distance=20, min_directions=2)     # --fill second_lowest,20,2
DEMO_OPTION = "second_lowest,20,2"


def _padded_map(w=130, h=35, pad=9, min_disparity=0):
    rng = np.random.default_rng(5)
    wide = np.full((h, w + pad), 12345, dtype=np.int16)
    d = (16 * rng.integers(-40, 200, size=(h, w)) + 3).astype(np.int16)
    d[rng.random((h, w)) < 0.6] = 16 * (min_disparity - 1)
    wide[:, :w] = d
    return wide, wide[:, :w]


@pytest.mark.parametrize("params,option", [
    (dict(min_disparity=0, rule=2, paths=8, max_distance=0, min_directions=1, wrap_x=0), None),
    (dict(min_disparity=-3, rule=1, paths=4, max_distance=5, min_directions=2, wrap_x=1), None),
    (dict(min_disparity=0, rule=2, paths=8, max_distance=0, min_directions=1, wrap_x=1), "lowest,3"),
], ids=["defaults", "all-fields", "option"])
def test_stereo_fill_equals_the_python_wrapper_on_a_padded_map(hip_device, bin_dir, params, option):  # noqa: F811
    wide, view = _padded_map(min_disparity=params["min_disparity"])
    exe = M._exe(bin_dir, "tests/native/mirror_fill.cpp")
    src, dst = str(bin_dir / "fill_in.bin"), str(bin_dir / "fill_out.bin")
    with open(src, "wb") as f:
        f.write(np.array([view.shape[1], view.shape[0], *[params[k] for k in FILL_NAMES]], np.int32).tobytes())
        f.write(np.ascontiguousarray(view).tobytes())
    r = M._run_child([exe, src, dst, *([option] if option else [])], bin_dir)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(dst, "rb").read()
    n = view.size
    assert len(raw) == 3 * n
    got, got_mask = np.frombuffer(raw, np.int16, n).reshape(view.shape), np.frombuffer(raw, np.uint8, n, 2 * n).reshape(view.shape)
    if option:
        params = dict(params, rule=lib.FILL_LOWEST, max_distance=3)
    out, mask = stereo.fill(view, device=hip_device, with_mask=True, **params)
    M._assert_same(got, out, "stereo_fill")
    M._assert_same(got_mask, mask, "mask")
    assert np.any(mask == 1) and np.all(wide[:, view.shape[1]:] == 12345)


def test_stereo_pair_demo_with_fill(hip_device, bin_dir, calib, tmp_path):  # noqa: F811
    """The demo's files against match -> filter -> fill -> points of the Python wrappers on the rectified pair and the
    descriptor that the header's own host arithmetic gives (dumped by tests/native/mirror_perception.cpp)."""
    pair = M._drive(bin_dir, "pair", M._pair_records(calib, M.PAIR_CASES[:1]))
    imgs = plane_scene()[2]
    M._write_pnm(str(tmp_path / "a.pgm"), imgs[0])
    M._write_pnm(str(tmp_path / "b.pgm"), imgs[1])
    opts = ["--speckle", "%d,%d" % (M.FILTER["speckle_window_size"], M.FILTER["speckle_range"]), "--median", M.FILTER["median"], "--fill", DEMO_OPTION]
    M._demo(bin_dir, "stereo_pair_demo", [*opts, calib[0], 0, 1, "a.pgm", "b.pgm", "disparity.pgm", "points.txt", W, H, M.STEREO["num_disparities"], M.STEREO["paths"]],
            tmp_path)
    left, right = pair["rect_0"]
    disp = stereo.match(left, right, device=hip_device, **M.STEREO)
    filtered = stereo.filter(disp, device=hip_device, min_disparity=0, **M.FILTER)
    M._assert_same(filtered, pair["filtered_0"], "the filtered map of the driver")
    filled, mask = stereo.fill(filtered, device=hip_device, with_mask=True, min_disparity=0, **DEMO_FILL)
    assert np.any(mask == 1)                                                  # the option did something
    pts, valid = stereo.points(filled, M._desc_of(pair["desc_0"][0], lib.PROJ_LONGLAT), float(pair["baseline"][0]), min_disparity=0, device=hip_device)
    assert valid.sum() > pair["valid_f_0"].astype(bool).sum()
    shown = np.where(valid, np.clip((filled.astype(np.int64) + 8) // 16, 0, 255), 0).astype(np.uint8)
    M._assert_same(M._read_pnm(str(tmp_path / "disparity.pgm")), shown, "disparity.pgm")
    rows = np.loadtxt(str(tmp_path / "points.txt"), ndmin=2)
    assert rows.shape == (int(valid.sum()), 5)
    yy, xx = np.nonzero(valid)
    assert np.array_equal(rows[:, 0], xx) and np.array_equal(rows[:, 1], yy)
    assert np.all(np.abs(rows[:, 2:] - pts[valid]) <= 5e-9 * np.abs(pts[valid]))


def test_sweep_demos_with_fill(hip_device, bin_dir, calib, tmp_path):  # noqa: F811
    """sweep_depth_demo and sweep_panorama_demo with --fill: the index map and the frame of Sweeper.depth -> stereo.fill
    (wrap_x = 1, as the sweep chains set it) -> Sweeper.compose at the filled map."""
    _, intr, Twc = calib
    grey, colour = M._sweep_frame()
    for k in range(4):
        M._write_pnm(str(tmp_path / f"cam{k}.pgm"), grey[k])
        M._write_pnm(str(tmp_path / f"cam{k}.ppm"), colour[k])
    common = ["--size", W, H, "--near", "%g" % M.NEAR, "--hypotheses", M.D, "--paths", M.PATHS, "--fill", DEMO_OPTION]
    M._demo(bin_dir, "sweep_depth_demo", [calib[0], *[f"cam{k}.pgm" for k in range(4)], *common], tmp_path)
    M._demo(bin_dir, "sweep_panorama_demo", [calib[0], *[f"cam{k}.ppm" for k in range(4)], *common], tmp_path)
    with sweep.Sweeper.from_rig(intr, Twc, (M.SRC_W, M.SRC_H), W, H, M._inv(), weights=None, device=hip_device, paths=M.PATHS) as s:
        idx = s.depth(list(grey))
        filled = stereo.fill(idx, device=hip_device, wrap_x=1, **DEMO_FILL)
        _, valid = s.points(filled)
        idx_c = s.depth([sweep.bgr_to_gray(x) for x in colour])
        filled_c = stereo.fill(idx_c, device=hip_device, wrap_x=1, **DEMO_FILL)
        ref = s.compose(list(colour), index16=filled_c, mode="multiband", levels=4)
        unfilled = s.compose(list(colour), index16=idx_c, mode="multiband", levels=4)
    assert not np.array_equal(filled, idx) and not np.array_equal(ref, unfilled)          # the option did something
    M._assert_same(M._read_pnm(str(tmp_path / "sweep_index.pgm")) - 16, filled.astype(np.int64), "sweep_index.pgm")
    ply = open(str(tmp_path / "sweep_points.ply")).read().split("end_header\n")
    assert f"element vertex {int(valid.sum())}\n" in ply[0]
    M._assert_same(M._read_pnm(str(tmp_path / "sweep_panorama.ppm")), ref, "sweep_panorama.ppm")
