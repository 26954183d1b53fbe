"""The weighted median through include/tscm/tscm_calib.hpp on the GPU: tscm::stereo_refine with tscm::range_weights, called by
tests/native/mirror_refine.cpp, equals stereo.refine bit for bit, and sweep_depth_demo and sweep_panorama_demo with --fill and
--refine write the bytes that the Python chain gives on the same inputs.  Built and run the way tests/test_gpu_cpp_mirror.py
does, whose scenes, files and child-process rule (one fresh child at a time, none after an abnormal end) are used here."""
import numpy as np
import pytest

from tests import test_gpu_cpp_mirror as M
from tests.test_gpu_cpp_mirror import bin_dir, calib  # noqa: F401  (fixtures)
from tscm_calib_amd import stereo, sweep

pytestmark = pytest.mark.gpu

W, H = M.W, M.H
REFINE_NAMES = ("min_disparity", "radius", "iterations", "fill_invalid", "wrap_x")
DEMO_FILL = dict(rule="second_lowest", max_distance=20, min_directions=2)     # --fill second_lowest,20,2
DEMO_REFINE = dict(radius=2, sigma=25.0, iterations=2, fill_invalid=1)        # --refine 2,25,2,1
FILL_OPTION, REFINE_OPTION = "second_lowest,20,2", "2,25,2,1"


def _map_and_guide(w=130, h=35, min_disparity=0):
    rng = np.random.default_rng(5)
    d = (16 * rng.integers(-40, 40, size=(h, w)) + 3).astype(np.int16)
    d[rng.random((h, w)) < 0.4] = 16 * (min_disparity - 1)
    g = (rng.integers(0, 8, size=(h, w)) * 30).astype(np.uint8)
    return d, g


@pytest.mark.parametrize("params,sigma,option", [
    (dict(min_disparity=0, radius=3, iterations=1, fill_invalid=0, wrap_x=0), -1.0, None),
    (dict(min_disparity=-3, radius=7, iterations=2, fill_invalid=1, wrap_x=1), 20.0, None),
    (dict(min_disparity=0, radius=3, iterations=1, fill_invalid=0, wrap_x=1), 20.0, "1,8.5,3,1"),
], ids=["defaults-no-table", "all-fields", "option"])
def test_stereo_refine_equals_the_python_wrapper(hip_device, bin_dir, params, sigma, option):  # noqa: F811
    d, g = _map_and_guide(min_disparity=params["min_disparity"])
    exe = M._exe(bin_dir, "tests/native/mirror_refine.cpp")
    src, dst = str(bin_dir / "refine_in.bin"), str(bin_dir / "refine_out.bin")
    with open(src, "wb") as f:
        f.write(np.array([d.shape[1], d.shape[0], *[params[k] for k in REFINE_NAMES]], np.int32).tobytes())
        f.write(np.array([sigma]).tobytes() + d.tobytes() + g.tobytes())
    r = M._run_child([exe, src, dst, *([option] if option else [])], bin_dir)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.frombuffer(open(dst, "rb").read(), np.int16).reshape(d.shape)
    if option:
        params, sigma = dict(params, radius=1, iterations=3, fill_invalid=1), 8.5
    want = stereo.refine(d, g, device=hip_device, sigma=None if sigma < 0 else sigma, **params)
    M._assert_same(got, want, "stereo_refine")
    assert not np.array_equal(want, d)


def test_sweep_demos_with_refine(hip_device, bin_dir, calib, tmp_path):  # noqa: F811
    """sweep_depth_demo and sweep_panorama_demo with --fill and --refine: the index map and the frame of
    Sweeper.depth -> stereo.fill -> stereo.refine guided by the SEAM frame at the filled map (wrap_x = 1, as the sweep chains
    set it) -> Sweeper.compose at the refined map."""
    _, intr, Twc = calib
    grey, colour = M._sweep_frame()
    for k in range(4):
        M._write_pnm(str(tmp_path / f"cam{k}.pgm"), grey[k])
        M._write_pnm(str(tmp_path / f"cam{k}.ppm"), colour[k])
    common = ["--size", W, H, "--near", "%g" % M.NEAR, "--hypotheses", M.D, "--paths", M.PATHS, "--fill", FILL_OPTION, "--refine", REFINE_OPTION]
    M._demo(bin_dir, "sweep_depth_demo", [calib[0], *[f"cam{k}.pgm" for k in range(4)], *common], tmp_path)
    M._demo(bin_dir, "sweep_panorama_demo", [calib[0], *[f"cam{k}.ppm" for k in range(4)], *common], tmp_path)
    with sweep.Sweeper.from_rig(intr, Twc, (M.SRC_W, M.SRC_H), W, H, M._inv(), weights=None, device=hip_device, paths=M.PATHS) as s:
        def chain(images):
            filled = stereo.fill(s.depth(images), device=hip_device, wrap_x=1, **DEMO_FILL)
            guide = s.compose(images, index16=filled, mode="seam", fallback_index=0)
            return filled, stereo.refine(filled, guide, device=hip_device, wrap_x=1, **DEMO_REFINE)

        filled, refined = chain(list(grey))
        _, valid = s.points(refined)
        filled_c, refined_c = chain([sweep.bgr_to_gray(x) for x in colour])
        ref = s.compose(list(colour), index16=refined_c, mode="multiband", levels=4)
    assert not np.array_equal(refined, filled) and not np.array_equal(refined_c, filled_c)          # the option did something
    M._assert_same(M._read_pnm(str(tmp_path / "sweep_index.pgm")) - 16, refined.astype(np.int64), "sweep_index.pgm")
    ply = open(str(tmp_path / "sweep_points.ply")).read().split("end_header\n")
    assert f"element vertex {int(valid.sum())}\n" in ply[0]
    M._assert_same(M._read_pnm(str(tmp_path / "sweep_panorama.ppm")), ref, "sweep_panorama.ppm")
