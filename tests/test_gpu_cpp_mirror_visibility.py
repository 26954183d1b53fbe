"""Per-camera visibility through include/tscm/tscm_calib.hpp on the GPU: tscm::Sweep::visibility and the tscm::Sweep::compose
overload under visibility, called by tests/native/mirror_visibility.cpp, equal Sweeper.visibility and Sweeper.compose bit for
bit, and sweep_panorama_demo with --visibility writes the bytes that the Python chain gives on the same inputs.  Built and run
the way tests/test_gpu_cpp_mirror.py does, whose files and child-process rule (one fresh child at a time, none after an
abnormal end) are used here; the frame is the occluder scene of tests/test_sweep_visibility_reference.py."""
import numpy as np
import pytest

from tests import test_gpu_cpp_mirror as M
from tests import test_sweep_visibility_reference as ref_scene
from tests.test_gpu_cpp_mirror import bin_dir, calib  # noqa: F401  (fixtures)
from tscm_calib_amd import lib, sweep

pytestmark = pytest.mark.gpu

W, H = M.W, M.H
NAMES = ("cell_shift", "tolerance", "dilate", "near_is_high")


@pytest.mark.parametrize("with_map,mode,ch,vp,option", [
    (1, "seam", 1, dict(ref_scene.VISIBILITY), None),
    (0, "feather", 3, dict(cell_shift=2, tolerance=2, dilate=0, near_is_high=1), None),
    (1, "multiband", 3, dict(cell_shift=0, tolerance=0, dilate=0, near_is_high=1), "3,1,1"),
], ids=["map-seam", "device-map-feather", "option-multiband"])
def test_visibility_and_compose_equal_the_python_wrapper(hip_device, bin_dir, calib, with_map, mode, ch, vp, option):  # noqa: F811
    path, intr, Twc = calib
    _, _, grey, _, truth_idx = ref_scene.ball_scene()
    frame = list(grey) if ch == 1 else [M._colour(g) for g in grey]
    exe = M._exe(bin_dir, "tests/native/mirror_visibility.cpp")
    src, dst = str(bin_dir / "visibility_in.bin"), str(bin_dir / "visibility_out.bin")
    with open(src, "wb") as f:
        f.write(np.array([M.SRC_W, M.SRC_H, W, H, M.D, M.PATHS, ch, lib.PANO_MODES[mode], *[vp[k] for k in NAMES], with_map], np.int32).tobytes())
        f.write(np.array([M.NEAR]).tobytes() + b"".join(np.ascontiguousarray(g).tobytes() for g in grey) + b"".join(np.ascontiguousarray(x).tobytes() for x in frame))
        if with_map:
            f.write(truth_idx.tobytes())
    r = M._run_child([exe, path, src, dst, *([option] if option else [])], bin_dir)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = np.frombuffer(open(dst, "rb").read(), np.uint8)
    assert raw.size == (4 + 1 + ch) * W * H
    got_use, got_state, got_out = raw[:4 * W * H].reshape(4, H, W), raw[4 * W * H:5 * W * H].reshape(H, W), raw[5 * W * H:].reshape((H, W) if ch == 1 else (H, W, ch))
    if option:
        vp = dict(vp, cell_shift=3, tolerance=1, dilate=1)
    with sweep.Sweeper.from_rig(intr, Twc, (M.SRC_W, M.SRC_H), W, H, M._inv(), weights=None, device=hip_device, paths=M.PATHS) as s:
        idx = s.depth(list(grey))
        at = truth_idx if with_map else None
        use, state = s.visibility(at, with_state=True, **vp)
        out = s.compose(frame, at, mode=mode, visibility=vp)
        plain = s.compose(frame, at, mode=mode)
    M._assert_same(got_use, use, "use")
    M._assert_same(got_state, state, "state")
    M._assert_same(got_out, out, "frame")
    assert (state == 3).sum() >= 10 and not np.array_equal(out, plain) and (idx >= 0).any()


def test_sweep_panorama_demo_with_visibility(hip_device, bin_dir, calib, tmp_path):  # noqa: F811
    """sweep_panorama_demo --visibility 2,2,1: Sweeper.depth on the grey values, Sweeper.compose under visibility at the map
    the depth pass left on the device."""
    _, intr, Twc = calib
    colour = [M._colour(g) for g in ref_scene.ball_scene()[2]]
    for k in range(4):
        M._write_pnm(str(tmp_path / f"cam{k}.ppm"), colour[k])
    M._demo(bin_dir, "sweep_panorama_demo", [calib[0], *[f"cam{k}.ppm" for k in range(4)], "--size", W, H, "--near", "%g" % M.NEAR, "--hypotheses", M.D, "--paths", M.PATHS,
                                            "--mode", "feather", "--visibility", "2,2,1"], tmp_path)
    vp = dict(cell_shift=2, tolerance=2, dilate=1)
    with sweep.Sweeper.from_rig(intr, Twc, (M.SRC_W, M.SRC_H), W, H, M._inv(), weights=None, device=hip_device, paths=M.PATHS) as s:
        s.depth([sweep.bgr_to_gray(x) for x in colour])
        ref = s.compose(colour, mode="feather", visibility=vp)
        plain = s.compose(colour, mode="feather")
    assert not np.array_equal(ref, plain)                                        # the option did something
    M._assert_same(M._read_pnm(str(tmp_path / "sweep_panorama.ppm")), ref, "sweep_panorama.ppm")
