"""The two calibration demos that take --ransac -- examples/calibrate_from_corners.cpp and calibrate_from_images.cpp on
TripleSphereCamera::set_ransac / parse_ransac_option of include/tscm/tscm_calib.hpp -- and the driver
tests/native/mirror_ransac.cpp build with plain g++ against libtscm_hip.so, the way tests/test_fill_demos_build.py does, and
refuse an option they cannot read."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, src):
    csrc = os.path.join(ROOT, "tscm_calib_amd", "csrc")
    exe = str(tmp_path / "a.out")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L", csrc, "-ltscm_hip", "-Wl,-rpath," + csrc, "-o", exe])
    return exe


@pytest.mark.parametrize("name", ["calibrate_from_corners", "calibrate_from_images"])
def test_a_demo_with_ransac_compiles_and_refuses_a_bad_option(tmp_path, name):
    exe = _build(tmp_path, os.path.join("examples", name + ".cpp"))
    for option in ("", "x", "0", "-2", "8,0", "8,4097", "8,64,", "8,64,4,1", "nan"):
        run = subprocess.run([exe, "in.txt", "out.yaml", "--ransac", option], capture_output=True, text=True)
        assert run.returncode == 2 and "usage" in run.stderr and "--ransac THRESHOLD" in run.stderr, option
    run = subprocess.run([exe, "in.txt", "out.yaml", "--ransac"], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr
    # a good option passes the parser: the run ends at the input file that is not there
    run = subprocess.run([exe, str(tmp_path / "missing.txt"), str(tmp_path / "out.yaml"), "--ransac", "2.5,128,30"], capture_output=True, text=True)
    assert run.returncode != 0 and "usage" not in run.stderr


def test_the_driver_compiles_and_parses_the_option(tmp_path):
    exe = _build(tmp_path, os.path.join("tests", "native", "mirror_ransac.cpp"))
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:                                                # no views: no device is needed
        f.write(np.array([0, 12, 4, 16, 0, 0], np.int32).tobytes())
        f.write(np.zeros(1 + 9 + 36).tobytes())
    assert subprocess.run([exe, src, dst, "2.5,64,8"], capture_output=True).returncode == 0 and os.path.getsize(dst) == 4
    assert subprocess.run([exe, src, dst, "2.5,64,"], capture_output=True).returncode == 2
    assert subprocess.run([exe, src, dst], capture_output=True).returncode == 3          # threshold_px 0 of the file is refused
