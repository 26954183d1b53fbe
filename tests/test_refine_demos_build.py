"""The three demos that take --refine -- examples/stereo_pair_demo.cpp, sweep_depth_demo.cpp and sweep_panorama_demo.cpp on
stereo_refine / range_weights / parse_refine_option of include/tscm/tscm_calib.hpp -- and the driver
tests/native/mirror_refine.cpp build with plain g++ against libtscm_hip.so, the way tests/test_fill_demos_build.py does, and
refuse an option that is not RADIUS,SIGMA[,ITERATIONS[,FILL]] within the library's ranges."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_OPTIONS = ("", "3", "x,10", "3,10,0", "3,10,1,2", "8,10")


def _build(tmp_path, src):
    csrc = os.path.join(ROOT, "tscm_calib_amd", "csrc")
    exe = str(tmp_path / "a.out")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L", csrc, "-ltscm_hip", "-Wl,-rpath," + csrc, "-o", exe])
    return exe


@pytest.mark.parametrize("name", ["stereo_pair_demo", "sweep_depth_demo", "sweep_panorama_demo"])
def test_a_demo_with_refine_compiles_and_refuses_a_malformed_option(tmp_path, name):
    exe = _build(tmp_path, os.path.join("examples", name + ".cpp"))
    for option in BAD_OPTIONS:
        # the pair demo takes its options anywhere, the sweep demos after the calibration file
        args = ["--refine", option, "calib.yaml", "0", "1", "a.pgm", "b.pgm", "d.pgm", "p.txt"] if name == "stereo_pair_demo" else \
            ["calib.yaml", "a.pgm", "b.pgm", "--refine", option]
        run = subprocess.run([exe, *args], capture_output=True, text=True)
        assert run.returncode == 2 and "usage" in run.stderr and "--refine RADIUS" in run.stderr, option


def test_the_driver_compiles_and_parses_the_option(tmp_path):
    exe = _build(tmp_path, os.path.join("tests", "native", "mirror_refine.cpp"))
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:                                                # an empty map needs no device
        f.write(np.array([0, 5, 0, 3, 1, 0, 0], np.int32).tobytes() + np.array([10.0]).tobytes())
    for option in ("3,10", "7,0.5,8,1", "1,4,2"):
        assert subprocess.run([exe, src, dst, option], capture_output=True).returncode == 0 and os.path.getsize(dst) == 0, option
    for option in BAD_OPTIONS + ("3,10,", "3,,1", " 3,10", "3,10,1,0,0", "3,ten"):
        assert subprocess.run([exe, src, dst, option], capture_output=True).returncode == 2, option
