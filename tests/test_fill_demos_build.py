"""The three demos that take --fill -- examples/stereo_pair_demo.cpp, sweep_depth_demo.cpp and sweep_panorama_demo.cpp on
stereo_fill / parse_fill_option of include/tscm/tscm_calib.hpp -- and the driver tests/native/mirror_fill.cpp build with plain
g++ against libtscm_hip.so, the way tests/test_sweep_demo_builds.py does, and refuse a rule they do not know."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, src):
    csrc = os.path.join(ROOT, "tscm_calib_amd", "csrc")
    exe = str(tmp_path / "a.out")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L", csrc, "-ltscm_hip", "-Wl,-rpath," + csrc, "-o", exe])
    return exe


@pytest.mark.parametrize("name", ["stereo_pair_demo", "sweep_depth_demo", "sweep_panorama_demo"])
def test_a_demo_with_fill_compiles_and_refuses_an_unknown_rule(tmp_path, name):
    exe = _build(tmp_path, os.path.join("examples", name + ".cpp"))
    for option in ("mean", "median,x", "median,1,2,3", ""):
        # the pair demo takes its options anywhere, the sweep demos after the calibration file
        args = ["--fill", option, "calib.yaml", "0", "1", "a.pgm", "b.pgm", "d.pgm", "p.txt"] if name == "stereo_pair_demo" else \
            ["calib.yaml", "a.pgm", "b.pgm", "--fill", option]
        run = subprocess.run([exe, *args], capture_output=True, text=True)
        assert run.returncode == 2 and "usage" in run.stderr and "--fill RULE" in run.stderr, option


def test_the_driver_compiles_and_parses_the_option(tmp_path):
    exe = _build(tmp_path, os.path.join("tests", "native", "mirror_fill.cpp"))
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr
    import numpy as np
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:                                                # an empty map needs no device
        f.write(np.array([0, 5, 0, 2, 8, 0, 1, 0], np.int32).tobytes())
    assert subprocess.run([exe, src, dst, "second_lowest,7,3"], capture_output=True).returncode == 0 and os.path.getsize(dst) == 0
    assert subprocess.run([exe, src, dst, "second_lowest,7,"], capture_output=True).returncode == 2
    assert subprocess.run([exe, src, dst, "lowest"], capture_output=True).returncode == 0
