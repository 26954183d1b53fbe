"""examples/sweep_panorama_demo.cpp with --visibility, on Sweep::compose under visibility and parse_visibility_option of
include/tscm/tscm_calib.hpp, and the driver tests/native/mirror_visibility.cpp build with plain g++ against libtscm_hip.so, the
way tests/test_refine_demos_build.py does; the option is accepted as SHIFT,TOLERANCE[,DILATE] within the library's ranges and
refused otherwise."""
import os
import subprocess

from tests.test_refine_demos_build import _build

GOOD_OPTIONS = {"2,2": (2, 2, 0), "0,0,0": (0, 0, 0), "8,255,2": (8, 255, 2), "3,17,1": (3, 17, 1)}
BAD_OPTIONS = ("", "2", "x,2", "2,x", "9,2", "-1,2", "2,256", "2,-1", "2,2,3", "2,2,-1", "2,2,1,0", "2,2,", "2,,1", " 2,2", "2.5,2", "2,2,1 ")


def test_the_demo_compiles_and_refuses_a_malformed_option(tmp_path):
    exe = _build(tmp_path, os.path.join("examples", "sweep_panorama_demo.cpp"))
    for option in BAD_OPTIONS:
        run = subprocess.run([exe, "calib.yaml", "a.pgm", "b.pgm", "--visibility", option], capture_output=True, text=True)
        assert run.returncode == 2 and "usage" in run.stderr and "--visibility SHIFT,TOLERANCE[,DILATE]" in run.stderr, option
    # a well-formed option passes the command line: the demo goes on to the calibration file, which is not there
    for option in GOOD_OPTIONS:
        run = subprocess.run([exe, str(tmp_path / "none.yaml"), "a.pgm", "b.pgm", "--visibility", option], capture_output=True, text=True)
        assert run.returncode == 1 and "usage" not in run.stderr, (option, run.stderr)


def test_the_driver_compiles_and_parses_the_option(tmp_path):
    exe = _build(tmp_path, os.path.join("tests", "native", "mirror_visibility.cpp"))
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(src, "wb").close()                                                   # an empty file: the option alone, no device
    run = subprocess.run([exe, "calib.yaml", src, dst], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.split() == ["2", "2", "0"]       # the library's defaults
    for option, fields in GOOD_OPTIONS.items():
        run = subprocess.run([exe, "calib.yaml", src, dst, option], capture_output=True, text=True)
        assert run.returncode == 0 and tuple(int(v) for v in run.stdout.split()) == fields, option
    for option in BAD_OPTIONS:
        assert subprocess.run([exe, "calib.yaml", src, dst, option], capture_output=True).returncode == 2, option
