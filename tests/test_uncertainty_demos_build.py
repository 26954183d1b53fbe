"""examples/calibrate_from_corners.cpp with --uncertainty and the driver tests/native/mirror_uncertainty.cpp (both on
MultiCalib::projection_uncertainty of include/tscm/tscm_calib.hpp) build with plain g++ against libtscm_hip.so, the way
tests/test_covariance_demos_build.py does, and the option passes the demo's parser.  No GPU."""
import os
import subprocess

from tests.test_ransac_demos_build import _build


def test_the_demo_takes_the_option(tmp_path):
    exe = _build(tmp_path, os.path.join("examples", "calibrate_from_corners.cpp"))
    for bad in (["--uncertainty"], ["--uncertainty", "0"], ["--uncertainty", "-4"], ["--uncertainty", "8,"], ["--uncertainty", "8,-1"],
                ["--uncertainty", "8,0.01,3"], ["--uncertainty", "x"]):
        run = subprocess.run([exe, "in.txt", "out.yaml"] + bad, capture_output=True, text=True)
        assert run.returncode == 2 and "usage" in run.stderr and "[--covariance]" in run.stderr and "[--uncertainty STEP[,INV_DISTANCE]]" in run.stderr, bad
    # the option passes the parser: the run ends at the input file that is not there
    for good in (["--uncertainty", "16"], ["--uncertainty", "16,0.002"], ["--covariance", "--uncertainty", "2.5,0"]):
        run = subprocess.run([exe, str(tmp_path / "missing.txt"), str(tmp_path / "out.yaml")] + good, capture_output=True, text=True)
        assert run.returncode == 1 and "usage" not in run.stderr, good


def test_the_driver_compiles(tmp_path):
    exe = _build(tmp_path, os.path.join("tests", "native", "mirror_uncertainty.cpp"))
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr
    run = subprocess.run([exe, str(tmp_path / "missing.txt"), str(tmp_path / "out.bin"), "12", "32", "0.01"], capture_output=True, text=True)
    assert run.returncode == 2 and not os.path.exists(tmp_path / "out.bin")
