"""examples/calibrate_from_corners.cpp with --covariance and the driver tests/native/mirror_covariance.cpp (both on
MultiCalib::covariance of include/tscm/tscm_calib.hpp) build with plain g++ against libtscm_hip.so, the way
tests/test_ransac_demos_build.py does, and the option passes the demo's parser.  No GPU."""
import os
import subprocess

from tests.test_ransac_demos_build import _build


def test_the_demo_takes_the_option(tmp_path):
    exe = _build(tmp_path, os.path.join("examples", "calibrate_from_corners.cpp"))
    run = subprocess.run([exe, "in.txt", "out.yaml", "--covariance", "now"], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr and "[--covariance]" in run.stderr
    # the option alone passes the parser: the run ends at the input file that is not there
    run = subprocess.run([exe, str(tmp_path / "missing.txt"), str(tmp_path / "out.yaml"), "--covariance"], capture_output=True, text=True)
    assert run.returncode == 1 and "usage" not in run.stderr


def test_the_driver_compiles(tmp_path):
    exe = _build(tmp_path, os.path.join("tests", "native", "mirror_covariance.cpp"))
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr
    run = subprocess.run([exe, str(tmp_path / "missing.txt"), str(tmp_path / "out.bin"), "12"], capture_output=True, text=True)
    assert run.returncode == 2 and not os.path.exists(tmp_path / "out.bin")
