"""examples/calibrate_from_corners.cpp and examples/calibrate_from_images.cpp with --residuals / --residual-bins / --prune and
the driver tests/native/mirror_residuals.cpp (all on MultiCalib::residual_report and prune_views of include/tscm/tscm_calib.hpp)
build with plain g++ against libtscm_hip.so, the way tests/test_covariance_demos_build.py does, and the options pass the demos'
parsers.  No GPU."""
import os
import subprocess

import pytest

from tests.test_ransac_demos_build import _build

GOOD = (["--residuals"], ["--residuals=report.txt"], ["--residual-bins", "8"], ["--prune", "3"], ["--prune", "2.5,2"], ["--prune", "3,2,0.1", "--residuals"])
BAD = (["--residuals="], ["--residual-bins"], ["--residual-bins", "0"], ["--residual-bins", "65"], ["--prune"], ["--prune", "x"], ["--prune", "3,0"],
       ["--prune", "3,1,1.5"], ["--prune", "3,1,0.2,7"], ["--prune", "-1"])


@pytest.mark.parametrize("demo", ["calibrate_from_corners.cpp", "calibrate_from_images.cpp"])
def test_the_demos_take_the_options(tmp_path, demo):
    exe = _build(tmp_path, os.path.join("examples", demo))
    for args in BAD:
        run = subprocess.run([exe, "in.txt", "out.yaml", *args], capture_output=True, text=True)
        assert run.returncode == 2 and "usage" in run.stderr and "[--prune K[,ROUNDS[,MAX_FRACTION]]]" in run.stderr, args
    # a well-formed option passes the parser: the run ends at the input file that is not there
    for args in GOOD:
        run = subprocess.run([exe, str(tmp_path / "missing.txt"), str(tmp_path / "out.yaml"), *args], capture_output=True, text=True)
        assert run.returncode != 0 and "usage" not in run.stderr, args


def test_the_driver_compiles(tmp_path):
    exe = _build(tmp_path, os.path.join("tests", "native", "mirror_residuals.cpp"))
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr
    run = subprocess.run([exe, str(tmp_path / "missing.txt"), str(tmp_path / "out.bin"), "3", "0.2"], capture_output=True, text=True)
    assert run.returncode == 2 and not os.path.exists(tmp_path / "out.bin")
