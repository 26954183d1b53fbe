"""The covariance stage through include/tscm/tscm_calib.hpp on the GPU: MultiCalib::covariance(), called by
tests/native/mirror_covariance.cpp behind the flow of examples/calibrate_from_corners.cpp, gives the bytes of api.covariance on
the same problem, and `calibrate_from_corners --covariance` prints the same standard deviations.  Built and run the way
tests/test_gpu_cpp_mirror_ransac.py does (one fresh child at a time, none after an abnormal end)."""
import re

import numpy as np
import pytest

from tests import test_gpu_cpp_mirror as M
from tests.test_gpu_cpp_mirror import bin_dir  # noqa: F401  (fixture)
from tscm_calib_amd import api, calib_io, lib, synth
from tscm_calib_amd.problem import Problem

pytestmark = pytest.mark.gpu
MASK = lib.FIX["cx"] | lib.FIX["cy"]


@pytest.fixture(scope="module")
def mirror(hip_device, bin_dir):  # noqa: F811
    """The rig of test_gpu_fixed's CLI test: corners file, the mirror program's output, the problem it solved."""
    p = synth.make_problem(4, 30, 99, noise_px=0.1)
    inp = synth.make_rig_input(p)
    corners = str(bin_dir / "corners.txt")
    calib_io.write_corners(corners, inp.has, inp.pix_u, inp.pix_v, 9, 6, 45.0)
    out = str(bin_dir / "cov.bin")
    r = M._run_child([M._exe(bin_dir, "tests/native/mirror_covariance.cpp"), corners, out, MASK], bin_dir)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(out, "rb").read()
    C, B, status, n_free = (int(x) for x in np.frombuffer(raw, np.int32, 4))
    at = [16]

    def take(dtype, *shape):
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at[0]).reshape(shape)
        at[0] += a.nbytes
        return a
    sigma2, min_pivot = take(np.float64, 2)
    got = dict(status=status, n_free=n_free, sigma2=sigma2, min_pivot_ratio=min_pivot, cam_rt=take(np.float64, C, 6), intr=take(np.float64, C, 9),
               board_rt=take(np.float64, B, 6), init=take(np.int32, B), cam_rt_std=take(np.float64, C, 6), intr_std=take(np.float64, C, 9),
               board_rt_std=take(np.float64, B, 6), cam_cov=take(np.float64, C, 15, C, 15), board_cov=take(np.float64, B, 6, 6))
    assert at[0] == len(raw)
    # MultiCalib::calibrate's problem: camera-major views of the initialised boards (tscm_calib.hpp: joint_problem)
    cams, boards = np.nonzero(inp.has.astype(bool) & got["init"].astype(bool)[None, :])
    V, n = cams.size, inp.n_points
    const = np.zeros(C, np.uint8); const[0] = 1
    q = Problem(C, B, inp.worlds[:, :2].copy(), cams.astype(np.int32), boards.astype(np.int32), (np.arange(V) * n).astype(np.int32),
                np.full(V, n, np.int32), inp.pix_u[cams, boards].ravel().copy(), inp.pix_v[cams, boards].ravel().copy(),
                got["cam_rt"].copy(), got["intr"].copy(), got["board_rt"].copy(), const, False).normalised()
    return corners, got, q


def test_multicalib_covariance_equals_api_covariance(hip_device, mirror):
    _, got, q = mirror
    want = api.covariance(q, hip_device, fixed=np.full(q.n_cameras, MASK))
    assert got["status"] == want["status"] == 0 and got["n_free"] == want["n_free"]
    for key in ("cam_cov", "board_cov", "cam_rt_std", "intr_std", "board_rt_std"):
        M._assert_same(got[key], want[key], key)
    assert got["sigma2"] == want["sigma2"] and got["min_pivot_ratio"] == want["min_pivot_ratio"]
    assert not got["intr_std"][:, 2:4].any() and np.all(got["intr_std"][:, [0, 1, 4, 5, 6]] > 0)


def test_cli_prints_the_same_standard_deviations(hip_device, bin_dir, mirror):  # noqa: F811
    corners, got, q = mirror
    exe = M._exe(bin_dir, "examples/calibrate_from_corners.cpp")
    plain = M._run_child([exe, corners, bin_dir / "plain.yaml", "--fix", "cx,cy"], bin_dir)
    r = M._run_child([exe, corners, bin_dir / "cov.yaml", "--fix", "cx,cy", "--covariance"], bin_dir)
    # (exit status 3: a mono calibration with held cx, cy did not report CONVERGENCE; the rig solve follows all the same)
    assert plain.returncode in (0, 3) and r.returncode == plain.returncode, (plain.stderr[-1000:], r.stderr[-1000:])
    # without the flag: the output as before, a prefix of the output with it; the YAML the same
    assert r.stdout.startswith(plain.stdout) and "+-" not in plain.stdout
    assert open(bin_dir / "plain.yaml").read() == open(bin_dir / "cov.yaml").read()
    names = ["r0", "r1", "r2", "t0", "t1", "t2", "fx", "fy", "cx", "cy", "xi", "lambda", "alpha"]
    rows = re.findall(r"^camera_(\d+) (\w+) (\S+) \+- (\S+)$", r.stdout, re.M)
    assert len(rows) == 13 * q.n_cameras
    for m, name, value, sd in rows:
        m, a = int(m), names.index(name)
        want_v, want_sd = (got["cam_rt"][m, a], got["cam_rt_std"][m, a]) if a < 6 else (got["intr"][m, a - 6], got["intr_std"][m, a - 6])
        assert float(value) == want_v and float(sd) == want_sd, (m, name)
    tail = re.search(r"^sigma (\S+)  min_pivot_ratio (\S+)  free columns (\d+)$", r.stdout, re.M)
    assert tail and float(tail.group(1)) == np.sqrt(got["sigma2"]) and float(tail.group(2)) == got["min_pivot_ratio"] and int(tail.group(3)) == got["n_free"]
