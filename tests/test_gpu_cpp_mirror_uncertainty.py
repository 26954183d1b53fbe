"""The projection uncertainty stage through include/tscm/tscm_calib.hpp on the GPU: MultiCalib::projection_uncertainty(),
called by tests/native/mirror_uncertainty.cpp behind the flow of examples/calibrate_from_corners.cpp, gives the bytes of
api.projection_uncertainty on the same problem, and `calibrate_from_corners --uncertainty` prints the largest and the median
of the same planes.  Built and run the way tests/test_gpu_cpp_mirror_covariance.py does (one fresh child at a time, none
after an abnormal end)."""
import re

import numpy as np
import pytest

from tests import test_gpu_cpp_mirror as M
from tests.test_gpu_cpp_mirror import bin_dir  # noqa: F401  (fixture)
from tscm_calib_amd import api, calib_io, lib, pipeline, synth
from tscm_calib_amd.problem import Problem

pytestmark = pytest.mark.gpu
MASK = lib.FIX["cx"] | lib.FIX["cy"]
STEP, INV = 64.0, 1.0 / 300


@pytest.fixture(scope="module")
def mirror(hip_device, bin_dir):  # noqa: F811
    """The rig of test_gpu_cpp_mirror_covariance: corners file, the mirror program's output, the problem it solved."""
    p = synth.make_problem(4, 30, 99, noise_px=0.1)
    inp = synth.make_rig_input(p)
    corners = str(bin_dir / "corners.txt")
    calib_io.write_corners(corners, inp.has, inp.pix_u, inp.pix_v, 9, 6, 45.0)
    out = str(bin_dir / "unc.bin")
    r = M._run_child([M._exe(bin_dir, "tests/native/mirror_uncertainty.cpp"), corners, out, MASK, repr(STEP), repr(INV)], bin_dir)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(out, "rb").read()
    C, B, R, nx, ny, _ = (int(x) for x in np.frombuffer(raw, np.int32, 6))
    at = [24]

    def take(dtype, *shape):
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at[0]).reshape(shape)
        at[0] += a.nbytes
        return a
    got = dict(cam_rt=take(np.float64, C, 6), intr=take(np.float64, C, 9), board_rt=take(np.float64, B, 6), init=take(np.int32, B))
    req = take(np.dtype([("a", np.int32), ("b", np.int32), ("i", np.float64)]), R)
    got.update(requests=[(int(x["a"]), int(x["b"]), float(x["i"])) for x in req], planes=take(np.float64, R, 7, ny, nx), max_sd=take(np.float64, R),
               n_valid=take(np.int64, R), flags=take(np.uint8, R, ny, nx))
    assert at[0] == len(raw)
    cams, boards = np.nonzero(inp.has.astype(bool) & got["init"].astype(bool)[None, :])
    V, n = cams.size, inp.n_points
    const = np.zeros(C, np.uint8); const[0] = 1
    q = Problem(C, B, inp.worlds[:, :2].copy(), cams.astype(np.int32), boards.astype(np.int32), (np.arange(V) * n).astype(np.int32),
                np.full(V, n, np.int32), inp.pix_u[cams, boards].ravel().copy(), inp.pix_v[cams, boards].ravel().copy(),
                got["cam_rt"].copy(), got["intr"].copy(), got["board_rt"].copy(), const, False).normalised()
    return corners, got, q


def test_multicalib_projection_uncertainty_equals_the_api(hip_device, mirror):
    _, got, q = mirror
    cov = api.covariance(q, hip_device, fixed=np.full(q.n_cameras, MASK))
    assert got["requests"] == pipeline.uncertainty_requests(q.n_cameras, (INV,))
    w, h = int(synth.IMG_W), int(synth.IMG_H)
    grid = api.uncertainty_grid(int((w - 1) // STEP) + 1, int((h - 1) // STEP) + 1, 0.0, 0.0, STEP, STEP, w, h)
    want = api.projection_uncertainty(q.cam_rt, q.intr, cov, got["requests"], grid, hip_device)
    assert got["planes"].shape == want["planes"].shape
    for key in ("planes", "flags", "max_sd", "n_valid"):
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key      # (bytes: the planes hold NaN)
    assert np.all(got["n_valid"] > 0) and np.all(got["max_sd"] > 0)


def test_cli_prints_the_largest_and_the_median(hip_device, bin_dir, mirror):  # noqa: F811
    corners, got, q = mirror
    exe = M._exe(bin_dir, "examples/calibrate_from_corners.cpp")
    plain = M._run_child([exe, corners, bin_dir / "cov.yaml", "--fix", "cx,cy", "--covariance"], bin_dir)
    r = M._run_child([exe, corners, bin_dir / "unc.yaml", "--fix", "cx,cy", "--uncertainty", f"{STEP!r},{INV!r}"], bin_dir)
    assert plain.returncode in (0, 3) and r.returncode == plain.returncode, (plain.stderr[-1000:], r.stderr[-1000:])
    # the option implies --covariance; its lines come behind the existing output; the YAML is unchanged
    assert r.stdout.startswith(plain.stdout) and "uncertainty" not in plain.stdout
    assert open(bin_dir / "cov.yaml").read() == open(bin_dir / "unc.yaml").read()
    cams = re.findall(r"^uncertainty camera_(\d+) sd_worst max (\S+) median (\S+) valid (\d+)$", r.stdout, re.M)
    pairs = re.findall(r"^uncertainty camera_(\d+)->camera_(\d+) sd_across max (\S+) median (\S+) valid (\d+)$", r.stdout, re.M)
    C = q.n_cameras
    assert len(cams) == C and len(pairs) == len(got["requests"]) - C
    rows = [(int(m), int(m), mx, med, nv) for m, mx, med, nv in cams] + [(int(a), int(b), mx, med, nv) for a, b, mx, med, nv in pairs]
    for k, (a, b, mx, med, nv) in enumerate(rows):
        assert (a, b) == got["requests"][k][:2] and int(nv) == got["n_valid"][k]
        v = np.sort(got["planes"][k, 5 if a == b else 6].ravel())
        v = v[~np.isnan(v)]
        assert float(mx) == v[-1] and float(med) == v[v.size // 2], (a, b)
        if a == b:
            assert float(mx) == got["max_sd"][k]
