"""The next-best-view stage through include/tscm/tscm_calib.hpp on the GPU: MultiCalib::view_gain() and view_gain_apply(),
called by tests/native/mirror_view_gain.cpp behind the flow of examples/calibrate_from_corners.cpp, give the bytes of
api.view_gain and api.view_gain_apply on the same problem, and `calibrate_from_corners --suggest` builds, runs and prints
its greedy choices behind the unchanged covariance report.  Built and run the way tests/test_gpu_cpp_mirror_covariance.py
does (one fresh child at a time, none after an abnormal end)."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import test_gpu_cpp_mirror as M
from tests.test_gpu_cpp_mirror import bin_dir  # noqa: F401  (fixture)
from tscm_calib_amd import api, calib_io, lib, synth
from tscm_calib_amd.problem import Problem

pytestmark = pytest.mark.gpu
MASK = lib.FIX["cx"] | lib.FIX["cy"]
BORDER, MIN_CORNERS = 10.0, 8


def test_multicalib_view_gain_equals_the_api(hip_device, bin_dir):  # noqa: F811
    p = synth.make_problem(4, 30, 99, noise_px=0.1)
    inp = synth.make_rig_input(p)
    corners = str(bin_dir / "corners.txt")
    calib_io.write_corners(corners, inp.has, inp.pix_u, inp.pix_v, 9, 6, 45.0)
    xy = inp.worlds[:, :2].copy()
    size = (int(synth.IMG_W), int(synth.IMG_H))
    # poses in the rig frame that do not depend on what the program solves: about the problem's start values
    cands = []
    for cam, pair in ((0, None), (1, 2), (3, 0)):
        cands += api.view_candidates(p.cam_rt, p.intr, cam, size, xy, grid=(3, 2), distances=(450.0,), tilts_deg=(0.0, 25.0), pair=pair)[0]
    arr = (lib.CViewCandidate * len(cands))()
    for k, (a, b, r) in enumerate(cands):
        arr[k].camera_a, arr[k].camera_b = a, b
        arr[k].board_rt[:] = [float(x) for x in r]
    cfile, out = str(bin_dir / "candidates.bin"), str(bin_dir / "view_gain.bin")
    with open(cfile, "wb") as f:
        f.write(np.array([len(cands), 0], np.int32).tobytes() + bytes(arr))
    r = M._run_child([M._exe(bin_dir, "tests/native/mirror_view_gain.cpp"), corners, cfile, out, MASK, repr(BORDER), MIN_CORNERS], bin_dir)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(out, "rb").read()
    Cn, B, R, _ = (int(x) for x in np.frombuffer(raw, np.int32, 4))
    at = [16]

    def take(dtype, *shape):
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at[0]).reshape(shape)
        at[0] += a.nbytes
        return a
    got = dict(cam_rt=take(np.float64, Cn, 6), intr=take(np.float64, Cn, 9), board_rt=take(np.float64, B, 6), init=take(np.int32, B),
               gain_logdet=take(np.float64, R), gain_trace=take(np.float64, R), n_visible=take(np.int32, R, 2), flags=take(np.int32, R))
    one = dict(gain_logdet=take(np.float64, 1), gain_trace=take(np.float64, 1), n_visible=take(np.int32, 2), flags=take(np.int32, 2)[0],
               cam_cov=take(np.float64, 15 * Cn, 15 * Cn))
    assert at[0] == len(raw) and R == len(cands) and C.sizeof(lib.CViewCandidate) == 56
    cams, boards = np.nonzero(inp.has.astype(bool) & got["init"].astype(bool)[None, :])
    V, n = cams.size, inp.n_points
    const = np.zeros(Cn, np.uint8); const[0] = 1
    q = Problem(Cn, B, xy, cams.astype(np.int32), boards.astype(np.int32), (np.arange(V) * n).astype(np.int32), np.full(V, n, np.int32),
                inp.pix_u[cams, boards].ravel().copy(), inp.pix_v[cams, boards].ravel().copy(), got["cam_rt"].copy(), got["intr"].copy(),
                got["board_rt"].copy(), const, False).normalised()
    cov = api.covariance(q, hip_device, fixed=np.full(Cn, MASK))
    want = api.view_gain(q.cam_rt, q.intr, cov, xy, size, cands, border=BORDER, min_corners=MIN_CORNERS, device=hip_device)
    for key in ("gain_logdet", "gain_trace", "n_visible", "flags"):
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
    assert ((got["flags"] & 3) == 3).any() and ((got["flags"] & 7) == 5).any() and np.all(got["gain_logdet"][(got["flags"] & 3) != 0] > 0)
    ap = api.view_gain_apply(q.cam_rt, q.intr, cov, xy, size, cands[0], border=BORDER, min_corners=MIN_CORNERS, device=hip_device)
    assert one["cam_cov"].tobytes() == ap["cam_cov"].tobytes() and one["flags"] == ap["flags"] and np.array_equal(one["n_visible"], ap["n_visible"])
    assert one["gain_logdet"][0] == ap["gain_logdet"] == got["gain_logdet"][0] and one["gain_trace"][0] == ap["gain_trace"]


def test_cli_suggest_builds_and_runs(hip_device, bin_dir):  # noqa: F811
    p = synth.make_problem(4, 30, 99, noise_px=0.1)
    inp = synth.make_rig_input(p)
    corners = str(bin_dir / "corners_cli.txt")
    calib_io.write_corners(corners, inp.has, inp.pix_u, inp.pix_v, 9, 6, 45.0)
    exe = M._exe(bin_dir, "examples/calibrate_from_corners.cpp")
    plain = M._run_child([exe, corners, bin_dir / "cov.yaml", "--fix", "cx,cy", "--covariance"], bin_dir)
    r = M._run_child([exe, corners, bin_dir / "sug.yaml", "--fix", "cx,cy", "--suggest", "3,400,800"], bin_dir)
    assert plain.returncode in (0, 3) and r.returncode == plain.returncode, (plain.stderr[-1000:], r.stderr[-1000:])
    # the option implies --covariance; its lines come behind the existing output; the YAML is unchanged
    assert r.stdout.startswith(plain.stdout) and "suggest" not in plain.stdout
    assert open(bin_dir / "cov.yaml").read() == open(bin_dir / "sug.yaml").read()
    rows = re.findall(r"^suggest (\d+) camera_(\d+)(?:\+camera_(\d+))? pixel (\S+) (\S+) distance (\S+) tilt (\S+) (\S+) gain_logdet (\S+) gain_trace (\S+) visible (\d+)(?:,(\d+))?$",
                      r.stdout, re.M)
    assert [int(x[0]) for x in rows] == list(range(len(rows))) and 1 <= len(rows) <= 3, r.stdout[-1500:]
    for x in rows:
        assert 0 <= int(x[1]) < 4 and float(x[5]) in (400.0, 800.0) and float(x[8]) > 0 and float(x[9]) > 0 and int(x[10]) + int(x[11] or 0) >= 8
        assert 0 <= float(x[3]) <= synth.IMG_W - 1 and 0 <= float(x[4]) <= synth.IMG_H - 1
    bad = M._run_child([exe, corners, bin_dir / "bad.yaml", "--suggest", "0"], bin_dir)
    assert bad.returncode == 2 and "--suggest" in bad.stderr
