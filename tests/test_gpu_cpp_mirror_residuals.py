"""The residual report through include/tscm/tscm_calib.hpp on the GPU: MultiCalib::residual_report(), called by
tests/native/mirror_residuals.cpp behind the flow of examples/calibrate_from_corners.cpp, gives the bytes of
api.residual_report on the same problem; tscm::view_outliers gives the flags of api.view_outliers; MultiCalib::prune_views
names those views and the calibrate() behind it is the solve with their weights 0.  Built and run the way
tests/test_gpu_cpp_mirror_covariance.py does (one fresh child at a time, none after an abnormal end)."""
import numpy as np
import pytest

from tests import test_gpu_cpp_mirror as M
from tests.test_gpu_cpp_mirror import bin_dir  # noqa: F401  (fixture)
from tscm_calib_amd import api, calib_io, synth
from tscm_calib_amd.problem import Problem

pytestmark = pytest.mark.gpu
K, MAX_FRACTION = 1.5, 0.25


@pytest.fixture(scope="module")
def mirror(hip_device, bin_dir):  # noqa: F811
    p = synth.make_problem(4, 30, 99, noise_px=0.1)                 # the rig of the covariance mirror test
    inp = synth.make_rig_input(p)
    corners = str(bin_dir / "corners.txt")
    calib_io.write_corners(corners, inp.has, inp.pix_u, inp.pix_v, 9, 6, 45.0)
    out = str(bin_dir / "residuals.bin")
    r = M._run_child([M._exe(bin_dir, "tests/native/mirror_residuals.cpp"), corners, out, K, MAX_FRACTION], bin_dir)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(out, "rb").read()
    C, B, V, N = (int(x) for x in np.frombuffer(raw, np.int32, 4))
    at = [16]

    def take(dtype, *shape):
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at[0]).reshape(shape)
        at[0] += a.nbytes
        return a
    got = dict(cam_rt=take(np.float64, C, 6), intr=take(np.float64, C, 9), board_rt=take(np.float64, B, 6), init=take(np.int32, B),
               view_camera=take(np.int32, V), view_board=take(np.int32, V), view_worst=take(np.int32, V), flags=take(np.int32, V),
               corner=take(np.float64, N, 6), view=take(np.float64, V, 8), camera=take(np.float64, C, 8))
    got["cost"], got["rmse"] = take(np.float64, 2)
    got.update(grid_count=take(np.int64, C, 3, 4, 2), angle_count=take(np.int64, C, 8, 2), grid_outside=take(np.int64, C), angle_outside=take(np.int64, C),
               grid=take(np.float64, C, 3, 4, 3), angle=take(np.float64, C, 8, 4))
    n_pairs = int(take(np.int32, 1)[0])
    got["pruned"] = take(np.int32, n_pairs, 2)
    got["rmse_first"], got["rmse_second"] = take(np.float64, 2)
    assert at[0] == len(raw)
    # MultiCalib::calibrate's problem: camera-major views of the initialised boards (tscm_calib.hpp: joint_problem)
    cams, boards = np.nonzero(inp.has.astype(bool) & got["init"].astype(bool)[None, :])
    n = inp.n_points
    const = np.zeros(C, np.uint8); const[0] = 1
    q = Problem(C, B, inp.worlds[:, :2].copy(), cams.astype(np.int32), boards.astype(np.int32), (np.arange(cams.size) * n).astype(np.int32),
                np.full(cams.size, n, np.int32), inp.pix_u[cams, boards].ravel().copy(), inp.pix_v[cams, boards].ravel().copy(),
                got["cam_rt"].copy(), got["intr"].copy(), got["board_rt"].copy(), const, False).normalised()
    return got, q


def test_multicalib_report_equals_api_report(hip_device, mirror):
    got, q = mirror
    assert np.array_equal(got["view_camera"], q.view_camera) and np.array_equal(got["view_board"], q.view_board)
    want = api.residual_report(q, hip_device, grid=(4, 3), image_size=(int(synth.IMG_W), int(synth.IMG_H)), angle_bins=8, max_angle=2.4)
    for key in ("corner", "view", "view_worst", "camera", "grid_count", "grid", "angle_count", "angle", "grid_outside", "angle_outside"):
        M._assert_same(got[key], want[key], key)
    assert got["cost"] == want["cost"] and got["rmse"] == want["rmse"]


def test_view_outliers_and_prune_views_agree_with_python(hip_device, mirror):
    got, q = mirror
    flags = api.view_outliers(dict(view=got["view"]), q, k=K, max_fraction=MAX_FRACTION)
    assert flags.any() and np.array_equal(got["flags"].astype(bool), flags)
    assert np.array_equal(got["pruned"], np.stack([q.view_camera[flags], q.view_board[flags]], axis=1))
    # the calibrate() behind prune_views: the solve from those parameters with the flagged views' weights 0
    s = api.calibrate(q, hip_device, weights=api.prune_weights(q, None, views=flags))
    assert s["rmse"] == got["rmse_second"] and got["rmse_second"] < got["rmse_first"]


def test_cli_prints_the_report_and_prunes(hip_device, bin_dir, mirror):  # noqa: F811
    import re
    got, q = mirror
    corners = str(bin_dir / "corners.txt")
    exe = M._exe(bin_dir, "examples/calibrate_from_corners.cpp")
    plain = M._run_child([exe, corners, bin_dir / "plain.yaml"], bin_dir)
    rep = M._run_child([exe, corners, bin_dir / "rep.yaml", f"--residuals={bin_dir / 'rep.txt'}", "--residual-bins", "8"], bin_dir)
    assert plain.returncode in (0, 3) and rep.returncode == plain.returncode, (plain.stderr[-1000:], rep.stderr[-1000:])
    # the report goes to the file: the output and the YAML are those of a run without the options
    assert rep.stdout == plain.stdout and open(bin_dir / "plain.yaml").read() == open(bin_dir / "rep.yaml").read()
    text = open(bin_dir / "rep.txt").read()
    rows = re.findall(r"^view (\d+) camera (\d+) board (\d+) corners (\d+) rms (\S+) max (\S+) worst (-?\d+)$", text, re.M)
    assert len(rows) == q.n_views
    for v, m, b, n, rms, mx, worst in rows:
        v = int(v)
        assert (int(m), int(b), int(n), int(worst)) == (q.view_camera[v], q.view_board[v], got["view"][v, 0], got["view_worst"][v])
        assert rms == "%.6f" % got["view"][v, 2] and mx == "%.6f" % got["view"][v, 4]
    assert len(re.findall(r"^camera_\d+ angle ", text, re.M)) == 8 * q.n_cameras
    # --prune: the views prune_views names leave, the joint solve runs again, the report is the pruned problem's
    pr = M._run_child([exe, corners, bin_dir / "pruned.yaml", "--prune", f"{K},1,{MAX_FRACTION}", "--residuals"], bin_dir)
    assert pr.returncode == plain.returncode, pr.stderr[-1000:]
    named = [(int(m), int(b)) for m, b in re.findall(r"^prune round 1: camera (\d+) board (\d+)$", pr.stdout, re.M)]
    assert named == [tuple(x) for x in got["pruned"].tolist()] and len(named) > 0
    assert re.search(r"^pruned solve 1: .* rmse %.4f px$" % got["rmse_second"], pr.stdout, re.M)
    assert len(re.findall(r"^view \d+ camera ", pr.stdout, re.M)) == q.n_views - len(named)
    assert open(bin_dir / "plain.yaml").read() != open(bin_dir / "pruned.yaml").read()
