"""calibrate_camera with RANSAC start poses: a garbage detection leaves the refinement, mislabelled rows are reported in
the masks, and without the option the function is the one it was."""
import numpy as np
import pytest

from tests import init_ransac_ref as Q
from tscm_calib_amd import api, pipeline, rig, synth
from tscm_calib_amd.problem import Problem

pytestmark = pytest.mark.gpu

COLS, ROWS, PITCH, SIZE = 9, 6, 45.0, (1280, 1080)
GARBAGE, SHIFTED = 3, (5, 9)


def _views():
    """12 views of the golden rig's camera 0 (0.1 px noise): clean, and with view 3 random pixels and a shifted row in 5, 9."""
    p = synth.make_problem(1, 12, 31, noise_px=0.1, perturb=False, cols=COLS, rows=ROWS, pitch=PITCH)
    n = COLS * ROWS
    pu, pv = p.obs_u.reshape(12, n).copy(), p.obs_v.reshape(12, n).copy()
    truth = p.meta["gt_intr"][0].copy()
    rng = np.random.default_rng(99)
    bu, bv, moved = pu.copy(), pv.copy(), np.zeros((12, n), dtype=bool)
    for k, kind in ((GARBAGE, "garbage"), (SHIFTED[0], "row_shift"), (SHIFTED[1], "row_shift")):
        bu[k], bv[k], moved[k] = Q.plant(rng, bu[k], bv[k], kind, COLS, truth)
    return truth, (pu, pv), (bu, bv), moved


def _model_distance(intr, truth):
    """RMS pixel distance of the two projections over a cone of 50 degrees: a distance of camera models that does not
    depend on how xi, lambda and alpha share the distortion."""
    th, ph = np.meshgrid(np.linspace(0.02, np.radians(50), 12), np.linspace(0, 2 * np.pi, 24, endpoint=False))
    P = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1).reshape(-1, 3) * 800.0
    ua, va, _ = synth.ts_project(np.asarray(intr, dtype=np.float64), P)
    ub, vb, _ = synth.ts_project(np.asarray(truth, dtype=np.float64), P)
    return float(np.sqrt(np.mean((ua - ub) ** 2 + (va - vb) ** 2)))


def test_garbage_view_is_dropped_and_shifted_rows_are_masked(hip_device):
    truth, clean, bad, moved = _views()
    has = np.ones(12, dtype=np.uint8)
    prm = rig.ransac_params(seed=0)
    loss = ("huber", 1.0)
    ci, cRt, cs = pipeline.calibrate_camera(*clean, has, COLS, ROWS, PITCH, SIZE, hip_device, loss=loss, ransac=prm)
    bi, bRt, bs = pipeline.calibrate_camera(*bad, has, COLS, ROWS, PITCH, SIZE, hip_device, loss=loss, ransac=prm)
    assert cs["ransac"]["has"].all() and cs["ransac"]["inlier"].all()
    f = bs["ransac"]
    assert f["code"][GARBAGE] not in (5, 6, 7) and not f["has"][GARBAGE] and not f["inlier"][GARBAGE].any()
    assert np.all(bRt[GARBAGE] == 0.0)                                        # no pose: the view was not in the refinement
    keep = np.arange(12) != GARBAGE
    assert f["has"][keep].all() and np.all(np.isin(f["code"][keep], (5, 6, 7)))
    assert np.array_equal(f["inlier"][keep], ~moved[keep])                    # exactly the shifted rows are out
    assert moved[SHIFTED[0]].sum() == moved[SHIFTED[1]].sum() == COLS
    assert bs["n_residual_blocks"] == 11 * COLS * ROWS
    d_clean, d_bad = _model_distance(ci, truth), _model_distance(bi, truth)
    print(f"\n[pipeline ransac] model distance to the truth: clean {d_clean:.4g} px, with outliers {d_bad:.4g} px")
    assert d_bad <= 2 * d_clean, (d_bad, d_clean)


def test_without_ransac_the_calls_are_todays(hip_device):
    truth, clean, bad, moved = _views()
    pu, pv = clean
    has = np.ones(12, dtype=np.uint8)
    has[7] = 0
    intr, Rt, s = pipeline.calibrate_camera(pu, pv, has, COLS, ROWS, PITCH, SIZE, hip_device, ransac=None)
    assert "ransac" not in s
    # the sequence calibrate_camera has always run: estimate_focal, estimate_extrinsic, poses, refinement
    n = COLS * ROWS
    W = pipeline.board_points(COLS, ROWS, PITCH)
    count = (has.astype(np.int32) * n).astype(np.int32)
    i0 = np.array([0.0, 0.0, SIZE[0] / 2 - 0.5, SIZE[1] / 2 - 0.5, 0.0, 0.0, 0.5, 0.0, 0.0])
    i0[0] = i0[1] = rig.estimate_focal(pu, pv, count, COLS, ROWS, i0[2], i0[3], hip_device)[0]
    Rt0, _ = rig.estimate_extrinsic(i0, pu, pv, count, W, COLS, hip_device)
    sel = np.flatnonzero(count > 0)
    V = sel.shape[0]
    q = Problem(1, V, W[:, :2].copy(), np.zeros(V, dtype=np.int32), np.arange(V, dtype=np.int32), (np.arange(V) * n).astype(np.int32),
                np.full(V, n, dtype=np.int32), pu[sel].ravel().copy(), pv[sel].ravel().copy(), np.zeros((1, 6)), i0[None, :].copy(),
                rig.poses_from_Rt(Rt0[sel]), np.ones(1, dtype=np.uint8), True).normalised()
    api.refinement(q, hip_device)
    R = synth.rodrigues(q.board_rt[:, :3])
    want = np.zeros((12, 3, 3))
    want[sel] = np.stack([R[:, :, 0], R[:, :, 1], q.board_rt[:, 3:]], axis=2)
    assert np.array_equal(intr, q.intr[0]) and np.array_equal(Rt, want)
