"""tscm_residual_report on the GPU against tests/residual_ref.py, on the smallest shapes that reach every path:
  a  2 cameras x 4 boards, 3 x 2 board (6 corners); one view with view_count 0, one partial view
  b  the same rig with a 9 x 8 board: 72 corners, the lanes stride
  c  a mono problem of 5 views (no camera pose)
  d  1 camera x 130 views of the 72-corner board, the plan's chunk target lowered: several field chunks per camera
Problems from synth.py at the ground truth with 0.2 px noise, then moved off the optimum (test_residual_reference.small).
Per-corner rows within 80 cond_ext 2^-53 of the row's scale, the sums within the summed bounds, every count and index exact
(residual_ref's docstring derives each bound; its assert_separated checks the preconditions of the exact ones on the CPU).
Every comparison prints its largest error / bound ratio."""
import numpy as np
import pytest

from tests import residual_ref as RR
from tests import robust_ref
from tests.test_residual_reference import small
from tscm_calib_amd import api, lib, pipeline, synth

pytestmark = pytest.mark.gpu
SIZE = (int(synth.IMG_W), int(synth.IMG_H))
ARRAYS = ("corner", "view", "view_worst", "camera", "grid_count", "grid", "angle_count", "angle", "grid_outside", "angle_outside")


def _nudge(p):
    p.intr[:, 0] *= 1.0 + 4e-4
    p.intr[:, 1] *= 1.0 - 3e-4
    p.intr[:, 2] += 0.3
    p.board_rt[:, 3] += 0.02 * (1 + np.arange(p.n_boards) % 7)
    return p


def _case(name):
    if name == "a":
        p = small(seed=5, cols=3, rows=2, views=4)
        p.view_count[2] = 0
        p.view_count[5] = 4
    elif name == "b":
        p = small(seed=5, cols=9, rows=8, views=4)
    elif name == "c":
        p = _nudge(synth.make_problem(1, 5, 11, cols=9, rows=8, perturb=False, noise_px=0.2))
    else:
        p = _nudge(synth.make_problem(1, 130, 12, cols=9, rows=8, perturb=False, noise_px=0.2))
    return p.normalised()


def _weights(p):
    """weights that differ from corner to corner, every seventh corner masked, and, in a problem of more than 5 views, view 1 all 0"""
    w = 0.5 + (np.arange(p.n_corners) % 4).astype(np.float64)
    w[3::7] = 0.0
    if p.n_views > 5:
        first = np.cumsum(p.view_count) - p.view_count
        w[first[1]:first[1] + p.view_count[1]] = 0.0
    return w


FIELD = dict(grid=(4, 3), image_size=SIZE, angle_bins=6, max_angle=2.4)       # the rig's fisheyes see 1.5 .. 2.6 rad: some corners beyond it
_ref_cache = {}


def _reference(name, weighted, **kw):
    """one reference per (case, options), shared by the tests that need it and left unchanged"""
    key = (name, weighted, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _ref_cache:
        p = _case(name)
        w = _weights(p) if weighted else None
        ref = RR.report(p, weights=w, **kw)
        RR.assert_separated(ref)
        _ref_cache[key] = (p, w, ref)
    return _ref_cache[key]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_report_against_reference(hip_device, name, weighted):
    p, w, ref = _reference(name, weighted, **FIELD)
    got = api.residual_report(p, hip_device, weights=w, **FIELD)
    RR.compare(got, ref, show=print)
    first = np.cumsum(p.view_count) - p.view_count
    for v in range(p.n_views):
        assert np.array_equal(got["corner_views"][v], got["corner"][first[v]:first[v] + p.view_count[v]])
    if name == "a":
        assert got["view"][2, 0] == 0 and got["view_worst"][2] == -1 and got["view"][5, 0] <= 4
    if weighted and p.n_views > 5:
        assert got["view"][1, 0] == 0 and got["view_worst"][1] == -1 and np.all(got["view"][1] == 0)
    assert got["n_used"] == ref["n_used"] and len(got["seconds_kernel"]) == 4


def test_clamp_and_a_planted_200_px_corner(hip_device):
    """a clamp of 0.35 px splits the corners; the corner moved by 200 px lands in n_clamped of the cell it is observed in"""
    p = _case("b")
    j = int(np.argmin(p.obs_u[p.view_offset[2]:p.view_offset[2] + p.view_count[2]]))
    at = int(p.view_offset[2]) + j
    p.obs_u[at] += 200.0
    assert p.obs_u[at] < SIZE[0] - 1                                 # still inside the image: a cell's n_clamped, not grid_outside
    kw = dict(FIELD, clamp=0.35)
    ref = RR.report(p, **kw)
    RR.assert_separated(ref)
    got = api.residual_report(p, hip_device, **kw)
    RR.compare(got, ref, show=print)
    assert got["grid_count"][..., 1].sum() > 0 and got["grid_count"][..., 0].sum() > 0
    full = api.residual_report(p, hip_device, **FIELD)                    # clamp 64: only the planted corner is beyond it
    m = int(p.view_camera[2])
    assert full["grid_count"][..., 1].sum() == 1 and full["grid_count"][m, ..., 1].sum() == 1 and full["angle_count"][m, :, 1].sum() == 1
    first = np.cumsum(p.view_count) - p.view_count
    assert full["view_worst"][2] == j and abs(full["corner"][first[2] + j, 0] - 200.0) < 5.0


def test_the_largest_grid(hip_device):
    """64 x 64 cells and 64 bins: the field kernel's tables take 130.5 KiB of LDS"""
    p, w, ref = _reference("b", True, grid=(64, 64), image_size=SIZE, angle_bins=64, max_angle=2.4)
    got = api.residual_report(p, hip_device, weights=w, grid=(64, 64), image_size=SIZE, angle_bins=64, max_angle=2.4)
    RR.compare(got, ref, show=print)


def _same_bytes(a, b, keys=ARRAYS):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    for k in ("cost", "rmse", "sum_w", "n_used", "n_views_used"):
        assert a[k] == b[k], k


def test_two_calls_and_two_chunkings_give_the_same_bytes(hip_device):
    p = _case("d")
    w = _weights(p)
    a = api.residual_report(p, hip_device, weights=w, **FIELD)
    _same_bytes(a, api.residual_report(p, hip_device, weights=w, **FIELD))
    try:
        for target in (500, 3000, 72):                               # 130 views x 72 corners: 22, 4 and 130 chunks
            lib.lib().tscm_residual_debug_chunk_target(target)
            _same_bytes(a, api.residual_report(p, hip_device, weights=w, **FIELD))
    finally:
        lib.lib().tscm_residual_debug_chunk_target(0)


def test_a_view_gives_the_same_bytes_wherever_it_sits(hip_device):
    p = _case("b")
    w = _weights(p)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    first = np.cumsum(p.view_count) - p.view_count
    q = p.copy().normalised()
    q.view_camera, q.view_board, q.view_offset, q.view_count = (x[perm].copy() for x in (p.view_camera, p.view_board, p.view_offset, p.view_count))
    rows = np.concatenate([np.arange(first[v], first[v] + p.view_count[v]) for v in perm])
    a = api.residual_report(p, hip_device, weights=w, loss=("huber", 0.3))
    b = api.residual_report(q, hip_device, weights=w[rows], loss=("huber", 0.3))
    assert a["corner"][rows].tobytes() == b["corner"].tobytes()
    assert a["view"][perm].tobytes() == b["view"].tobytes() and np.array_equal(a["view_worst"][perm], b["view_worst"])


def test_masked_corners_with_nan_observations(hip_device):
    p = _case("a")
    w = _weights(p)
    first = np.cumsum(p.view_count) - p.view_count
    w[first[1]:first[1] + p.view_count[1]] = 0.0                       # one view all 0
    view_of = np.repeat(np.arange(p.n_views), p.view_count)
    at = (p.view_offset[view_of] + np.arange(p.n_corners) - first[view_of])[w == 0]
    q = p.copy().normalised()
    q.obs_u[at] = np.nan
    q.obs_v[at] = np.inf
    a = api.residual_report(p, hip_device, weights=w, **FIELD)
    b = api.residual_report(q, hip_device, weights=w, **FIELD)
    _same_bytes(a, b)
    assert np.all(b["corner"][w == 0] == 0) and not np.signbit(b["corner"][w == 0]).any()
    assert b["view"][1, 0] == 0 and b["view_worst"][1] == -1 and np.all(b["view"][1] == 0)
    assert np.isfinite(b["view"]).all() and np.isfinite(b["camera"]).all() and np.isfinite(b["cost"])


def test_huber_rho1_and_cost(hip_device):
    p, w, ref0 = _reference("b", True)
    scale = 0.3
    ref = RR.report(p, weights=w, loss=("huber", scale))
    got = api.residual_report(p, hip_device, weights=w, loss=("huber", scale))
    RR.compare(got, ref, show=print)
    s = np.sum(got["corner"][:, :2] ** 2, axis=1)
    r1 = robust_ref.rho("huber", scale, s)[1]
    used = w > 0
    assert 0 < np.count_nonzero(s[used] > scale * scale) < used.sum()                  # both branches of Huber run
    assert np.max(np.abs(got["corner"][used, 5] - r1[used])) <= 8 * 2.0 ** -53
    want = api.normal_equations(p, hip_device, loss=("huber", scale), weights=w)["cost"]
    ratio = abs(got["cost"] - want) / (float(ref["cond_ext"].max()) * want)
    print(f"cost against normal_equations: {ratio:.3g} (bound 1e-13)")
    assert ratio <= 1e-13


def test_consistent_with_reprojection_error(hip_device):
    """b = c = 0 and no weights: camera.mean_err and info.rmse are tscm_reprojection_error's, within the summed bounds"""
    p, _, ref = _reference("b", False)
    assert np.all(p.intr[:, 7:] == 0)
    got = api.residual_report(p, hip_device)
    per, _, rmse = api.reprojection_error(p, hip_device)
    assert np.all(np.abs(got["camera"][:, 3] - per) <= 2 * np.asarray(ref["bound"]["camera"][:, 3], dtype=np.float64))
    assert abs(got["rmse"] - rmse) <= 2 * float(ref["bound"]["rmse"])


# ------------------------------------------------------------------------------------------------ pruning
def _shifted_rig():
    """2 cameras x 24 boards (54 corners) of known pose (board_pose_constant: the intrinsics and the rig's pose are solved),
    0.2 px noise; two views of camera 1 observed 3 px off.  With free boards the least squares shares a shifted view's 3 px with
    the other camera's view of the same board, which then stands out as much: of the seeds 1 .. 79 none flags exactly the two
    shifted views at k = 3 (the CPU oracle's solve), so the boards are held.  Seed 13: every view's rms is at least 0.05 px away
    from its camera's threshold, on either side."""
    p = synth.make_problem(2, 24, 13, perturb=False, noise_px=0.2)
    p.board_pose_constant = np.ones(p.n_boards, dtype=np.uint8)
    bad = np.nonzero(p.view_camera == 1)[0][[3, 17]]
    for v in bad:
        sl = slice(int(p.view_offset[v]), int(p.view_offset[v] + p.view_count[v]))
        p.obs_u[sl] += 3.0
    return p.normalised(), bad


def test_view_outliers_finds_the_shifted_views_and_pruning_is_the_sequence_by_hand(hip_device):
    p, bad = _shifted_rig()
    by_hand = p.copy().normalised()
    s0 = api.calibrate(by_hand, hip_device)
    rep = api.residual_report(by_hand, hip_device)
    flags = api.view_outliers(rep, by_hand, k=3.0)
    assert np.array_equal(np.nonzero(flags)[0], bad)
    w = api.prune_weights(by_hand, None, views=flags)
    s1 = api.calibrate(by_hand, hip_device, weights=w)
    final = api.residual_report(by_hand, hip_device, weights=w)
    # the pipeline's loop: the same calls
    q = p.copy().normalised()
    t0 = api.calibrate(q, hip_device)
    assert t0["final_cost"] == s0["final_cost"]
    pr = pipeline.prune_solve(q, lambda cw: api.calibrate(q, hip_device, weights=cw), hip_device, prune=dict(k=3.0))
    assert pr["prune_rounds"] == 1 and np.array_equal(pr["pruned_views"], flags) and not pr["pruned_corners"].any()
    assert np.array_equal(pr["weights"], w)
    for k in ("cam_rt", "intr", "board_rt"):
        assert getattr(q, k).tobytes() == getattr(by_hand, k).tobytes(), k
    assert pr["summaries"][-1]["final_cost"] == s1["final_cost"] and pr["summaries"][-1]["rmse"] == s1["rmse"]
    _same_bytes(pr["residuals"], final, keys=("corner", "view", "view_worst", "camera"))
    assert final["rmse"] < rep["rmse"] and s1["rmse"] < s0["rmse"]
    assert final["view"][bad, 0].sum() == 0 and final["n_views_used"] == p.n_views - 2
    # a second round finds nothing more: the loop ends without another solve
    again = pipeline.prune_solve(q, lambda cw: api.calibrate(q, hip_device, weights=cw), hip_device, weights=w, prune=dict(k=3.0, rounds=3, floor=1.0))
    assert again["prune_rounds"] == 0 and np.array_equal(again["weights"], w)
    with pytest.raises(TypeError):
        pipeline.prune_solve(q, None, hip_device, prune=dict(threshold=1.0))


def test_calibrate_rig_prune_is_the_sequence_by_hand(hip_device):
    from tests.test_gpu_pipeline import _render_rig
    images = _render_rig(31, 10)[2]
    prune = dict(k=1.0, max_fraction=0.3, angle_bins=8)
    plain = pipeline.calibrate_rig(images, 9, 6, 45.0, device=hip_device)
    assert "residuals" not in plain
    prob = plain["problem"]                                            # at the joint solve's parameters
    rep = api.residual_report(prob, hip_device)
    flags = api.view_outliers(rep, prob, k=1.0, max_fraction=0.3)
    assert flags.any()
    w = api.prune_weights(prob, None, views=flags)
    s1 = api.calibrate(prob, hip_device, weights=w)
    out = pipeline.calibrate_rig(images, 9, 6, 45.0, device=hip_device, prune=prune, covariance=True)
    assert out["prune_rounds"] == 1 and np.array_equal(out["pruned_views"], flags)
    for k in ("cam_rt", "intr", "board_rt"):
        assert getattr(out["problem"], k).tobytes() == getattr(prob, k).tobytes(), k
    assert out["summary"]["final_cost"] == s1["final_cost"] and out["summary"]["rmse"] < plain["summary"]["rmse"]
    final = api.residual_report(prob, hip_device, weights=w, angle_bins=8)
    _same_bytes(out["residuals"], final, keys=("corner", "view", "view_worst", "camera", "angle_count", "angle"))
    cov = api.covariance(prob, hip_device, weights=w)
    assert out["covariance"]["cam_cov"].tobytes() == cov["cam_cov"].tobytes() and out["covariance"]["n_residuals"] == 2 * int((w > 0).sum())


def test_calibrate_camera_prune_is_the_sequence_by_hand(hip_device):
    """the mono route: a garbage view and two views with a shifted row; the refinement behind the flags is api.refinement with
    the pruned weights, and without the keyword the result is today's"""
    from tests.test_gpu_pipeline_ransac import COLS, PITCH, ROWS, SIZE, _views
    _, _, bad, _ = _views()
    has = np.ones(12, dtype=np.uint8)
    prune = dict(k=3.0, max_fraction=0.25, corner_threshold=2.0, rounds=2)
    plain = pipeline.calibrate_camera(*bad, has, COLS, ROWS, PITCH, SIZE, hip_device, loss=("huber", 1.0))
    assert "residuals" not in plain[2]
    intr, Rt, s = pipeline.calibrate_camera(*bad, has, COLS, ROWS, PITCH, SIZE, hip_device, loss=("huber", 1.0), prune=prune)
    assert s["prune_rounds"] >= 1 and (s["pruned_views"].any() or s["pruned_corners"].any())
    # by hand from the pipeline's own preparation
    q, count, sel, _ = pipeline._prepare_camera(*bad, has, COLS, ROWS, PITCH, SIZE, hip_device, None, "ts", None)
    api.refinement(q, hip_device, loss=("huber", 1.0))
    w = None
    for _ in range(s["prune_rounds"]):
        rep = api.residual_report(q, hip_device, weights=w, loss=("huber", 1.0))
        fv = api.view_outliers(rep, q, 3.0, 0.0, 0.25)
        fc = api.corner_outliers(rep, 2.0) & ~np.repeat(fv, q.view_count)
        w = api.prune_weights(q, w, views=fv, corners=fc)
        _, last = api.refinement(q, hip_device, loss=("huber", 1.0), weights=w)
    hi, hRt = pipeline._finish_camera(q, count, sel)
    assert np.array_equal(hi, intr) and np.array_equal(hRt, Rt) and last["final_cost"] == s["final_cost"]
    assert np.array_equal(w == 0, s["pruned_corners"] | np.repeat(s["pruned_views"], q.view_count))
    assert s["rmse"] < plain[2]["rmse"] and s["residuals"]["n_used"] == int((w > 0).sum())
