"""The residual report without a GPU (tscm.h: tscm_residual_report): the exports and every refusal through the
library, in the stated order; the reference (tests/residual_ref.py) against itself and against robust_ref; the negative
control -- the comparison of the GPU tests rejects every planted mistake; view_outliers / corner_outliers / prune_weights on
hand-made numbers; and the host plan's native check (tests/native/residual_plan_check.cpp)."""
import ctypes as C

import numpy as np
import pytest

from tests import native_check as N
from tests import residual_ref as RR
from tests import robust_ref
from tscm_calib_amd import api, lib, synth
from tscm_calib_amd.problem import Problem

LD = np.longdouble


def small(seed=5, cols=3, rows=2, views=4, noise=0.2):
    """2 cameras x `views` boards at the ground truth with `noise` px noise, then moved off the optimum: fx, fy, cx of every
    camera and every board's translation, so that the biases are not zero and the residuals stay around a pixel."""
    p = synth.make_problem(2, views, seed, cols=cols, rows=rows, perturb=False, noise_px=noise)
    p.intr[:, 0] *= 1.0 + 4e-4
    p.intr[:, 1] *= 1.0 - 3e-4
    p.intr[:, 2] += 0.3
    p.board_rt[:, 3] += 0.02 * (1 + np.arange(p.n_boards))
    return p


# ------------------------------------------------------------------------------------------------ the library, no GPU
def _call(p, weights=None, over=None, info_size=None, null=(), field_arrays=True):
    q = lib.CResidualParams()
    lib.lib().tscm_residual_default_params(C.byref(q))
    for k, v in (over or {}).items():
        setattr(q, k, v)
    info = lib.CResidualInfo(struct_size=C.sizeof(lib.CResidualInfo) if info_size is None else info_size)
    cp = lib.c_problem(p)
    gc, g = np.zeros(2 * p.n_cameras * 64 * 64, dtype=np.int64), np.zeros(3 * p.n_cameras * 64 * 64)
    ac, a = np.zeros(2 * p.n_cameras * 64, dtype=np.int64), np.zeros(4 * p.n_cameras * 64)
    llp = lambda x: x.ctypes.data_as(C.POINTER(C.c_longlong))
    rc = lib.lib().tscm_residual_report(None if "problem" in null else C.byref(cp), 0, lib.dptr(weights), None if "params" in null else C.byref(q),
                                        None, None, None, None, llp(gc) if field_arrays and "grid_count" not in null else None,
                                        lib.dptr(g) if field_arrays and "grid" not in null else None,
                                        llp(ac) if field_arrays and "angle_count" not in null else None,
                                        lib.dptr(a) if field_arrays and "angle" not in null else None, None if "info" in null else C.byref(info))
    return rc, lib.lib().tscm_last_error().decode()


def test_exports_and_defaults():
    L = lib.lib()
    for name in ("tscm_residual_default_params", "tscm_residual_report", "tscm_residual_debug_chunk_target"):
        assert name in lib.EXPORTS and getattr(L, name) is not None
    q = lib.CResidualParams()
    L.tscm_residual_default_params(C.byref(q))
    assert q.struct_size == C.sizeof(lib.CResidualParams) == 56
    assert (q.loss_kind, q.grid_w, q.grid_h, q.n_angle_bins, q.clamp) == (0, 0, 0, 0, 64.0) and q.max_angle == np.pi / 2
    assert C.sizeof(lib.CResidualInfo) == 40 + 2 * 32 * 8 + 32
    assert L.tscm_abi_version() == 6


GRID = dict(grid_w=4, grid_h=3, image_width=int(synth.IMG_W), image_height=int(synth.IMG_H))
REFUSALS = [
    ("problem", dict(null=("problem",)), "problem is NULL"),
    ("params", dict(null=("params",)), "params is NULL"),
    ("info", dict(null=("info",)), "info is NULL"),
    ("params_size", dict(over=dict(struct_size=48)), "struct_size"),
    ("info_size", dict(info_size=8), "info: struct_size"),
    ("loss_kind", dict(over=dict(loss_kind=7)), "loss_kind"),
    ("loss_scale", dict(over=dict(loss_kind=1, loss_scale=0.0)), "loss_scale"),
    ("loss_scale_nan", dict(over=dict(loss_kind=2, loss_scale=float("nan"))), "loss_scale"),
    ("grid_w", dict(over=dict(GRID, grid_w=65)), "grid_w"),
    ("grid_h", dict(over=dict(GRID, grid_h=-1)), "grid_w"),
    ("grid_half", dict(over=dict(GRID, grid_h=0)), "grid_w"),
    ("bins", dict(over=dict(n_angle_bins=65)), "n_angle_bins"),
    ("image", dict(over=dict(GRID, image_width=0)), "image_width"),
    ("max_angle", dict(over=dict(n_angle_bins=4, max_angle=4.0)), "max_angle"),
    ("max_angle_nan", dict(over=dict(n_angle_bins=4, max_angle=float("nan"))), "max_angle"),
    ("clamp", dict(over=dict(clamp=65.0)), "clamp"),
    ("clamp_zero", dict(over=dict(clamp=0.0)), "clamp"),
    ("clamp_inf", dict(over=dict(clamp=float("inf"))), "clamp"),
    ("grid_count", dict(over=GRID, null=("grid_count",)), "grid_count is NULL"),
    ("grid", dict(over=GRID, null=("grid",)), "grid is NULL"),
    ("angle_count", dict(over=dict(n_angle_bins=4), null=("angle_count",)), "angle_count is NULL"),
    ("angle", dict(over=dict(n_angle_bins=4), null=("angle",)), "angle is NULL"),
]


@pytest.mark.parametrize("name,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_before_any_device(name, kw, text):
    rc, msg = _call(small(), **kw)
    assert rc == -1 and text in msg, (rc, msg)


def test_refusals_of_the_problem_and_the_weights():
    p = small()
    bad = p.copy().normalised()
    bad.view_board[0] = 10 ** 6
    rc, msg = _call(bad)
    assert rc == -1 and msg.startswith("problem: ") and "view_board" in msg
    for value, at in ((-1.0, 3), (float("nan"), 0), (float("inf"), p.n_corners - 1)):
        w = np.ones(p.n_corners)
        w[at] = value
        rc, msg = _call(p, weights=w)
        assert rc == -1 and f"weights[{at}]" in msg, msg


def test_the_order_of_the_refusals():
    """one call that breaks several rules is refused by the first of tscm.h's list"""
    p = small()
    bad = p.copy().normalised()
    bad.view_board[0] = 10 ** 6
    w = -np.ones(p.n_corners)
    rc, msg = _call(bad, weights=w, over=dict(struct_size=48, loss_kind=9, clamp=0.0))
    assert "struct_size" in msg
    rc, msg = _call(bad, weights=w, over=dict(loss_kind=9, grid_w=99, clamp=0.0))
    assert "loss_kind" in msg
    rc, msg = _call(bad, weights=w, over=dict(grid_w=99, grid_h=2, n_angle_bins=4, max_angle=-1.0, clamp=0.0))
    assert "grid_w" in msg
    rc, msg = _call(bad, weights=w, over=dict(n_angle_bins=4, max_angle=-1.0, clamp=0.0))
    assert "max_angle" in msg
    rc, msg = _call(bad, weights=w, over=dict(clamp=0.0))
    assert "clamp" in msg
    rc, msg = _call(bad, weights=w, over=GRID, field_arrays=False)
    assert "grid_count is NULL" in msg
    rc, msg = _call(bad, weights=w)
    assert msg.startswith("problem: ")
    rc, msg = _call(p, weights=w)
    assert "weights[0]" in msg


def test_an_all_zero_view_is_not_refused():
    """unlike a solve: the call gets past every argument check (TSCM_E_NO_DEVICE without a GPU, TSCM_OK with one)"""
    p = small()
    w = np.ones(p.n_corners)
    w[:p.view_count[0]] = 0.0
    rc, msg = _call(p, weights=w, over=dict(GRID, n_angle_bins=8))
    if lib.lib().tscm_device_count() > 0:
        assert rc == 0, msg
    else:
        assert rc == -2 and "no HIP device" in msg, (rc, msg)
    with pytest.raises(ValueError):
        api.residual_report(p, weights=np.ones(3))


# ------------------------------------------------------------------------------------------------ the reference against itself
def test_weight_zero_equals_the_view_removed():
    p = small()
    n0 = int(p.view_count[0] + p.view_count[1])
    w = np.ones(p.n_corners)
    w[p.view_count[0]:n0] = 0.0                                     # view 1 out
    p_nan = p.copy().normalised()
    p_nan.obs_u[p.view_offset[1]:p.view_offset[1] + p.view_count[1]] = np.nan
    a = RR.report(p_nan, weights=w, grid=(4, 3), image_size=(synth.IMG_W, synth.IMG_H), angle_bins=6)
    keep = np.arange(p.n_views) != 1
    q = Problem(p.n_cameras, p.n_boards, p.board_xy, p.view_camera[keep], p.view_board[keep], p.view_offset[keep], p.view_count[keep],
                p.obs_u, p.obs_v, p.cam_rt, p.intr, p.board_rt, p.cam_pose_constant, False, meta={}).normalised()
    b = RR.report(q, grid=(4, 3), image_size=(synth.IMG_W, synth.IMG_H), angle_bins=6)
    rows = np.ones(p.n_corners, bool)
    rows[p.view_count[0]:n0] = False
    assert np.all(a["corner"][~rows] == 0) and np.array_equal(a["corner"][rows], b["corner"])
    assert np.array_equal(a["view"][keep], b["view"]) and np.all(a["view"][1] == 0) and a["view_worst"][1] == -1
    assert np.array_equal(a["camera"][:, :5], b["camera"][:, :5]) and np.array_equal(a["camera"][:, 6], b["camera"][:, 6])
    for k in ("grid_count", "grid", "angle_count", "angle", "grid_outside", "angle_outside"):
        assert np.array_equal(a[k], b[k]), k
    assert a["cost"] == b["cost"] and a["rmse"] == b["rmse"] and a["n_used"] == b["n_used"] == p.n_corners - int(p.view_count[1])


@pytest.mark.parametrize("kind", ["huber", "soft_l1", "cauchy"])
def test_cost_and_rho1_against_robust_ref(kind):
    p = small(views=6)
    ref = RR.report(p)
    scale = float(np.median(ref["err"]))
    r = RR.report(p, loss=(kind, scale))
    s = np.asarray(np.sum(ref["res"] ** 2, axis=1), dtype=np.float64)
    r0, r1, _ = robust_ref.rho(kind, scale, s)
    assert abs(float(r["cost"]) - 0.5 * r0.sum()) <= 1e-13 * float(r["cost"])
    assert np.max(np.abs(np.asarray(r["corner"][:, 5], dtype=np.float64) - r1)) <= 4e-16
    assert abs(float(r["cost"]) - robust_ref.robust_cost(np.asarray(ref["res"], dtype=np.float64), kind, scale)) <= 1e-13 * float(r["cost"])
    if kind == "huber":
        assert 0 < np.count_nonzero(s > scale * scale) < s.size      # both branches


def test_no_loss_gives_rho1_one_and_half_the_squares():
    p = small()
    r = RR.report(p)
    assert np.all(r["corner"][:, 5] == 1)
    assert abs(float(r["cost"] - LD(0.5) * np.sum(r["res"] ** 2))) <= 1e-18 * float(r["cost"])
    w = np.linspace(0.5, 2.0, p.n_corners)
    rw = RR.report(p, weights=w)
    assert abs(float(rw["cost"] - LD(0.5) * np.sum(w.astype(LD) * np.sum(r["res"] ** 2, axis=1)))) <= 1e-18 * float(rw["cost"])
    assert np.array_equal(rw["corner"], r["corner"])                 # weights scale no per-corner output


# ------------------------------------------------------------------------------------------------ the negative control
def control_case():
    """weights that differ, a clamp of 0.35 px that some corners exceed, a grid and bins; one corner moved 200 px"""
    p = small(seed=5, views=6)
    p.obs_u[p.view_offset[2] + 1] += 200.0
    w = 0.5 + (np.arange(p.n_corners) % 4).astype(np.float64)
    w[7] = 0.0
    return p, dict(weights=w, grid=(4, 3), image_size=(synth.IMG_W, synth.IMG_H), angle_bins=6, max_angle=1.2, clamp=0.35)


def test_the_comparison_accepts_the_reference():
    p, kw = control_case()
    ref = RR.report(p, **kw)
    RR.assert_separated(ref)
    ratios = RR.compare(RR.as_candidate(ref), ref)
    assert max(ratios.values()) <= 1.0
    assert ref["grid_count"][..., 1].sum() > 0 and ref["grid_count"][..., 0].sum() > 0      # the clamp splits the corners


@pytest.mark.parametrize("mistake", RR.MISTAKES)
def test_the_comparison_rejects_every_planted_mistake(mistake):
    p, kw = control_case()
    ref = RR.report(p, **kw)
    wrong = RR.as_candidate(RR.report(p, mistake=mistake, **kw))
    with pytest.raises(AssertionError):
        RR.compare(wrong, ref)


# ------------------------------------------------------------------------------------------------ flags and pruning, hand-made numbers
def _report_of(rms, n_used=None):
    view = np.zeros((len(rms), 8))
    view[:, 2] = rms
    view[:, 0] = 6 if n_used is None else n_used
    return dict(view=view)


def _views(cams):
    cams = np.asarray(cams, dtype=np.int32)
    z = np.zeros(cams.size, dtype=np.int32)
    return Problem(int(cams.max()) + 1, cams.size, np.zeros((6, 2)), cams, np.arange(cams.size, dtype=np.int32), z, z + 6, np.zeros(0), np.zeros(0),
                   np.zeros((int(cams.max()) + 1, 6)), np.zeros((int(cams.max()) + 1, 9)), np.zeros((cams.size, 6)), np.zeros(int(cams.max()) + 1, np.uint8))


def test_view_outliers_rule():
    # camera 0: ten views, median 1.05, MAD 0.15 -> threshold 1.05 + 3 * 1.4826 * 0.15 = 1.717; views 8, 9 beyond it
    rms = [0.9, 1.1, 0.9, 1.1, 1.0, 1.0, 0.8, 1.2, 5.0, 3.0]
    p = _views([0] * 10)
    assert np.array_equal(np.nonzero(api.view_outliers(_report_of(rms), p))[0], [8, 9])
    # the cap: floor(0.1 * 10) = 1 view, the worst first
    assert np.array_equal(np.nonzero(api.view_outliers(_report_of(rms), p, max_fraction=0.1))[0], [8])
    assert not api.view_outliers(_report_of(rms), p, max_fraction=0.05).any()
    # ties: two equal rms beyond the threshold and room for one: the lower view
    tie = [0.9, 1.1, 0.9, 4.0, 1.0, 1.0, 0.8, 1.2, 4.0, 1.0]
    assert np.array_equal(np.nonzero(api.view_outliers(_report_of(tie), p, max_fraction=0.1))[0], [3])
    # the floor: 5.0 and 3.0 stand out, only 5.0 is above 4 px
    assert np.array_equal(np.nonzero(api.view_outliers(_report_of(rms), p, floor=4.0))[0], [8])
    # a larger k moves the threshold: 1.05 + 15 * 1.4826 * 0.15 = 4.386
    assert np.array_equal(np.nonzero(api.view_outliers(_report_of(rms), p, k=15.0))[0], [8])


def test_view_outliers_edge_cases():
    # a camera with one view: median = its rms, nothing beyond it
    assert not api.view_outliers(_report_of([7.0]), _views([0])).any()
    # MAD = 0: every rms above the median is beyond the threshold; the cap still holds (floor(0.2 * 6) = 1)
    rms = [1.0, 1.0, 1.0, 1.0, 1.0, 1.5]
    assert np.array_equal(np.nonzero(api.view_outliers(_report_of(rms), _views([0] * 6)))[0], [5])
    assert not api.view_outliers(_report_of([1.0] * 6), _views([0] * 6)).any()
    # per camera, and views without used corners take no part (view 2 of camera 1 would otherwise be its worst)
    cams = [0, 1] * 6
    rms = [1.0, 2.0, 1.1, 9.0, 0.9, 2.1, 1.0, 1.9, 1.05, 2.0, 4.0, 2.05]
    used = [6, 6, 6, 0, 6, 6, 6, 6, 6, 6, 6, 6]
    flags = api.view_outliers(_report_of(rms, used), _views(cams), max_fraction=0.5)
    assert np.array_equal(np.nonzero(flags)[0], [10])


def test_corner_outliers_and_prune_weights():
    corner = np.zeros((5, 6))
    corner[:, 0] = [3.0, 0.0, 0.6, -3.0, 1.0]
    corner[:, 1] = [4.0, 0.0, 0.8, 4.0, 0.0]
    assert np.array_equal(api.corner_outliers(dict(corner=corner), 1.0), [True, False, False, True, False])      # |r| = 1 is not > 1
    p = small()
    n = p.view_count
    w = api.prune_weights(p, None, views=[1])
    assert w.dtype == np.float64 and w.sum() == p.n_corners - n[1] and np.all(w[n[0]:n[0] + n[1]] == 0)
    flags = np.zeros(p.n_views, bool); flags[[0, 3]] = True
    w0 = np.full(p.n_corners, 2.0)
    w = api.prune_weights(p, w0, views=flags, corners=[n[0] + 1])
    assert np.all(w0 == 2.0), "the input is left alone"
    assert np.all(w[:n[0]] == 0) and w[n[0] + 1] == 0 and w[n[0]] == 2.0 and w.sum() == 2.0 * (p.n_corners - n[0] - n[3] - 1)
    assert np.array_equal(api.prune_weights(p, w0, views=[], corners=np.zeros(p.n_corners, bool)), w0)
    q = p.copy()
    q.weights = np.full(p.n_corners, 3.0)
    assert np.all(api.prune_weights(q)[:] == 3.0)


# ------------------------------------------------------------------------------------------------ the host plan
checker = N.checker_fixture("residual_plan_check.cpp", "residual_plan_check")


def _plan_input(cases):
    out = [str(len(cases))]
    for C_, target, views in cases:
        out.append(f"{C_} {len(views)} {target}")
        out.extend(f"{m} {n}" for m, n in views)
    return "\n".join(out) + "\n"


@N.NEEDS_GXX
def test_plan_native_check(checker):
    N.assert_plain_cpp17("tscm_residual_plan.h")
    rng = np.random.default_rng(3)
    big = [(int(m), int(n)) for m, n in zip(rng.integers(0, 3, 200), rng.choice([0, 6, 54, 72, 88], 200))]
    cases = [
        (2, 100, [(0, 72), (1, 72), (0, 0), (1, 30), (0, 72), (0, 72), (1, 72)]),       # cuts at 100: one view per chunk but the short one
        (3, 0, [(0, 54), (2, 54), (0, 54)]),                                            # camera 1 without views, the default target
        (1, 50, [(0, 20), (0, 72), (0, 20), (0, 20), (0, 20)]),                         # one view larger than the target
        (2, 1, [(1, 6), (1, 6), (0, 6)]),                                               # every view a chunk
        (1, 10, []),                                                                    # no views at all
        (2, 10, [(0, 0), (1, 0)]),                                                      # no corners at all
        (3, 500, big), (3, 88, big), (3, 1 << 30, big),
    ]
    got = N.run(checker, "plan", stdin=_plan_input(cases))
    for (C_, target, views), r in zip(cases, got):
        assert r["rc"] == 0 and r["ok"], (C_, target)
        cam, cnt = np.array([v[0] for v in views], int), np.array([v[1] for v in views], int)
        assert r["N"] == cnt.sum() and r["view_first"] == [0] + list(np.cumsum(cnt))
        assert r["field_views"] == [int(v) for m in range(C_) for v in np.nonzero((cam == m) & (cnt > 0))[0]]
        assert r["cam_views"] == [int(v) for m in range(C_) for v in np.nonzero(cam == m)[0]]
    assert got[1]["chunk_camera"] == [0, 2]
    assert got[2]["chunk_begin"] == [0, 1, 2, 4] and got[2]["chunk_end"] == [1, 2, 4, 5]
    assert len(got[3]["chunk_begin"]) == 3 and got[4]["chunk_begin"] == [] and got[5]["field_views"] == []
    assert len(got[8]["chunk_begin"]) == 3                                               # a huge target: one chunk per camera
    assert N.run(checker, "refuse")["all"]
