"""The next-best-view stage on the GPU (tscm_view_gain, tscm_view_gain_apply) against the longdouble restatement
of tests/view_gain_ref.py.  Sigma comes from cov_ref (rounded to float64: the same input for the device and the
restatement), so Sigma's own error stays out; one end-to-end test takes it from api.covariance and compares with
api.covariance of the problem that really has the view.  Tolerance: a device gain may differ from the reference by
8 max(e64, n_terms 2^-52 amp) in view_gain_ref.gain_errors' measure, per output (view_gain_ref.tolerance);
tests/test_view_gain_reference.py shows on the CPU that this bound rejects every planted mistake.  Flags and visible counts
must be equal except at the (at most 1 %) candidates with a corner within 1e-9 of a visibility threshold.  Each test prints
its figures."""
import numpy as np
import pytest

from tests import cov_ref as CR
from tests import view_gain_ref as V
from tscm_calib_amd import api, pipeline

pytestmark = pytest.mark.gpu


def _run(inp, device, candidates=None):
    args, kw = V.call_args(inp)
    if candidates is not None:
        args = args[:5] + (candidates,)
    return api.view_gain(*args, device=device, **kw)


def _compare(label, got, ref, e64, amp, tol):
    same, near = V.discrete_agree(got, ref)
    e = V.gain_errors(got, ref)
    print(f"{label}: device error {e}, e64 {e64}, amp {amp}, tolerance {tol}, device / tolerance "
          f"{ {k: e[k] / tol[k] for k in tol} }, near candidates {near:.4f}, flags {dict(zip(*np.unique(got['flags'], return_counts=True)))}, "
          f"kernel {got['seconds_kernel']:.2e} s")
    assert same and near <= 0.01
    assert V.within(e, tol), (label, e, tol)
    use = ~ref["near"]
    numbers = (got["flags"] & 4) != 0
    assert np.all(got["gain_logdet"][use & numbers] >= 0) and np.all(got["gain_trace"][use & numbers] >= -tol["trace"] * ref["terms_trace"][use & numbers])
    none = (got["flags"] & 3) == 0
    assert np.all(got["gain_logdet"][none] == 0) and np.all(got["gain_trace"][none] == 0) and np.all((got["flags"][none] & 12) == 4)
    return e


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_view_gain_against_extended_precision(hip_device, name):
    """Sigma of rig4, mixed65 with cx, cy held, mixed65 with Double Sphere on camera 1 and mono7; boards of 6, 54 and 65 corners
    (one past a 64-lane pass); 1, 3 and 67 candidates (two launches, 13 and 26 columns, several workgroups each).  The 67 mix
    one camera and pairs, camera 0 (w = 0: the small-angle branch) and Rodrigues cameras, w_board = 0, boards fully visible,
    half outside, wholly outside and behind a camera, pairs of which one camera contributes, and visible counts of exactly
    min_corners and one less (tests/test_view_gain_reference.py checks that mix on the CPU)."""
    inp, ref, e64, amp, tol = V.case(name)
    got = _run(inp, hip_device)
    _compare(name, got, ref, e64, amp, tol)


def test_two_calls_give_the_same_bytes(hip_device):
    inp = V.case("rig4-54x67")[0]
    a, b = _run(inp, hip_device), _run(inp, hip_device)
    for key in ("gain_logdet", "gain_trace", "n_visible", "flags"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_a_candidates_bytes_do_not_depend_on_its_place(hip_device):
    """The same candidates first or last in the batch of 67, and alone: the same bytes (no dependence on the wave's slot)."""
    inp = V.case("mixed65-cx_cy-65x67")[0]
    cands = list(inp["candidates"])
    full = _run(inp, hip_device)
    turned = _run(inp, hip_device, cands[::-1])
    for key in ("gain_logdet", "gain_trace", "n_visible", "flags"):
        assert full[key].tobytes() == turned[key][::-1].tobytes(), key
    for i in (0, 37, 66):
        alone = _run(inp, hip_device, [cands[i]])
        for key in ("gain_logdet", "gain_trace", "n_visible", "flags"):
            assert alone[key][0].tobytes() == full[key][i].tobytes(), (key, i)


def _apply(inp, cand, cov, device):
    args, kw = V.call_args(inp)
    return api.view_gain_apply(args[0], args[1], cov, args[3], args[4], cand, device=device, **kw)


@pytest.mark.parametrize("name", ["rig4-54x67", "mixed65-ds1-6x67", "mono7-54x3"])
def test_apply_against_extended_precision(hip_device, name):
    """Sigma' of a one-camera candidate, a pair, a pair of which one camera contributes and a candidate nobody sees: against
    the reference's Sigma', symmetric, zero rows kept, the scalars the bytes of the batch call."""
    inp, ref, e64, amp, tol = V.case(name)
    args, kw = V.call_args(inp)
    batch = _run(inp, hip_device)
    fl = ref["flags"]
    a_ne_b = np.array([c[0] != c[1] for c in inp["candidates"]])
    picks = [int(np.nonzero(sel & ~ref["near"])[0][0]) for sel in ((fl & 3) == 1, (fl & 3) == 3, a_ne_b & ((fl & 3) == 1), (fl & 3) == 0) if (sel & ~ref["near"]).any()]
    S = np.asarray(inp["cam_cov"]).reshape(15 * inp["cam_rt"].shape[0], -1)
    for i in picks:
        cand = inp["candidates"][i]
        got = _apply(inp, cand, inp["cam_cov"], hip_device)
        r = V.candidate_ref(*args[:5], cand, **kw)
        r64 = V.candidate_ref(*args[:5], cand, dtype=np.float64, **kw)
        e, e64c = V.cov_error(got["cam_cov"], r["cam_cov"]), V.cov_error(r64["cam_cov"], r["cam_cov"])
        tol_c = V.tolerance(e64c, inp["board_xy"].shape[0], r["amp_logdet"])
        print(f"{name} candidate {i} flags {got['flags']}: Sigma' device error {e:.3e}, e64 {e64c:.3e}, amp {r['amp_logdet']:.3e}, tolerance {tol_c:.3e}")
        assert e <= tol_c
        out = got["cam_cov"].reshape(S.shape)
        assert np.array_equal(out, out.T)
        zero = ~S.any(axis=1)
        assert not out[zero].any() and not out[:, zero].any()
        if (got["flags"] & 3) == 0:
            assert out.tobytes() == S.tobytes()
        for key in ("gain_logdet", "gain_trace"):
            assert np.float64(got[key]).tobytes() == batch[key][i].tobytes(), key
        assert got["flags"] == batch["flags"][i]
        assert np.array_equal(got["n_visible"], batch["n_visible"][i])


def test_chain_rule_through_two_applies(hip_device):
    """gain(1) + gain(2 | Sigma after 1) == gain(2) + gain(1 | Sigma after 2) = log det Sigma - log det Sigma'': two orders of
    the same two views.  Both sums carry each gain's tolerance.  On mixed65 with Double Sphere on camera 1: the smallest
    eigenvalue of its correlation matrix (1.4e-9) is far above the error Sigma' carries there (1e-10; rig4's 4e-10 is not, and
    a second view on its Sigma' may answer with bit 3: DESIGN 29)."""
    inp, ref, e64, amp, tol = V.case("mixed65-ds1-6x67")
    fl = ref["flags"]
    i, j = [int(k) for k in np.nonzero(((fl & 3) == 3) & ~ref["near"])[0][:2]]
    c1, c2 = inp["candidates"][i], inp["candidates"][j]
    a1, a2 = _apply(inp, c1, inp["cam_cov"], hip_device), _apply(inp, c2, inp["cam_cov"], hip_device)
    a12, a21 = _apply(inp, c2, a1["cam_cov"], hip_device), _apply(inp, c1, a2["cam_cov"], hip_device)
    s12, s21 = a1["gain_logdet"] + a12["gain_logdet"], a2["gain_logdet"] + a21["gain_logdet"]
    bound = 4 * tol["logdet"] * max(s12, 1.0)
    print(f"chain rule: {s12!r} against {s21!r}, difference {abs(s12 - s21):.3e}, bound {bound:.3e}")
    assert abs(s12 - s21) <= bound and a12["gain_logdet"] <= a2["gain_logdet"] + bound
    assert V.cov_error(a12["cam_cov"], a21["cam_cov"]) <= 4 * tol["logdet"]


def test_end_to_end_against_a_covariance_that_has_the_view(hip_device):
    """The candidate appended to the rig4 problem as a new board -- one view per contributing camera, observations equal to
    the projections, invisible corners at corner weight 0 (the chosen pose has none, so that cov_ref, which knows no weights,
    can restate the augmented problem) -- and api.covariance of that problem, against view_gain_apply on api.covariance of
    the original problem; gain_logdet against the two slogdets over the free columns.  e64: the disagreement of the two
    routes' float64 restatements with their longdouble forms (the conditioning of the reduced system enters both)."""
    p, kw, ref1, e64_1, _ = CR.case("rig4")
    assert not kw, "the rig4 case is a plain solve"
    cov = api.covariance(p, hip_device)
    assert cov["status"] == 0
    size = np.tile(np.array([[V.IMG_W, V.IMG_H]], dtype=np.int32), (p.n_cameras, 1))
    xy = np.asarray(p.board_xy, dtype=np.float64)
    n = xy.shape[0]
    Ra, Rb = api._rotation_matrix(p.cam_rt[1, :3]), api._rotation_matrix(p.cam_rt[2, :3])
    pose = api.board_pose_facing(p.cam_rt[1], np.array([0.0, 0.0, 1.0]) + Ra @ Rb.T @ np.array([0.0, 0.0, 1.0]), 420.0, xy, tilt_x_deg=20.0, roll_deg=12.0)
    cand = (1, 2, pose)
    got = api.view_gain_apply(p.cam_rt, p.intr, cov, xy, size, cand, border=0.0, min_corners=8, device=hip_device)
    assert (got["flags"] & 15) == 7, got["flags"]
    # the augmented problem
    q = p.copy()
    views, us, vs, ws = [], [], [], []
    for c, m in enumerate(cand[:2]):
        if (got["flags"] >> c) & 1:
            visible = V.corner_rows(p.cam_rt, p.intr, m, pose, xy, size, 0.0)["visible"]
            uv = api.project(p.intr[m], _camera_points(p.cam_rt[m], pose, xy), hip_device)
            views.append(m); us.append(uv[:, 0]); vs.append(uv[:, 1]); ws.append(visible.astype(np.float64))
    q.board_rt = np.concatenate([np.asarray(p.board_rt), pose[None]])
    q.n_boards = p.n_boards + 1
    q.view_camera = np.concatenate([p.view_camera, views])
    q.view_board = np.concatenate([p.view_board, [p.n_boards] * len(views)])
    q.view_offset = np.concatenate([p.view_offset, p.n_corners + n * np.arange(len(views))])
    q.view_count = np.concatenate([p.view_count, [n] * len(views)])
    q.obs_u, q.obs_v = np.concatenate([p.obs_u] + us), np.concatenate([p.obs_v] + vs)
    if p.board_pose_constant is not None:
        q.board_pose_constant = np.concatenate([p.board_pose_constant, [0]])
    q = q.normalised()
    weights = np.concatenate([np.ones(p.n_corners)] + ws)
    assert weights.all(), "choose a pose every corner of which is visible"
    cov2 = api.covariance(q, hip_device, weights=weights)
    assert cov2["status"] == 0
    n15 = 15 * p.n_cameras
    S1, S2, Sa = cov["cam_cov"].reshape(n15, n15), cov2["cam_cov"].reshape(n15, n15), got["cam_cov"].reshape(n15, n15)
    free = np.nonzero(np.diag(S1) > 0)[0]
    ld = np.linalg.slogdet(S1[np.ix_(free, free)])[1] - np.linalg.slogdet(S2[np.ix_(free, free)])[1]
    # e64: this stage's restatement on the device's Sigma, and cov_ref's of both problems
    args = (p.cam_rt, p.intr, cov["cam_cov"], xy, size, cand)
    r, r64 = V.candidate_ref(*args), V.candidate_ref(*args, dtype=np.float64)
    e_stage = max(V.cov_error(r64["cam_cov"], r["cam_cov"]), abs(float(r64["gain_logdet"] - r["gain_logdet"])))
    jets = CR.H.orc.evaluate(q, jets=True)
    e64_2 = CR.cov_errors(CR.cov_ref(q, jets=jets, dtype=np.float64), CR.cov_ref(q, jets=jets))
    e64 = e_stage + CR.worst(e64_1) + CR.worst(e64_2)
    tol = V.tolerance(e64, n, r["amp_logdet"])
    err_cov, err_ld = V.cov_error(Sa, S2), abs(got["gain_logdet"] - ld) / max(ld, 1.0)
    print(f"end to end: Sigma' against the covariance with the view {err_cov:.3e}, gain_logdet {got['gain_logdet']!r} against slogdets {ld!r} ({err_ld:.3e}), "
          f"e64 {e64:.3e} (stage {e_stage:.3e}, covariance {CR.worst(e64_1):.3e} and {CR.worst(e64_2):.3e}), amp {r['amp_logdet']:.3e}, tolerance {tol:.3e}")
    assert err_cov <= tol and err_ld <= tol


def _camera_points(cam_rt_m, board_rt, xy):
    Rb, Rm = api._rotation_matrix(board_rt[:3]), api._rotation_matrix(cam_rt_m[:3])
    P = np.concatenate([xy, np.zeros((xy.shape[0], 1))], axis=1) @ Rb.T + board_rt[3:]
    return P @ Rm.T + np.asarray(cam_rt_m)[3:]


def test_plan_views_is_greedy(hip_device):
    """plan_views(n_views=3): every step's chosen gain is the batch maximum and the apply's gain; successive gains of the same
    candidate do not increase (information only shrinks what is left to gain), up to the tolerance."""
    inp, ref, e64, amp, tol = V.case("mixed65-ds1-6x67")
    args, kw = V.call_args(inp)
    steps = api.plan_views(*args, n_views=3, device=hip_device, **kw)
    assert len(steps) == 3
    prev = None
    for s in steps:
        sc = s["scores"]
        ok = (sc["flags"] & 4) != 0
        assert s["gain_logdet"] == sc["gain_logdet"][s["index"]] == sc["gain_logdet"][ok].max()
        if prev is not None:
            assert np.all(sc["gain_logdet"][ok] <= prev[ok] + 4 * tol["logdet"] * np.maximum(prev[ok], 1.0))
        prev = np.where(ok, sc["gain_logdet"], np.inf)
    print("plan_views:", [(s["index"], s["gain_logdet"], s["gain_trace"]) for s in steps])
    by_trace = api.plan_views(*args, n_views=1, criterion="gain_trace", device=hip_device, **kw)
    sc = by_trace[0]["scores"]
    assert by_trace[0]["gain_trace"] == sc["gain_trace"][(sc["flags"] & 4) != 0].max()


def test_pipeline_suggest_is_plan_views(hip_device):
    """calibrate_rig(..., suggest=dict(n_views, ...)) on the two-camera rendered rig of test_gpu_pipeline.py: implies the
    covariance; result["suggested_views"] is pipeline.suggest_views on the returned problem and covariance -- the candidates of
    each camera alone and of the pair (0, 1), planned greedily -- to the byte.  Without the argument the result has no such key."""
    import inspect
    from tests.test_gpu_pipeline import _render_rig
    _, _, images = _render_rig(31, 10)
    kw = dict(n_views=2, grid=(3, 2), distances=(400.0,), tilts_deg=(0.0, 25.0))
    out = pipeline.calibrate_rig(images, 9, 6, 45.0, device=hip_device, suggest=kw)
    views, cov = out["suggested_views"], out["covariance"]
    h, w = images[0][0].shape[:2]
    again = pipeline.suggest_views(out["problem"], cov, (w, h), device=hip_device, **kw)
    assert cov["status"] == 0 and 1 <= len(views) <= 2 and len(again) == len(views)
    for a, b in zip(views, again):
        assert a["board_rt"].tobytes() == b["board_rt"].tobytes() and (a["camera_a"], a["camera_b"]) == (b["camera_a"], b["camera_b"])
        assert a["gain_logdet"] == b["gain_logdet"] > 0 and a["gain_trace"] == b["gain_trace"] and (a["flags"] & 4)
        assert {"pixel", "distance", "tilt_x", "tilt_y", "roll", "n_visible"} <= set(a)
    print("rendered rig: suggested", [(v["camera_a"], v["camera_b"], v["pixel"], v["distance"], v["tilt_x"], v["tilt_y"], v["gain_logdet"]) for v in views])
    assert inspect.signature(pipeline.calibrate_rig).parameters["suggest"].default is None
