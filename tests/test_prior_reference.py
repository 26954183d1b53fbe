"""Gaussian priors on camera parameters, without a GPU: the host plan (tscm_spec.h: check_camera_priors, effective_priors;
plan_exec's `priors` input) through tests/native/prior_check.cpp, and the reference of tests/prior_ref.py against finite
differences, against a direct solve of the first LM step, and on the problem the GPU's whole-solve test uses."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import api, lib, synth
from tests import helpers as H
from tests import native_check as N
from tests import prior_ref as PR

E_INVALID = -1

pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("prior_check.cpp", "prior_check")


def test_refusals(checker):
    r = N.run(checker, "refusals")
    size = "priors: struct_size is not sizeof(tscm_camera_priors)"
    bad_w = "is negative, NaN or infinite"
    bad_m = "is not finite where its weight is > 0"
    assert r == {
        "null": [0, ""], "ok": [0, ""], "ok_no_arrays": [0, ""],
        "struct_size": [E_INVALID, size], "struct_size_zero": [E_INVALID, size],
        "cam_mean_alone": [E_INVALID, "priors: cam_rt_mean is given without its cam_rt_weight"],
        "cam_weight_alone": [E_INVALID, "priors: cam_rt_weight is given without its cam_rt_mean"],
        "intr_mean_alone": [E_INVALID, "priors: intr_mean is given without its intr_weight"],
        "intr_weight_alone": [E_INVALID, "priors: intr_weight is given without its intr_mean"],
        "w_negative": [E_INVALID, f"priors: intr_weight[13] (camera 1, coordinate 4) {bad_w}"],
        "w_nan": [E_INVALID, f"priors: cam_rt_weight[7] (camera 1, coordinate 1) {bad_w}"],
        "w_inf": [E_INVALID, f"priors: intr_weight[2] (camera 0, coordinate 2) {bad_w}"],
        "mean_nan_live": [E_INVALID, f"priors: intr_mean[9] (camera 1, coordinate 0) {bad_m}"],
        "mean_inf_live": [E_INVALID, f"priors: intr_mean[17] (camera 1, coordinate 8) {bad_m}"],
        "mean_nan_dead": [0, ""],
        "w_beyond_n": [E_INVALID, f"priors: intr_weight[17] (camera 1, coordinate 8) {bad_w}"], "one_camera": [0, ""],
    }


def _table_problem():
    """prior_check's `table` example as a Problem: 3 cameras, camera 0's pose constant, camera 2 without a view"""
    p = synth.make_problem(3, 2, 11)
    keep = np.asarray(p.view_camera) != 2
    cnt = np.where(keep, p.view_count, 0).astype(np.int32)
    p.view_count = cnt
    p.cam_pose_constant = np.array([1, 0, 0], dtype=np.uint8)
    return p.normalised()


def test_effective_weights_against_the_host_plan(checker):
    """effective_priors on plan_columns' free columns gives what prior_ref.effective gives from tscm.h's rules on the problem:
    the pose of a constant camera, held intrinsics, b and c, and a camera without corners carry no prior."""
    p = _table_problem()
    C = 3
    cw = np.tile(np.arange(1.0, 7.0), (C, 1))
    cm = 100.0 * np.arange(C)[:, None] + np.arange(6.0)
    iw = np.tile(np.arange(7.0, 16.0), (C, 1))
    im = 100.0 * np.arange(C)[:, None] + 6.0 + np.arange(9.0)
    pr = lib.CameraPriors(cm, cw, im, iw)
    fixed = np.array([0, lib.FIX["cx"] | lib.FIX["lambda"], 0], dtype=np.uint16)
    w, mu = PR.effective(p, pr, fixed)
    r = N.run(checker, "table")
    got_w, got_m = np.array(r["weight"]).reshape(C, 16), np.array(r["mean"]).reshape(C, 16)
    assert np.array_equal(got_w[:, :15], w) and np.array_equal(got_m[:, :15], mu) and not got_w[:, 15].any()
    assert r["n"] == int(np.sum(w > 0)) == 7 + 6 + 5
    assert not w[0, :6].any() and not w[2].any() and not w[:, 13:].any() and w[1, 8] == 0 and w[1, 11] == 0 and w[1, 0] == 1


@pytest.mark.parametrize("seed", [1, 2])
def test_effective_weights_on_random_problems(checker, seed):
    r = N.run(checker, "effective", seed, 300)
    assert r["ok"], r
    assert min(r[k] for k in ("held", "const_pose", "mono", "inactive", "bc", "kept")) > 0 and r["cases"] > 200, r


def test_a_plan_with_priors_keeps_the_reductions_in_launches_of_their_own(checker):
    """plan_exec(priors = true) for rings of 1..32 cameras and random problems, both tiers, every exec_flags combination: the
    plan of TSCM_EXEC_SEPARATE_STATS (k_finalize_eval and k_control where k_reduce_control would run), and in the launch
    sequence every evaluation is followed by exactly one k_reduce_stats -- the one kernel that adds the prior."""
    r = N.run(checker, "plan", 5, 60)
    assert r["ok"], r
    assert r["would_ride"] > 0 and min(r["tails"]) > 0 and r["plans"] > 10000, r


def _priors(p, seed):
    """weights on every coordinate but a sixth of them, means off the parameters"""
    rng = np.random.default_rng(seed)
    C = p.n_cameras
    cw, iw = rng.uniform(0.5, 50.0, (C, 6)), rng.uniform(1e-4, 20.0, (C, 9))
    cw[rng.random((C, 6)) < 1 / 6] = 0.0
    iw[rng.random((C, 9)) < 1 / 6] = 0.0
    cm = p.cam_rt.reshape(C, 6) + rng.normal(0, 0.05, (C, 6))
    im = p.intr.reshape(C, 9) * (1 + rng.normal(0, 0.02, (C, 9))) + rng.normal(0, 0.01, (C, 9))
    return lib.CameraPriors(cm, cw, im, iw)


def test_gradient_against_finite_differences():
    p = H.small_rig(3, 4, seed=31).normalised()
    pr = _priors(p, 1)
    fixed = ("cy", "alpha")
    w, mu = PR.effective(p, pr, fixed)
    assert np.sum(w > 0) > 10 and not w[0, :6].any() and not w[:, 9].any()
    g = PR.prior_gradient(p, w, mu)
    x = PR.params(p)
    for m, k in zip(*np.nonzero(w > 0)):
        h = 1e-3 * max(1.0, abs(x[m, k]))       # (the prior is quadratic: the central difference is exact but for rounding, cost * eps / h)
        q0, q1 = p.copy().normalised(), p.copy().normalised()
        for q, s in ((q0, -h), (q1, h)):
            if k < 6:
                q.cam_rt[m, k] += s
            else:
                q.intr[m, k - 6] += s
        fd = (PR.prior_cost(q1, w, mu) - PR.prior_cost(q0, w, mu)) / (2 * h)
        assert abs(fd - g[m, k]) <= 1e-7 * max(1.0, abs(g[m, k])), (m, k, fd, g[m, k])
    # the normal equations: only the camera's own diagonal, gradient and the cost move
    o = H.oracle_normal_equations(p)
    a = PR.add_to_normal_equations(o, p, w, mu)
    assert all(a[k] is o[k] for k in ("board_gram", "board_grad", "view_cross"))
    d = a["cam_gram"] - o["cam_gram"]
    assert np.array_equal(d[:, np.arange(15), np.arange(15)] != 0, w > 0) and np.count_nonzero(d) == np.sum(w > 0)
    assert abs(a["cost"] - o["cost"] - PR.prior_cost(p, w, mu)) <= 1e-12 * a["cost"]


def _direct_step(p, cols, t, radius=1e4, lo=1e-6, hi=1e32):
    """The first LM step on the whole system [cameras x 13 | boards x 6] of the terms t, free columns only: Jacobi scaling and
    LM diagonal from the diagonal, one solve, no elimination (fp64).  -> (dcam [C,13], dboard [B,6])"""
    C, B = p.n_cameras, p.n_boards
    n = 13 * C + 6 * B
    A, g = np.zeros((n, n)), np.zeros(n)
    cnt, vc, vb = np.asarray(p.view_count), np.asarray(p.view_camera), np.asarray(p.view_board)
    for v in np.nonzero(cnt > 0)[0]:
        c0, b0 = 13 * vc[v], 13 * C + 6 * vb[v]
        A[c0:c0 + 13, c0:c0 + 13] += np.asarray(t["FF"][v], dtype=np.float64)
        A[b0:b0 + 6, b0:b0 + 6] += np.asarray(t["EE"][v], dtype=np.float64)
        A[b0:b0 + 6, c0:c0 + 13] += np.asarray(t["EF"][v], dtype=np.float64)
        A[c0:c0 + 13, b0:b0 + 6] += np.asarray(t["EF"][v], dtype=np.float64).T
        g[c0:c0 + 13] += np.asarray(t["Fr"][v], dtype=np.float64)
        g[b0:b0 + 6] += np.asarray(t["Er"][v], dtype=np.float64)
    free = np.r_[cols["cam_free"].ravel(), np.repeat(cols["board_free"], 6)]
    A, g = A[np.ix_(free, free)], g[free]
    nrm = np.diagonal(A).copy()
    s = 1.0 / (1.0 + np.sqrt(nrm))
    As = s[:, None] * A * s[None, :]
    As[np.arange(As.shape[0]), np.arange(As.shape[0])] += np.clip(s * s * nrm, lo, hi) / radius
    y = np.linalg.solve(As, s * g)
    d = np.zeros(n)
    d[free] = -s * y
    return d[:13 * C].reshape(C, 13), d[13 * C:].reshape(B, 6)


def test_first_step_reference_against_a_direct_solve():
    """helpers.reference_step on prior_ref.add_to_terms is the LM step of the stacked problem [J; sqrt(W)]: against one dense
    solve of the whole system with the prior on its diagonal and in its gradient.  With held intrinsics and a constant pose
    the priors there count for nothing."""
    p = H.small_rig(3, 5, seed=32).normalised()
    pr = _priors(p, 2)
    fixed = ("cx", "xi")
    w, mu = PR.effective(p, pr, fixed)
    cols = PR.columns(p, fixed)
    t0 = H.step_terms(p)
    t = PR.add_to_terms(t0, p, w, mu)
    ref = H.reference_step(p, terms=t, cols=cols)
    plain = H.reference_step(p, terms=t0, cols=cols)
    assert ref["ok"] and plain["ok"]
    dc, db = _direct_step(p, cols, t)
    scale = max(np.max(np.abs(dc)), np.max(np.abs(db)))
    assert np.max(np.abs(np.asarray(ref["cam"], dtype=np.float64) - dc)) <= 1e-8 * scale
    assert np.max(np.abs(np.asarray(ref["board"], dtype=np.float64) - db)) <= 1e-8 * scale
    assert np.max(np.abs(np.asarray(ref["cam"] - plain["cam"], dtype=np.float64))) > 1e-3 * np.max(np.abs(dc))     # the prior moves the step
    # all weights on columns that are not free: the plain step, bit for bit
    dead = lib.CameraPriors(pr.cam_rt_mean, np.where(np.arange(3)[:, None] == 0, pr.cam_rt_weight, 0.0), pr.intr_mean,
                            np.where(np.isin(np.arange(9), [2, 4, 7, 8])[None, :], pr.intr_weight, 0.0))
    w0, mu0 = PR.effective(p, dead, fixed)
    assert not w0.any() and not mu0.any()
    same = H.reference_step(p, terms=PR.add_to_terms(t0, p, w0, mu0), cols=cols)
    assert np.array_equal(same["cam"], plain["cam"]) and np.array_equal(same["board"], plain["board"])


def test_camera_priors_builder():
    p = H.small_rig(2, 3, seed=33).normalised()
    pr = api.camera_priors(p, intr_sigma={"xi": 0.1, "fx": 5.0}, cam_rt_sigma=[0.01, 0.01, 0.01, 2.0, 2.0, np.inf], pixel_sigma=0.5)
    assert np.array_equal(pr.intr_mean, p.intr) and np.array_equal(pr.cam_rt_mean, p.cam_rt)
    want = np.zeros((2, 9)); want[:, 4] = (0.5 / 0.1) ** 2; want[:, 0] = (0.5 / 5.0) ** 2
    assert np.array_equal(pr.intr_weight, want)
    assert np.array_equal(pr.cam_rt_weight, np.tile([2500.0, 2500.0, 2500.0, 0.0625, 0.0625, 0.0], (2, 1)))
    mean = p.intr + 1.0
    assert np.array_equal(api.camera_priors(p, intr_sigma={"alpha": 1.0}, mean={"intr": mean}).intr_mean, mean)
    none = api.camera_priors(p)
    assert none.intr_weight is None and none.cam_rt_weight is None
    with pytest.raises(ValueError):
        api.camera_priors(p, intr_sigma={"kappa": 1.0})
    with pytest.raises(ValueError):
        api.camera_priors(p, cam_rt_sigma=-1.0)
    with pytest.raises(ValueError):
        lib.CameraPriors(intr_mean=np.zeros(9), intr_weight=np.zeros(9)).c_struct(2)


def test_the_whole_solve_problem_tells_a_solve_with_priors_from_one_without():
    """prior_ref.whole_solve_problem: the SciPy optimum of the oracle's residuals WITH the prior rows differs in cost from the
    one WITHOUT by at least 100 times the 1e-4 band of test_oracle.py::test_lm_matches_scipy_optimum -- so the GPU test that asks
    for the first inside that band cannot be passed by a solve that ignores the priors."""
    p, pr = PR.whole_solve_problem()
    w, mu = PR.effective(p, pr)
    assert np.array_equal(np.nonzero(w[0])[0], [10, 11, 12]) and np.all(w[0, 10:13] == (1.0 / PR.SIGMA) ** 2)
    c0, q0 = PR.scipy_optimum(p)
    c1, q = PR.scipy_optimum(p, w, mu)
    print(f"optimum without priors {c0:.6f} (xi lambda alpha {q0.intr[0, 4:7]}), with {c1:.6f} ({q.intr[0, 4:7]}), prior means {mu[0, 10:13]}")
    assert abs(c1 - c0) >= 100 * PR.BAND * max(c0, c1), (c0, c1)
    # the augmented optimum is one: its pixel part is worse than the free optimum, its prior part is not zero and smaller than
    # the prior cost of the free optimum
    pix = orc.evaluate(q, jets=False)[0]
    assert abs(pix + PR.prior_cost(q, w, mu) - c1) <= 1e-9 * c1 and pix > c0
    assert 0 < PR.prior_cost(q, w, mu) < PR.prior_cost(q0, w, mu)


def test_the_rig_problem_tells_a_solve_with_pose_priors_from_one_without():
    p, pr, start = PR.whole_solve_rig()
    w, mu = PR.effective(p, pr)
    assert not w[0].any() and np.all(w[1, :6] > 0) and not w[1, 6:].any()
    c0, q0 = PR.scipy_optimum(p, start=start, method="lm")
    c1, q = PR.scipy_optimum(p, w, mu, start=start, method="lm")
    assert abs(PR.scipy_optimum(p, w, mu, start=start, method="trf", max_nfev=1000)[0] - c1) <= 1e-9 * c1
    print(f"rig optimum without priors {c0:.6f}, with {c1:.6f}")
    assert abs(c1 - c0) >= 100 * PR.BAND * max(c0, c1), (c0, c1)
    assert np.array_equal(q.cam_rt[0], p.cam_rt[0]) and 0 < PR.prior_cost(q, w, mu) < PR.prior_cost(q0, w, mu)


def test_pipeline_refuses_priors_on_the_batched_mono_route():
    from tscm_calib_amd import pipeline
    with pytest.raises(ValueError, match="batch_mono"):
        pipeline.calibrate_rig([], 9, 6, 30.0, batch_mono=True, priors=dict(intr_sigma={"xi": 0.1}))
    p = H.small_rig(2, 3, seed=33).normalised()
    assert pipeline._priors_kw(p, None) == {}
    kw = pipeline._priors_kw(p, dict(intr_sigma={"xi": 0.1}, pixel_sigma=0.2))
    assert np.array_equal(kw["priors"].intr_mean, p.intr) and kw["priors"].intr_weight[1, 4] == (0.2 / 0.1) ** 2
    with pytest.raises(ValueError, match="start values"):
        pipeline._priors_kw(p, dict(intr_sigma={"xi": 0.1}, mean={"intr": p.intr}))
