"""Gaussian priors on camera parameters on the GPU against the reference of tests/prior_ref.py.

1. Normal equations with priors (k_reduce_stats_prior behind both Gram tiers), without and with a loss, at the bounds of
   test_gpu_weights.py; the board blocks and view_cross keep the bits of the call without priors.
2. No priors, all-zero weights, weights on columns that are not free, and priors set and cleared: the plain solve, bit for bit.
3. The first trust-region step through each reduced-camera solver with priors on free and held intrinsics and on free and
   constant poses, under every exec_flags bit that leaves a plan with priors something to choose.
4. Whole solves -- the CPU-vetted mono problem (priors on xi, lambda, alpha) and a two-camera rig (priors on a pose) -- against
   the SciPy optimum of the augmented residuals.
5. Covariance with the prior in the blocks, the cost and the degrees of freedom.
6. Refusals and the two routes without priors (sharded solvers, the batched mono solve).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import api, lib, synth
from tests import cov_ref as CR
from tests import helpers as H
from tests import prior_ref as PR
from tests import robust_ref as R
from tests import weights_ref as W
from tests import test_gpu_step as S
from tests import test_gpu_weights as GW

pytestmark = pytest.mark.gpu

BOARD_BLOCKS = ("board_gram", "board_grad", "view_cross")


def scattered_priors(p, seed):
    """Priors on every coordinate of every camera but an eighth of them -- constant poses, b and c included, which must count for
    nothing -- about values one sigma or so off the problem's: sigma 2 px on fx fy cx cy, 0.02 on xi lambda alpha, 0.005 on
    rotations, 1 on translations."""
    rng = np.random.default_rng(seed)
    Cn = p.n_cameras
    isig = np.tile([2.0, 2.0, 2.0, 2.0, 0.02, 0.02, 0.02, 1.0, 1.0], (Cn, 1))
    csig = np.tile([0.005] * 3 + [1.0] * 3, (Cn, 1))
    isig[rng.random((Cn, 9)) < 0.125] = np.inf
    csig[rng.random((Cn, 6)) < 0.125] = np.inf
    mean = dict(intr=p.intr.reshape(Cn, 9) + rng.normal(0, 1, (Cn, 9)) * np.where(np.isfinite(isig), isig, 0.0),
                cam_rt=p.cam_rt.reshape(Cn, 6) + rng.normal(0, 1, (Cn, 6)) * np.where(np.isfinite(csig), csig, 0.0))
    return api.camera_priors(p, intr_sigma=isig, cam_rt_sigma=csig, mean=mean)


def mixed_fixed(p):
    """held intrinsics that differ between the cameras: camera 0 holds cx and lambda, the last camera alpha"""
    f = np.zeros(p.n_cameras, dtype=np.uint16)
    f[0] = lib.FIX["cx"] | lib.FIX["lambda"]
    f[-1] |= lib.FIX["alpha"]
    return f


# ----------------------------------------------------------------------------- 1. normal equations
@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["9x6", "11x8", "mono", "ragged"])
@pytest.mark.parametrize("kind", [None, "huber"])
def test_normal_equations(hip_device, kind, name, fp32):
    p, _, jets, a = GW._problem(name)
    pr = scattered_priors(p, 40 + len(name))
    w, mu = PR.effective(p, pr)
    assert np.sum(w > 0) >= (5 if p.mono else 8 * p.n_cameras) and (p.mono or not w[0, :6].any())
    plain = H.normal_equations_from(p, *jets[1:]) if kind is None else R.robust_normal_equations(p, kind, a, jets=jets)
    o = PR.add_to_normal_equations(plain, p, w, mu)
    assert o["cost"] > plain["cost"] * (1 + 1e-6)
    g = api.normal_equations(p, hip_device, jacobian_fp32=fp32, loss=GW._loss(kind, a), priors=pr)
    g0 = api.normal_equations(p, hip_device, jacobian_fp32=fp32, loss=GW._loss(kind, a))
    GW._check(g, o, p, fp32)
    for k in BOARD_BLOCKS:
        assert np.array_equal(g[k], g0[k]), k
    # the prior is exactly the difference to the call without: the diagonal, the gradient, the cost -- nothing off the diagonal
    d = g["cam_gram"] - g0["cam_gram"]
    idx = np.arange(15)
    off = d.copy(); off[:, idx, idx] = 0.0
    assert not off.any() and np.array_equal(d[:, idx, idx] != 0, w > 0)
    assert np.array_equal((g["cam_grad"] - g0["cam_grad"]) != 0, (w > 0) & (PR.params(p) != mu))
    # ... and a second call gives the same bytes
    g2 = api.normal_equations(p, hip_device, jacobian_fp32=fp32, loss=GW._loss(kind, a), priors=pr)
    assert all(np.array_equal(g[k], g2[k]) for k in GW.BLOCKS) and g["cost"] == g2["cost"]


def test_normal_equations_as_solved_take_the_solver_s_mask(hip_device):
    """tscm_solver_eval_normal_equations(as_solved) includes the solver's priors under its held intrinsics; releasing them
    re-derives the effective weights."""
    p = GW._problem("9x6")[0]
    pr = scattered_priors(p, 7)
    fixed = mixed_fixed(p)
    outs = lambda: dict(board_gram=np.zeros((p.n_boards, 6, 6)), cam_gram=np.zeros((p.n_cameras, 15, 15)), cam_grad=np.zeros((p.n_cameras, 15)))
    o = lib.default_options(False)
    got = []
    with api.Solver(p.copy().normalised(), hip_device, priors=pr) as s:
        for f in (fixed, None):
            s.set_fixed_intrinsics(f)
            b, cost = outs(), C.c_double(0.0)
            lib.check(lib.lib().tscm_solver_eval_normal_equations(s._h, C.byref(o), 1, lib.dptr(b["board_gram"]), None, None, lib.dptr(b["cam_gram"]),
                                                                   lib.dptr(b["cam_grad"]), C.byref(cost)))
            got.append((b, cost.value))
    plain = api.normal_equations(p, hip_device, as_solved=True)
    idx = np.arange(15)
    for (b, cost), f in zip(got, (fixed, None)):
        w, mu = PR.effective(p, pr, f)
        assert np.array_equal(b["board_gram"], plain["board_gram"])
        assert np.allclose(b["cam_gram"][:, idx, idx] - plain["cam_gram"][:, idx, idx], w, rtol=1e-9, atol=0) and np.array_equal((b["cam_gram"] - plain["cam_gram"])[:, idx, idx] != 0, w > 0)
        assert abs(cost - plain["cost"] - PR.prior_cost(p, w, mu)) <= 1e-12 * cost
    assert got[0][1] < got[1][1]


# ----------------------------------------------------------------------------- 2. zero is plain
@pytest.mark.parametrize("case_id", ["ring4", "ring6", "big12", "mono"])
def test_zero_is_plain_bit_for_bit(hip_device, case_id):
    p = S.problem(S.CASE_BY_ID[case_id][1]).normalised()
    Cn = p.n_cameras
    zero = lib.CameraPriors(np.ones((Cn, 6)), np.zeros((Cn, 6)), np.full((Cn, 9), np.nan), np.zeros((Cn, 9)))
    # weights only where no column is free: b and c, and the pose of the constant camera (every pose of a mono problem)
    iw = np.zeros((Cn, 9)); iw[:, 7:] = 3.0
    cw = np.zeros((Cn, 6)); cw[np.asarray(p.cam_pose_constant, dtype=bool) | bool(p.mono)] = 5.0
    dead = lib.CameraPriors(np.ones((Cn, 6)), cw, np.ones((Cn, 9)), iw)
    live = scattered_priors(p, 3)

    def run(priors=None, then=None):
        q = p.copy().normalised()
        with api.Solver(q, hip_device, priors=priors) as s:
            r = s.solve()
            if then is not None:
                q.cam_rt[:], q.intr[:], q.board_rt[:] = p.cam_rt, p.intr, p.board_rt
                s.set_camera_priors(then[0])
                r = s.solve()
        return r, q

    r0, q0 = run()
    assert cw.any() and r0["n_residual_blocks"] == p.n_corners
    rl, ql = run(live)
    assert rl["iterations"] != r0["iterations"] and rl["n_residual_blocks"] == p.n_corners
    for name, (r, q) in dict(zero=run(zero), dead=run(dead), cleared=run(live, then=(None,)), zeroed=run(live, then=(zero,))).items():
        for k in GW.SUMMARY_FIELDS:
            assert r[k] == r0[k], (name, k)
        assert np.array_equal(q.intr, q0.intr) and np.array_equal(q.cam_rt, q0.cam_rt) and np.array_equal(q.board_rt, q0.board_rt), name
    # the one-shot entry point with NULL priors is the legacy one
    q1 = p.copy().normalised()
    r1 = (api.refinement(q1, priors=None)[1] if p.mono else api.calibrate(q1, priors=None))
    assert r1["iterations"] == r0["iterations"] and np.array_equal(q1.intr, q0.intr)


# ----------------------------------------------------------------------------- 3. first step
def _step_check(hip_device, case, kind, p, pr, fixed, opt, tag):
    a = R.median_scale(p)
    ones = np.ones(p.n_corners)
    w, mu = PR.effective(p, pr, fixed)
    jets = W.weighted_jets(p, ones, kind, a)
    t = PR.add_to_terms(H.step_terms(p, jets=jets), p, w, mu)
    ref = H.reference_step(p, terms=t, cols=PR.columns(p, fixed), **{k: v for k, v in opt.items() if k not in ("exec_flags", "jacobian_fp32")})
    assert ref["ok"]
    g = api.step(p, hip_device, loss=GW._loss(kind, a), fixed=fixed, priors=pr, **opt)
    assert g["valid"]
    e = H.step_errors(p, ref, g)
    rc = H.reference_candidate(p, ref)
    q = p.copy().normalised()
    q.cam_rt[:], q.intr[:], q.board_rt[:] = rc["cam_rt"], rc["intr"], rc["board_rt"]
    cand = W.weighted_cost(orc.evaluate(q, jets=False)[1], ones, kind, a) + PR.prior_cost(q, w, mu)
    rd_ref = (ref["cost"] - cand) / ref["model_cost_change"]
    tau_b, tau_f, tau_rd = S.tolerances(case, ref["kappa"], ref["cost"], ref["model_cost_change"])
    it = g["summary"]["iterations"]
    print(f"[priors] {tag}: backward {e['backward']:.2e} (bound {tau_b:.0e}), forward {max(e[k] for k in e if k.startswith('forward')):.2e} ({tau_f:.1e}), "
          f"relative decrease {it[1]['relative_decrease']:.6f} against {rd_ref:.6f} ({tau_rd:.1e}), {int(np.sum(w > 0))} effective priors")
    assert e["backward"] <= tau_b, e
    for k in ("forward_cam_pose", "forward_intr", "forward_board"):
        assert not e[k] > tau_f, (k, e[k], tau_f)
    assert abs(it[0]["cost"] - ref["cost"]) <= 1e-12 * ref["cost"]
    assert abs(it[1]["relative_decrease"] - rd_ref) <= tau_rd * max(1.0, abs(rd_ref)), (it[1]["relative_decrease"], rd_ref, tau_rd)
    assert g["summary"]["n_residual_blocks"] == p.n_corners
    # held intrinsics and constant poses come back as they went in, whatever their priors say
    words = lib.fixed_masks(fixed, p.n_cameras)
    for m in range(p.n_cameras):
        for k in range(7):
            if (int(words[m]) >> k) & 1:
                assert g["intr"][m, k] == p.intr[m, k]
    return g, ref


def _step_inputs(case_id):
    case = S.CASE_BY_ID[case_id]
    p = S.problem(case[1]).normalised()
    pr = scattered_priors(p, 17)
    fixed = mixed_fixed(p)
    # (whatever the draw left out: priors on the held cx, lambda and alpha, on camera 0's pose and on the last camera's)
    pr.intr_weight[0, 2], pr.intr_weight[0, 5], pr.intr_weight[-1, 6] = 0.25, 2500.0, 2500.0
    pr.cam_rt_weight[0, :], pr.cam_rt_weight[-1, 3:] = 1.0, 1.0
    w_all = PR.effective(p, pr)[0]
    w = PR.effective(p, pr, fixed)[0]
    # the case mixes priors on held and free intrinsics and on a constant and a free pose
    assert np.sum(w_all > 0) > np.sum(w > 0) > 0 and pr.intr_weight[0, 2] > 0 and pr.intr_weight[0, 5] > 0
    if not p.mono:
        assert pr.cam_rt_weight[0].any() and np.asarray(p.cam_pose_constant)[0] and w[1:, :6].any() and not w[0, :6].any()
    return case, p, pr, fixed


@pytest.mark.parametrize("case_id", GW.STEP_CASES)
@pytest.mark.parametrize("kind", [None, "huber"])
def test_first_step(hip_device, kind, case_id):
    case, p, pr, fixed = _step_inputs(case_id)
    g, ref = _step_check(hip_device, case, kind, p, pr, fixed, dict(case[2]), f"{case_id} {kind}")
    # the prior moves the step: the reference without it is another one
    plain = H.reference_step(p, terms=H.step_terms(p, jets=W.weighted_jets(p, np.ones(p.n_corners), kind, R.median_scale(p))), cols=PR.columns(p, fixed))
    assert np.max(np.abs(np.asarray(ref["cam"] - plain["cam"], dtype=np.float64))) > 1e-6 * np.max(np.abs(np.asarray(plain["cam"], dtype=np.float64)))


# every exec_flags bit that leaves a solve with priors a choice (TSCM_EXEC_SEPARATE_STATS is what such a solve plans anyway;
# TSCM_EXEC_KEEP_SINGLE_RANK_COMM needs a communicator), and all of them together; 16x16 has no loss kernel
STEP_FLAGS = [lib.EXEC_SEPARATE_T_REDUCE, lib.EXEC_SEPARATE_BACKSUB, lib.EXEC_SEPARATE_CONTROL, lib.EXEC_SEPARATE_STATS, lib.EXEC_DENSE_REDUCED_ORDER,
              lib.EXEC_GRAPH_REDUCED_ORDER, lib.EXEC_GRAM_16X16,
              lib.EXEC_SEPARATE_T_REDUCE | lib.EXEC_SEPARATE_BACKSUB | lib.EXEC_SEPARATE_CONTROL | lib.EXEC_SEPARATE_STATS]


@pytest.mark.parametrize("case_id", ["ring4", "ring6", "big12", "mono"])
def test_first_step_under_exec_flags(hip_device, case_id):
    case, p, pr, fixed = _step_inputs(case_id)
    base = api.step(p, hip_device, fixed=fixed, priors=pr)
    same = 0
    for f in STEP_FLAGS:
        g, _ = _step_check(hip_device, case, None, p, pr, fixed, dict(case[2], exec_flags=f), f"{case_id} flags {f}")
        same += all(np.array_equal(g[k], base[k]) for k in ("cam_rt", "intr", "board_rt"))
    print(f"[priors] {case_id}: {same} of {len(STEP_FLAGS)} flag settings give the default launches' candidate bit for bit")


# ----------------------------------------------------------------------------- 4. whole solves
TIGHT = dict(function_tolerance=1e-14, gradient_tolerance=1e-14, parameter_tolerance=1e-14, max_num_iterations=200)


def _whole_solve(hip_device, p, pr, c_with, c_without):
    assert abs(c_with - c_without) >= 100 * PR.BAND * max(c_with, c_without)
    w, mu = PR.effective(p, pr)
    q = p.copy().normalised()
    with api.Solver(q, hip_device, priors=pr) as s:
        r = s.solve(**TIGHT)
        first = (q.cam_rt.copy(), q.intr.copy(), q.board_rt.copy())
        q.cam_rt[:], q.intr[:], q.board_rt[:] = p.cam_rt, p.intr, p.board_rt
        r2 = s.solve(**TIGHT)
    print(f"[priors] whole solve: final cost {r['final_cost']:.9f} in {r['num_iterations']} iterations ({r['message']}), SciPy with priors {c_with:.9f}, "
          f"without {c_without:.9f}; rmse {r['rmse']:.6f}")
    assert abs(r["final_cost"] - c_with) <= PR.BAND * c_with, (r["final_cost"], c_with)
    assert abs(r["final_cost"] - c_without) > PR.BAND * c_without
    # the cost is the pixel cost plus the prior's; the rmse is the pixels' alone
    assert abs(r["final_cost"] - (orc.evaluate(q, jets=False)[0] + PR.prior_cost(q, w, mu))) <= 1e-10 * r["final_cost"]
    assert abs(r["rmse"] - orc.rmse(q)) <= 1e-12 * orc.rmse(q)
    assert r["n_residual_blocks"] == p.n_corners
    for k in GW.SUMMARY_FIELDS:
        assert r2[k] == r[k], k
    assert all(np.array_equal(x, y) for x, y in zip(first, (q.cam_rt, q.intr, q.board_rt)))
    return r, q


def test_whole_solve_mono(hip_device):
    p, pr = PR.whole_solve_problem()
    w, mu = PR.effective(p, pr)
    c0 = PR.scipy_optimum(p)[0]
    c1 = PR.scipy_optimum(p, w, mu)[0]
    r, q = _whole_solve(hip_device, p, pr, c1, c0)
    # the one-shot entry point is the same solve
    q1 = p.copy().normalised()
    ok, r1 = api.refinement(q1, priors=pr, **TIGHT)
    assert r1["iterations"] == r["iterations"] and np.array_equal(q1.intr, q.intr) and np.array_equal(q1.board_rt, q.board_rt) and r1["rmse"] == r["rmse"]


def test_whole_solve_rig_with_pose_priors(hip_device):
    p, pr, start = PR.whole_solve_rig()
    w, mu = PR.effective(p, pr)
    c0 = PR.scipy_optimum(p, start=start, method="lm")[0]
    c1 = PR.scipy_optimum(p, w, mu, start=start, method="lm")[0]
    r, q = _whole_solve(hip_device, p, pr, c1, c0)
    assert np.array_equal(q.cam_rt[0], p.cam_rt[0])
    q1 = p.copy().normalised()
    r1 = api.calibrate(q1, priors=pr, **TIGHT)
    assert r1["iterations"] == r["iterations"] and np.array_equal(q1.cam_rt, q.cam_rt) and np.array_equal(q1.intr, q.intr)


# ----------------------------------------------------------------------------- 5. covariance
@pytest.mark.parametrize("fixed", [None, "mixed"])
def test_covariance(hip_device, fixed):
    p = H.small_rig(4, 8, seed=23).normalised()
    pr = scattered_priors(p, 5)
    f = mixed_fixed(p) if fixed else None
    w, mu = PR.effective(p, pr, f)
    n_prior = int(np.sum(w > 0))
    cam_free, board_free = CR.free_columns(p, f)
    idx = np.arange(15)

    def reference(dtype):
        blk = CR.blocks_from_terms(p, H.step_terms(p, dtype=dtype))
        blk["cam_gram"][:, idx, idx] += w.astype(dtype)
        return CR.cov_from_blocks(p.view_camera, p.view_board, blk["board_gram"], blk["view_cross"], blk["cam_gram"], cam_free, board_free, dtype), blk["cost"]

    ref, cost = reference(np.longdouble)
    e64 = CR.worst(CR.cov_errors(reference(np.float64)[0], ref))
    tol = CR.tolerance(e64, ref["n_free"])
    got = api.covariance(p, hip_device, fixed=f, priors=pr)
    plain = api.covariance(p, hip_device, fixed=f)
    err = CR.cov_errors({k: got[k] for k in ("cam_cov", "board_cov")}, ref)
    print(f"[priors] covariance fixed={fixed}: {n_prior} prior rows, error {err}, e64 {e64:.2e}, tolerance {tol:.2e}")
    assert got["status"] == 0 and CR.worst(err) <= tol, (err, tol)
    total = cost + PR.prior_cost(p, w, mu)
    assert got["n_residuals"] == 2 * p.n_corners + n_prior and got["n_free"] == ref["n_free"] == plain["n_free"]
    assert got["dof"] == 2 * p.n_corners + n_prior - got["n_free"] and plain["dof"] == 2 * p.n_corners - plain["n_free"]
    assert abs(got["cost"] - total) <= 1e-12 * total and got["sigma2"] == 2.0 * got["cost"] / got["dof"]
    # a prior only ever adds information: no variance of a camera column grows
    dg, dp = np.diagonal(got["cam_cov"].reshape(60, 60)), np.diagonal(plain["cam_cov"].reshape(60, 60))
    assert np.all(dg <= dp * (1 + 1e-9)) and np.any(dg < 0.9 * dp)
    sd = np.sqrt(got["sigma2"] * dg).reshape(4, 15)
    assert np.allclose(got["intr_std"], np.where(cam_free[:, 6:], sd[:, 6:], 0.0), rtol=1e-12) and np.array_equal(got["intr_std"] == 0, ~cam_free[:, 6:])
    again = api.covariance(p, hip_device, fixed=f, priors=pr)
    assert np.array_equal(again["cam_cov"], got["cam_cov"]) and np.array_equal(again["board_cov"], got["board_cov"]) and again["sigma2"] == got["sigma2"]


def test_covariance_of_a_parameter_only_the_prior_determines(hip_device):
    """A rig without a constant camera pose has a gauge freedom: the reduced system's smallest pivot is rounding.  Priors on one
    camera's pose fix the gauge, and its variance is finite."""
    p = S.problem("free_gauge3").normalised()
    free = api.covariance(p, hip_device)
    cw = np.zeros((3, 6)); cw[0] = [1e4, 1e4, 1e4, 1.0, 1.0, 1.0]
    pr = lib.CameraPriors(p.cam_rt.copy(), cw, None, None)
    got = api.covariance(p, hip_device, priors=pr)
    print(f"[priors] gauge: min_pivot_ratio {free['min_pivot_ratio']:.3e} (status {free['status']}) without priors, {got['min_pivot_ratio']:.3e} with")
    assert got["status"] == 0 and np.all(np.isfinite(got["cam_rt_std"])) and np.all(got["cam_rt_std"] > 0)
    assert free["status"] != 0 or got["min_pivot_ratio"] > 1e3 * free["min_pivot_ratio"]
    assert got["n_residuals"] == 2 * p.n_corners + 6


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals(hip_device):
    p = H.small_rig(4, 8, seed=22).normalised()
    good = scattered_priors(p, 6)

    def bad(**kw):
        d = dict(cam_rt_mean=good.cam_rt_mean.copy(), cam_rt_weight=good.cam_rt_weight.copy(), intr_mean=good.intr_mean.copy(), intr_weight=good.intr_weight.copy())
        for k, (i, v) in kw.items():
            if i is None:
                d[k] = None
            else:
                d[k].reshape(-1)[i] = v
        return lib.CameraPriors(**d)

    live = int(np.nonzero(good.intr_weight.reshape(-1) > 0)[0][0])
    cases = {"intr_weight[5]": bad(intr_weight=(5, -1.0)), "cam_rt_weight[7]": bad(cam_rt_weight=(7, np.nan)), "intr_weight[0]": bad(intr_weight=(0, np.inf)),
             f"intr_mean[{live}]": bad(intr_mean=(live, np.nan)), "intr_mean is given without": bad(intr_weight=(None, 0)),
             "cam_rt_weight is given without": bad(cam_rt_mean=(None, 0))}
    q = p.copy().normalised()
    with api.Solver(q, hip_device) as s:
        for text, pr in cases.items():
            for f in (lambda: s.set_camera_priors(pr), lambda: api.calibrate(q, priors=pr), lambda: api.step(q, hip_device, priors=pr),
                      lambda: api.normal_equations(q, hip_device, priors=pr), lambda: api.covariance(q, hip_device, priors=pr)):
                with pytest.raises(lib.TscmError) as e:
                    f()
                assert e.value.code == -1 and "priors" in str(e.value) and text in str(e.value), (text, str(e.value))
        # a refused call leaves the solver as it was: it still solves the plain problem
        assert s.solve()["n_residual_blocks"] == p.n_corners
        st = good.c_struct(4)
        st.struct_size -= 8
        rc = lib.lib().tscm_solver_set_camera_priors(s._h, C.byref(st))
        assert rc == -1 and "struct_size" in lib.lib().tscm_last_error().decode()
    assert np.array_equal(q.cam_rt[0], p.cam_rt[0])
    with pytest.raises(TypeError):
        api.calibrate(p.copy().normalised(), priors=dict(xi=0.1))


def test_routes_without_priors_refuse_them(hip_device):
    p = H.small_rig(4, 8, seed=22).normalised()
    pr = scattered_priors(p, 6)
    with api.Solver(p.copy().normalised(), hip_device, 0, 2) as s:
        with pytest.raises(lib.TscmError) as e:
            s.set_camera_priors(pr)
        assert e.value.code == -5 and "sharded" in str(e.value)
        s.set_camera_priors(None)               # clearing what was never set is not an error
    with pytest.raises(lib.TscmError) as e:
        api.Solver(p.copy().normalised(), hip_device, 1, 3, priors=pr)
    assert e.value.code == -5
    m, mpr = PR.whole_solve_problem()
    # the batched mono route has no priors argument in the C ABI: the Python layer refuses
    with pytest.raises(ValueError, match="batched mono route"):
        api.refinement_batch([m.copy().normalised()], hip_device, priors=[mpr])
