"""Reference of Gaussian priors on camera parameters (tscm.h: tscm_camera_priors), on top of the references of the loss and the
corner weights.

Every coordinate k of a camera's pose (6) or intrinsic (9) block with a weight w_k > 0 that is a free column of the solve is one
more residual sqrt(w_k) (x_k - mean_k): Jacobian sqrt(w_k), no loss.  So, with d = x - mean on the effective weights,
  cost      += 1/2 sum w d^2
  cam_gram  += diag(w)          (the camera's own 15 x 15 block; nothing else changes)
  cam_grad  += w d
and the first LM step is helpers.reference_step on terms whose FF, Fr and cost carry the prior of a camera in one of its live
views (they sum to the camera block; W = E^T F is left alone).
"""
import numpy as np

from oracle import pyoracle as orc
from tests import cov_ref as CR
from tests import helpers as H
from tscm_calib_amd import lib


def effective(p, priors, fixed=None):
    """(weight [C,15], mean [C,15]) in the column order pose 6 | fx fy cx cy xi lambda alpha b c: the weight 0 (and the mean 0
    with it) where the column is not free by tscm.h's rules (cov_ref.free_columns) or carries no prior."""
    C = p.n_cameras
    w, mu = np.zeros((C, 15)), np.zeros((C, 15))
    if priors is None:
        return w, mu
    if priors.cam_rt_weight is not None:
        w[:, :6], mu[:, :6] = priors.cam_rt_weight.reshape(C, 6), priors.cam_rt_mean.reshape(C, 6)
    if priors.intr_weight is not None:
        w[:, 6:], mu[:, 6:] = priors.intr_weight.reshape(C, 9), priors.intr_mean.reshape(C, 9)
    live = CR.free_columns(p, fixed)[0] & (w > 0.0)
    return np.where(live, w, 0.0), np.where(live, mu, 0.0)


def params(p):
    """x [C,15] of the problem: pose | intrinsics"""
    return np.concatenate([np.asarray(p.cam_rt, dtype=np.float64).reshape(-1, 6), np.asarray(p.intr, dtype=np.float64).reshape(-1, 9)], axis=1)


def prior_cost(p, w, mu, dtype=np.longdouble):
    d = (params(p) - mu).astype(dtype)
    return float(np.sum(w.astype(dtype) * d * d) / 2)


def prior_gradient(p, w, mu):
    """d cost / d x [C,15]"""
    return w * (params(p) - mu)


def add_to_normal_equations(o, p, w, mu):
    """The normal equations `o` (helpers.normal_equations_from's dict) with the effective priors added: a new dict, the board
    blocks and view_cross shared with `o`."""
    out = dict(o)
    cg, gr = np.array(o["cam_gram"], dtype=np.float64), np.array(o["cam_grad"], dtype=np.float64)
    k = np.arange(15)
    cg[:, k, k] += w
    gr += prior_gradient(p, w, mu)
    out.update(cam_gram=cg, cam_grad=gr, cost=float(np.longdouble(o["cost"]) + np.longdouble(prior_cost(p, w, mu))))
    return out


def add_to_terms(t, p, w, mu):
    """helpers.step_terms' dict with the prior of every camera in its first live view: FF diagonal, Fr and the cost."""
    out = dict(t)
    ld = t["FF"].dtype
    FF, Fr = t["FF"].copy(), t["Fr"].copy()
    cnt, vc = np.asarray(p.view_count), np.asarray(p.view_camera)
    d = (params(p) - mu).astype(ld)
    k = np.arange(H.CAM_W)
    for m in range(p.n_cameras):
        vs = np.nonzero((cnt > 0) & (vc == m))[0]
        if vs.size == 0:
            assert not np.any(w[m] > 0)
            continue
        FF[vs[0], k, k] += w[m, :H.CAM_W].astype(ld)
        Fr[vs[0]] += (w[m].astype(ld) * d[m])[:H.CAM_W]
    out.update(FF=FF, Fr=Fr, cost=float(np.longdouble(t["cost"]) + np.longdouble(prior_cost(p, w, mu))))
    return out


def columns(p, fixed=None):
    """helpers.step_columns with the intrinsics of `fixed` held (anything lib.fixed_masks takes)"""
    cols = H.step_columns(p)
    words = lib.fixed_masks(fixed, p.n_cameras)
    cf = cols["cam_free"].copy()
    for m, word in enumerate(words):
        for k in range(H.N_INTR_FREE):
            if (int(word) >> k) & 1:
                cf[m, 6 + k] = False
    cols["cam_free"] = cf
    return cols


def scipy_optimum(p, w=None, mu=None, max_nfev=300, start=None, method="dogbox"):
    """The optimum of the oracle's residuals -- with the prior rows sqrt(w) (x - mean) of the effective weights w [C,15] when
    given -- by SciPy's dogbox as tests/test_oracle.py::test_lm_matches_scipy_optimum runs it, from the problem's parameters,
    over the solve's free parameters (every camera and board of p has views; no held intrinsics).  start: a problem whose
    parameters the search starts from instead (a rig: dogbox from a rig's initial guess needs thousands of evaluations, so it
    is started from the oracle's own LM solution of the prior-free problem, and with method "lm" -- MINPACK, which "trf"
    confirms to 1e-12 there while dogbox has not arrived after 10,000 evaluations; on the mono valley it is the other way
    round, see test_oracle.py).  -> (cost, problem at the optimum)"""
    from scipy.optimize import least_squares
    C, B = p.n_cameras, p.n_boards
    cf = CR.free_columns(p)[0][:, :13]                     # [C,13] free camera-side columns
    col = np.full((C, 13), -1)
    col[cf] = np.arange(int(cf.sum()))
    nc = int(cf.sum())
    work = p.copy().normalised()
    wf = np.zeros(nc) if w is None else w[:, :13][cf]
    rows = np.nonzero(wf > 0)[0]
    muf = np.zeros(nc) if mu is None else mu[:, :13][cf]
    view_of = np.repeat(np.arange(p.n_views), p.view_count)
    cam, board = np.asarray(p.view_camera)[view_of], np.asarray(p.view_board)[view_of]

    def unpack(x):
        xc = params(work)[:, :13]
        xc[cf] = x[:nc]
        if not p.mono:
            work.cam_rt[:] = xc[:, :6]
        work.intr[:, :7] = xc[:, 6:]
        work.board_rt[:] = x[nc:].reshape(B, 6)

    def fun(x):
        unpack(x)
        r = orc.evaluate(work, jets=False)[1].ravel()
        return np.r_[r, (np.sqrt(wf) * (x[:nc] - muf))[rows]]

    def jac(x):
        unpack(x)
        _, _, Jc, Jb, Ji = orc.evaluate(work, jets=True)
        N = Jb.shape[0]
        J = np.zeros((2 * N + rows.size, nc + 6 * B))
        r = np.arange(2 * N)
        F = np.concatenate([Jc.reshape(N, 2, 6), Ji.reshape(N, 2, 9)[:, :, :7]], axis=2)
        for k in range(13):
            c = np.repeat(col[cam, k], 2)
            ok = c >= 0
            J[r[ok], c[ok]] = F[:, :, k].reshape(2 * N)[ok]
        for k in range(6):
            J[r, nc + 6 * np.repeat(board, 2) + k] = Jb[:, :, k].reshape(2 * N)
        J[2 * N + np.arange(rows.size), rows] = np.sqrt(wf[rows])
        return J

    x0 = np.r_[params(start or p)[:, :13][cf], (start or p).board_rt.ravel()]
    r = least_squares(fun, x0, jac=jac, method=method, x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=None if method == "lm" else max_nfev)
    unpack(r.x)
    return float(r.cost), work


# ----------------------------------------------------------------------------- the whole-solve problem
# make_problem(1, 6, SEED), mono: few views, so xi, lambda and alpha trade off along the flat valley of
# test_oracle.py::test_lm_matches_scipy_optimum.  Priors on the three about values moved off the truth by OFFSETS, sigma SIGMA in
# the unit of a pixel (weight 1 / SIGMA^2).  tests/test_prior_reference.py asserts on the CPU that the optimum with the prior
# rows differs in cost from the one without by at least 100 times that test's 1e-4 band, so a solve that ignores the priors
# cannot pass for one that takes them.
SEED = 3
OFFSETS = {"xi": 0.3, "lambda": -0.2, "alpha": 0.1}
SIGMA = 0.05
BAND = 1e-4


def whole_solve_problem():
    from tscm_calib_amd import api, synth
    p = synth.make_problem(1, 6, SEED).normalised()
    gt = np.asarray(p.meta["gt_intr"], dtype=np.float64).reshape(1, 9)
    mean = gt.copy()
    for name, off in OFFSETS.items():
        mean[0, lib.INTRINSIC_NAMES.index(name)] += off
    pr = api.camera_priors(p, intr_sigma={name: SIGMA for name in OFFSETS}, mean={"intr": mean})
    return p, pr


# ... and a 2-camera rig with few frames: priors on the second camera's pose about values moved off the truth (camera 0 is the
# constant one: its weights count for nothing)
RIG_SEED = 4
RIG_OFFSET = np.array([0.004, -0.006, 0.004, 1.5, -1.0, 1.0])
RIG_SIGMA = np.array([0.002, 0.002, 0.002, 0.5, 0.5, 0.5])


def whole_solve_rig():
    """-> problem, priors, the oracle's LM solution of the problem without priors (where scipy_optimum starts, method "lm")"""
    from tscm_calib_amd import api, synth
    p = synth.make_problem(2, 4, RIG_SEED).normalised()
    mean = np.asarray(p.meta["gt_cam_rt"], dtype=np.float64).reshape(2, 6) + RIG_OFFSET
    pr = api.camera_priors(p, cam_rt_sigma=RIG_SIGMA, mean={"cam_rt": mean})
    q = p.copy().normalised()
    orc.solve(q)
    return p, pr, q
