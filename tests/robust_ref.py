"""Reference of the robust losses (tscm.h: TSCM_LOSS_*), from the oracle's dual-number jets.

Ceres' HuberLoss, SoftLOneLoss and CauchyLoss (loss_function.cc) in numpy, and the corrected jets of a problem: every
corner's residual and Jacobian rows scaled by w = sqrt(rho'(s)) (Ceres' Corrector, alpha = 0 branch: rho'' <= 0 for all
three), cost = sum rho / 2.  The result feeds helpers.normal_equations_from and helpers.step_terms / reference_step.
"""
import numpy as np

from oracle import pyoracle as orc
from tscm_calib_amd import lib
from tests import helpers as H

KINDS = {"huber": lib.LOSS_HUBER, "soft_l1": lib.LOSS_SOFT_L1, "cauchy": lib.LOSS_CAUCHY}
DBL_MIN = np.finfo(np.float64).tiny


def rho(kind, a, s):
    """(rho, rho', rho'') of loss `kind` with scale a at s = |r|^2 (arrays), Ceres' operations."""
    s = np.asarray(s, dtype=np.float64)
    b = a * a
    c = 1.0 / b
    if kind == "huber":
        big = s > b
        r = np.sqrt(np.where(big, s, 1.0))
        r0 = np.where(big, 2.0 * a * r - b, s)
        r1 = np.where(big, np.maximum(DBL_MIN, a / r), 1.0)
        r2 = np.where(big, -r1 / (2.0 * np.where(big, s, 1.0)), 0.0)
    elif kind == "soft_l1":
        tmp = np.sqrt(1.0 + s * c)
        r0 = 2.0 * b * (tmp - 1.0)
        r1 = np.maximum(DBL_MIN, 1.0 / tmp)
        r2 = -(c * r1) / (2.0 * (1.0 + s * c))
    elif kind == "cauchy":
        inv = 1.0 / (1.0 + s * c)
        r0 = b * np.log1p(s * c)
        r1 = np.maximum(DBL_MIN, inv)
        r2 = -c * (inv * inv)
    else:
        raise ValueError(kind)
    return r0, r1, r2


def robust_cost(res, kind, a):
    res = np.asarray(res, dtype=np.float64).reshape(-1, 2)
    return 0.5 * float(np.sum(rho(kind, a, np.sum(res * res, axis=1))[0]))


def robust_jets(p, kind, a, jets=None, weight_of=None):
    """orc.evaluate(p, jets=True) with every corner's rows scaled by sqrt(rho'), cost = sum rho / 2.
    weight_of (tests of the tolerances): maps the [N] weights sqrt(rho') and the [N] rho' to the [N] factors applied instead."""
    cost, res, Jc, Jb, Ji = orc.evaluate(p, jets=True) if jets is None else jets
    s = np.sum(res.reshape(-1, 2) ** 2, axis=1)
    r0, r1, _ = rho(kind, a, s)
    w = np.sqrt(r1)
    f = w if weight_of is None else weight_of(w, r1)
    return (0.5 * float(np.sum(r0)), res * f[:, None], Jc * f[:, None, None], Jb * f[:, None, None], Ji * f[:, None, None])


def robust_normal_equations(p, kind, a, jets=None):
    cost, res, Jc, Jb, Ji = robust_jets(p, kind, a, jets)
    out = H.normal_equations_from(p, res, Jc, Jb, Ji)
    out["cost"] = cost
    return out


def median_scale(p):
    """A scale that puts about half of p's corners beyond b (both branches of Huber run)."""
    res = orc.evaluate(p, jets=False)[1]
    return float(np.median(np.sqrt(np.sum(res.reshape(-1, 2) ** 2, axis=1))))


def fraction_beyond(p, a):
    res = orc.evaluate(p, jets=False)[1]
    return float(np.mean(np.sum(res.reshape(-1, 2) ** 2, axis=1) > a * a))
