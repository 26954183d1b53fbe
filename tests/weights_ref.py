"""Reference of corner weights and corner masks (tscm.h: corner weights), from the oracle's dual-number jets.

The semantics are those of Ceres' ScaledLoss:
  - every corner i has a weight omega_i >= 0, with s_i = r_u^2 + r_v^2;
  - loss rho of kind None is rho(s) = s, rho' = 1;
  - block cost is omega_i rho(s_i) / 2;
  - residual and Jacobian rows are scaled by w_i = sqrt(omega_i rho'(s_i)), rho' clamped at DBL_MIN before the multiplication
    by omega, so omega_i = 0 gives w_i = 0 exactly;
  - omega_i = 0 takes the corner out; n_residual_blocks counts omega_i > 0 and rmse = sqrt(sum omega_i s_i / sum omega_i).
The weighted jets feed helpers.normal_equations_from and helpers.step_terms / reference_step, as robust_ref's do.
"""
import numpy as np

from oracle import pyoracle as orc
from tests import helpers as H
from tests import robust_ref as R


def rho(kind, a, s):
    """(rho, rho') at s; kind None: (s, 1)."""
    s = np.asarray(s, dtype=np.float64)
    if kind is None:
        return s, np.ones_like(s)
    r0, r1, _ = R.rho(kind, a, s)
    return r0, r1


def weighted_jets(p, w, kind=None, a=1.0, jets=None):
    """orc.evaluate(p, jets=True) with every corner's rows scaled by sqrt(omega rho'), cost = sum omega rho / 2."""
    cost, res, Jc, Jb, Ji = orc.evaluate(p, jets=True) if jets is None else jets
    w = np.asarray(w, dtype=np.float64)
    s = np.sum(res.reshape(-1, 2) ** 2, axis=1)
    r0, r1 = rho(kind, a, s)
    f = np.sqrt(w * r1)
    return (0.5 * float(np.sum(w * r0)), res * f[:, None], Jc * f[:, None, None], Jb * f[:, None, None], Ji * f[:, None, None])


def weighted_cost(res, w, kind=None, a=1.0):
    res = np.asarray(res, dtype=np.float64).reshape(-1, 2)
    return 0.5 * float(np.sum(np.asarray(w, dtype=np.float64) * rho(kind, a, np.sum(res * res, axis=1))[0]))


def weighted_normal_equations(p, w, kind=None, a=1.0, jets=None):
    cost, res, Jc, Jb, Ji = weighted_jets(p, w, kind, a, jets)
    out = H.normal_equations_from(p, res, Jc, Jb, Ji)
    out["cost"] = cost
    return out


def weighted_rmse(p, w):
    res = orc.evaluate(p, jets=False)[1].reshape(-1, 2)
    w = np.asarray(w, dtype=np.float64)
    return float(np.sqrt(np.sum(w * np.sum(res * res, axis=1)) / np.sum(w)))


def scattered_weights(p, seed, zero_frac=0.2, mask=False, boundary=None):
    """20 % zeros scattered inside the views -- the first, the last and an interior corner of some view and, with `boundary`
    (corners of a pass), the corners on both sides of a pass boundary among them -- the rest uniform in [0.25, 4] (mask: 1).
    Every view keeps a corner."""
    rng = np.random.default_rng(seed)
    cnt = np.asarray(p.view_count, dtype=np.int64)
    first = np.cumsum(cnt) - cnt
    n = int(cnt.sum())
    w = np.ones(n) if mask else rng.uniform(0.25, 4.0, n)
    w[rng.random(n) < zero_frac] = 0.0
    full = np.nonzero(cnt >= 3)[0]
    v0, v1, v2 = full[0], full[len(full) // 2], full[-1]
    w[first[v0]] = 0.0
    w[first[v1] + cnt[v1] - 1] = 0.0
    w[first[v2] + cnt[v2] // 2] = 0.0
    if boundary is not None:
        for v in full[:4]:
            if cnt[v] > boundary:
                w[first[v] + boundary - 1] = 0.0
                w[first[v] + boundary] = 0.0
    for v in np.nonzero(cnt > 0)[0]:                    # no view without a corner
        seg = slice(first[v], first[v] + cnt[v])
        if not np.any(w[seg] > 0.0):
            w[first[v] + (cnt[v] - 1) // 2] = 1.0
    return w


def suffix_mask(p, keep):
    """0/1 weights that keep the first keep[v] corners of view v; and the problem with view_count shortened to keep (the
    oracle, which has no weights, anchors the masked semantics this way)."""
    cnt = np.asarray(p.view_count, dtype=np.int64)
    keep = np.minimum(np.asarray(keep, dtype=np.int64), cnt)
    w = np.concatenate([(np.arange(c) < k).astype(np.float64) for c, k in zip(cnt, keep)]) if cnt.size else np.zeros(0)
    q = p.copy()
    q.view_count = keep.astype(np.int32)
    q.weights = None
    return w, q.normalised()
