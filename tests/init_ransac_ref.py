"""Extended-precision restatement of tscm_estimate_extrinsic_ransac (definition: tscm.h, "outlier-tolerant pose
initialisation"), with a-priori bounds on the difference of k_estimate_extrinsic_ransac (fp64) from it.

Integer part (bit for bit): the samples.  word(seed, k, h, d) = mix(mix(mix(mix(seed + 0x9e3779b9) + k) + h) + d) with
mix = MurmurHash3's fmix32; draw d takes position d + ((word * (n - d)) >> 32) of a Fisher-Yates shuffle that is carried
out here on a real list (the kernel keeps only the swapped entries).  A sample is rejected when one of its corners is
not usable or three of them are collinear on the lattice (i mod w, i div w); its hypothesis scores -1.

Floating part in np.longdouble: T, x, y as init_ref (look_at, unit_sphere); H_h by the two projective bases of tscm.h;
the score's du^2 + dv^2 per (hypothesis, corner).  Its rounding bound is a running error analysis of exactly that closed
form: every product, sum and quotient carries |error| <= (propagated input errors) + u |result| (u = 2^-53; a fused
multiply-add rounds less, never more), started from the bound of init_ref on x, y (64 bT (1 + r^2), bT the bound on T).
Differences of nearly equal cross-product terms lose digits there and the bound grows with them: that is the conditioning
of the hypothesis' 4-point system, measured and not estimated.  The mapped point's error goes through T^T (its entries
within bT) and through the projection with the projection's Jacobian (central differences in long double), doubled, plus
256 u of the pixel's own size for the projection's arithmetic.  A decision (du^2 + dv^2 <= thr^2, or w > 0, or the sign of
H_h at the first sampled point) closer to its limit than the bound is OPEN.
lo_h = inliers that are certain, hi_h = lo_h + open decisions.  A view is DECISIVE when the reference's winner has no
open decision and no other hypothesis can reach it: hi_h < score_w for h < w, hi_h <= score_w for h > w.  Then winner,
mask, n_inliers and the two new exit codes are exact.  Otherwise the device's winner must be one with
hi_h >= max_g lo_g.  A hypothesis' own score is compared wherever that hypothesis has no open decision.

Refit: init_ref.extrinsic_view's DLT, column step and Gauss-Newton with their bounds (bHn, bpose0, bpose), restated on the
masked corners (the look-at turn and its reference corner stay those of the whole view).
"""
from __future__ import annotations

import itertools

import numpy as np

from tests import init_ref as R
from tscm_calib_amd import synth

U, LD = R.U, R.LD
NO_HYPOTHESIS, FEW_INLIERS = 8, 9
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ samples
def mix(h: int) -> int:
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def word(seed: int, k: int, h: int, d: int) -> int:
    return mix(mix(mix(mix(seed + 0x9E3779B9) + k) + h) + d)


def sample(seed: int, k: int, h: int, n: int) -> list:
    perm = list(range(n))
    for d in range(4):
        j = d + ((word(seed, k, h, d) * (n - d)) >> 32)
        perm[d], perm[j] = perm[j], perm[d]
    return perm[:4]


def collinear(s, board_w: int) -> bool:
    pts = [(i % board_w, i // board_w) for i in s]
    for a, b, c in itertools.combinations(pts, 3):
        if (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) == 0:
            return True
    return False


def default_min_inliers(n: int) -> int:
    return max(4, (n + 1) // 2)


# ------------------------------------------------------------------------------------------------ running error
def _mul(a, b):
    v = a[0] * b[0]
    return v, np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1] + U * np.abs(v)


def _add(a, b):
    v = a[0] + b[0]
    return v, a[1] + b[1] + U * np.abs(v)


def _sub(a, b):
    v = a[0] - b[0]
    return v, a[1] + b[1] + U * np.abs(v)


def _basis(px, py):
    """c_j = p_{j+1} x p_{j+2} and lam_j = c_j . p_4; px, py: 4 (value, error) pairs."""
    c, lam = [], []
    for j in range(3):
        a, b = (j + 1) % 3, (j + 2) % 3
        cj = [_sub(py[a], py[b]), _sub(px[b], px[a]), _sub(_mul(px[a], py[b]), _mul(px[b], py[a]))]
        c.append(cj)
        lam.append(_add(_add(_mul(cj[0], px[3]), _mul(cj[1], py[3])), cj[2]))
    return c, lam


def homographies(X, Y, x, y, ex):
    """H [m,3,3] (value, error) of m samples; X, Y, x, y: [m,4] long double, ex [m,4] the bound on x and y."""
    z = np.zeros_like(X)
    bX, bY = [(X[:, j], z[:, j]) for j in range(4)], [(Y[:, j], z[:, j]) for j in range(4)]
    bx, by = [(x[:, j], ex[:, j]) for j in range(4)], [(y[:, j], ex[:, j]) for j in range(4)]
    c, lam = _basis(bX, bY)
    _, mu = _basis(bx, by)
    Hv, He, Ha = (np.zeros(X.shape[:1] + (3, 3), dtype=LD) for _ in range(3))
    for j in range(3):
        g = _mul(mu[j], _mul(lam[(j + 1) % 3], lam[(j + 2) % 3]))
        q = [_mul(g, bx[j]), _mul(g, by[j]), g]
        for r in range(3):
            for cc in range(3):
                t = _mul(q[r], c[j][cc])
                Hv[:, r, cc] += t[0]
                He[:, r, cc] += t[1]
                Ha[:, r, cc] += np.abs(t[0])
    He += 3 * U * Ha                                              # the three-term sums
    w1 = Hv[:, 2, 0] * X[:, 0] + Hv[:, 2, 1] * Y[:, 0] + Hv[:, 2, 2]
    e1 = He[:, 2, 0] * np.abs(X[:, 0]) + He[:, 2, 1] * np.abs(Y[:, 0]) + He[:, 2, 2] + 4 * U * np.abs(w1)
    Hv = np.where((w1 < 0)[:, None, None], -Hv, Hv)
    return Hv, He, np.abs(w1) <= e1


def project_ld(intr, P):
    """TS.cpp:332-344 with skew terms, long double, rays P [...,3]."""
    fx, fy, cx, cy, xi, lam, al, b, c = (LD(float(a)) for a in intr)
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d1 = np.sqrt(X * X + Y * Y + Z * Z)
        z1 = Z + xi * d1
        d2 = np.sqrt(X * X + Y * Y + z1 * z1)
        z2 = z1 + lam * d2
        d3 = np.sqrt(X * X + Y * Y + z2 * z2)
        ks = z2 + al / (1 - al) * d3
        return fx * X / ks + b * Y / ks + cx, c * X / ks + fy * Y / ks + cy


def distances(intr, T, bT, Hv, He, W, u, v):
    """d2 [m,n] = du^2 + dv^2 of every (hypothesis, corner), its bound, w and w's bound."""
    X, Y = W[None, :, 0].astype(LD), W[None, :, 1].astype(LD)
    aX, aY = np.abs(X), np.abs(Y)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        val = [Hv[:, r, 0, None] * X + Hv[:, r, 1, None] * Y + Hv[:, r, 2, None] for r in range(3)]
        err = [He[:, r, 0, None] * aX + He[:, r, 1, None] * aY + He[:, r, 2, None] + 4 * U * (np.abs(Hv[:, r, 0, None]) * aX + np.abs(Hv[:, r, 1, None]) * aY + np.abs(Hv[:, r, 2, None]))
               for r in range(3)]
        a, b, w = val
        den = np.abs(w) - err[2]
        xn, yn = a / w, b / w
        exn = (err[0] + np.abs(xn) * err[2]) / den + U * np.abs(xn)
        eyn = (err[1] + np.abs(yn) * err[2]) / den + U * np.abs(yn)
        q = np.stack([xn, yn, np.ones_like(xn)], -1)
        ray = q @ T                                                        # T^T q
        aT = np.abs(T)
        eray = np.stack([aT[0, j] * exn + aT[1, j] * eyn for j in range(3)], -1) + 3 * bT * (np.abs(xn) + np.abs(yn) + 1)[..., None] + 4 * U * np.abs(ray)
        pu, pv = project_ld(intr, ray)
        eu, ev = np.zeros_like(pu), np.zeros_like(pu)
        for j in range(3):
            h = LD(1e-7) * np.maximum(np.abs(ray[..., j]), LD(1e-3))
            rp, rm = ray.copy(), ray.copy()
            rp[..., j] += h
            rm[..., j] -= h
            up, vp = project_ld(intr, rp)
            um, vm = project_ld(intr, rm)
            eu += np.abs((up - um) / (2 * h)) * eray[..., j]
            ev += np.abs((vp - vm) / (2 * h)) * eray[..., j]
        c0, c1 = abs(LD(float(intr[2]))), abs(LD(float(intr[3])))
        eu = 2 * eu + 256 * U * (np.abs(pu) + c0 + 1)
        ev = 2 * ev + 256 * U * (np.abs(pv) + c1 + 1)
        du, dv = u[None, :].astype(LD) - pu, v[None, :].astype(LD) - pv
        d2 = du * du + dv * dv
        bd = 2 * (np.abs(du) * eu + np.abs(dv) * ev) + eu * eu + ev * ev + 8 * U * d2
    return d2, bd, w, err[2]


# ------------------------------------------------------------------------------------------------ refit
def refit(T, bT, x, y, worlds, mask) -> dict:
    """init_ref.extrinsic_view from the Hartley normalisation on, over the corners of `mask`."""
    out = dict(code=None, H=None, rv0=None, rv=None, t=None, Rt=None, decisive_code=True, capped_ref=False, bT=bT)
    idx = np.flatnonzero(mask)
    n = idx.shape[0]
    x, y = x[idx], y[idx]
    Wl = worlds[idx].astype(LD)
    cx, cy = Wl[:, 0].mean(), Wl[:, 1].mean()
    md = np.mean(np.sqrt((Wl[:, 0] - cx) ** 2 + (Wl[:, 1] - cy) ** 2))
    if not md > 0:
        out["code"] = R.DEGENERATE_BOARD
        return out
    s = np.sqrt(LD(2)) / md
    X, Y = (Wl[:, 0] - cx) * s, (Wl[:, 1] - cy) * s
    z, o = np.zeros(n, dtype=LD), np.ones(n, dtype=LD)
    r1 = np.stack([X, Y, o, z, z, z, -x * X, -x * Y], 1)
    r2 = np.stack([z, z, z, X, Y, o, -y * X, -y * Y], 1)
    with np.errstate(invalid="ignore", over="ignore"):
        N = r1.T @ r1 + r2.T @ r2
        rhs = r1.T @ x + r2.T @ y
    if not (np.all(np.isfinite(N)) and np.all(np.isfinite(rhs))):
        out["code"] = R.DLT_FAILED
        return out
    L, rmin = R.chol_ld(N)
    kappa = R.scaled_cond(N)
    if L is None:
        out["code"] = R.DLT_FAILED
        out["decisive_code"] = bool(np.any(np.diag(N) == 0))
        return out
    out["decisive_code"] = bool(rmin > 1e3 * 8 * U * kappa)
    hn = R.chol_solve_ld(L, rhs)
    Hn = np.append(hn, LD(1)).reshape(3, 3)
    Nt = np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]], dtype=LD)
    H = Hn @ Nt
    out.update(H=H, Hn=Hn, Nt=Nt, kappa_dlt=kappa)
    r2max = float(np.max(x * x + y * y))
    eHn = (32 * n * U * kappa + 64 * bT * (1 + r2max)) * float(np.max(np.abs(Hn)))
    out["bHn"] = eHn
    sq = H[:, :2] ** 2
    zero_col = [bool(np.all(sq[:, j] < R.HALF_SUBNORMAL)) for j in range(2)]
    if any(zero_col):
        out["code"] = R.ZERO_COLUMN
        return out
    rv0, t0, info = R.column_pose(H)
    out.update(rv0=rv0, t0=t0, rod=info)
    force = (info["branch"], info.get("sign_rule"))
    Jc, Jx = np.zeros((6, 8)), np.zeros((9, 8))
    for j in range(8):
        h = 1e-7 * max(abs(float(Hn.flat[j])), 1e-3 * float(np.max(np.abs(Hn))))
        Hp, Hm = Hn.copy(), Hn.copy()
        Hp.flat[j] += LD(h)
        Hm.flat[j] -= LD(h)
        a = R.column_pose(Hp @ Nt, force, None, exact=False)
        b = R.column_pose(Hm @ Nt, force, None, exact=False)
        Jc[:3, j] = ((a[0] - b[0]) / (2 * h)).astype(np.float64)
        Jc[3:, j] = ((a[1] - b[1]) / (2 * h)).astype(np.float64)
        Jx[:, j] = ((a[2]["X"] - b[2]["X"]) / (2 * h)).astype(np.float64).ravel()
    e = eHn + 64 * U * float(np.max(np.abs(Hn)))
    out["bpose0"] = 2 * np.abs(Jc).sum(axis=1) * e
    eX = 2 * float(np.abs(Jx).sum(axis=1).max()) * e + 8 * U
    if info["branch"] == "pi":
        out["bpose0"][:3] = R.near_pi_bound(info, eX)
    bs = 2 * eX
    if info["branch"] != "generic" or abs(float(info["s"]) - 1e-5) < 1e3 * bs:
        out["rod_decisive"] = abs(float(info["s"]) - 1e-5) > 2 * bs
        if info["branch"] == "pi":
            margins = [abs(float(info["x5"])), abs(abs(float(info["rx"])) - abs(float(info["ry"]))),
                       abs(abs(float(info["rx"])) - abs(float(info["rz"]))), abs(float(info["ry"] * info["rz"]))]
            out["rod_decisive"] = out["rod_decisive"] and min(margins) > 1e-6
    else:
        out["rod_decisive"] = True
    rv, t, steps, code, kap, hist, jmax = R.gauss_newton(rv0, t0, Wl, x, y, 10, None)
    out.update(steps=steps, code=code, kappa_gn=kap, hist=hist)
    if code == R.GN_CHOLESKY:
        out["decisive_code"] = bool(jmax > LD(1.01) * LD(R.DBL_MAX))
    tmax = float(np.max(np.abs(t))) if np.all(np.isfinite(t)) else np.inf
    bmin = np.concatenate([np.full(3, 64 * U * kap + 1e-12 + 16 * bT),
                           64 * U * kap * tmax + 1e-12 * np.maximum(1, np.abs(t.astype(np.float64))) + 16 * bT * tmax])
    if code == R.CONVERGED:
        out["decisive_code"] = out["decisive_code"] and steps <= 8 and 64 * U * kap < 1e-12
    elif code == R.ITERATION_CAP:
        out["capped_ref"] = True
        out["decisive_code"] = False
        bmin = bmin + out["bpose0"]
    out["bpose"] = bmin
    out.update(rv=rv, t=t)
    Rm, _ = R.rotation(rv)
    out["Rt"] = np.stack([T.T @ Rm[:, 0], T.T @ Rm[:, 1], T.T @ t], axis=1)
    return out


def rms_px(intr, T, rv, t, worlds, u, v, mask):
    """Pixel RMS of the masked corners at the pose (rv, t) of the turned frame, through the full model, long double."""
    idx = np.flatnonzero(mask)
    Rm, _ = R.rotation(np.asarray(rv, dtype=LD))
    P = worlds[idx].astype(LD) @ Rm.T + np.asarray(t, dtype=LD)
    pu, pv = project_ld(intr, P @ np.asarray(T, dtype=LD))
    return np.sqrt(np.sum((u[idx].astype(LD) - pu) ** 2 + (v[idx].astype(LD) - pv) ** 2) / idx.shape[0])


# ------------------------------------------------------------------------------------------------ one view
def ransac_view(intr, u, v, worlds, board_w, k, threshold_px=8.0, n_hypotheses=256, min_inliers=0, seed=0, with_refit=True) -> dict:
    """One view with a board.  samples [H,4] (-1 rejected), score [H] (-1 rejected), lo / hi [H], clean [H] (no open
    decision), winner, mask, n_inliers, code, decisive, allowed (the winners open decisions allow), refit dict."""
    n = worlds.shape[0]
    Hn = n_hypotheses
    min_inl = min_inliers if min_inliers else default_min_inliers(n)
    ref = n // 2 - board_w // 2 - 1
    p = R.unit_sphere(intr, u[ref], v[ref])
    T = R.look_at(p)
    bT = 256 * U * (1 + 1 / np.sqrt(max(float(1 - p[1] ** 2), 1e-300))) if np.isfinite(float(p[1])) else np.inf
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        Pq = R.unit_sphere(intr, u, v) @ T.T
        x, y = Pq[:, 0] / Pq[:, 2], Pq[:, 1] / Pq[:, 2]
        usable = np.isfinite(u) & np.isfinite(v) & np.isfinite(x.astype(np.float64)) & np.isfinite(y.astype(np.float64)) & (Pq[:, 2] > 0)
        exy = 64 * bT * (1 + x * x + y * y)
    out = dict(T=T, bT=bT, x=x, y=y, usable=usable)
    samples = np.full((Hn, 4), -1, dtype=np.int32)
    score = np.full(Hn, -1, dtype=np.int32)
    acc, S = [], []
    for h in range(Hn):
        s = sample(seed, k, h, n)
        if all(usable[i] for i in s) and not collinear(s, board_w):
            samples[h] = s
            acc.append(h)
            S.append(s)
    lo, hi = score.copy(), score.copy()
    inl = np.zeros((Hn, n), dtype=bool)
    Hs, Hes = np.full((Hn, 3, 3), np.nan, dtype=LD), np.full((Hn, 3, 3), np.nan, dtype=LD)
    if acc:
        S = np.array(S)
        Wl = worlds.astype(LD)
        xs, ys = np.where(usable, x, 0), np.where(usable, y, 0)
        Hv, He, unstable = homographies(Wl[S, 0], Wl[S, 1], xs[S], ys[S], np.where(usable, exy, 0)[S])
        uu, vv = np.where(usable, u, 0.0), np.where(usable, v, 0.0)
        d2, bd, w, ew = distances(intr, T, bT, Hv, He, worlds, uu, vv)
        thr2 = LD(threshold_px) ** 2
        with np.errstate(invalid="ignore"):
            yes = usable[None, :] & (w > 0) & (d2 <= thr2)
            openw = np.abs(w) <= ew
            opend = ~openw & (w > 0) & ~(np.abs(d2 - thr2) > bd)
            opn = usable[None, :] & (openw | opend | unstable[:, None])
        inl[acc] = yes
        Hs[acc], Hes[acc] = Hv, He
        score[acc] = yes.sum(1)
        lo[acc] = (yes & ~opn).sum(1)
        hi[acc] = (yes | opn).sum(1)
    out.update(samples=samples, score=score, lo=lo, hi=hi, clean=lo == hi)
    best = int(score.max())
    if best < 0:
        out.update(code=NO_HYPOTHESIS, winner=-1, decisive=True, mask=np.zeros(n, dtype=bool), n_inliers=0, allowed={-1}, refit=None)
        return out
    wdx = int(np.argmax(score))                                   # the first of the maxima: ties to the lowest h
    others_lo = np.arange(Hn) < wdx
    decisive = bool(lo[wdx] == hi[wdx] and np.all(hi[others_lo] < best) and np.all(hi[~others_lo & (np.arange(Hn) != wdx)] <= best))
    fro = np.sqrt(np.sum(Hs[wdx] ** 2))
    eb = (Hes[wdx] / fro).astype(np.float64)                      # H_best at unit Frobenius norm: the norm moves by at most sum(eb)
    out.update(winner=wdx, decisive=decisive, allowed={int(h) for h in np.flatnonzero(hi >= lo.max())}, H_best=Hs[wdx] / fro,
               bH_best=2 * (eb + np.abs((Hs[wdx] / fro).astype(np.float64)) * eb.sum()) + 16 * U)
    if best < min_inl:
        out.update(code=FEW_INLIERS, mask=np.zeros(n, dtype=bool), n_inliers=0, refit=None)
        return out
    out.update(mask=inl[wdx].copy(), n_inliers=best)
    if with_refit:
        out["refit"] = refit(T, bT, x, y, worlds, out["mask"])
        out["code"] = out["refit"]["code"]
    return out


def ransac_refs(intr, pu, pv, count, worlds, board_w, **kw) -> list:
    return [dict(code=R.NO_BOARD, decisive=True) if count[k] == 0 else ransac_view(intr, pu[k], pv[k], worlds, board_w, k, **kw)
            for k in range(count.shape[0])]


# ------------------------------------------------------------------------------------------------ cases
# (name, cols, rows, views, hypotheses, seed, threshold_px): 3 x 2 is the smallest board that passes the board-width rule
# and holds a non-collinear sample; 64 / 65 / 88 corners fill one lane round, loop twice, and end inside the second;
# hypotheses and views below, at and above one round of 64 lanes.
CASES = [("b3x2_v1_h1", 3, 2, 1, 1, 0, 8.0), ("b3x2_v5_h256", 3, 2, 5, 256, 7, 8.0), ("b8x8_v63_h63", 8, 8, 63, 63, 0, 8.0),
         ("b13x5_v64_h64", 13, 5, 64, 64, 12345, 2.0), ("b11x8_v65_h65", 11, 8, 65, 65, 0, 8.0),
         ("b9x6_v64_h256", 9, 6, 64, 256, 0xDEADBEEF, 3.0), ("b9x6_v1_h1", 9, 6, 1, 1, 3, 8.0)]
SMALL = [("b9x6_v6_h32", 9, 6, 6, 32, 5, 8.0), ("b3x2_v3_h16", 3, 2, 3, 16, 1, 8.0)]           # CPU tests


def _view_kind(k, cols):
    if cols < 5:
        return {1: "outlier1", 3: "no_board"}.get(k, "clean")
    table = {1: "outliers5", 2: "row_shift", 3: "no_board", 4: "nan_pixel", 5: "all_nan", 6: "garbage", 7: "outliers20", 8: "outlier1"}
    return table.get(k % 16, "clean")


def plant(rng, u, v, kind, cols, intr):
    """u, v with the outliers of `kind` and the indices that were moved."""
    n = u.shape[0]
    u, v = u.copy(), v.copy()
    moved = np.zeros(n, dtype=bool)
    share = {"outlier1": 1.0 / n, "outliers5": 0.05, "outliers20": 0.20}.get(kind)
    if share is not None:
        idx = rng.choice(n, size=max(1, int(round(share * n))), replace=False)
        ang, r = rng.uniform(0, 2 * np.pi, idx.size), rng.uniform(30, 200, idx.size)
        u[idx] += r * np.cos(ang)
        v[idx] += r * np.sin(ang)
        moved[idx] = True
    elif kind == "row_shift":                                       # one board row labelled one column late
        row = int(rng.integers(0, n // cols))
        sl = slice(row * cols, (row + 1) * cols)
        du, dv = u[sl][1] - u[sl][0], v[sl][1] - v[sl][0]
        u[sl] = np.concatenate([u[sl][1:], [u[sl][-1] + du]])
        v[sl] = np.concatenate([v[sl][1:], [v[sl][-1] + dv]])
        moved[sl] = True
    elif kind == "nan_pixel":
        u[3] = np.nan
        moved[3] = True
    elif kind == "all_nan":
        u[:] = np.nan
        moved[:] = True
    elif kind == "garbage":
        u[:], v[:] = rng.uniform(0, 2 * intr[2], n), rng.uniform(0, 2 * intr[3], n)
        moved[:] = True
    return u, v, moved


def case(name):
    """intr, pu, pv [V,n], count, worlds [n,3], board_w, hypotheses, seed, threshold, kinds, moved [V,n]."""
    _, cols, rows, V, Hn, seed, thr = next(r for r in CASES + SMALL if r[0] == name)
    n = cols * rows
    rng = np.random.default_rng(sum(map(ord, name)) * 15485863 + V)
    intr = synth.CALIB_INTR[0].copy()
    bxy = synth.board_points(cols, rows, 40.0)
    ref = n // 2 - cols // 2 - 1
    pu, pv, moved = np.zeros((V, n)), np.zeros((V, n)), np.zeros((V, n), dtype=bool)
    count = np.full(V, n, dtype=np.int32)
    kinds = []
    for k in range(V):
        kind = _view_kind(k, cols)
        kinds.append(kind)
        al, be = rng.uniform(-0.6, 0.6), rng.uniform(-0.5, 0.5)
        Rt = R.axis_angle(rng.normal(size=3), rng.uniform(0.1, 0.7))
        u, v = R.turned_view(intr, bxy, al, be, Rt, rng.uniform(500, 1200), ref)
        u, v = u + 0.1 * rng.normal(size=n), v + 0.1 * rng.normal(size=n)
        pu[k], pv[k], moved[k] = plant(rng, u, v, kind, cols, intr)
        if kind == "no_board":
            count[k] = 0
    W = np.concatenate([bxy, np.zeros((n, 1))], 1)
    return intr, pu, pv, count, W, cols, Hn, seed, thr, kinds, moved


# ------------------------------------------------------------------------------------------------ pose-level robustness
ROBUST_KINDS = ["clean", "outlier1", "outliers5", "outliers20", "row_shift"]      # 0, 1 corner (1 %), 5 %, 20 %, one shifted row
ROBUST_PARAMS = dict(threshold_px=2.0, n_hypotheses=256, seed=11)                 # 0.1 px noise: 2 px is 20 sigma


def robust_case(kind, views=8):
    """Views of the golden rig's camera 0 (synth.make_problem, true intrinsics, 0.1 px noise) with the outliers of `kind`
    planted in every view: intr, pu, pv, count, worlds, board_w, moved [V,n], the true [r1 r2 t] per view."""
    p = synth.make_problem(1, views, 31, noise_px=0.1, perturb=False)
    n = p.board_xy.shape[0]
    pu, pv = p.obs_u.reshape(views, n).copy(), p.obs_v.reshape(views, n).copy()
    W = np.concatenate([p.board_xy, np.zeros((n, 1))], 1)
    gt = p.meta["gt_board_rt"]
    Rt_true = np.stack([np.column_stack([synth.rodrigues(g[:3])[:, :2], g[3:]]) for g in gt])
    rng = np.random.default_rng(1000 + len(kind))
    moved = np.zeros((views, n), dtype=bool)
    intr = p.meta["gt_intr"][0].copy()
    for k in range(views):
        pu[k], pv[k], moved[k] = plant(rng, pu[k], pv[k], kind, 9, intr)
    return intr, pu, pv, np.full(views, n, dtype=np.int32), W, 9, moved, Rt_true


def pose_errors(Rt, Rt_true):
    """Largest entry of |[r1 r2] - truth| and largest |t - truth| / |truth| over the views."""
    rot = np.max(np.abs(Rt[:, :, :2] - Rt_true[:, :, :2]))
    tr = np.max(np.linalg.norm(Rt[:, :, 2] - Rt_true[:, :, 2], axis=1) / np.linalg.norm(Rt_true[:, :, 2], axis=1))
    return float(rot), float(tr)
