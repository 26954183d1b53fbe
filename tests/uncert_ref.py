"""Reference of the projection uncertainty stage (tscm.h: tscm_projection_uncertainty; test infrastructure): the
definition restated in np.longdouble or np.float64, vectorised over the grid's pixels, with `mistake=` switches that alter
the computation the way a kernel or its host code could get it wrong; the whole chain (unproject -> transfer -> project) in
50-digit mpmath for derivative and Monte Carlo checks; the error measure, the flag margins, the tolerance rule and the
cases the CPU and the GPU tests share."""
from __future__ import annotations

import functools

import numpy as np

MISTAKES = ("sigma_ab_dropped", "sigma2_forgotten", "ra_not_transposed", "dr_dIa_omitted", "ta_sign", "bc_not_skipped")
# a mistake about camera a or about the pair shows in transfer requests only
TRANSFER_ONLY = ("sigma_ab_dropped", "ra_not_transposed", "dr_dIa_omitted", "ta_sign", "bc_not_skipped")
EPS = 2.0 ** -52
DBL_EPSILON = 2.0 ** -52
PLANES = ("u_b", "v_b", "c_uu", "c_uv", "c_vv", "sd_worst", "sd_across")
NEAR = 1e-9                      # a deciding quantity this close (relative) to its threshold: the pixel's flags are not compared


# ----------------------------------------------------------------------------- the model, in a numpy dtype
def rotation_and_derivatives(w, dtype=np.longdouble):
    """R [3,3] and dR [3,3,3] (dR[k] = dR / dw_k) of an angle-axis vector, both branches of ceres::AngleAxisRotatePoint."""
    dt = np.dtype(dtype).type
    w = np.asarray(w, dtype=dtype)
    theta2 = w @ w
    dR = np.zeros((3, 3, 3), dtype)
    if theta2 > dt(DBL_EPSILON):
        theta = np.sqrt(theta2)
        c, s = np.cos(theta), np.sin(theta)
        k = w / theta

        def cross(v):
            return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=dtype)
        R = c * np.eye(3, dtype=dtype) + s * cross(k) + (1 - c) * np.outer(k, k)
        for i in range(3):
            dk = -k[i] * k / theta
            dk[i] += 1 / theta
            dR[i] = (-s * k[i] * np.eye(3, dtype=dtype) + c * k[i] * cross(k) + s * cross(dk) + s * k[i] * np.outer(k, k)
                     + (1 - c) * (np.outer(dk, k) + np.outer(k, dk)))
        return R, dR
    R = np.array([[1, -w[2], w[1]], [w[2], 1, -w[0]], [-w[1], w[0], 1]], dtype=dtype)
    dR[0, 1, 2], dR[0, 2, 1] = -1, 1
    dR[1, 0, 2], dR[1, 2, 0] = 1, -1
    dR[2, 0, 1], dR[2, 1, 0] = -1, 1
    return R, dR


def project_jacobian(I, p):
    """The functor's projection of points p [P,3] with I (7) and its derivatives: u, v, k [P], A [P,2,3], G [P,2,7], and
    the margin of k > 0 (|k| relative to the size of its terms)."""
    fx, fy, cx, cy, xi, lam, al = (I[i] for i in range(7))
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    rho2 = X * X + Y * Y
    d1 = np.sqrt(rho2 + Z * Z)
    z1 = Z + xi * d1
    d2 = np.sqrt(rho2 + z1 * z1)
    z2 = z1 + lam * d2
    d3 = np.sqrt(rho2 + z2 * z2)
    oma = 1 - al
    beta = al / oma
    k = z2 + beta * d3
    mx, my = X / k, Y / k
    u, v = fx * mx + cx, fy * my + cy
    c1, c2, c3 = 1 + xi * Z / d1, 1 + lam * z1 / d2, 1 + beta * z2 / d3
    g = beta / d3 + c3 * (lam / d2 + c2 * xi / d1)
    kz = c1 * c2 * c3
    fxk, fyk = fx / k, fy / k
    A = np.zeros(p.shape[:1] + (2, 3), p.dtype)
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2] = fxk * (1 - X * mx * g), -fxk * mx * Y * g, -fxk * mx * kz
    A[:, 1, 0], A[:, 1, 1], A[:, 1, 2] = -fyk * my * X * g, fyk * (1 - Y * my * g), -fyk * my * kz
    hu, hv = fxk * mx, fyk * my
    kxi, klam, kal = c3 * c2 * d1, c3 * d2, d3 / (oma * oma)
    G = np.zeros(p.shape[:1] + (2, 7), p.dtype)
    G[:, 0, 0], G[:, 1, 1], G[:, 0, 2], G[:, 1, 3] = mx, my, 1, 1
    for c, kk in enumerate((kxi, klam, kal)):
        G[:, 0, 4 + c], G[:, 1, 4 + c] = -hu * kk, -hv * kk
    margin = np.abs(k) / (np.abs(z2) + np.abs(beta * d3))
    return u, v, k, A, G, margin


def unproject(I, px, py):
    """get_unit_sphere_coordinate with b = c = 0 on pixels px, py [P]: rays [P,3], ok [P] (every square-root argument > 0)
    and the smallest margin of the three arguments (|argument| relative to the size of its terms)."""
    fx, fy, cx, cy, xi, lam, al = (I[i] for i in range(7))
    x, y = px - cx, py - cy
    mx, my = x / fx, y / fy
    ksai = al / (1 - al)
    r2 = mx * mx + my * my
    with np.errstate(invalid="ignore"):
        a1 = 1 + (1 - ksai * ksai) * r2
        gamma = (ksai + np.sqrt(a1)) / (r2 + 1)
        gk = gamma - ksai
        a2 = (gk * gk - 1) * lam * lam + 1
        yita = lam * gk + np.sqrt(a2)
        ml = yita * gk - lam
        a3 = xi * xi * (ml * ml - 1) + 1
        mu = xi * ml + np.sqrt(a3)
        ray = np.stack([mu * yita * gamma * mx, mu * yita * gamma * my, mu * ml - xi], axis=1)
        ok1, ok2, ok3 = a1 > 0, a2 > 0, a3 > 0
        m1 = np.abs(a1) / (1 + np.abs((1 - ksai * ksai) * r2))
        m2 = np.abs(a2) / (1 + np.abs((gk * gk - 1) * lam * lam))
        m3 = np.abs(a3) / (1 + np.abs(xi * xi * (ml * ml - 1)))
    # a later argument exists only behind the earlier ones
    big = np.asarray(np.inf, dtype=px.dtype)
    margin = np.minimum(m1, np.where(ok1, np.minimum(m2, np.where(ok2, m3, big)), big))
    return ray, ok1 & ok2 & ok3, margin


def sigma_theta(cam_cov, a: int, b: int, dtype=np.longdouble, mistake=None):
    """Sigma_theta [n,n] (n = 26, or 13 with a == b) from cam_cov [C,15,C,15]: the lower triangle of the gathered rows,
    mirrored."""
    cc = np.asarray(cam_cov, dtype=dtype)
    n15 = cc.shape[0] * 15
    cc = cc.reshape(n15, n15)
    stride = 13 if mistake == "bc_not_skipped" else 15
    idx = np.array([stride * a + c for c in range(13)] + ([] if a == b else [stride * b + c for c in range(13)]))
    S = np.tril(cc[np.ix_(idx, idx)])
    S = S + np.tril(S, -1).T
    if mistake == "sigma_ab_dropped" and a != b:
        S[:13, 13:] = 0
        S[13:, :13] = 0
    return S


def jacobian(cam_rt, intr, a: int, b: int, iota, px, py, dtype=np.longdouble, mistake=None) -> dict:
    """The chain on pixels px, py [P] of camera a: u, v [P], J [P,2,n], e [P,2] (d q_b / d iota; zeros in observe mode),
    ok0 / ok1 [P] (unprojects / projects), margin0 / margin1 [P]."""
    dt = np.dtype(dtype).type
    rt, I = np.asarray(cam_rt, dtype=dtype), np.asarray(intr, dtype=dtype)[:, :7]
    px, py, iota = np.asarray(px, dtype=dtype), np.asarray(py, dtype=dtype), dt(iota)
    Ra, dRa = rotation_and_derivatives(rt[a, :3], dtype)
    Rb, dRb = rotation_and_derivatives(rt[b, :3], dtype)
    ta, tb = rt[a, 3:], rt[b, 3:]
    if mistake == "ra_not_transposed":
        Ra, dRa = Ra.T, np.swapaxes(dRa, 1, 2)
    r, ok0, margin0 = unproject(I[a], px, py)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = r - iota * ta
        D = s @ Ra                                          # R_a^T s
        p = D @ Rb.T + iota * tb
        u, v, k, A, G, margin1 = project_jacobian(I[b], p)
        P = px.size
        transfer = a != b
        n, ob = (26, 13) if transfer else (13, 0)
        J = np.zeros((P, 2, n), dtype)
        for kk in range(3):
            J[:, :, ob + kk] = np.einsum("pej,pj->pe", A, D @ dRb[kk].T)
        J[:, :, ob + 3:ob + 6] = iota * A
        J[:, :, ob + 6:ob + 13] = G
        e = np.zeros((P, 2), dtype)
        if transfer:
            AR = A @ Rb
            M = AR @ Ra.T
            for kk in range(3):
                J[:, :, kk] = np.einsum("pej,pj->pe", AR, s @ dRa[kk])      # AR (dR_a,k)^T s
            J[:, :, 3:6] = (iota if mistake == "ta_sign" else -iota) * M
            if mistake != "dr_dIa_omitted":
                _, _, _, Aa, Ga, _ = project_jacobian(I[a], r)
                W = Aa @ np.swapaxes(Aa, 1, 2)
                det = W[:, 0, 0] * W[:, 1, 1] - W[:, 0, 1] * W[:, 0, 1]
                Winv = np.empty_like(W)
                Winv[:, 0, 0], Winv[:, 1, 1] = W[:, 1, 1] / det, W[:, 0, 0] / det
                Winv[:, 0, 1] = Winv[:, 1, 0] = -W[:, 0, 1] / det
                J[:, :, 6:13] = -(M @ np.swapaxes(Aa, 1, 2) @ Winv @ Ga)
            e = A @ tb - M @ ta
    return dict(u=u, v=v, J=J, e=e, ok0=ok0, ok1=ok0 & (k > 0), margin0=margin0, margin1=margin1)


def grid_pixels(grid: dict, dtype=np.longdouble):
    dt = np.dtype(dtype).type
    col, row = np.meshgrid(np.arange(grid["nx"]), np.arange(grid["ny"]))
    return dt(grid["x0"]) + col.ravel().astype(dtype) * dt(grid["dx"]), dt(grid["y0"]) + row.ravel().astype(dtype) * dt(grid["dy"])


def request_ref(cam_rt, intr, cam_cov, sigma2, request, grid: dict, dtype=np.longdouble, mistake=None) -> dict:
    """One request (a, b, iota) on a grid dict(nx, ny, x0, y0, dx, dy, width_b=0, height_b=0): planes [7,ny,nx] in `dtype`,
    flags [ny,nx] uint8, near [ny,nx] (a flag decided within NEAR of its threshold), amp [ny,nx] (the cancellation of the
    quadratic form: |J| |Sigma| |J|^T over sqrt(c_uu c_vv), largest of the three entries)."""
    a, b, iota = int(request[0]), int(request[1]), request[2]
    dt = np.dtype(dtype).type
    px, py = grid_pixels(grid, dtype)
    j = jacobian(cam_rt, intr, a, b, iota, px, py, dtype, mistake)
    S = sigma_theta(cam_cov, a, b, dtype, mistake)
    s2 = dt(1) if mistake == "sigma2_forgotten" else dt(sigma2)
    with np.errstate(invalid="ignore", divide="ignore"):
        cov = s2 * np.einsum("pei,ij,pfj->pef", j["J"], S, j["J"])
        cuu, cuv, cvv = cov[:, 0, 0], (cov[:, 0, 1] + cov[:, 1, 0]) / 2, cov[:, 1, 1]
        worst_ = np.sqrt((cuu + cvv + np.sqrt((cuu - cvv) ** 2 + 4 * cuv * cuv)) / 2)
        eu, ev = j["e"][:, 0], j["e"][:, 1]
        e2 = eu * eu + ev * ev
        across = np.where(e2 > 0, np.sqrt((ev * ev * cuu - 2 * eu * ev * cuv + eu * eu * cvv) / e2), dt(np.nan)) if a != b else np.full(px.shape, np.nan, dtype)
        along = np.where(e2 > 0, np.sqrt((eu * eu * cuu + 2 * eu * ev * cuv + ev * ev * cvv) / e2), dt(np.nan)) if a != b else np.full(px.shape, np.nan, dtype)
        if mistake is None:
            absq = s2 * np.einsum("pei,ij,pfj->pef", np.abs(j["J"]), np.abs(S), np.abs(j["J"]))
            amp = np.max(absq.reshape(-1, 4), axis=1) / np.sqrt(cuu * cvv)
        else:
            amp = np.zeros(px.shape, dtype)                 # (a planted mistake is compared, never a reference)
    valid = j["ok1"]
    planes = np.stack([j["u"], j["v"], cuu, cuv, cvv, worst_, across])
    planes[:, ~valid] = np.nan
    w, h = int(grid.get("width_b", 0)), int(grid.get("height_b", 0))
    u, v = j["u"], j["v"]
    with np.errstate(invalid="ignore"):
        inside = valid & (w > 0) & (h > 0) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
        near = j["margin0"] < NEAR
        near |= j["ok0"] & (j["margin1"] < NEAR)
        if w > 0 and h > 0:
            for x, hi in ((u, w - 1), (v, h - 1)):
                for bound in (0, hi):
                    near |= valid & (np.abs(x - bound) <= NEAR * np.maximum(np.abs(x), max(abs(bound), 1)))
    flags = j["ok0"].astype(np.uint8) | (valid.astype(np.uint8) << 1) | (inside.astype(np.uint8) << 2)
    shape = (grid["ny"], grid["nx"])
    return dict(planes=planes.reshape((7,) + shape), flags=flags.reshape(shape), near=np.asarray(near, dtype=bool).reshape(shape),
                amp=np.where(valid, amp, 0).astype(np.float64).reshape(shape), sd_along=np.where(valid, along, dt(np.nan)).reshape(shape), J=j["J"])


def uncertainty_ref(cam_rt, intr, cam_cov, sigma2, requests, grid: dict, dtype=np.longdouble, mistake=None) -> dict:
    """All requests of a call: planes [R,7,ny,nx], flags, near, amp [R,ny,nx], and the summary max_sd, n_valid [R] as the
    stage defines it."""
    rs = [request_ref(cam_rt, intr, cam_cov, sigma2, rq, grid, dtype, mistake) for rq in requests]
    out = {k: np.stack([r[k] for r in rs]) for k in ("planes", "flags", "near", "amp")}
    out.update(summary(out["planes"], out["flags"]))
    return out


def summary(planes, flags) -> dict:
    """max_sd, n_valid [R] of planes [R,7,ny,nx], flags [R,ny,nx]: a numpy reduction in the stage's definition."""
    R = planes.shape[0]
    valid = (flags & 3) == 3
    sd = np.asarray(planes[:, 5], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        take = valid & (sd > 0)
    return dict(max_sd=np.array([sd[r][take[r]].max() if take[r].any() else 0.0 for r in range(R)]), n_valid=valid.reshape(R, -1).sum(axis=1))


# ----------------------------------------------------------------------------- error measure and tolerance
def uncertainty_errors(got_planes, ref: dict) -> dict:
    """Over the pixels the reference calls valid and not `near`: covariance entries scaled by sqrt(c_uu c_vv), the two
    standard deviations and q_b (by its norm) relatively.  Each the largest over all requests."""
    ld = np.longdouble
    g, r = np.asarray(got_planes, dtype=ld), np.asarray(ref["planes"], dtype=ld)
    use = ((ref["flags"] & 3) == 3) & ~ref["near"]
    err = dict(q=0.0, cov=0.0, sd_worst=0.0, sd_across=0.0)
    if not use.any():
        return err
    G, Rf = np.moveaxis(g, 1, 0)[:, use], np.moveaxis(r, 1, 0)[:, use]
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.sqrt(Rf[2] * Rf[4])
        err["q"] = _max(np.hypot(G[0] - Rf[0], G[1] - Rf[1]) / np.hypot(Rf[0], Rf[1]))
        err["cov"] = _max(np.max(np.abs(G[2:5] - Rf[2:5]), axis=0) / scale)
        err["sd_worst"] = _max(np.abs(G[5] - Rf[5]) / Rf[5])
        has = ~np.isnan(Rf[6])
        if has.any():
            err["sd_across"] = _max(np.abs(G[6][has] - Rf[6][has]) / Rf[6][has])
        if np.isnan(G[6][~has]).sum() != (~has).sum():
            err["sd_across"] = float("inf")                 # a number where the definition has none
    return err


def _max(x) -> float:
    x = np.asarray(x, dtype=np.float64)
    return float("inf") if np.isnan(x).any() else float(np.max(x))


def worst(err: dict) -> float:
    v = list(err.values())
    return float("inf") if any(x != x for x in v) else max(v)


def tolerance(e64: float, amp: float) -> float:
    """What a device result may differ from the longdouble reference (DESIGN 25's rule on this stage): 8 max(e64, 26 2^-52
    amp), e64 the error of the float64 restatement on the same case and amp the largest cancellation of the quadratic form
    among the compared pixels.  The 8 covers another summation order, nothing else."""
    return 8.0 * max(e64, 26 * EPS * amp)


def flags_agree(got_flags, ref: dict):
    """(equal outside the near pixels, share of near pixels)"""
    near = ref["near"]
    return bool(np.array_equal(np.asarray(got_flags)[~near], ref["flags"][~near])), float(near.mean())


# ----------------------------------------------------------------------------- 50 digits
def mp_chain(cam_rt, intr, a: int, b: int, iota, q, D=None):
    """q_b of one pixel in 50-digit mpmath from mpmath parameters cam_rt [C][6], intr [C][7]: unproject -> transfer ->
    project, both rotation branches.  D given (observe mode): the held rig-frame point.  Returns (u, v), D."""
    import mpmath as mp

    def rot(w):
        t2 = w[0] ** 2 + w[1] ** 2 + w[2] ** 2
        if t2 > mp.mpf(DBL_EPSILON):
            th = mp.sqrt(t2)
            k = [x / th for x in w]
            c, s = mp.cos(th), mp.sin(th)
            K = mp.matrix([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            kk = mp.matrix(3, 3)
            for i in range(3):
                for j in range(3):
                    kk[i, j] = k[i] * k[j]
            return c * mp.eye(3) + s * K + (1 - c) * kk
        return mp.matrix([[1, -w[2], w[1]], [w[2], 1, -w[0]], [-w[1], w[0], 1]])

    def unproj(I, x, y):
        fx, fy, cx, cy, xi, lam, al = I
        mx, my = (x - cx) / fx, (y - cy) / fy
        ks = al / (1 - al)
        r2 = mx * mx + my * my
        gamma = (ks + mp.sqrt(1 + (1 - ks * ks) * r2)) / (r2 + 1)
        gk = gamma - ks
        yita = lam * gk + mp.sqrt((gk * gk - 1) * lam * lam + 1)
        ml = yita * gk - lam
        mu = xi * ml + mp.sqrt(xi * xi * (ml * ml - 1) + 1)
        return mp.matrix([mu * yita * gamma * mx, mu * yita * gamma * my, mu * ml - xi])

    def proj(I, p):
        fx, fy, cx, cy, xi, lam, al = I
        X, Y, Z = p
        rho2 = X * X + Y * Y
        d1 = mp.sqrt(rho2 + Z * Z)
        z1 = Z + xi * d1
        d2 = mp.sqrt(rho2 + z1 * z1)
        z2 = z1 + lam * d2
        d3 = mp.sqrt(rho2 + z2 * z2)
        k = z2 + al / (1 - al) * d3
        return fx * X / k + cx, fy * Y / k + cy

    Rb, tb = rot(cam_rt[b][:3]), mp.matrix(cam_rt[b][3:])
    if D is None:
        Ra, ta = rot(cam_rt[a][:3]), mp.matrix(cam_rt[a][3:])
        r = unproj(intr[a], q[0], q[1])
        D = Ra.T * (r - iota * ta)
    p = Rb * D + iota * tb
    return proj(intr[b], p), D


def mp_jacobian(cam_rt, intr, a: int, b: int, iota, q, h=None):
    """J [2,n] of one pixel by central differences of mp_chain at 50 digits (step 1e-20 relative: truncation 1e-40)."""
    import mpmath as mp
    mp.mp.dps = 50
    h = mp.mpf(10) ** -20 if h is None else h
    rt = [[mp.mpf(float(x)) for x in row] for row in np.asarray(cam_rt, dtype=np.float64)]
    I = [[mp.mpf(float(x)) for x in row[:7]] for row in np.asarray(intr, dtype=np.float64)]
    q = (mp.mpf(float(q[0])), mp.mpf(float(q[1])))
    iota = mp.mpf(float(iota))
    transfer = a != b
    D = None if transfer else mp_chain(rt, I, a, b, iota, q)[1]
    cols = [(a, c) for c in range(13)] + [(b, c) for c in range(13)] if transfer else [(b, c) for c in range(13)]
    J = np.zeros((2, len(cols)), np.longdouble)
    for n, (m, c) in enumerate(cols):
        arr, i = (rt[m], c) if c < 6 else (I[m], c - 6)
        x0 = arr[i]
        step = h * max(abs(x0), mp.mpf(1))
        arr[i] = x0 + step
        (up, vp), _ = mp_chain(rt, I, a, b, iota, q, D)
        arr[i] = x0 - step
        (um, vm), _ = mp_chain(rt, I, a, b, iota, q, D)
        arr[i] = x0
        J[0, n], J[1, n] = _ld((up - um) / (2 * step)), _ld((vp - vm) / (2 * step))
    return J


def _ld(x):
    """an mpmath number rounded to longdouble: its double and what that left"""
    hi = float(x)
    return np.longdouble(hi) + np.longdouble(float(x - hi))


# ----------------------------------------------------------------------------- the shared cases
IMG_W, IMG_H = 1280, 1080
IOTAS = (0.0, 1.0 / 5000, 1.0 / 300)


def grids() -> dict:
    """67 x 5 and 1 x 1 (no multiple of a block shape), 24 x 16 over the whole image, and a 9 x 7 grid that reaches far
    outside the image (and, where the model has one, outside the disc of pixels that unproject)."""
    return {
        "67x5": dict(nx=67, ny=5, x0=101.25, y0=203.5, dx=16.0, dy=170.0, width_b=IMG_W, height_b=IMG_H),
        "1x1": dict(nx=1, ny=1, x0=640.5, y0=511.25, dx=1.0, dy=1.0, width_b=IMG_W, height_b=IMG_H),
        "24x16": dict(nx=24, ny=16, x0=0.5, y0=0.5, dx=(IMG_W - 2) / 23.0, dy=(IMG_H - 2) / 15.0, width_b=IMG_W, height_b=IMG_H),
        "wide9x7": dict(nx=9, ny=7, x0=-200.25, y0=-150.75, dx=210.5, dy=230.25, width_b=0, height_b=0),
    }


def rig_requests(C: int):
    """At least five requests that mix the modes, the cameras and the three inverse distances."""
    if C == 1:
        return [(0, 0, i) for i in IOTAS]
    return [(0, 0, IOTAS[1]), (C - 1, C - 1, IOTAS[0]), (0, 1, IOTAS[2]), (1, 0, IOTAS[0]), (1, 2 % C, IOTAS[1]), (C - 1, 0, IOTAS[2]), (2 % C, C - 1, IOTAS[1])]


CASE_NAMES = ("rig4", "mixed65-cx_cy", "mixed65-ds1", "mono7")
# (case, grid) of the GPU tests; the CPU tests run their negative controls and flag margins on the same list
GPU_CASES = [("rig4", "67x5"), ("rig4", "1x1"), ("rig4", "24x16"), ("rig4", "wide9x7"), ("mixed65-cx_cy", "67x5"), ("mixed65-ds1", "24x16"),
             ("mono7", "67x5"), ("mono7", "1x1")]


@functools.lru_cache(maxsize=None)
def inputs(name: str):
    """(cam_rt, intr, cam_cov [C,15,C,15] float64, sigma2, requests) of a case: Sigma from cov_ref's longdouble reference
    rounded to float64 -- the input of the device and of every restatement alike."""
    from tests import cov_ref as CR
    p, kw, ref, _, _ = CR.case(name)
    cam_cov = np.asarray(ref["cam_cov"], dtype=np.float64)
    n15 = p.n_cameras * 15
    flat = cam_cov.reshape(n15, n15)
    flat[:] = np.tril(flat) + np.tril(flat, -1).T           # exactly symmetric, as the device's own cam_cov is
    return np.array(p.cam_rt, dtype=np.float64), np.array(p.intr, dtype=np.float64), cam_cov, float(ref["sigma2"]), rig_requests(p.n_cameras)


@functools.lru_cache(maxsize=None)
def behind_inputs():
    """rig4 with alpha of camera 2 below 1/2 (with alpha >= 1/2, k = z2 + beta d3 > 0 everywhere): camera 2 sees part of
    the other cameras' rays behind it, k <= 0.  Sigma stays rig4's: the comparison is with the restatement on the same input."""
    cam_rt, intr, cam_cov, sigma2, _ = inputs("rig4")
    intr = intr.copy()
    intr[2, 6] = 0.3
    return cam_rt, intr, cam_cov, sigma2, [(0, 2, IOTAS[2]), (1, 2, IOTAS[0]), (2, 2, IOTAS[1]), (3, 2, IOTAS[1]), (2, 0, IOTAS[2])]


@functools.lru_cache(maxsize=None)
def case(name: str, grid_name: str):
    """(inputs, grid, longdouble reference, e64 errors, amp, tolerance) of a case on a grid, computed once per process."""
    inp = behind_inputs() if name == "behind" else inputs(name)
    grid = grids()[grid_name]
    ref = uncertainty_ref(*inp[:4], inp[4], grid)
    e64 = uncertainty_errors(uncertainty_ref(*inp[:4], inp[4], grid, dtype=np.float64)["planes"], ref)
    use = ((ref["flags"] & 3) == 3) & ~ref["near"]
    amp = float(ref["amp"][use].max()) if use.any() else 1.0
    return inp, grid, ref, e64, amp, tolerance(worst(e64), amp)
