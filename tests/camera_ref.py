"""The camera model in extended precision (np.longdouble: 64-bit mantissa), with derivatives by forward-mode dual numbers.

A plain restatement of what a residual block computes (multi_calib.h:146-195, TS.h:100-131): angle-axis rotation with the
two branches of ceres::AngleAxisRotatePoint (Rodrigues for theta^2 > DBL_EPSILON, p + w x p otherwise), board -> rig ->
camera, the Triple Sphere projection in the functor form (no skew), residual = observed - projected, and the Jacobian of
both residual rows with respect to the camera pose (6), the board pose (6) and the intrinsics fx fy cx cy xi lambda alpha
(7; the b, c columns are zero in the functor form).  The derivatives are carried by dual numbers through exactly these
operations: nothing here is taken from the hand-derived formulas of tscm_math.h / tscm_geometry.h, which this module is
the yardstick of.  The branch of a rotation is decided on the fp64 inputs, as the device and Ceres decide it.

Also: TripleSphereCamera::project (TS.cpp:332-344, with the skew terms b, c) and get_unit_sphere_coordinate (TS.h:39-57).

Per corner the module returns k (the projection's denominator) and
    cond = (|z2| + |beta| d3) / |k|,        k = z2 + beta d3,
the amplification of the rounding errors of z2 and d3 in k.  Measured against a plain fp64 evaluation this formula misses
three things (tests/test_camera_reference.py), so the module also returns cond_ext = cond_k + E / rho and rotation_cond:
  * z2 inherits the rounding of P_c = R_c (R_b p + t_b) + t_c, whose size is that of what was summed, E = max(d1, |p| +
    |t_b| + |t_c|), not |z2| (the pinhole limit next to 90 degrees: k = Z is itself a small difference):
        cond_k = (E (1 + |xi|) + |lambda| d2 + |beta| d3) / |k|;
  * where all rays of a view run next to a coordinate axis of the camera frame, the entries in proportion to the small
    components are small differences as well (X, Y next to the optical axis; the derivative along the ray, which is zero
    for a central projection): E / rho, rho the view's largest distance from the nearest axis;
    The board's translation is expressed in the rig frame, so its three columns carry the same term for the rig's axes
    as well (cond_rig; the camera frame is the rig frame of a mono problem);
  * the derivative of a Rodrigues rotation by its vector: rotation_cond, for the three columns of that rotation only.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
DBL_EPSILON = float(np.finfo(np.float64).eps)
N_PARAM = 19                  # derivative directions: camera pose 0-5, board pose 6-11, fx fy cx cy xi lambda alpha 12-18


class Dual:
    """value [n] and derivatives [n, N_PARAM] in longdouble; d = None is a constant."""
    __slots__ = ("v", "d")
    __array_ufunc__ = None        # numpy scalars and arrays defer to the reflected operators below

    def __init__(self, v, d=None):
        self.v = np.asarray(v, dtype=LD)
        self.d = d

    @staticmethod
    def lift(x):
        return x if isinstance(x, Dual) else Dual(x)

    def _d(self):
        return 0 if self.d is None else self.d

    def __add__(self, o):
        o = Dual.lift(o)
        d = None if self.d is None and o.d is None else self._d() + o._d()
        return Dual(self.v + o.v, d)
    __radd__ = __add__

    def __neg__(self):
        return Dual(-self.v, None if self.d is None else -self.d)

    def __sub__(self, o):
        return self + (-Dual.lift(o))

    def __rsub__(self, o):
        return Dual.lift(o) + (-self)

    def __mul__(self, o):
        o = Dual.lift(o)
        if self.d is None and o.d is None:
            return Dual(self.v * o.v)
        d = 0
        if self.d is not None:
            d = d + self.d * np.asarray(o.v)[..., None]
        if o.d is not None:
            d = d + o.d * np.asarray(self.v)[..., None]
        return Dual(self.v * o.v, d)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual.lift(o)
        q = self.v / o.v
        if self.d is None and o.d is None:
            return Dual(q)
        # (a / b)' = (a' - q b') / b
        d = (self._d() - (0 if o.d is None else o.d * np.asarray(q)[..., None])) / np.asarray(o.v)[..., None]
        return Dual(q, d)

    def __rtruediv__(self, o):
        return Dual.lift(o) / self


def _un(x, f, df):
    x = Dual.lift(x)
    return Dual(f(x.v), None if x.d is None else x.d * np.asarray(df(x.v))[..., None])


def dsqrt(x):
    return _un(x, np.sqrt, lambda v: LD(0.5) / np.sqrt(v))


def dsin(x):
    return _un(x, np.sin, np.cos)


def dcos(x):
    return _un(x, np.cos, lambda v: -np.sin(v))


def _where(m, a, b):
    a, b = Dual.lift(a), Dual.lift(b)
    if a.d is None and b.d is None:
        return Dual(np.where(m, a.v, b.v))
    z = np.zeros(np.shape(m) + (N_PARAM,), dtype=LD)
    return Dual(np.where(m, a.v, b.v), np.where(np.asarray(m)[..., None], z + a._d(), z + b._d()))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def small_angle(w, eps=DBL_EPSILON):
    """The branch of ceres::AngleAxisRotatePoint for the fp64 vectors w [..., 3]: True where theta^2 <= eps."""
    w = np.asarray(w, dtype=np.float64)
    return ~(w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1] + w[..., 2] * w[..., 2] > eps)


def rotate(w, p, small):
    """ceres::AngleAxisRotatePoint on lists of three Duals; `small` [n] bool picks the branch."""
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    # the Rodrigues branch on a harmless angle where the other branch is taken (no 0 / 0 in the lanes not used)
    t2s = _where(small, Dual(np.ones_like(t2.v)), t2)
    th = dsqrt(t2s)
    c, s = dcos(th), dsin(th)
    k = [w[i] / th for i in range(3)]
    kxp = _cross(k, p)
    h = dsin(th / 2)
    tmp = (k[0] * p[0] + k[1] * p[1] + k[2] * p[2]) * (2 * h * h)       # 1 - cos theta without its cancellation at small theta
    wxp = _cross(w, p)
    return [_where(small, p[i] + wxp[i], p[i] * c + kxp[i] * s + k[i] * tmp) for i in range(3)]


def triple_sphere(P, I):
    """P, I lists of Duals (I: fx fy cx cy xi lambda alpha) -> u, v and the intermediates z2, d3, beta, k."""
    X, Y, Z = P
    fx, fy, cx, cy, xi, lam, al = I
    r2 = X * X + Y * Y
    d1 = dsqrt(r2 + Z * Z)
    z1 = Z + xi * d1
    d2 = dsqrt(r2 + z1 * z1)
    z2 = z1 + lam * d2
    d3 = dsqrt(r2 + z2 * z2)
    beta = al / (1 - al)
    k = z2 + beta * d3
    return fx * X / k + cx, fy * Y / k + cy, dict(d1=d1, d2=d2, z2=z2, d3=d3, beta=beta, k=k)


def _seed(values, first):
    """Columns of an fp64 array [n, m] as Duals with unit derivatives in directions first .. first + m - 1."""
    out = []
    for j in range(values.shape[1]):
        d = np.zeros((values.shape[0], N_PARAM), dtype=LD)
        d[:, first + j] = 1
        out.append(Dual(values[:, j], d))
    return out


def corner_index(p):
    """view [N] and board point [N] of every corner, views in problem order (the oracle's and the device's order), and
    the corner's place in obs_u / obs_v."""
    cnt = np.asarray(p.view_count, dtype=np.int64)
    view = np.repeat(np.arange(p.n_views), cnt)
    start = np.cumsum(cnt) - cnt
    j = np.arange(int(cnt.sum())) - start[view]
    return view, j, np.asarray(p.view_offset, dtype=np.int64)[view] + j


def evaluate(p, eps_cam=DBL_EPSILON, eps_board=DBL_EPSILON) -> dict:
    """Every corner of problem p at p's parameters: res [N, 2], Jc [N, 2, 6], Jb [N, 2, 6], Ji [N, 2, 9] (b, c columns
    zero; Jc zero for a mono problem, which has no camera block), Pc [N, 3] and its derivatives dPc [N, 3, 12] by the pose
    parameters, pix [N, 2], k [N], cond, cond_k, cond_ext, cond_rig [N] (module docstring), rot_cam / rot_board [N] (rotation_cond),
    small_cam / small_board [N] (the branch each rotation took), view [N]; all longdouble.  eps_cam / eps_board move the branch threshold
    (tests/test_camera_reference.py: a branch taken on the wrong side of DBL_EPSILON)."""
    view, j, at = corner_index(p)
    vc, vb = np.asarray(p.view_camera, dtype=np.int64)[view], np.asarray(p.view_board, dtype=np.int64)[view]
    cam = _seed(np.asarray(p.cam_rt, dtype=np.float64)[vc], 0)
    brd = _seed(np.asarray(p.board_rt, dtype=np.float64)[vb], 6)
    I = _seed(np.asarray(p.intr, dtype=np.float64)[vc][:, :7], 12)
    xy = np.asarray(p.board_xy, dtype=np.float64)[j]
    pt = [Dual(xy[:, 0]), Dual(xy[:, 1]), Dual(np.zeros(len(j)))]
    sb = small_angle(np.asarray(p.board_rt)[vb, :3], eps_board)
    Pw = rotate(brd[:3], pt, sb)
    Pw = [Pw[i] + brd[3 + i] for i in range(3)]
    if p.mono:
        sc = np.ones(len(j), dtype=bool)
        Pc = Pw
    else:
        sc = small_angle(np.asarray(p.cam_rt)[vc, :3], eps_cam)
        Pc = rotate(cam[:3], Pw, sc)
        Pc = [Pc[i] + cam[3 + i] for i in range(3)]
    u, v, q = triple_sphere(Pc, I)
    ru, rv = np.asarray(p.obs_u, dtype=np.float64)[at] - u, np.asarray(p.obs_v, dtype=np.float64)[at] - v
    n = len(j)
    full = lambda x: np.zeros((n, N_PARAM), dtype=LD) + x._d()
    J = np.stack([full(ru), full(rv)], axis=1)                        # [N, 2, 19]
    Ji = np.zeros((n, 2, 9), dtype=LD)
    Ji[:, :, :7] = J[:, :, 12:]
    k = q["k"].v
    # the extended condition number (module docstring): the size of what was summed into P_c, over d1 and over the
    # view's largest distance from the optical axis
    wc, wb, ic = np.asarray(p.cam_rt, dtype=np.float64)[vc], np.asarray(p.board_rt, dtype=np.float64)[vb], np.asarray(p.intr, dtype=np.float64)[vc]
    d1 = q["d1"].v
    E = np.maximum(d1, np.hypot(xy[:, 0], xy[:, 1]) + np.linalg.norm(wb[:, 3:], axis=1) + (0.0 if p.mono else np.linalg.norm(wc[:, 3:], axis=1)))
    # a view's largest distance from each coordinate axis of the camera frame, the smallest of the three
    ax = [view_max(np.sqrt(Pc[a].v ** 2 + Pc[b].v ** 2), view, p.n_views)[view] for a, b in ((1, 2), (0, 2), (0, 1))]
    rho_view = np.minimum(np.minimum(ax[0], ax[1]), ax[2])
    beta_d3 = np.abs(q["beta"].v) * q["d3"].v
    # the same for the axes of the rig frame, in which the board's translation is expressed (dP_c / dt_b = R_c)
    dPc = np.stack([full(c)[:, :12] for c in Pc], axis=1)
    ray = np.einsum("nji,nj->ni", dPc[:, :, 9:12], np.stack([c.v for c in Pc], axis=1))
    far = np.sqrt(np.maximum(np.sum(ray ** 2, axis=1)[:, None] - ray ** 2, 0))
    rho_rig = view_max(far[:, 0], view, p.n_views)[view]
    for a in (1, 2):
        rho_rig = np.minimum(rho_rig, view_max(far[:, a], view, p.n_views)[view])
    cond_rig = np.zeros(n) if p.mono else np.where(rho_rig > 0, E / np.where(rho_rig > 0, rho_rig, 1), 0)
    cond_k = (E * (1 + np.abs(ic[:, 4])) + np.abs(ic[:, 5]) * q["d2"].v + beta_d3) / np.abs(k)
    cond_dir = np.where(rho_view > 0, E / np.where(rho_view > 0, rho_view, 1), 0)
    return dict(res=np.stack([ru.v, rv.v], axis=1), Jc=J[:, :, :6].copy(), Jb=J[:, :, 6:12].copy(), Ji=Ji,
                Pc=np.stack([c.v for c in Pc], axis=1), dPc=dPc, cond_rig=cond_rig, k=k, cond=(np.abs(q["z2"].v) + beta_d3) / np.abs(k), cond_k=cond_k, cond_ext=cond_k + cond_dir,
                rot_cam=np.zeros(n) if p.mono else rotation_cond(wc[:, :3], sc), rot_board=rotation_cond(wb[:, :3], sb),
                pix=np.stack([u.v, v.v], axis=1), small_cam=sc, small_board=sb, view=view)


def rotation_cond(w, small):
    """What the derivative of a rotation adds to the condition number of its three columns: 0 in the small-angle branch
    (p + w x p: exact), |cos theta| / theta in the Rodrigues branch, where 1 - cos theta is formed with an absolute
    error of 2^-53 |cos theta| and then multiplied by the derivative of the unit axis, 1 / theta."""
    th = np.linalg.norm(np.asarray(w, dtype=np.float64), axis=-1)
    return np.where(small, 0.0, np.abs(np.cos(th)) / np.where(small, 1.0, th))


def view_max(values, view, n_views):
    """Largest of a per-corner quantity in every view (0 for an empty view)."""
    out = np.zeros(n_views, dtype=np.asarray(values).dtype)
    np.maximum.at(out, view, values)
    return out


def project(intr, P):
    """TripleSphereCamera::project (TS.cpp:332-344) for points P [n, 3] (fp64 inputs, longdouble arithmetic):
    pixels [n, 2], k [n], cond_k [n] (module docstring, E = d1: the point is given, not summed)."""
    I = [Dual(np.full(len(P), float(x))) for x in np.asarray(intr, dtype=np.float64).ravel()]
    P = np.asarray(P, dtype=np.float64)
    Pd = [Dual(P[:, i]) for i in range(3)]
    _, _, q = triple_sphere(Pd, I[:7])
    k = q["k"].v
    u = I[0].v * Pd[0].v / k + I[7].v * Pd[1].v / k + I[2].v
    v = I[8].v * Pd[0].v / k + I[1].v * Pd[1].v / k + I[3].v
    cond_k = (q["d1"].v * (1 + np.abs(I[4].v)) + np.abs(I[5].v) * q["d2"].v + np.abs(q["beta"].v) * q["d3"].v) / np.abs(k)
    return np.stack([u, v], axis=1), k, cond_k


def unproject(intr, pix, jacobian=False):
    """get_unit_sphere_coordinate (TS.h:39-57, transform = identity) for pixels [n, 2] (fp64 inputs, longdouble
    arithmetic): rays [n, 3]; with jacobian=True also d ray / d pixel [n, 3, 2] (dual numbers in directions 0, 1)."""
    fx, fy, cx, cy, xi, lam, al, b, c = (LD(float(x)) for x in np.asarray(intr, dtype=np.float64).ravel())
    px = _seed(np.asarray(pix, dtype=np.float64).reshape(-1, 2), 0)
    x, y = px[0] - cx, px[1] - cy
    det = fx * fy - b * c
    mx = (fy * x - b * y) / det
    my = (fx * y - c * x) / det
    ks = al / (1 - al)
    r2 = mx * mx + my * my
    gamma = (ks + dsqrt(1 + (1 - ks * ks) * r2)) / (r2 + 1)
    gk = gamma - ks
    yita = lam * gk + dsqrt((gk * gk - 1) * lam * lam + 1)
    mz = yita * gk
    ml = mz - lam
    mu = xi * ml + dsqrt(xi * xi * (ml * ml - 1) + 1)
    ray = [mu * yita * gamma * mx, mu * yita * gamma * my, mu * ml - xi]
    out = np.stack([r.v for r in ray], axis=1)
    if not jacobian:
        return out
    return out, np.stack([r.d[:, :2] for r in ray], axis=1)
