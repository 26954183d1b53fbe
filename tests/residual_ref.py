"""Reference of the residual report (tscm.h: tscm_residual_report) in np.longdouble, on tests/camera_ref.py.

report(): every quantity of the stage -- the per-corner rows, the view and camera rows, the call's totals and the field
statistics with their 2^-24 quantisation -- from camera_ref.evaluate's residuals, pixels and camera-frame points, with
cond_ext per corner and the error bounds of DESIGN 30 next to every array.  compare(): the comparison the GPU tests make,
array by array against those bounds; it raises AssertionError.  mistake=: one planted mistake, for the negative control
of tests/test_residual_reference.py.

Bounds (u = 2^-53).  b_i = 80 cond_ext_i u (|pix_i - c| + |c|), the project's bound of a residual (test_gpu_camera_extremes.py,
fan_problems.row_ratios), per corner.
  r_u, r_v          b_i
  |r|               sqrt(2) b_i                       s = |r|^2:  ds_i = 2 sqrt(2) |r| b_i + 4 u s
  r_rad, r_tan      r . e with e = (p - c) / |p - c|: |dr| |e| + |r| |de|, |de| <= 2 |dp| / |p - c|, both |dr|, |dp| <=
                    sqrt(2) b_i:  sqrt(2) b_i (1 + 2 |r| / |p - c|) + 4 u |r|
  angle             atan2(rho, Z) moves by at most |dP_c| / d1, and |dP_c| / d1 is within the same cond_ext u as the pixel
                    relative to its scale: 80 cond_ext_i u (scale 1 rad) + 4 u pi
  rho1              rho'(s) of all three losses has |d rho' / ds| <= rho' / s:  rho1 (ds_i / s + 8 u)
  a weighted mean   sum omega bound_i / sum omega + n u sum omega |x_i| / sum omega (the summation); rms through the mean
                    square m: dm / (2 rms); max_err: the largest sqrt(2) b_i + 2 u max
  field means       2^-24 (half a quantum on either side) + the largest per-corner bound of the cell or bin; rms compared
                    as the mean square, within 2^-24 + the largest ds_i (+ 8 u m for the root and the square)
Exact: n_used, worst, worst_view, n_views_used, every count, n_clamped and *_outside -- assert_separated() checks on the CPU
that the inputs decide them (no angle within 1e-9 rad of a bin edge, no |r_u|, |r_v| within 1e-6 px of the clamp, the two
largest errors of a view, and the two largest view maxima of a camera, further apart than their bounds)."""
import dataclasses

import numpy as np

from tests import camera_ref as R

LD = np.longdouble
U = LD(2.0) ** -53
Q = LD(2.0) ** 24
K_BOUND = 80
CORNER = ("r_u", "r_v", "r_rad", "r_tan", "angle", "rho1")
MISTAKES = ("rtan_sign", "unweighted_mean", "cell_from_projected", "clamped_summed")


def rho(kind, a, s):
    """(rho, rho') of Ceres' HuberLoss / SoftLOneLoss / CauchyLoss at s (longdouble), rho' clamped at DBL_MIN; kind None: (s, 1)."""
    s = np.asarray(s, dtype=LD)
    if kind is None:
        return s.copy(), np.ones_like(s)
    a = LD(a)
    b = a * a
    tiny = LD(np.finfo(np.float64).tiny)
    if kind == "huber":
        big = s > b
        r = np.sqrt(np.where(big, s, LD(1)))
        return np.where(big, 2 * a * r - b, s), np.where(big, np.maximum(tiny, a / r), LD(1))
    if kind == "soft_l1":
        t = np.sqrt(1 + s / b)
        return 2 * b * (t - 1), np.maximum(tiny, 1 / t)
    if kind == "cauchy":
        return b * np.log1p(s / b), np.maximum(tiny, 1 / (1 + s / b))
    raise ValueError(kind)


def _loss(loss):
    if loss is None:
        return None, 1.0
    return (loss, 1.0) if isinstance(loss, str) else (loss[0], float(loss[1]))


def _wmean(w, x, bound, group, n_groups):
    """Weighted mean of x per group with its bound: (mean, bound, sum_w, n)."""
    sw = np.zeros(n_groups, dtype=LD); sx = np.zeros(n_groups, dtype=LD); sb = np.zeros(n_groups, dtype=LD); sa = np.zeros(n_groups, dtype=LD)
    n = np.zeros(n_groups, dtype=np.int64)
    np.add.at(sw, group, w); np.add.at(sx, group, w * x); np.add.at(sb, group, w * bound); np.add.at(sa, group, w * np.abs(x)); np.add.at(n, group, 1)
    d = np.where(sw > 0, sw, LD(1))
    return sx / d, sb / d + (n + 4) * U * sa / d, sw, n


def _group_stats(used, om, q, group, n_groups, mistake):
    """The rows of a view or a camera over the used corners: dict of arrays [n_groups] and their bounds."""
    g = group[used]
    w = om[used] if mistake != "unweighted_mean" else np.ones(int(used.sum()), dtype=LD)
    err, b = q["err"][used], q["b"][used]
    out, bnd = {}, {}
    out["mean_err"], bnd["mean_err"], sw, n = _wmean(w, err, np.sqrt(LD(2)) * b, g, n_groups)
    out["bias_u"], bnd["bias_u"], _, _ = _wmean(w, q["r"][used, 0], b, g, n_groups)
    out["bias_v"], bnd["bias_v"], _, _ = _wmean(w, q["r"][used, 1], b, g, n_groups)
    out["mean_rad"], bnd["mean_rad"], _, _ = _wmean(w, q["r_rad"][used], q["b_rt"][used], g, n_groups)
    ms, dms, _, _ = _wmean(w, q["s"][used], q["ds"][used], g, n_groups)
    out["rms"] = np.sqrt(ms)
    bnd["rms"] = np.where(ms > 0, dms / (2 * np.where(ms > 0, out["rms"], LD(1))), np.sqrt(dms)) + 4 * U * out["rms"]
    swt = np.zeros(n_groups, dtype=LD); np.add.at(swt, g, om[used])
    out["sum_w"], bnd["sum_w"] = swt, (n + 4) * U * swt
    out["n_used"], bnd["n_used"] = n.astype(LD), np.zeros(n_groups, dtype=LD)
    mx = np.zeros(n_groups, dtype=LD); np.maximum.at(mx, g, err)
    mb = np.zeros(n_groups, dtype=LD); np.maximum.at(mb, g, np.sqrt(LD(2)) * b)
    out["max_err"], bnd["max_err"] = mx, mb + 2 * U * mx
    return out, bnd


def report(p, weights=None, loss=None, grid=None, image_size=None, angle_bins=0, max_angle=np.pi / 2, clamp=64.0, mistake=None) -> dict:
    """The residual report of problem p (normalised) in longdouble: the arrays of api.residual_report under the same names,
    "bound" (a dict of the same names), cond_ext [N] and the intermediates assert_separated() looks at."""
    assert mistake is None or mistake in MISTAKES
    view, j, at = R.corner_index(p)
    N, V, C = len(view), p.n_views, p.n_cameras
    om = np.ones(N, dtype=LD) if weights is None else np.asarray(weights, dtype=np.float64).astype(LD)
    used = om > 0
    # a masked observation may hold anything and is read as (0, 0)
    ou, ov = np.array(p.obs_u, dtype=np.float64), np.array(p.obs_v, dtype=np.float64)
    ou[at[~used]] = 0.0; ov[at[~used]] = 0.0
    ev = R.evaluate(dataclasses.replace(p, obs_u=ou, obs_v=ov, weights=None))
    r, pix, Pc = ev["res"], ev["pix"], ev["Pc"]
    cam = np.asarray(p.view_camera, dtype=np.int64)[view]
    c = np.asarray(p.intr, dtype=np.float64)[cam][:, 2:4].astype(LD)
    s = r[:, 0] ** 2 + r[:, 1] ** 2
    err = np.sqrt(s)
    d = pix - c
    dn = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
    e = np.where(dn[:, None] > 0, d / np.where(dn > 0, dn, LD(1))[:, None], np.array([1, 0], dtype=LD)[None, :])
    r_rad = r[:, 0] * e[:, 0] + r[:, 1] * e[:, 1]
    r_tan = e[:, 0] * r[:, 1] - e[:, 1] * r[:, 0]
    if mistake == "rtan_sign":
        r_tan = -r_tan
    angle = np.arctan2(np.sqrt(Pc[:, 0] ** 2 + Pc[:, 1] ** 2), Pc[:, 2])
    kind, a = _loss(loss)
    rho0, rho1 = rho(kind, a, s)
    # ---- bounds per corner
    cond = np.asarray(ev["cond_ext"], dtype=LD)
    scale = np.max(np.abs(d) + np.abs(c), axis=1)
    b = K_BOUND * cond * U * scale
    ds = 2 * np.sqrt(LD(2)) * err * b + 4 * U * s
    b_rt = np.sqrt(LD(2)) * b * (1 + 2 * err / np.where(dn > 0, dn, LD(1))) + 4 * U * err
    b_angle = K_BOUND * cond * U + 4 * U * LD(np.pi)
    b_rho1 = rho1 * (ds / np.where(s > 0, s, LD(1)) + 8 * U)
    corner = np.stack([r[:, 0], r[:, 1], r_rad, r_tan, angle, rho1], axis=1)
    corner_bound = np.stack([b, b, b_rt, b_rt, b_angle, b_rho1], axis=1)
    corner[~used] = 0
    corner_bound[~used] = 0
    q = dict(r=r, s=s, err=err, r_rad=r_rad, b=b, ds=ds, b_rt=b_rt)
    # ---- views and cameras
    names = ("n_used", "sum_w", "rms", "mean_err", "max_err", "bias_u", "bias_v", "mean_rad")
    vs, vb = _group_stats(used, om, q, view, V, mistake)
    view_rows = np.stack([vs[k] for k in names], axis=1)
    view_bound = np.stack([vb[k] for k in names], axis=1)
    view_worst = -np.ones(V, dtype=np.int64)
    for v in range(V):
        m = used & (view == v)
        if m.any():
            view_worst[v] = j[m][np.argmax(err[m])]               # argmax: the first, the lowest index
    cs, cb = _group_stats(used, om, q, cam, C, mistake)
    view_cam = np.asarray(p.view_camera, dtype=np.int64)
    worst_view = -np.ones(C, dtype=LD)
    n_views_used = np.zeros(C, dtype=LD)
    for m in range(C):
        vv = np.nonzero((view_cam == m) & (vs["n_used"] > 0))[0]
        n_views_used[m] = len(vv)
        if len(vv):
            worst_view[m] = vv[np.argmax(vs["max_err"][vv])]
    cnames = ("n_used", "sum_w", "rms", "mean_err", "max_err")
    camera = np.stack([cs[k] for k in cnames] + [worst_view, n_views_used, np.zeros(C, dtype=LD)], axis=1)
    camera_bound = np.stack([cb[k] for k in cnames] + [np.zeros(C, dtype=LD)] * 3, axis=1)
    # ---- the call
    wu = om[used]
    n_used = int(used.sum())
    sum_w = wu.sum() if n_used else LD(0)
    cost = LD(0.5) * (wu * rho0[used]).sum() if n_used else LD(0)
    ms = (wu * s[used]).sum() / sum_w if n_used else LD(0)
    dms = (wu * ds[used]).sum() / sum_w + (n_used + 4) * U * ms if n_used else LD(0)
    rmse = np.sqrt(ms)
    out = dict(corner=corner, view=view_rows, view_worst=view_worst, camera=camera, cost=cost, rmse=rmse, n_used=n_used,
               n_views_used=int(n_views_used.sum()), sum_w=sum_w, cond_ext=cond, used=used, view_of=view, cam_of=cam, err=err, angle_ld=angle,
               res=r, err_bound=np.sqrt(LD(2)) * b, view_camera=view_cam)
    bound = dict(corner=corner_bound, view=view_bound, camera=camera_bound,
                 cost=LD(0.5) * ((wu * ds[used]).sum() if n_used else LD(0)) + (n_used + 4) * U * cost,     # rho' <= 1: d rho <= ds
                 rmse=(dms / (2 * rmse) if rmse > 0 else np.sqrt(dms)) + 4 * U * rmse, sum_w=(n_used + 4) * U * sum_w)
    # ---- the field
    beyond = np.maximum(np.abs(r[:, 0]), np.abs(r[:, 1])) > LD(clamp)
    summed = used & (~beyond if mistake != "clamped_summed" else np.ones(N, dtype=bool))
    out["clamp_margin"] = np.min(np.abs(np.abs(r[used]) - LD(clamp))) if n_used else LD(np.inf)

    def table(index, inside, n_index, columns, col_bounds, roots):
        """count / n_clamped [C, n_index, 2], the quantised means [C, n_index, len(columns)] and their bounds, outside [C]"""
        count = np.zeros((C, n_index, 2), dtype=np.int64)
        mean = np.zeros((C, n_index, len(columns)), dtype=LD)
        bnd = np.zeros((C, n_index, len(columns)), dtype=LD)
        outside = np.zeros(C, dtype=np.int64)
        np.add.at(outside, cam[used & ~inside], 1)
        for m in range(C):
            for i in range(n_index):
                sel = used & inside & (cam == m) & (index == i)
                cl = sel & beyond
                sm = sel & summed
                count[m, i] = (int((sel & ~beyond).sum()), int(cl.sum()))
                n = int(sm.sum())
                if mistake == "clamped_summed":
                    count[m, i, 0] = n
                if n == 0:
                    continue
                for k, (x, bx) in enumerate(zip(columns, col_bounds)):
                    total = sum(int(t) for t in np.rint(x[sm] * Q))
                    v = LD(total) / Q / n
                    if k in roots:                                  # rms: the root of the mean square; its bound is the mean square's
                        mean[m, i, k] = np.sqrt(v)
                        bnd[m, i, k] = 1 / Q + bx[sm].max() + 8 * U * v
                    else:
                        mean[m, i, k] = v
                        bnd[m, i, k] = 1 / Q + bx[sm].max()
        return count, mean, bnd, outside

    if grid is not None:
        gw, gh = int(grid[0]), int(grid[1])
        W, Hh = int(image_size[0]), int(image_size[1])
        if mistake == "cell_from_projected":
            gu, gv = np.asarray(pix[:, 0], dtype=np.float64), np.asarray(pix[:, 1], dtype=np.float64)
        else:
            gu, gv = ou[at], ov[at]
        fx, fy = np.floor(gu * float(gw) / float(W)), np.floor(gv * float(gh) / float(Hh))        # fp64, the device's operations
        inside = (fx >= 0) & (fx < gw) & (fy >= 0) & (fy < gh)
        cell = np.where(inside, fy * gw + fx, 0).astype(np.int64)
        cnt, mean, bnd, outside = table(cell, inside, gw * gh, (r[:, 0], r[:, 1], s), (b, b, ds), {2})
        out.update(grid_count=cnt.reshape(C, gh, gw, 2), grid=mean.reshape(C, gh, gw, 3), grid_outside=outside)
        bound["grid"] = bnd.reshape(C, gh, gw, 3)
    if angle_bins:
        K, amax = int(angle_bins), LD(max_angle)
        inside = (angle >= 0) & (angle <= amax)
        pos = angle * K / amax
        bins = np.minimum(np.floor(pos), K - 1).astype(np.int64)
        bins = np.where(inside, bins, 0)
        edge = np.abs(pos - np.rint(pos)) * amax / K
        out["angle_margin"] = np.min(edge[used]) if n_used else LD(np.inf)
        cnt, mean, bnd, outside = table(bins, inside, K, (r_rad, r_tan, s, angle), (b_rt, b_rt, ds, b_angle), {2})
        out.update(angle_count=cnt, angle=mean, angle_outside=outside)
        bound["angle"] = bnd
    out["bound"] = bound
    return out


def assert_separated(ref: dict) -> None:
    """The preconditions of the exact comparisons, on the CPU (module docstring): chosen seeds satisfy them, none is skipped."""
    used, err, eb, view = ref["used"], ref["err"], ref["err_bound"], ref["view_of"]
    for v in np.unique(view[used]):
        m = used & (view == v)
        if m.sum() < 2:
            continue
        order = np.argsort(-err[m])
        top, second = err[m][order[0]], err[m][order[1]]
        assert top - second > eb[m][order[0]] + eb[m][order[1]], ("the two largest errors of view", int(v), top, second)
    vmax, vb = ref["view"][:, 4], ref["bound"]["view"][:, 4]
    for m in range(ref["camera"].shape[0]):
        vv = np.nonzero((ref["view"][:, 0] > 0) & (ref["view_camera"] == m))[0]
        if len(vv) < 2:
            continue
        order = np.argsort(-vmax[vv])
        assert vmax[vv][order[0]] - vmax[vv][order[1]] > vb[vv][order[0]] + vb[vv][order[1]], ("the two largest view maxima of camera", m)
    assert ref["clamp_margin"] > 1e-6, ("a residual component within 1e-6 px of the clamp", ref["clamp_margin"])
    if "angle_margin" in ref:
        assert ref["angle_margin"] > 1e-9, ("an angle within 1e-9 rad of a bin edge", ref["angle_margin"])


def as_candidate(ref: dict) -> dict:
    """A reference report in the form api.residual_report returns (float64 arrays): the candidate of the negative control."""
    out = {}
    for k in ("corner", "view", "camera", "grid", "angle"):
        if k in ref:
            out[k] = np.asarray(ref[k], dtype=np.float64)
    for k in ("view_worst", "grid_count", "angle_count", "grid_outside", "angle_outside"):
        if k in ref:
            out[k] = np.asarray(ref[k]).astype(np.int64)
    for k in ("cost", "rmse", "sum_w"):
        out[k] = float(ref[k])
    out["n_used"], out["n_views_used"] = ref["n_used"], ref["n_views_used"]
    return out


def compare(got: dict, ref: dict, show=None) -> dict:
    """api.residual_report's dict against the reference: exact where DESIGN 30 says exact, within ref["bound"] elsewhere.
    Returns the largest error / bound ratio per array (show: a print function for them); raises AssertionError."""
    ratios = {}
    bound = ref["bound"]

    def within(name, a, r, b, square=None):
        a, r, b = np.asarray(a, dtype=LD), np.asarray(r, dtype=LD), np.asarray(b, dtype=LD)
        assert a.shape == r.shape, (name, a.shape, r.shape)
        if square is not None:                                          # the listed last-axis columns are compared as squares
            a, r = a.copy(), r.copy()
            a[..., square] = a[..., square] ** 2
            r[..., square] = r[..., square] ** 2
        diff = np.abs(a - r)
        bad = ~(diff <= b)
        ratios[name] = float(np.max(np.where(b > 0, diff / np.where(b > 0, b, LD(1)), LD(0)))) if diff.size else 0.0
        if show:
            show(f"{name}: largest error / bound = {ratios[name]:.3g}")
        assert not bad.any(), (name, "first miss at", tuple(int(x) for x in np.argwhere(bad)[0]), "error", float(diff[bad][0]), "bound", float(b[bad][0]))

    def exact(name, a, r):
        assert np.array_equal(np.asarray(a).astype(np.int64), np.asarray(r).astype(np.int64)), (name, np.asarray(a), np.asarray(r))

    within("corner", got["corner"], ref["corner"], bound["corner"])
    exact("view.n_used", got["view"][:, 0], ref["view"][:, 0])
    within("view", got["view"], ref["view"], bound["view"])
    exact("view_worst", got["view_worst"], ref["view_worst"])
    for col, nm in ((0, "n_used"), (5, "worst_view"), (6, "n_views_used"), (7, "zero")):
        exact("camera." + nm, got["camera"][:, col], ref["camera"][:, col])
    within("camera", got["camera"], ref["camera"], bound["camera"])
    within("cost", got["cost"], ref["cost"], bound["cost"])
    within("rmse", got["rmse"], ref["rmse"], bound["rmse"])
    within("sum_w", got["sum_w"], ref["sum_w"], bound["sum_w"])
    assert got["n_used"] == ref["n_used"] and got["n_views_used"] == ref["n_views_used"]
    for f in ("grid", "angle"):
        if f in ref:
            exact(f + "_count", got[f + "_count"], ref[f + "_count"])
            exact(f + "_outside", got[f + "_outside"], ref[f + "_outside"])
            within(f, got[f], ref[f], bound[f], square=[2])
    return ratios
