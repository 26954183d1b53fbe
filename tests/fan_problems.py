"""Problems with prescribed corner geometry: every view is one board placed relative to the camera that sees it.

synth.make_problem and the rigs of tests/helpers.py put their boards on the bisector between two cameras and use the four
calibrated lens sets: no corner beyond 117 degrees of incidence, every lens a Triple Sphere next to the calibrated one,
every free camera rotation far from the small-angle branch.  Here the board centre of a view sits at a prescribed
incidence angle (0 .. 170 degrees, two azimuths off the image axes, 300 .. 900 mm away, the board tilted 0.3 rad off the
line of sight), the lens sets reach the Double Sphere (lambda = 0), the UCM (xi = lambda = 0), the pinhole limit, alpha
near 1, xi > 0 and alpha < 0, and the rotation vectors of free cameras and of boards step through both branches of the
angle-axis rotation and up to pi.  Two views are exact: corner (0, 0) on the optical axis of an identity camera
(X = Y = 0), and a board in the plane Z = 0.  Each frame is seen by one camera (legal: helpers.mixed_visibility_rig).

The parameters of a problem are its ground truth; the observations are the extended-precision projection
(tests/camera_ref.py) rounded to fp64 plus deterministic noise of 0.3 px, and every seventeenth corner is an outlier of
25 px, so that a robust loss of scale 1 px has corners on both sides of its knee.

A view is left out when the reference has k <= 0, or cond > 100 or cond_k > 100 (camera_ref) at one of its corners: outside
the model's domain, or next to its pole; the builder asserts that this stays the exception (conditions()).  The boards are
25 mm across (under 5 degrees at 300 mm), so that the view at 85 degrees stays inside the pinhole limit's half space.

The second half of the module holds the measures of the tests on these problems: errors in units of cond 2^-53.
"""
from __future__ import annotations

import functools

import numpy as np

from tscm_calib_amd import synth
from tscm_calib_amd.problem import Problem
from tests import camera_ref as R

ANGLES = (0.0, 30.0, 60.0, 85.0, 89.9, 90.0, 90.1, 95.0, 120.0, 150.0, 170.0)        # incidence of the board centre, degrees
AZIMUTHS = (0.6, 3.9)                                                                # radians; neither on an image axis
ROTATION_ANGLES = (60.0, 120.0)                                                      # incidence of the rotation-case views
COND_MAX = 100.0

#                         fx      fy      cx     cy     xi     lambda  alpha  b    c
LENS = dict(
    calibrated=synth.CALIB_INTR[0].copy(),
    ds=np.array([430.0, 430.0, 640.0, 520.0, -0.2, 0.0, 0.59, 0.0, 0.0]),
    ucm=np.array([430.0, 430.0, 640.0, 520.0, 0.0, 0.0, 0.62, 0.0, 0.0]),
    pinhole=np.array([430.0, 430.0, 640.0, 520.0, 0.0, 0.0, 0.0, 0.0, 0.0]),
    large_alpha=np.array([430.0, 430.0, 640.0, 520.0, -0.27, -0.088, 0.9, 0.0, 0.0]),
    positive_xi=np.array([300.0, 300.0, 640.0, 520.0, 0.8, 0.3, 0.5, 0.0, 0.0]),
    negative_alpha=np.array([430.0, 430.0, 640.0, 520.0, 0.3, 0.2, -0.3, 0.0, 0.0]),
    skewed=np.concatenate([synth.CALIB_INTR[1][:7], [0.8, -0.6]]),
)
GROUPS = dict(A=("calibrated", "ds", "ucm", "pinhole"), B=("large_alpha", "positive_xi", "negative_alpha", "skewed"))

# rotation vectors of free cameras and of boards: 0, both sides of theta^2 = DBL_EPSILON (1.49e-8 squared), small, next to pi
ROTATION_LENGTHS = (0.0, 1e-9, 1.2e-8, 1.6e-8, 1e-4, np.pi - 1e-6, 3.1415)
_AXES = np.array([[0.36, -0.48, 0.8], [-0.6, 0.64, 0.48], [0.48, 0.8, -0.36], [0.8, 0.36, 0.48],
                  [-0.48, 0.6, 0.64], [0.64, -0.48, -0.6], [0.6, 0.48, 0.64]])


def rotation_vector(i: int) -> np.ndarray:
    """Rotation case i: a generic axis (no zero component) times ROTATION_LENGTHS[i]."""
    a = _AXES[i] / np.linalg.norm(_AXES[i])
    return a * ROTATION_LENGTHS[i]


BOARDS = {"2x2": (2, 2), "9x6": (9, 6), "11x8": (11, 8)}          # KS = 1 and KS = 14 single-pass, two passes (g4_plan)
NAMES = tuple(f"{b}-{g}" for b in BOARDS for g in GROUPS) + tuple(f"{b}-mono" for b in BOARDS)


def _face(d):
    """Rotation whose third column is the unit vector d (the board's normal along the line of sight)."""
    up = np.array([0.0, 1.0, 0.0]) if abs(d[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, d); x /= np.linalg.norm(x)
    return np.stack([x, np.cross(d, x), d], axis=1)


def _direction(theta_deg, phi):
    t = np.deg2rad(theta_deg)
    return np.array([np.sin(t) * np.cos(phi), np.sin(t) * np.sin(phi), np.cos(t)])


def _views_of_camera(cam_rt, identity, centre, rng_u):
    """View specs of one camera: (kind, angle, board_rt) with the board pose in the rig frame.  kind: "fan" (the grid),
    "rot<i>" (board rotation case i), "axis" / "plane" (the exact views, identity cameras only)."""
    Rc, tc = synth.rodrigues(cam_rt[:3]), cam_rt[3:]
    out = []
    n = 0

    def dist():
        nonlocal n
        n += 1
        return 300.0 + 600.0 * rng_u[n % len(rng_u)]

    for a in ANGLES:
        for phi in AZIMUTHS:
            d = _direction(a, phi)
            Rv = _face(d) @ synth.rodrigues(np.array([0.3 * np.cos(phi + 1.0), 0.3 * np.sin(phi + 1.0), 0.0]))
            tv = dist() * d - Rv @ centre
            Rb = Rc.T @ Rv
            out.append(("fan", a, np.concatenate([synth.rotmat_to_aa(Rb), Rc.T @ (tv - tc)])))
    for i in range(len(ROTATION_LENGTHS)):
        for a, phi in zip(ROTATION_ANGLES, (1.1, 4.4)):
            wb = rotation_vector(i)
            Rv = Rc @ synth.rodrigues(wb)
            tv = dist() * _direction(a, phi) - Rv @ centre
            out.append((f"rot{i}", a, np.concatenate([wb, Rc.T @ (tv - tc)])))
    if identity:
        out.append(("axis", 0.0, np.array([0.0, 0.0, 0.0, 0.0, 0.0, dist()])))
        out.append(("plane", 90.0, np.array([0.0, 0.0, 0.0, dist(), 0.0, 0.0])))
    return out


@functools.lru_cache(maxsize=None)
def fan_problem(name: str) -> Problem:
    """Problem `name` of NAMES: "<board>-<A|B>" a 4-camera rig with the lens sets of GROUPS, "<board>-mono" the mono problem
    (calibrated lens).  Treat the result as read-only (it is cached).  meta: view_kind, view_angle, view_lens [V],
    left_out (the (lens, angle) pairs of the grid that lost a view), index (the rig's number: which rotations its cameras
    have)."""
    board, group = name.split("-")
    cols, rows = BOARDS[board]
    mono = group == "mono"
    index = NAMES.index(name)
    extent = np.hypot(cols - 1, rows - 1)
    pitch = 25.0 / extent                       # 25 mm across: under 5 degrees at 300 mm, so cond varies little inside a view
    bxy = synth.board_points(cols, rows, pitch)
    npts = bxy.shape[0]
    centre = np.array([0.5 * (cols - 1) * pitch, 0.5 * (rows - 1) * pitch, 0.0])
    rng = synth.CounterRNG(4100 + index)
    if mono:
        lenses, cam_rt = ("calibrated",), np.zeros((1, 6))
    else:
        lenses = GROUPS[group]
        cam_rt = np.zeros((4, 6))
        for m in range(4):
            i = (4 * index + m) % len(ROTATION_LENGTHS)
            cam_rt[m, :3] = rotation_vector(i)
            if i != 0:                          # rotation 0 goes with translation 0: an identity camera
                cam_rt[m, 3:] = (m + 1) * np.array([120.0, -80.0, 60.0])
    C = len(lenses)
    intr = np.stack([LENS[l] for l in lenses])
    specs = []
    for m in range(C):
        ident = not cam_rt[m].any()
        for kind, a, brt in _views_of_camera(cam_rt[m], ident, centre, rng.uniform(50 + m, np.arange(64))):
            specs.append((m, kind, a, brt))
    V = len(specs)
    cnt = np.full(V, npts, dtype=np.int32)
    if board == "2x2":
        cnt[4::10] = 1                          # a tenth of the views hold one corner: nothing averages in their products

    def problem(sel, obs_u, obs_v):
        s = [specs[i] for i in sel]
        n = len(s)
        return Problem(C, n, bxy, np.array([x[0] for x in s], dtype=np.int32), np.arange(n, dtype=np.int32),
                       (np.arange(n) * npts).astype(np.int32), cnt[sel], obs_u, obs_v, cam_rt.copy(), intr.copy(),
                       np.stack([x[3] for x in s]), np.zeros(C, dtype=np.uint8), mono).normalised()

    # every candidate view through the reference: leave out what is outside the model's domain or next to its pole
    cand = problem(np.arange(V), np.zeros(V * npts), np.zeros(V * npts))
    ref = R.evaluate(cand)
    bad = np.zeros(V, dtype=bool)
    np.logical_or.at(bad, ref["view"], ~((ref["k"] > 0) & (ref["cond"] <= COND_MAX) & (ref["cond_k"] <= COND_MAX)))
    keep = np.nonzero(~bad)[0]
    pix = np.zeros((V * npts, 2))
    _, _, at = R.corner_index(cand)
    pix[at] = np.asarray(ref["pix"], dtype=np.float64)
    pix = pix.reshape(V, npts, 2)[keep].reshape(-1, 2)
    k = np.arange(pix.shape[0])
    obs_u = pix[:, 0] + 0.3 * rng.normal(20, k)
    obs_v = pix[:, 1] + 0.3 * rng.normal(21, k)
    obs_u[::17] += np.where(k[::17] % 2 == 0, 25.0, -25.0)
    p = problem(keep, obs_u, obs_v)
    kept = [specs[i] for i in keep]
    p.meta = dict(name=name, index=index, lenses=lenses, view_kind=np.array([x[1] for x in kept]),
                  view_angle=np.array([x[2] for x in kept]), view_lens=np.array([lenses[x[0]] for x in kept]),
                  left_out=sorted({(lenses[specs[i][0]], specs[i][2]) for i in np.nonzero(bad)[0] if specs[i][1] == "fan"}),
                  dropped_kinds=sorted({(lenses[specs[i][0]], specs[i][1], specs[i][2]) for i in np.nonzero(bad)[0] if specs[i][1] != "fan"}))
    conditions(p)
    return p


def conditions(p: Problem) -> None:
    """What keeps the fan problems from being hollowed out by a later edit: at most a third of a problem's (lens, angle)
    pairs left out, no lens without an angle above 60 degrees, every board rotation case present for every camera, the
    problem small enough for a test of a few seconds."""
    lenses = p.meta["lenses"]
    assert len(p.meta["left_out"]) * 3 <= len(lenses) * len(ANGLES), p.meta["left_out"]
    fan = p.meta["view_kind"] == "fan"
    for l in lenses:
        mine = p.meta["view_lens"] == l
        assert (p.meta["view_angle"][fan & mine] > 60.0).any(), l
        for i in range(len(ROTATION_LENGTHS)):
            assert (mine & (p.meta["view_kind"] == f"rot{i}")).any(), (l, i)
    assert 0 < p.n_views < 2000


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """camera_ref.evaluate of fan_problem(name), with cond_view [V] (the largest cond of each view's corners; read-only)."""
    p = fan_problem(name)
    ref = R.evaluate(p)
    ref["cond_view"] = np.asarray(R.view_max(ref["cond_ext"], ref["view"], p.n_views), dtype=np.float64)
    return ref


# ----------------------------------------------------------------------------- error measures
U = 2.0 ** -53
# the columns of one unit: rotations (px / rad), translations (px / mm), focal lengths (px / px), centre (exact), xi lambda alpha (px)
BLOCKS = dict(cam_rot=("Jc", slice(0, 3)), cam_t=("Jc", slice(3, 6)), board_rot=("Jb", slice(0, 3)), board_t=("Jb", slice(3, 6)),
              focal=("Ji", slice(0, 2)), centre=("Ji", slice(2, 4)), shape=("Ji", slice(4, 7)))


def column_cond(p: Problem, ref: dict, amplify=None):
    """The condition number of every Jacobian column of every view: cE [V, 6] (board pose), cF [V, 15] (camera pose,
    intrinsics, b, c), cr [V] (residual).  cond_ext of the view's worst corner, plus the rotation's own term in the three
    columns of a rotation vector (camera_ref.rotation_cond) and cond_rig in the three columns of the board's translation.  amplify [N]: a factor per corner on everything of its view
    (robust_amplification), the largest of the view."""
    V = p.n_views
    cv = ref["cond_view"]
    if amplify is not None:
        cv = cv * np.asarray(R.view_max(np.asarray(amplify, dtype=np.float64), ref["view"], V))
    rb = np.asarray(R.view_max(ref["rot_board"], ref["view"], V), dtype=np.float64)
    rc = np.asarray(R.view_max(ref["rot_cam"], ref["view"], V), dtype=np.float64)
    rig = np.asarray(R.view_max(ref["cond_rig"], ref["view"], V), dtype=np.float64) * (cv / ref["cond_view"])
    cE = np.repeat(cv[:, None], 6, axis=1); cE[:, :3] += rb[:, None]; cE[:, 3:] += rig[:, None]
    cF = np.repeat(cv[:, None], 15, axis=1); cF[:, :3] += rc[:, None]
    return cE, cF, cv


def _ratio(err, scale, cond):
    err, scale = np.asarray(err, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0)) / (cond * U)


def row_ratios(p: Problem, ref: dict, res, Jc, Jb, Ji) -> dict:
    """Per corner, the error of a candidate's residuals and Jacobian rows against the reference in units of cond 2^-53:
    each Jacobian entry relative to the largest entry of its block (BLOCKS: the columns of one unit) over the corner's
    view; each residual relative to |f m| + |c|, the size of the terms
    of the pixel it is taken from.  One array [N] per block of BLOCKS and "residual"."""
    view = ref["view"]
    cE, cF, cr = column_cond(p, ref)
    cand = dict(Jc=np.asarray(Jc).reshape(-1, 2, 6), Jb=np.asarray(Jb).reshape(-1, 2, 6), Ji=np.asarray(Ji).reshape(-1, 2, 9))
    cond = dict(Jc=cF[:, :6], Jb=cE, Ji=cF[:, 6:])
    out = {}
    for name, (key, cols) in BLOCKS.items():
        if p.mono and key == "Jc":
            continue
        a, b = cand[key][:, :, cols], ref[key][:, :, cols]
        scale = np.zeros(p.n_views, dtype=b.dtype)
        np.maximum.at(scale, view, np.abs(b).max(axis=(1, 2)))
        out[name] = _ratio(np.abs(a - b).max(axis=1), scale[view][:, None], cond[key][:, cols][view]).max(axis=1)
    c = np.asarray(p.intr)[np.asarray(p.view_camera)[view]][:, 2:4]
    scale = np.abs(ref["pix"] - c) + np.abs(c)
    out["residual"] = _ratio(np.abs(np.asarray(res).reshape(-1, 2) - ref["res"]), scale, cr[view][:, None]).max(axis=1)
    return out


def _group_max(values, index, n):
    out = np.zeros((n,) + values.shape[1:])
    np.maximum.at(out, index, values)
    return out


def gram_ratios(p: Problem, ref: dict, g: dict, o: dict, unit=None, weights=None, amplify=None) -> dict:
    """The entry errors of helpers.gram_entry_errors (Cauchy-Schwarz units) over the entry's condition number times
    2^-53: per view for view_cross [V], per board for board_gram / board_grad [B], per camera for cam_gram / cam_grad
    [C] (the largest condition number among the views of that board or camera; of an entry's two columns, the larger).
    A gradient entry sum a_i r carries the error of r as well, and r = observed - pixel is rounded like the pixel, a sum
    of terms of size s = |f m| + |c|, not like |r|: its condition number is that of the entry times 1 + |s| / |r| (2-norms
    over the board's or the camera's corners; weights [N]: the factors both were scaled by).
    unit: a dict of per-key tolerances (as TOL_F32 of test_gpu_gram_kernels.py) that replaces 2^-53, times max(1, cond)."""
    from tests import helpers as H
    e = H.gram_entry_errors(g, o, p)
    keep = e["columns"]
    cE, cF, cr = column_cond(p, ref, amplify)
    vb, vc = np.asarray(p.view_board), np.asarray(p.view_camera)
    cEb, crb = _group_max(cE, vb, p.n_boards), _group_max(cr, vb, p.n_boards)
    cFc, crc = _group_max(cF, vc, p.n_cameras)[:, keep], _group_max(cr, vc, p.n_cameras)
    cF = cF[:, keep]
    c = np.asarray(p.intr)[vc[ref["view"]]][:, 2:4]
    ss = np.asarray(np.sum((np.abs(ref["pix"] - c) + np.abs(c)) ** 2, axis=1), dtype=np.float64) * (1.0 if weights is None else np.asarray(weights, dtype=np.float64) ** 2)
    rr_b, rr_c = np.asarray(o["board_rr"], dtype=np.float64), np.asarray(o["cam_rr"], dtype=np.float64)
    gb = 1.0 + np.sqrt(np.bincount(vb[ref["view"]], weights=ss, minlength=p.n_boards) / np.where(rr_b > 0, rr_b, 1.0))
    gc = 1.0 + np.sqrt(np.bincount(vc[ref["view"]], weights=ss, minlength=p.n_cameras) / np.where(rr_c > 0, rr_c, 1.0))
    cond = dict(view_cross=np.maximum(cE[:, :, None], cF[:, None, :]), board_gram=np.maximum(cEb[:, :, None], cEb[:, None, :]),
                board_grad=np.maximum(cEb, crb[:, None]) * gb[:, None], cam_gram=np.maximum(cFc[:, :, None], cFc[:, None, :]),
                cam_grad=np.maximum(cFc, crc[:, None]) * gc[:, None])
    out = {}
    board_corners = np.bincount(vb, weights=p.view_count, minlength=p.n_boards)
    short = dict(view_cross=np.asarray(p.view_count) < 4, board_gram=board_corners < 4, board_grad=board_corners < 4)
    for key, c in cond.items():
        if unit is None:
            r = e[key] / (c * U)
        else:
            tol = np.full(e[key].shape[0], unit[key])
            if key in short:
                tol[short[key]] = unit[key + "_short"]
            r = e[key] / (np.maximum(1.0, c) * tol.reshape((-1,) + (1,) * (c.ndim - 1)))
        out[key] = r.reshape(r.shape[0], -1).max(axis=1) if r.size else np.zeros(r.shape[0])
    return out


def reference_normal_equations(p: Problem, ref: dict, weights=None, rows=None) -> dict:
    """The reference's rows as normal equations (helpers.normal_equations_from in longdouble).  weights [N]: every corner's
    rows scaled (a robust loss: sqrt(rho')); rows: (res, Jc, Jb, Ji) instead of the reference's own."""
    from tests import helpers as H
    res, Jc, Jb, Ji = (ref["res"], ref["Jc"], ref["Jb"], ref["Ji"]) if rows is None else rows
    if weights is not None:
        w = np.asarray(weights, dtype=np.longdouble)
        res, Jc, Jb, Ji = res * w[:, None], Jc * w[:, None, None], Jb * w[:, None, None], Ji * w[:, None, None]
    return H.normal_equations_from(p, res, Jc, Jb, Ji, dtype=np.longdouble)


def robust_weights(p: Problem, ref: dict, kind: str, a: float = 1.0):
    """Ceres' HuberLoss / SoftLOneLoss / CauchyLoss of scale a at the reference's residuals, in longdouble:
    (sqrt(rho') [N], sum rho / 2, amplification [N], s = |r|^2 [N]).  The weight is a function of s, which a kernel
    knows only as well as its residual: d(rho') / rho' = (rho'' / rho') 2 |r| dr with dr = cond 2^-53 S, S = |f m| + |c|
    the size of the pixel's terms -- every product of the corner carries 1 + |rho'' / rho'| 2 |r| S times the rounding of
    a plain one."""
    LD = np.longdouble
    s = np.sum(ref["res"] ** 2, axis=1)
    b = LD(a) * LD(a)
    if kind == "huber":
        big = s > b
        rs = np.sqrt(np.where(big, s, 1))
        rho, r1, q = np.where(big, 2 * a * rs - b, s), np.where(big, a / rs, 1), np.where(big, 1 / (2 * np.where(big, s, 1)), 0)
    elif kind == "soft_l1":
        t = np.sqrt(1 + s / b)
        rho, r1, q = 2 * b * (t - 1), 1 / t, 1 / (2 * (b + s))
    elif kind == "cauchy":
        rho, r1, q = b * np.log1p(s / b), 1 / (1 + s / b), 1 / (b + s)
    else:
        raise ValueError(kind)
    c = np.asarray(p.intr)[np.asarray(p.view_camera)[ref["view"]]][:, 2:4]
    S = np.sqrt(np.sum((np.abs(ref["pix"] - c) + np.abs(c)) ** 2, axis=1))
    return np.sqrt(r1), float(LD(0.5) * np.sum(rho)), np.asarray(1 + q * 2 * np.sqrt(s) * S, dtype=np.float64), s
