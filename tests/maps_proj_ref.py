"""fp64 numpy reference of the remap tables with an output image that is not a pinhole (tscm.h TSCM_PROJ_*:
tscm_build_maps_ex) and of the point direction (tscm_rectify_points).  Independent of the library: only numpy.

Every function takes a tscm_calib_amd.maps.MapDesc-like object (attributes intr, R, fx, fy, cx, cy, width, height,
offset_x, offset_y, out_offset, out_stride, check_w2, w2, projection as an integer kind)."""
import functools

import numpy as np

PERSPECTIVE, LONGLAT, CYLINDRICAL, STEREOGRAPHIC, EQUIRECT = 0, 1, 2, 3, 4
KINDS = (PERSPECTIVE, LONGLAT, CYLINDRICAL, STEREOGRAPHIC, EQUIRECT)
NAMES = {PERSPECTIVE: "perspective", LONGLAT: "longlat", CYLINDRICAL: "cylindrical", STEREOGRAPHIC: "stereographic", EQUIRECT: "equirect"}
W2_BAND = 1e-9          # |Z + w2 d1| < W2_BAND d1: the w2 rule is decided by rounding there


def ray(kind, a, b):
    """The ray before R of normalised output coordinates a = (j - cx)/fx, b = (i - cy)/fy -> [..., 3]."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    if kind == PERSPECTIVE:
        r = (a, b, np.ones_like(a))
    elif kind == LONGLAT:
        r = (np.sin(a), np.cos(a) * np.sin(b), np.cos(a) * np.cos(b))
    elif kind == CYLINDRICAL:
        r = (np.sin(a), b, np.cos(a))
    elif kind == STEREOGRAPHIC:
        h = 0.25 * (a * a + b * b)
        r = (a / (1.0 + h), b / (1.0 + h), (1.0 - h) / (1.0 + h))
    elif kind == EQUIRECT:
        r = (np.cos(b) * np.sin(a), np.sin(b), np.cos(b) * np.cos(a))
    else:
        raise ValueError(kind)
    return np.stack(r, axis=-1)


def inverse_ray(kind, r):
    """(a, b, inside the kind's domain) of rays [..., 3] (any positive length)."""
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    ok = np.ones(x.shape, dtype=bool)
    with np.errstate(all="ignore"):
        if kind == PERSPECTIVE:
            a, b, ok = x / z, y / z, z > 0.0
        elif kind == LONGLAT:
            a, b = np.arctan2(x, np.hypot(y, z)), np.arctan2(y, z)
        elif kind == CYLINDRICAL:
            h = np.hypot(x, z)
            a, b, ok = np.arctan2(x, z), y / h, h != 0.0
        elif kind == STEREOGRAPHIC:
            d = np.sqrt(x * x + y * y + z * z) + z
            a, b, ok = 2.0 * x / d, 2.0 * y / d, d > 0.0
        elif kind == EQUIRECT:
            a, b = np.arctan2(x, z), np.arctan2(y, np.hypot(x, z))
        else:
            raise ValueError(kind)
    return a, b, ok


def project_ref(intr, P):
    """TripleSphereCamera::project with the skew terms: P [..., 3] -> u, v, Z, d1."""
    fx, fy, cx, cy, xi, lam, al, sb, sc = [float(t) for t in np.asarray(intr, dtype=np.float64).ravel()]
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    with np.errstate(all="ignore"):
        rho2 = X * X + Y * Y
        d1 = np.sqrt(rho2 + Z * Z)
        z1 = Z + xi * d1
        d2 = np.sqrt(rho2 + z1 * z1)
        z2 = z1 + lam * d2
        d3 = np.sqrt(rho2 + z2 * z2)
        ksai = z2 + al / (1.0 - al) * d3
        u = fx * X / ksai + sb * Y / ksai + cx
        v = sc * X / ksai + fy * Y / ksai + cy
    return u, v, Z, d1


def unproject_ref(intr, px):
    """get_unit_sphere_coordinate with the identity transform: pixels [..., 2] -> unit rays [..., 3] (NaN outside the domain)."""
    fx, fy, cx, cy, xi, lam, al, sb, sc = [float(t) for t in np.asarray(intr, dtype=np.float64).ravel()]
    x, y = px[..., 0] - cx, px[..., 1] - cy
    det = fx * fy - sb * sc
    mx, my = (fy * x - sb * y) / det, (-sc * x + fx * y) / det
    ksai = al / (1.0 - al)
    r2 = mx * mx + my * my
    with np.errstate(all="ignore"):
        gamma = (ksai + np.sqrt(1.0 + (1.0 - ksai * ksai) * r2)) / (r2 + 1.0)
        gk = gamma - ksai
        yita = lam * gk + np.sqrt((gk * gk - 1.0) * lam * lam + 1.0)
        ml = yita * gk - lam
        mu = xi * ml + np.sqrt(xi * xi * (ml * ml - 1.0) + 1.0)
        return np.stack([mu * yita * gamma * mx, mu * yita * gamma * my, mu * ml - xi], axis=-1)


def source_pixels(d, i, j):
    """Output elements (i, j) of map `d` -> (u, v) in the sampled camera BEFORE the offsets, fails_w2, near_w2."""
    R = np.asarray(d.R, dtype=np.float64).reshape(3, 3)
    a = (np.asarray(j, dtype=np.float64) - d.cx) / d.fx
    b = (np.asarray(i, dtype=np.float64) - d.cy) / d.fy
    r = ray(int(d.projection), a, b)
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    P = np.stack([R[k, 0] * x + R[k, 1] * y + R[k, 2] * z for k in range(3)], axis=-1)
    u, v, Z, d1 = project_ref(d.intr, P)
    return u, v, Z <= -d.w2 * d1, np.abs(Z + d.w2 * d1) < W2_BAND * d1


def build_map_ref(d):
    """One table: mapx, mapy (float32 [height, width]) and the elements whose w2 decision is a matter of rounding."""
    i, j = np.meshgrid(np.arange(d.height), np.arange(d.width), indexing="ij")
    u, v, fails, near = source_pixels(d, i, j)
    if d.check_w2:
        u, v = np.where(fails, -1.0, u), np.where(fails, -1.0, v)
    else:
        near = np.zeros_like(near)
    with np.errstate(over="ignore"):
        return (u + d.offset_x).astype(np.float32), (v + d.offset_y).astype(np.float32), near


def build_maps_ref(descs, n_elems):
    """A batch as tscm_build_maps_ex lays it out: flat mapx, mapy (zeros where no map writes), written mask, near-w2 mask."""
    mapx, mapy = np.zeros(n_elems, dtype=np.float32), np.zeros(n_elems, dtype=np.float32)
    written, near = np.zeros(n_elems, dtype=bool), np.zeros(n_elems, dtype=bool)
    for d in descs:
        if d.width == 0 or d.height == 0:
            continue
        mx, my, nr = build_map_ref(d)
        idx = d.out_offset + np.arange(d.height)[:, None] * d.out_stride + np.arange(d.width)[None, :]
        mapx[idx], mapy[idx], written[idx], near[idx] = mx, my, True, nr
    return mapx, mapy, written, near


def rectify_points_ref(d, pixels):
    """tscm_rectify_points: pixels [n, 2] of the sampled camera -> (xy [n, 2] in the output image, valid [n])."""
    px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
    R = np.asarray(d.R, dtype=np.float64).reshape(3, 3)
    c = unproject_ref(d.intr, px)
    ok = np.all(np.isfinite(c), axis=-1)
    with np.errstate(all="ignore"):
        if d.check_w2:
            ok &= ~(c[:, 2] <= -d.w2 * np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]))
        r = np.stack([R[0, k] * c[:, 0] + R[1, k] * c[:, 1] + R[2, k] * c[:, 2] for k in range(3)], axis=-1)      # R^T
        a, b, inside = inverse_ray(int(d.projection), r)
        ok &= inside
        xy = np.stack([a * d.fx + d.cx, b * d.fy + d.cy], axis=-1)
    xy[~ok] = np.nan
    return xy, ok


# ---- the round trip of the reference itself: the yardstick of the device tolerances
class Desc:
    """The attributes of a MapDesc, for tests that must not need the library."""
    def __init__(self, intr, R, fx, fy, cx, cy, width, height, projection, check_w2=0, w2=0.42399, offset_x=0.0, offset_y=0.0,
                 out_offset=0, out_stride=0):
        self.intr, self.R = np.asarray(intr, dtype=np.float64), np.asarray(R, dtype=np.float64).reshape(3, 3)
        self.fx, self.fy, self.cx, self.cy, self.width, self.height = fx, fy, cx, cy, width, height
        self.projection, self.check_w2, self.w2, self.offset_x, self.offset_y = projection, check_w2, w2, offset_x, offset_y
        self.out_offset, self.out_stride = out_offset, out_stride or width


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def round_trip_desc(kind, intr, R=None):
    """A 640 x 320 output image of `kind` (the default size of maps.rectify_pair_descs) that spans 150 x 100 degrees
    (PERSPECTIVE, STEREOGRAPHIC: the same extent in their own units), sampled from camera `intr`."""
    w, h = 640, 320
    ax, ay = np.radians(75.0), np.radians(50.0)
    ex = {PERSPECTIVE: np.tan(ax), STEREOGRAPHIC: 2 * np.tan(ax / 2)}.get(kind, ax)
    ey = {PERSPECTIVE: np.tan(ay), STEREOGRAPHIC: 2 * np.tan(ay / 2), CYLINDRICAL: np.tan(ay)}.get(kind, ay)
    return Desc(intr, np.eye(3) if R is None else R, 0.5 * w / ex, 0.5 * h / ey, 0.5 * w, 0.5 * h, w, h, kind)


def round_trip(d, step=5):
    """Every step-th output element -> source pixels -> rectify_points_ref: (largest |error| in output pixels over the elements whose
    source pixel exists, the grid [n, 2] as (x, y), the source pixels [n, 2])."""
    i, j = np.meshgrid(np.arange(0, d.height, step), np.arange(0, d.width, step), indexing="ij")
    u, v, _, _ = source_pixels(d, i, j)
    src = np.stack([u.ravel(), v.ravel()], axis=-1)
    grid = np.stack([j.ravel(), i.ravel()], axis=-1).astype(np.float64)
    xy, ok = rectify_points_ref(d, src)
    return float(np.max(np.abs(xy[ok] - grid[ok]))), grid, src, ok


@functools.lru_cache(maxsize=None)
def round_trip_error(kind):
    """The largest round-trip error (output pixels) of the reference for `kind` over the four cameras of the golden
    calibration, with and without a rotation: what fp64 and numpy's own sin / atan2 leave of an identity."""
    from tscm_calib_amd import synth
    rng = np.random.default_rng(1234)
    worst = 0.0
    for intr in synth.CALIB_INTR:
        for R in (None, rotation(rng) if kind != PERSPECTIVE else None):
            err, _, _, ok = round_trip(round_trip_desc(kind, intr, None if R is None else _small(R)))
            assert ok.all()
            worst = max(worst, err)
    return worst


def _small(R):
    """A rotation by at most ~17 degrees in the direction of R (keeps the round-trip image inside every camera's domain)."""
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    w = 0.3 * w / max(np.linalg.norm(w), 1e-300)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def point_tolerance(kind):
    """tscm_rectify_points against the reference: 64 x the reference's own round-trip error, at least 1e-10 px."""
    return max(64.0 * round_trip_error(kind), 1e-10)


def pair_points(n=200, seed=77):
    """n world points in front of the camera pair (0, 1) of synth.CALIB_*, and their pixels in both cameras."""
    from tscm_calib_amd import synth
    rng = np.random.default_rng(seed)
    T = synth.CALIB_TWC
    x = T[1][:, 3] - T[0][:, 3]
    x /= np.linalg.norm(x)
    z = np.array([-x[2], 0.0, x[0]])
    z /= np.linalg.norm(z)
    Rp = np.stack([x, np.cross(z, x), z], axis=1)
    out = []
    while len(out) < n:
        a, b = rng.uniform(-0.6, 0.6), rng.uniform(-0.5, 0.5)
        Pw = 0.5 * (T[0][:, 3] + T[1][:, 3]) + rng.uniform(800.0, 6000.0) * (Rp @ ray(LONGLAT, a, b))
        px = []
        for k in (0, 1):
            Pc = T[k][:, :3].T @ (Pw - T[k][:, 3])
            u, v, Z, d1 = project_ref(synth.CALIB_INTR[k], Pc)
            if 0 <= u < synth.IMG_W and 0 <= v < synth.IMG_H and Z > 0.2 * d1:
                px.append((u, v))
        if len(px) == 2:
            out.append((Pw, px[0], px[1]))
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])
