"""Host restatement of the sphere sweep defined in include/tscm/tscm.h (tscm_sweep_*, tscm_build_sweep_maps): sample, alpha,
census, the pair cost, aggregation, winner and the points.  Integer arithmetic up to the index map, so the device result is
compared with array_equal.  It restates only what is new -- the wrap of the census window, the pair cost, the rule of the
uncovered winner, the interpolation of the points, the centre term of the tables -- and imports the rest: the samples from
tests/pano_ref.py, the census, the aggregation and the winner from tests/stereo_ref.py, the rays and the projection from
tests/maps_proj_ref.py."""
import numpy as np

from tests import maps_proj_ref as mref
from tests import pano_ref, stereo_ref

INVALID = -16
DEFAULTS = dict(p1=8, p2=32, paths=8, uniqueness_ratio=10, wrap_x=True)


# ------------------------------------------------------------------------------------------------ tables
def source_pixels(d, center, inv, i, j):
    """maps_proj_ref.source_pixels with the centre term: the ray in front of R is dir - inv * center."""
    R = np.asarray(d.R, dtype=np.float64).reshape(3, 3)
    a = (np.asarray(j, dtype=np.float64) - d.cx) / d.fx
    b = (np.asarray(i, dtype=np.float64) - d.cy) / d.fy
    r = mref.ray(int(d.projection), a, b) - float(inv) * np.asarray(center, dtype=np.float64)
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    P = np.stack([R[k, 0] * x + R[k, 1] * y + R[k, 2] * z for k in range(3)], axis=-1)
    u, v, Z, d1 = mref.project_ref(d.intr, P)
    return u, v, Z <= -d.w2 * d1, np.abs(Z + d.w2 * d1) < mref.W2_BAND * d1


def build_sweep_maps_ref(descs, centers, inv_distance):
    """mapx, mapy float32 [n, D, h, w] and the elements whose w2 decision is a matter of rounding."""
    n, D = len(descs), len(inv_distance)
    h, w = descs[0].height, descs[0].width
    mapx, mapy = np.zeros((n, D, h, w), np.float32), np.zeros((n, D, h, w), np.float32)
    near = np.zeros((n, D, h, w), bool)
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for k, d in enumerate(descs):
        for z, inv in enumerate(inv_distance):
            u, v, fails, nr = source_pixels(d, centers[k], inv, i, j)
            if d.check_w2:
                u, v = np.where(fails, -1.0, u), np.where(fails, -1.0, v)
                near[k, z] = nr
            with np.errstate(over="ignore"):
                mapx[k, z], mapy[k, z] = (u + d.offset_x).astype(np.float32), (v + d.offset_y).astype(np.float32)
    return mapx, mapy, near


# ------------------------------------------------------------------------------------------------ sweep
def census(plane, wrap: bool) -> np.ndarray:
    """stereo_ref.census of one plane; wrap: 4 columns of the other end on each side, cropped again, so that the clamped
    census stays the single source (the padded columns are all a 9-wide window can reach)."""
    plane = np.asarray(plane)
    if not wrap:
        return stereo_ref.census(plane)
    return stereo_ref.census(np.pad(plane, ((0, 0), (4, 4)), mode="wrap"))[:, 4:-4]


def cost_volume(cen, a) -> np.ndarray:
    """cen uint64 [n, D, ph, pw], a [n, D, ph, pw] -> C uint8 [ph, pw, D]"""
    n = cen.shape[0]
    on = np.asarray(a) > 0
    cnt = on.sum(axis=0).astype(np.int64)
    total = np.zeros(cnt.shape, dtype=np.int64)
    for p in range(n):
        for q in range(p + 1, n):
            total += np.where(on[p] & on[q], stereo_ref.popcount64(cen[p] ^ cen[q]), 0)
    P = cnt * (cnt - 1) // 2
    C = np.where(cnt >= 2, (total + (P >> 1)) // np.maximum(P, 1), 64)
    return np.moveaxis(C, 0, -1).astype(np.uint8)


def index_map(S, C, uniqueness_ratio: int) -> np.ndarray:
    out = stereo_ref.disparity(S, 0, uniqueness_ratio, -1)
    ks = S.astype(np.int64).argmin(axis=-1)
    uncovered = np.take_along_axis(C, ks[..., None], axis=-1)[..., 0] == 64
    return np.where(uncovered, INVALID, out).astype(np.int16)


def stages(images, weights, mapx, mapy, **params) -> dict:
    """Everything tscm_sweep_stages / tscm_sweep_depth give for one frame.  images: n arrays [h, w] uint8; weights: None or
    n entries (None or [h, w] uint8); mapx, mapy: [n, D, ph, pw] float32."""
    p = dict(DEFAULTS, **params)
    n, D = mapx.shape[:2]
    h, w = images[0].shape
    v = np.stack([np.stack([pano_ref.sample(images[k], mapx[k, z], mapy[k, z])[..., 0] for z in range(D)]) for k in range(n)])
    a = np.stack([np.stack([pano_ref.alpha(None if weights is None else weights[k], w, h, mapx[k, z], mapy[k, z]) for z in range(D)]) for k in range(n)])
    cen = np.stack([np.stack([census(v[k, z], p["wrap_x"]) for z in range(D)]) for k in range(n)])
    C = cost_volume(cen, a)
    S = stereo_ref.aggregate(C, p["p1"], p["p2"], p["paths"])
    return dict(sampled=v, alpha=a, census=cen, cost=C, aggregated=S, index16=index_map(S, C, p["uniqueness_ratio"]), params=p)


def points(index16, d, inv_distance):
    """tscm_sweep_points by the header's formulas -> (points [h, w, 3] in the output frame, valid [h, w])."""
    idx = np.asarray(index16).astype(np.int64)
    inv_distance = np.asarray(inv_distance, dtype=np.float64)
    h, w = idx.shape
    D = inv_distance.size
    ok = idx >= 0
    s = np.where(ok, idx, 0) / 16.0
    k0 = np.minimum(np.floor(s).astype(np.int64), D - 2)
    inv = inv_distance[k0] + (s - k0) * (inv_distance[k0 + 1] - inv_distance[k0])
    ok &= inv > 0
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    r = mref.ray(int(d.projection), (j - d.cx) / d.fx, (i - d.cy) / d.fy)
    P = r / np.where(ok, inv, 1.0)[..., None]
    P[~ok] = np.nan
    return P, ok
