"""Host restatement of the stereo matcher defined in include/tscm/tscm.h (tscm_stereo_*): 9 x 7 census, Hamming cost,
semi-global aggregation, winner / uniqueness / left-right check / sub-pixel, and the points of a disparity map.  Integer
arithmetic throughout, so the device result is compared with array_equal.  Written row-parallel (a whole image row per
step), unlike the kernels, which walk one scanline per wave."""
import numpy as np

DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))
DEFAULTS = dict(min_disparity=0, num_disparities=128, p1=8, p2=32, paths=8, uniqueness_ratio=10, disp12_max_diff=1)

_POP8 = np.array([bin(v).count("1") for v in range(256)], dtype=np.uint8)


def popcount64(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return _POP8[a.view(np.uint8).reshape(a.shape + (8,))].sum(axis=-1).astype(np.int32)


def census(img) -> np.ndarray:
    img = np.asarray(img).astype(np.int32)
    h, w = img.shape
    pad = np.pad(img, ((3, 3), (4, 4)), mode="edge")             # clamped coordinates
    code = np.zeros((h, w), dtype=np.uint64)
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            nb = pad[3 + dy:3 + dy + h, 4 + dx:4 + dx + w]
            code = (code << np.uint64(1)) | (nb < img).astype(np.uint64)
    return code


def cost_volume(cl, cr, min_disparity: int, D: int) -> np.ndarray:
    h, w = cl.shape
    C = np.full((h, w, D), 64, dtype=np.uint8)
    xs = np.arange(w)
    for k in range(D):
        xr = xs - (min_disparity + k)
        ok = (xr >= 0) & (xr < w)
        if ok.any():
            C[:, ok, k] = popcount64(cl[:, ok] ^ cr[:, xr[ok]])
    return C


def path_step(c, prev, p1: int, p2: int):
    """L_r(p, .) from C(p, .) and L_r(p - r, .); the last axis is k."""
    m = prev.min(axis=-1, keepdims=True)
    best = np.minimum(prev, m + p2)
    best[..., 1:] = np.minimum(best[..., 1:], prev[..., :-1] + p1)
    best[..., :-1] = np.minimum(best[..., :-1], prev[..., 1:] + p1)
    return c + best - m


def aggregate_direction(C, dx: int, dy: int, p1: int, p2: int) -> np.ndarray:
    C = C.astype(np.int32)
    h, w, _ = C.shape
    L = np.zeros_like(C)
    if dy == 0:
        prev = None
        for x in (range(w) if dx > 0 else range(w - 1, -1, -1)):
            L[:, x] = C[:, x] if prev is None else path_step(C[:, x], prev, p1, p2)
            prev = L[:, x]
        return L
    prev_row = None
    for y in (range(h) if dy > 0 else range(h - 1, -1, -1)):
        L[y] = C[y]
        if prev_row is not None:
            src = np.arange(w) - dx
            ok = (src >= 0) & (src < w)                          # elsewhere the predecessor is outside: L = C
            L[y, ok] = path_step(C[y, ok], prev_row[src[ok]], p1, p2)
        prev_row = L[y]
    return L


def aggregate(C, p1: int, p2: int, paths: int) -> np.ndarray:
    S = np.zeros(C.shape, dtype=np.int32)
    for dx, dy in DIRECTIONS[:paths]:
        S += aggregate_direction(C, dx, dy, p1, p2)
    assert S.max() < 65536
    return S.astype(np.uint16)


def right_winner(S, min_disparity: int) -> np.ndarray:
    S = S.astype(np.int32)
    h, w, D = S.shape
    kR = np.full((h, w), -1, dtype=np.int32)
    for x2 in range(w):
        ks = np.array([k for k in range(D) if 0 <= x2 + min_disparity + k < w], dtype=np.int64)
        if ks.size:
            kR[:, x2] = ks[S[:, x2 + min_disparity + ks, ks].argmin(axis=1)]      # argmin: the first, i.e. lowest, k
    return kR


def disparity(S, min_disparity: int, uniqueness_ratio: int, disp12_max_diff: int) -> np.ndarray:
    S = S.astype(np.int64)
    h, w, D = S.shape
    ks = S.argmin(axis=-1)
    yy, xx = np.mgrid[0:h, 0:w]
    smin = S[yy, xx, ks]
    valid = np.ones((h, w), dtype=bool)
    if uniqueness_ratio > 0:
        far = np.abs(np.arange(D)[None, None, :] - ks[..., None]) > 1
        valid &= ~(far & (S * (100 - uniqueness_ratio) < smin[..., None] * 100)).any(axis=-1)
    if disp12_max_diff >= 0:
        kR = right_winner(S, min_disparity)
        x2 = xx - (min_disparity + ks)
        inside = (x2 >= 0) & (x2 < w)
        valid &= inside
        valid &= np.abs(kR[yy, np.clip(x2, 0, w - 1)] - ks) <= disp12_max_diff
    out = 16 * (min_disparity + ks)
    inner = (ks > 0) & (ks < D - 1)
    sm, sp = S[yy, xx, np.clip(ks - 1, 0, D - 1)], S[yy, xx, np.clip(ks + 1, 0, D - 1)]
    den = np.maximum(sm + sp - 2 * smin, 1)
    out = np.where(inner, out + ((sm - sp) * 16 + den) // (2 * den), out)         # floor division
    return np.where(valid, out, 16 * (min_disparity - 1)).astype(np.int16)


def stages(left, right, **params) -> dict:
    p = dict(DEFAULTS, **params)
    cl, cr = census(left), census(right)
    C = cost_volume(cl, cr, p["min_disparity"], p["num_disparities"])
    S = aggregate(C, p["p1"], p["p2"], p["paths"])
    return dict(census_left=cl, census_right=cr, cost=C, aggregated=S, params=p)


def match(left, right, **params) -> np.ndarray:
    st = stages(left, right, **params)
    p = st["params"]
    return disparity(st["aggregated"], p["min_disparity"], p["uniqueness_ratio"], p["disp12_max_diff"])


def points(disp, fx, fy, cx, cy, baseline, projection: str, min_disparity: int = 0):
    """tscm_stereo_points by the header's formulas -> (points [h, w, 3], valid [h, w])."""
    disp = np.asarray(disp)
    h, w = disp.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    valid = (disp != 16 * (min_disparity - 1)) & (disp > 0)
    d = np.where(valid, disp, 16) / 16.0
    if projection == "perspective":
        Z = fx * baseline / d
        P = np.stack([(xx - cx) / fx * Z, (yy - cy) / fy * Z, Z], axis=-1)
    else:
        aL, da, b = (xx - cx) / fx, d / fx, (yy - cy) / fy
        r = baseline * np.cos(aL - da) / np.sin(da)
        P = r[..., None] * np.stack([np.sin(aL), np.cos(aL) * np.sin(b), np.cos(aL) * np.cos(b)], axis=-1)
    P[~valid] = np.nan
    return P, valid


def shifted_noise_pair():
    """The synthetic-shift pair: 48 x 96, disparity 5 on the top half and 12 on the bottom half."""
    R = np.random.default_rng(7).integers(0, 256, (48, 160)).astype(np.uint8)
    right = R[:, 32:128].copy()
    d = np.where(np.arange(48) < 24, 5, 12)
    left = np.stack([R[y, 32 - d[y]:128 - d[y]] for y in range(48)])
    return left, right, d
