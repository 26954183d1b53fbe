"""Host restatement of the panorama composer defined in include/tscm/tscm.h (tscm_panorama_*): sample, alpha, label,
coverage, SEAM, FEATHER, the MULTIBAND pyramids and the overlap sums.  Integer arithmetic throughout, so the device result
is compared with array_equal.  The bilinear sample is oracle.pyoracle.remap, which is bit-identical to the remap kernel.
Written on whole arrays with index tables for the clamp / wrap rules, unlike the kernels, which work on tiles with halos."""
import numpy as np

from oracle import pyoracle as orc

SEAM, FEATHER, MULTIBAND = 0, 1, 2
TAPS = np.array([1, 4, 6, 4, 1], dtype=np.int64)


def sample(img, mapx, mapy) -> np.ndarray:
    """v_k of one camera: uint8 [ph, pw, C] (C = 1 for a 2-D image)."""
    out = orc.remap(np.ascontiguousarray(img, dtype=np.uint8), mapx, mapy)
    return out[..., None] if out.ndim == 2 else out


def alpha(weight, width, height, mapx, mapy) -> np.ndarray:
    """a_k: the same arithmetic on the weight image; None is a constant 255 image, whose border taps ramp to 0."""
    w = np.full((height, width), 255, dtype=np.uint8) if weight is None else np.ascontiguousarray(weight, dtype=np.uint8)
    assert w.shape == (height, width)
    return orc.remap(w, mapx, mapy)


def apply_gain(v, g: int) -> np.ndarray:
    return np.minimum(255, (v.astype(np.int64) * int(g) + 128) >> 8)


def label_coverage(a):
    """a [n, ph, pw] -> label (the lowest k whose a_k is maximal, 255 when that maximum is 0), coverage."""
    a = np.asarray(a).astype(np.int64)
    lab = np.argmax(a, axis=0)                      # the first of equal maxima
    lab = np.where(a.max(axis=0) > 0, lab, 255).astype(np.uint8)
    return lab, (a > 0).sum(axis=0).astype(np.uint8)


def seam(v, lab) -> np.ndarray:
    """v [n, ph, pw, C] -> out [ph, pw, C]"""
    n = v.shape[0]
    out = np.zeros(v.shape[1:], dtype=np.int64)
    for k in range(n):
        out[lab == k] = v[k][lab == k]
    return out.astype(np.uint8)


def feather(v, a) -> np.ndarray:
    a = np.asarray(a).astype(np.int64)
    A = a.sum(axis=0)
    num = (a[..., None] * v.astype(np.int64)).sum(axis=0) + (A >> 1)[..., None]
    return np.where(A[..., None] > 0, num // np.maximum(A, 1)[..., None], 0).astype(np.uint8)


def _rows(idx, H):
    return np.clip(idx, 0, H - 1)


def _cols(idx, W, wrap):
    return np.mod(idx, W) if wrap else np.clip(idx, 0, W - 1)


def reduce(x, wrap: bool) -> np.ndarray:
    """R(x): [H, W] integers -> [H/2, W/2]"""
    x = np.asarray(x).astype(np.int64)
    H, W = x.shape
    i, j = np.arange(H // 2), np.arange(W // 2)
    acc = np.zeros((H // 2, W // 2), dtype=np.int64)
    for a in range(5):
        for b in range(5):
            acc += TAPS[a] * TAPS[b] * x[_rows(2 * i + a - 2, H)[:, None], _cols(2 * j + b - 2, W, wrap)[None, :]]
    return (acc + 128) >> 8


def expand(x, wrap: bool) -> np.ndarray:
    """E(x): [Hc, Wc] integers on the half-size grid -> [2 Hc, 2 Wc]"""
    x = np.asarray(x).astype(np.int64)
    Hc, Wc = x.shape
    i, j = np.arange(2 * Hc), np.arange(2 * Wc)
    acc = np.zeros((2 * Hc, 2 * Wc), dtype=np.int64)
    for a in range(-2, 3):
        for b in range(-2, 3):
            ri, cj = i + a, j + b
            even = ((ri % 2 == 0)[:, None] & (cj % 2 == 0)[None, :]).astype(np.int64)
            acc += TAPS[a + 2] * TAPS[b + 2] * even * x[_rows(ri // 2, Hc)[:, None], _cols(cj // 2, Wc, wrap)[None, :]]
    return (acc + 32) >> 6


def pyramid(x, levels: int, wrap: bool) -> list:
    out = [np.asarray(x).astype(np.int64)]
    for _ in range(levels):
        out.append(reduce(out[-1], wrap))
    return out


def multiband(v, lab, cov, levels: int, wrap: bool) -> dict:
    """v [n, ph, pw, C] after the gain -> out uint8 [ph, pw, C] and the pyramids as lists over the levels:
    mask[l] [n, h_l, w_l], lap[l] [n, C, h_l, w_l], blend[l] [C, h_l, w_l] (B^l, before the collapse)."""
    n, ph, pw, C = v.shape
    assert ph % (1 << levels) == 0 and pw % (1 << levels) == 0
    M = [pyramid(np.where(lab == k, 255, 0), levels, wrap) for k in range(n)]
    G = [[pyramid(v[k, :, :, c], levels, wrap) for c in range(C)] for k in range(n)]
    mask = [np.stack([M[k][l] for k in range(n)]) for l in range(levels + 1)]
    lap = []
    for l in range(levels + 1):
        lap.append(np.stack([np.stack([G[k][c][l] - (expand(G[k][c][l + 1], wrap) if l < levels else 0) for c in range(C)]) for k in range(n)]))
    blend = []
    for l in range(levels + 1):
        W = mask[l].sum(axis=0)
        num = (mask[l][:, None] * lap[l]).sum(axis=0) + (W >> 1)[None]
        blend.append(np.where(W[None] > 0, np.floor_divide(num, np.maximum(W, 1)[None]), 0))        # floor division
    R = blend[levels]
    for l in range(levels - 1, -1, -1):
        R = blend[l] + np.stack([expand(R[c], wrap) for c in range(C)])
    out = np.where(cov[None] > 0, np.clip(R, 0, 255), 0)
    return dict(out=np.moveaxis(out, 0, -1).astype(np.uint8), mask=mask, lap=lap, blend=blend)


def flat(levels_list, lead: int) -> np.ndarray:
    """A pyramid as the stage outputs lay it out: the levels one after the other behind `lead` leading axes."""
    return np.concatenate([x.reshape(x.shape[:lead] + (-1,)) for x in levels_list], axis=-1)


def luminance(v) -> np.ndarray:
    v = v.astype(np.int64)
    if v.shape[-1] == 1:
        return v[..., 0]
    return (v[..., 0] * 1868 + v[..., 1] * 9617 + v[..., 2] * 4899 + (1 << 13)) >> 14


def overlap(v, a):
    """v [n, ph, pw, C] BEFORE any gain, a [n, ph, pw] -> count [n, n], sum [n, n] (int64)"""
    n = v.shape[0]
    on = np.asarray(a) > 0
    count, total = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    for p in range(n):
        lum = luminance(v[p])
        for q in range(n):
            both = on[p] & on[q]
            count[p, q] = both.sum()
            total[p, q] = lum[both].sum()
    return count, total


def compose(images, weights, mapx, mapy, mode=MULTIBAND, levels=4, wrap=True, gains=None) -> dict:
    """Everything tscm_panorama_compose / _stages / _overlap give for one frame.  images: n arrays [h, w] or [h, w, 3];
    weights: None or n entries (None or [h, w] uint8); mapx, mapy: [n, ph, pw] float32."""
    n = len(images)
    h, w = images[0].shape[:2]
    raw = np.stack([sample(images[k], mapx[k], mapy[k]) for k in range(n)])
    a = np.stack([alpha(None if weights is None else weights[k], w, h, mapx[k], mapy[k]) for k in range(n)])
    g = [256] * n if gains is None else list(gains)
    v = np.stack([apply_gain(raw[k], g[k]) for k in range(n)])
    lab, cov = label_coverage(a)
    res = dict(sampled=v.astype(np.uint8), alpha=a, label=lab, coverage=cov)
    res["count"], res["sum"] = overlap(raw, a)
    if mode == SEAM:
        res["out"] = seam(v, lab)
    elif mode == FEATHER:
        res["out"] = feather(v, a)
    else:
        res.update(multiband(v, lab, cov, levels, wrap))
    return res
