"""Host restatement of tscm_stereo_refine (include/tscm/tscm.h), written twice with different algorithms:

  refine_literal   per pixel: the participants of the window as a Python list, a stable sort by value, a running sum of the
                   weights until twice the sum reaches W
  refine           vectorised: the window as [h, w, N] stacks; for each candidate k the weight of all participants at or
                   below its value, then the smallest value that qualifies

Integers only; both give the bits of the device.  tests/test_stereo_refine_reference.py compares them on random maps."""
import math

import numpy as np

DEFAULTS = dict(min_disparity=0, radius=3, iterations=1, fill_invalid=0, wrap_x=0)


def invalid_value(min_disparity: int = 0) -> int:
    return 16 * (min_disparity - 1)


def range_weights(sigma: float) -> np.ndarray:
    """lut[k] = floor(255 exp(-k / sigma) + 0.5); 255, 0, 0, ... for a sigma that is not > 0 (NaN included)"""
    if not sigma > 0:
        return np.array([255] + [0] * 255, dtype=np.uint8)
    return np.array([int(math.floor(255.0 * math.exp(-k / sigma) + 0.5)) for k in range(256)], dtype=np.uint8)


def _table(weights) -> np.ndarray:
    return np.full(256, 255, dtype=np.int64) if weights is None else np.asarray(weights).astype(np.int64)


# ------------------------------------------------------------------------------------------------ literal
def pass_literal(d, g, weights=None, **params):
    """One pass -> (out int16, weight_sum int32, count uint8)."""
    p = dict(DEFAULTS, **params)
    d, g, lut = np.asarray(d), np.asarray(g), _table(weights)
    h, w = d.shape
    inv, r = invalid_value(p["min_disparity"]), p["radius"]
    out, wsum, count = np.zeros((h, w), np.int16), np.zeros((h, w), np.int32), np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            part = []
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    yy, xx = y + dy, x + dx
                    if not 0 <= yy < h:
                        continue
                    if p["wrap_x"]:
                        xx %= w
                    elif not 0 <= xx < w:
                        continue
                    if int(d[yy, xx]) != inv:
                        part.append((int(d[yy, xx]), int(lut[abs(int(g[y, x]) - int(g[yy, xx]))])))
            W = sum(wq for _, wq in part)
            wsum[y, x], count[y, x] = W, len(part)
            if int(d[y, x]) == inv and not p["fill_invalid"]:
                out[y, x] = inv
            elif W == 0:
                out[y, x] = d[y, x]
            else:
                part.sort(key=lambda t: t[0])                # stable; equal values end up adjacent and accumulate
                s = 0
                for k, (v, wq) in enumerate(part):
                    s += wq
                    if 2 * s >= W and (k + 1 == len(part) or part[k + 1][0] != v):
                        out[y, x] = v
                        break
    return out, wsum, count


def refine_literal(d, g, weights=None, **params) -> np.ndarray:
    p = dict(DEFAULTS, **params)
    d = np.asarray(d)
    for _ in range(p["iterations"]):
        d = pass_literal(d, g, weights, **p)[0]
    return d


# ------------------------------------------------------------------------------------------------ vectorised
def window(d, g, weights=None, **params):
    """-> (values int64 [h, w, N], weights int64 [h, w, N] with 0 for the offsets that do not take part, part bool [h, w, N])"""
    p = dict(DEFAULTS, **params)
    d, g, lut = np.asarray(d).astype(np.int64), np.asarray(g).astype(np.int64), _table(weights)
    h, w = d.shape
    inv, r = invalid_value(p["min_disparity"]), p["radius"]
    yy, xx = np.mgrid[0:h, 0:w]
    vals, wts, part = [], [], []
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, xs = yy + dy, xx + dx
            ok = (ys >= 0) & (ys < h)
            if p["wrap_x"]:
                xs = xs % w
            else:
                ok &= (xs >= 0) & (xs < w)
            ys, xs = np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)
            v = d[ys, xs]
            ok &= v != inv
            vals.append(v)
            part.append(ok)
            wts.append(np.where(ok, lut[np.abs(g - g[ys, xs])], 0))
    return np.stack(vals, -1), np.stack(wts, -1), np.stack(part, -1)


def pass_vectorised(d, g, weights=None, **params):
    """One pass -> (out int16, weight_sum int32, count uint8)."""
    p = dict(DEFAULTS, **params)
    d = np.asarray(d)
    inv = invalid_value(p["min_disparity"])
    vals, wts, part = window(d, g, weights, **p)
    W = wts.sum(-1)
    above = 1 << 20
    best = np.full(d.shape, above, dtype=np.int64)
    for k in range(vals.shape[-1]):
        below = (wts * (vals <= vals[..., k:k + 1])).sum(-1)         # non-participants carry weight 0
        ok = part[..., k] & (2 * below >= W)
        best = np.where(ok & (vals[..., k] < best), vals[..., k], best)
    out = np.where(W == 0, d.astype(np.int64), best)
    if not p["fill_invalid"]:
        out = np.where(d.astype(np.int64) == inv, inv, out)
    assert np.all(out != above)
    return out.astype(np.int16), W.astype(np.int32), part.sum(-1).astype(np.uint8)


def stages(d, g, weights=None, **params) -> dict:
    out, wsum, count = pass_vectorised(d, g, weights, **params)
    return dict(weight_sum=wsum, count=count, first_pass=out)


def refine(d, g, weights=None, **params) -> np.ndarray:
    p = dict(DEFAULTS, **params)
    d = np.asarray(d)
    if d.size == 0:
        return d.copy()
    for _ in range(p["iterations"]):
        d = pass_vectorised(d, g, weights, **p)[0]
    return d
