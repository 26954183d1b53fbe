"""Extended-precision reference of the corner detector's image planes (DetectCorner/findCorner.cpp:30-34, :103-142),
written from the definition of the operation in numpy long double:

  x       = (g - min) / (max - min)                                     the normalisation
  t, Ig   = separable Gaussian of x: rows, then columns, with the fp64 taps of getGaussianKernel as given (the taps
            are an input of the operation) and BORDER_REFLECT_101 through index arrays (refl101 below)
  Ix, Iy  = (1 0 -1) differences of Ig along rows / columns, I45 = Ix c4 + Iy s4
  Ixy     = (1 0 -1) difference of Ix along columns; I45_x, I45_y likewise of I45; I45_45 = I45_x cn4 + I45_y sn4,
            In45 = Ix cn4 + Iy sn4 (c4, s4, cn4, sn4 = cos / sin(+-pi / 4) in fp64, inputs like the taps)
  cxy     = max(0, sigma^2 |Ixy| - 1.5 sigma (|I45| + |In45|)),  c45 = max(0, sigma^2 |I45_45| - 1.5 sigma (|Ix| + |Iy|))
  metric  = cxy + c45

Every plane comes with an a-priori bound on the error of an fp64 evaluation of the same formulas, computed alongside
as a running error bound (in long double, from the exact values):
  - a rounded quotient, sum, difference or product by an fp64 constant adds u |result| to the propagated input errors;
  - a sum of n products in any order: gamma_n sum |k_q| |x_q| (Higham, Accuracy and Stability, Lemma 3.1 / (3.5)), the
    column pass with its paired taps (centre, then k (a + b) pairs) counts H + 2 roundings per term;
  - |.| and max(0, .) are 1-Lipschitz and pass the error through.
u = 2^-53 + 2^-64: the bound also covers the long-double rounding of the reference itself (the same formulas with
u = 2^-64; the bounds are polynomials in u with non-negative coefficients, so the two add up below the bound at their
sum).  Nothing here is fitted to measured errors.
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
U = LD(2) ** -53 + LD(2) ** -64
# the fp64 constants of the +-45 degree terms, as the C library computes them
C4, CN4, S4, SN4 = (LD(math.cos(math.pi / 4)), LD(math.cos(-math.pi / 4)), LD(math.sin(math.pi / 4)), LD(math.sin(-math.pi / 4)))


def gamma(n: int):
    return n * U / (1 - n * U)


def border_interpolate(p: int, n: int, delta: int) -> int:
    """cv::borderInterpolate for BORDER_REFLECT_101 (delta = 1: gfedcb|abcdefgh|gfedcba) and BORDER_REFLECT (delta = 0:
    fedcba|abcdefgh|hgfedcba): mirror at the nearer end, again and again until the index lies inside [0, n)."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p - 1 + delta if p < 0 else n - 1 - (p - n) - delta
    return p


def refl101(p: int, n: int) -> int:
    return border_interpolate(p, n, 1)


def gaussian_taps_ld(sigma: int) -> np.ndarray:
    """getGaussianKernel(7 sigma + 1, sigma) in long double: exp(-x^2 / (2 sigma^2)) / sum"""
    n = 7 * sigma + 1
    x = np.arange(n, dtype=LD) - LD(n - 1) / 2
    k = np.exp(-(x * x) / (2 * LD(sigma) * LD(sigma)))
    return k / k.sum()


def _index(n: int, lo: int, hi: int, border) -> np.ndarray:
    """border(p, n) for p = lo .. hi - 1"""
    return np.array([border(p, n) for p in range(lo, hi)], dtype=np.int64)


# ---- running error bounds: a plane is (value, bound) ------------------------------------------------------------------

def _add(a, b):
    v = a[0] + b[0]
    return v, (a[1] + b[1]) * (1 + U) + U * np.abs(v)


def _sub(a, b):
    v = a[0] - b[0]
    return v, (a[1] + b[1]) * (1 + U) + U * np.abs(v)


def _scale(a, c):
    c = LD(c)
    v = c * a[0]
    return v, abs(c) * a[1] * (1 + U) + U * np.abs(v)


def _abs(a):
    return np.abs(a[0]), a[1]


def _pos(a):
    return np.maximum(a[0], 0), a[1]


def _cols(a, d: int, border=refl101):
    """plane[i, border(j + d)]"""
    w = a[0].shape[1]
    idx = _index(w, d, w + d, border)
    return a[0][:, idx], a[1][:, idx]


def _rows(a, d: int, border=refl101):
    """plane[border(i + d), j]"""
    h = a[0].shape[0]
    idx = _index(h, d, h + d, border)
    return a[0][idx, :], a[1][idx, :]


# ---- the stages -------------------------------------------------------------------------------------------------------

def normalise(gray):
    """(g - min) / (max - min): one rounded quotient of exact operands (NaN planes for a flat image)"""
    g = np.asarray(gray).astype(LD)
    mn, mx = g.min(), g.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        x = (g - mn) / (mx - mn)
    return x, U * np.abs(x)


def blur_rows(a, taps, border=refl101):
    """t[i, j] = sum_q k_q x[i, border(j + q - H)], sequential sum of n products"""
    k = np.asarray(taps, dtype=np.float64).astype(LD)
    n, H, w = k.shape[0], k.shape[0] // 2, a[0].shape[1]
    idx = _index(w, -H, w + H, border)
    xv, xe = a[0][:, idx], a[1][:, idx]
    v = np.zeros(a[0].shape, dtype=LD)
    mag = np.zeros(a[0].shape, dtype=LD)
    prop = np.zeros(a[0].shape, dtype=LD)
    for q in range(n):
        v += k[q] * xv[:, q:q + w]
        mag += abs(k[q]) * (np.abs(xv[:, q:q + w]) + xe[:, q:q + w])
        prop += abs(k[q]) * xe[:, q:q + w]
    return v, gamma(n) * mag + prop


def blur_cols(a, taps, border=refl101):
    """Ig[i, j] = k_H t[i, j] + sum_{q=1..H} k_{H+q} (t[border(i + q), j] + t[border(i - q), j])"""
    k = np.asarray(taps, dtype=np.float64).astype(LD)
    n, H, h = k.shape[0], k.shape[0] // 2, a[0].shape[0]
    idx = _index(h, -H, h + H, border)
    tv, te = a[0][idx, :], a[1][idx, :]
    v = np.zeros(a[0].shape, dtype=LD)
    mag = np.zeros(a[0].shape, dtype=LD)
    prop = np.zeros(a[0].shape, dtype=LD)
    for q in range(n):
        v += k[q] * tv[q:q + h, :]
        mag += abs(k[q]) * (np.abs(tv[q:q + h, :]) + te[q:q + h, :])
        prop += abs(k[q]) * te[q:q + h, :]
    return v, gamma(H + 2) * mag + prop


def metric(g, sigma: int, border=refl101) -> dict:
    """secondDerivCornerMetric after the blur: (value, bound) of metric = cxy + c45 and of Ixy"""
    ix = _sub(_cols(g, -1, border), _cols(g, 1, border))                        # du = (1 0 -1)
    iy = _sub(_rows(g, -1, border), _rows(g, 1, border))
    i45 = _add(_scale(ix, C4), _scale(iy, S4))
    ixy = _sub(_rows(ix, -1, border), _rows(ix, 1, border))
    i45x = _sub(_cols(i45, -1, border), _cols(i45, 1, border))
    i45y = _sub(_rows(i45, -1, border), _rows(i45, 1, border))
    i4545 = _add(_scale(i45x, CN4), _scale(i45y, SN4))
    in45 = _add(_scale(ix, CN4), _scale(iy, SN4))
    s2, s15 = LD(sigma * sigma), LD(1.5 * sigma)
    cxy = _pos(_sub(_scale(_abs(ixy), s2), _scale(_add(_abs(i45), _abs(in45)), s15)))
    c45 = _pos(_sub(_scale(_abs(i4545), s2), _scale(_add(_abs(ix), _abs(iy)), s15)))
    return dict(metric=_add(cxy, c45), ixy=ixy)


def planes(gray, sigma: int, taps) -> dict:
    """{'ig' | 'metric' | 'ixy': (long-double value, fp64 error bound)} of a (H, W) uint8 image; taps: the fp64
    Gaussian taps under test."""
    if np.min(gray) == np.max(gray):                  # 0 / 0 normalisation: every plane is NaN
        nan = np.full(np.shape(gray), np.nan, dtype=LD)
        return {k: (nan, nan) for k in ("ig", "metric", "ixy")}
    with np.errstate(invalid="ignore"):
        g = blur_cols(blur_rows(normalise(gray), taps), taps)
        out = metric(g, sigma)
    out["ig"] = g
    return out


def excess(got, ref) -> tuple:
    """Compare an fp64 plane with a (value, bound) pair: (largest |got - value|, largest |got - value| / bound, number
    of pixels beyond the bound).  NaN must meet NaN (a flat image); a pixel whose NaN-ness differs counts as beyond."""
    v, b = ref
    got = np.asarray(got)
    nan_g, nan_r = np.isnan(got), np.isnan(v)
    bad = int(np.count_nonzero(nan_g != nan_r))
    ok = ~(nan_g | nan_r)
    if not ok.any():
        return 0.0, 0.0, bad
    err = np.abs(got[ok].astype(LD) - v[ok])
    bnd = b[ok]
    bad += int(np.count_nonzero(err > bnd))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0, LD(0), err / bnd)
    return float(err.max()), float(ratio.max()), bad
