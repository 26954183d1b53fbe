"""CPU tests of the long-double reference of the corner detector's planes (tests/corner_ref.py): the oracle's Ig,
cxy + c45 and Ixy (orc_corner_planes) lie within its a-priori fp64 error bound, the oracle's Gaussian taps lie within
the error bound of an fp64 evaluation of getGaussianKernel's formula, kernel-shaped mistakes exceed the bound by far, and the GPU case table of
tests/test_gpu_corner_planes.py reaches every kernel instantiation and seam of the host's dispatch."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as orc
from tests import corner_ref as R
from tests import test_gpu_corner_planes as G
from tests.test_corners_oracle import _scene

PLANES = ("ig", "metric", "ixy")


def _taps(sigma):
    k = np.zeros(7 * sigma + 1)
    orc.lib().orc_gaussian_kernel(sigma, k.ctypes.data_as(C.POINTER(C.c_double)))
    return k


def tap_bound(sigma):
    """A-priori bound on |fp64 tap - exact tap| for the fp64 evaluation of getGaussianKernel's formula
    (scale = -0.5 / sigma^2, e_i = exp(scale x_i x_i), taps = e_i * (1 / sum e)): the argument carries <= 3 roundings
    (gamma_3 |A_i|, amplified by exp), exp itself < 1 ulp (2 u relative), the sum gamma_{n-1}, the reciprocal and the
    product one rounding each."""
    u, n = R.U, 7 * sigma + 1
    x = np.arange(n, dtype=R.LD) - R.LD(n - 1) / 2
    A = np.abs(x * x / (2 * R.LD(sigma) ** 2))
    e = np.exp(-A)
    eps = np.exp(R.gamma(3) * A) * (1 + 2 * u) - 1                      # relative error of e_i
    eps_s = ((eps * e).sum() + R.gamma(n - 1) * ((1 + eps) * e).sum()) / e.sum()
    eps_inv = (1 + u) / (1 - eps_s) - 1
    return ((1 + eps) * (1 + eps_inv) * (1 + u) - 1) * R.gaussian_taps_ld(sigma)


@pytest.mark.parametrize("sigma", [2, 4, 6, 8])
def test_taps_are_the_gaussian_kernel_within_the_fp64_bound(sigma):
    """The taps are exp(-x^2 / (2 sigma^2)) / sum evaluated in fp64 (the formula of getGaussianKernel), not the
    correctly rounded values: measured against the long-double kernel they are up to 0.8, 2.0, 2.5 and 5.3 ulp away at
    sigma = 4, 2, 8 and 6 (at 2 and 6 the rounded argument is amplified by exp in the tails), so 1 ulp is not a bound."""
    k = _taps(sigma)
    ref = R.gaussian_taps_ld(sigma)
    d = np.abs(k.astype(R.LD) - ref)
    b = tap_bound(sigma)
    ulp = d / np.spacing(ref.astype(np.float64)).astype(R.LD)
    print(f"sigma {sigma}: taps within {float(ulp.max()):.2f} ulp of the long-double kernel, {float((d / b).max()):.3f} x the bound")
    assert np.all(d <= b), sigma
    assert np.array_equal(k, k[::-1]) and abs(float(ref.sum()) - 1) < 1e-18


def test_refl101_is_borderinterpolate():
    # gfedcb|abcdefgh|gfedcba, periodic with period 2 (n - 1): every index of a few periods, n = 1 .. 6
    for n in range(1, 7):
        period = [0] if n == 1 else list(range(n)) + list(range(n - 2, 0, -1))
        for p in range(-5 * n - 3, 6 * n + 3):
            assert R.refl101(p, n) == period[p % len(period)], (p, n)
    # BORDER_REFLECT: fedcba|abcdefgh|hgfedcba, period 2 n
    for n in range(2, 6):
        period = list(range(n)) + list(range(n - 1, -1, -1))
        for p in range(-4 * n, 5 * n):
            assert R.border_interpolate(p, n, 0) == period[p % len(period)], (p, n)


def _images():
    full, uv = _scene(3, 0)
    x0, y0 = int(uv[:, 0].min()) - 60, int(uv[:, 1].min()) - 50
    rng = np.random.default_rng(7)
    out = [("board-320x240", np.ascontiguousarray(full[y0:y0 + 240, x0:x0 + 320]), 4),
           ("board-1280x1080", full, 4),
           ("noise-333x247", rng.integers(0, 256, size=(247, 333), dtype=np.uint8), 4),
           ("board-257x33-s8", np.ascontiguousarray(full[y0:y0 + 33, x0:x0 + 257]), 8),
           ("noise-258x17-s2", rng.integers(0, 256, size=(17, 258), dtype=np.uint8), 2),
           ("noise-256x9-s6", rng.integers(0, 256, size=(9, 256), dtype=np.uint8), 6),
           ("flat-40x30", np.full((30, 40), 9, dtype=np.uint8), 4)]
    for s in (4, 8):
        for w, h in [(2, 2), (5, 5), (14, 3), (15, 29), (29, 2), (1, 1), (255, 1)]:
            out.append((f"noise-{w}x{h}-s{s}", rng.integers(0, 256, size=(h, w), dtype=np.uint8), s))
    return out


_IMAGES = _images()


@pytest.mark.parametrize("name,img,sigma", _IMAGES, ids=[c[0] for c in _IMAGES])
def test_oracle_planes_lie_within_the_bound(name, img, sigma):
    o = orc.corner_planes(img, sigma)
    ref = R.planes(img, sigma, _taps(sigma))
    rep = []
    for k in PLANES:
        err, ratio, bad = R.excess(o[k], ref[k])
        assert bad == 0, f"{name} {k}: {bad} pixels beyond the bound (largest error {err:.3g}, {ratio:.3g} x bound)"
        rep.append(f"{k} {err:.2g} ({ratio:.2g} x bound)")
    if img.min() == img.max():
        assert all(np.isnan(o[k]).all() for k in PLANES)
    print(f"{name}: " + ", ".join(rep))


def test_the_strided_oracle_reads_the_same_image():
    img = _IMAGES[2][1]
    buf = np.full((img.shape[0], img.shape[1] + 11), 255, dtype=np.uint8)
    buf[:, :img.shape[1]] = img
    a, b = orc.corner_planes(img), orc.corner_planes(buf[:, :img.shape[1]])
    assert all(np.array_equal(a[k], b[k]) for k in PLANES)
    d = orc.detect_corners(img, planes=True)
    assert np.array_equal(d["metric"], a["metric"]) and np.array_equal(d["ixy"], a["ixy"])


# ---- negative control: kernel-shaped mistakes applied to a copy of the reference ------------------------------------

def _signal(mut, ref):
    """largest |mutant - reference| / bound over the pixels (the comparison the GPU test makes)"""
    v, b = ref
    d = np.abs(np.asarray(mut, dtype=R.LD) - v)
    return float(np.max(np.where(d == 0, R.LD(0), d / b)))


def _reflect_in_columns(img, sigma, taps):
    """the column pass mirrors with BORDER_REFLECT (the edge row repeated) instead of REFLECT_101"""
    with np.errstate(invalid="ignore"):
        rows = R.blur_rows(R.normalise(img), taps)
        return R.blur_cols(rows, taps, border=lambda p, n: R.border_interpolate(p, n, 0))[0], "ig"


def _strip_tail(img, sigma, taps):
    """h = 16 k + 1: the lone last row of the last 16-row strip takes its neighbour's value"""
    g = R.planes(img, sigma, taps)["ig"][0].copy()
    g[-1] = g[-2]
    return g, "ig"


def _zero_seam(img, sigma, taps):
    """the metric tile of columns [256 k, 256 k + 256) zero-fills columns 256 k - 2, 256 k - 1 instead of reading them"""
    ref = R.planes(img, sigma, taps)
    g = (ref["ig"][0].copy(), ref["ig"][1].copy())
    m = ref["metric"][0].copy()
    for j0 in range(256, img.shape[1], 256):
        z = (g[0].copy(), g[1])
        z[0][:, j0 - 2:j0] = 0
        mz = R.metric(z, sigma)["metric"][0]
        m[:, j0:j0 + 2] = mz[:, j0:j0 + 2]
    return m, "metric"


def _single_bounce(img, sigma, taps):
    """refl101 mirrors once (then clamps) where the half-kernel is wider than the row"""
    def once(p, n):
        if n == 1:
            return 0
        p = -p if p < 0 else (2 * (n - 1) - p if p >= n else p)
        return min(max(p, 0), n - 1)
    with np.errstate(invalid="ignore"):
        return R.blur_cols(R.blur_rows(R.normalise(img), taps, border=once), taps)[0], "ig"


_MUTANTS = [("border_reflect_in_column_pass", _reflect_in_columns, (40, 37), 4),
            ("strip_tail_h_16k_plus_1", _strip_tail, (300, 33), 4),
            ("zero_fill_at_tile_seam", _zero_seam, (513, 20), 4),
            ("single_bounce_w5_sigma4", _single_bounce, (5, 21), 4),
            ("single_bounce_w14_sigma8", _single_bounce, (14, 9), 8)]


def test_negative_controls_exceed_the_bound():
    rng = np.random.default_rng(11)
    ratios = {}
    for name, mutate, (w, h), sigma in _MUTANTS:
        img = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        taps = _taps(sigma)
        ref = R.planes(img, sigma, taps)
        mut, plane = mutate(img, sigma, taps)
        ratios[name] = _signal(mut, ref[plane])
        # and the unmutated oracle plane stays within the bound on the same image
        assert R.excess(orc.corner_planes(img, sigma)[plane], ref[plane])[2] == 0
    worst = min(ratios, key=ratios.get)
    print("negative controls, largest |mutant - reference| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items())
          + f"; smallest: {worst} {ratios[worst]:.3g}")
    assert all(v >= 20 for v in ratios.values()), ratios


# ---- coverage of the GPU case table ---------------------------------------------------------------------------------

def kernels(w, h, sigma, contiguous):
    """the kernels tscm_detect_corners_batch launches up to the metric (a copy of the host's dispatch rules)"""
    ntap = 7 * sigma + 1
    ks = {"k_grey_extremes_flat" if contiguous else "k_grey_extremes"}
    if ntap == 29:
        ks |= {"k_norm_lut", "k_gauss_rows_n<29,5>" if 1024 < w <= 1280 else "k_gauss_rows_n<29,4>", "k_gauss_cols_strip<29>"}
    else:
        ks |= {"k_gauss_rows", "k_gauss_cols"}
    return ks | {"k_corner_metric"}


def seams(case):
    """the seam classes of section 4 of the plan: tile / strip / band edges, reflection bounces, batch layouts"""
    w, h, s, H = case.w, case.h, case.sigma, (7 * case.sigma + 1) // 2
    out = set()
    for k, name in ((255, "w=256k-1"), (0, "w=256k"), (1, "w=256k+1"), (2, "w=256k+2")):
        if w >= 255 and w % 256 == k:
            out.add(name)
    out |= {f"w={v}" for v in (1024, 1025, 1280, 1281) if w == v}
    if h > 8 and h % 8 == 1:
        out.add("h=8k+1")
    if s == 4 and h > 16 and h % 16 == 1:
        out.add("strip h=16k+1")
    if s == 4 and h % 16 == 15:
        out.add("strip h=16k+15")
    if w <= H and w > 1:
        out.add("rows bounce twice")
    if h <= H and h > 1:
        out.add("columns bounce twice")
    out.add(f"sigma {s}")
    n = len(case.kinds)
    if n > 1:
        out.add("batch")
        if case.stride is None and (w * h) % 16:
            out.add("batch, contiguous, w h % 16 != 0")
        if case.stride is not None:
            out.add("batch, strided")
        if "flat" in case.kinds:
            out.add("flat image in a batch")
    if case.stride is not None and "range" in case.kinds:
        out.add(f"padding {case.pad} around [17, 230]")
    if w * h >= 1280 * 1000 and case.kinds[0] in ("noise", "checker"):
        out.add(f"dense {case.kinds[0]}")
    if case.kinds == ("xcorners",):
        out.add("x-corners 9-17 px from the border")
    return out


def test_the_gpu_case_table_reaches_every_kernel_and_seam():
    every_kernel = {"k_grey_extremes_flat", "k_grey_extremes", "k_norm_lut", "k_gauss_rows_n<29,4>", "k_gauss_rows_n<29,5>",
                    "k_gauss_rows", "k_gauss_cols_strip<29>", "k_gauss_cols", "k_corner_metric"}
    every_seam = ({"w=256k-1", "w=256k", "w=256k+1", "w=256k+2", "w=1024", "w=1025", "w=1280", "w=1281", "h=8k+1", "strip h=16k+1",
                   "strip h=16k+15", "rows bounce twice", "columns bounce twice", "batch", "batch, contiguous, w h % 16 != 0",
                   "batch, strided", "flat image in a batch", "padding 0 around [17, 230]", "padding 255 around [17, 230]",
                   "dense noise", "dense checker", "x-corners 9-17 px from the border"} | {f"sigma {s}" for s in (2, 4, 6, 8)})
    reached_k, reached_s = set(), set()
    for c in G.ALL_CASES:
        reached_k |= kernels(c.w, c.h, c.sigma, c.stride is None)
        reached_s |= seams(c)
    assert reached_k == every_kernel, every_kernel - reached_k
    assert every_seam <= reached_s, every_seam - reached_s
    # sigma 2, 6 and 8 on every width class of the sigma = 4 table
    for s in (2, 6, 8):
        cls = {x for c in G.ALL_CASES if c.sigma == s for x in seams(c) if x.startswith("w=256k")}
        assert cls == {"w=256k-1", "w=256k", "w=256k+1", "w=256k+2"}, (s, cls)
        assert any(1024 < c.w <= 1280 for c in G.ALL_CASES if c.sigma == s) and any(c.w > 1280 for c in G.ALL_CASES if c.sigma == s)
    # the tiny images bounce more than once at sigma 4 and at sigma 8, in both directions
    for s in (4, 8):
        assert {"rows bounce twice", "columns bounce twice"} <= set().union(*(seams(c) for c in G.TINY if c.sigma == s))
    # the arena sequence: large, smaller, large again
    sizes = [c.w * c.h for c in G.ARENA]
    assert sizes[0] > sizes[1] < sizes[2] and sizes[2] > 100 * sizes[1]
