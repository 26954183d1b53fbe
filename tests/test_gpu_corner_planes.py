"""Plane-level parity of the corner detector (tscm_corners.hip) on every kernel path: the planes of
tscm_corner_planes_batch -- Ig, cxy + c45 and Ixy, from the launches tscm_detect_corners_batch makes -- must be
bit-identical to the oracle's (orc_corner_planes), lie within the a-priori fp64 error bound of the long-double
reference (tests/corner_ref.py), and give the oracle's candidate list.  The case table reaches every dispatch path and
the tile / strip / reflection seams; tests/test_corner_reference.py checks that it does, from the host's dispatch rules."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

from tests import corner_ref as R

pytestmark = pytest.mark.gpu

PLANES = ("ig", "metric", "ixy")

# kinds: content of each image of the batch; stride: None = contiguous rows, else the row stride of the batch;
# pad: value of the row padding bytes (strided cases)
Case = namedtuple("Case", "name w h sigma kinds stride pad", defaults=(("board",), None, 0))

SHAPES = [Case(f"s4-{w}x{h}", w, h, 4, (kind,)) for w, h, kind in [
    (255, 247, "board"), (255, 1, "noise"), (256, 9, "noise"), (256, 17, "board"), (257, 17, "board"), (257, 247, "noise"),
    (258, 16, "noise"), (258, 3, "board"), (513, 15, "board"), (513, 9, "noise"), (1023, 8, "noise"), (1023, 247, "board"),
    (1024, 5, "board"), (1024, 247, "noise"), (1025, 247, "board"), (1025, 15, "noise"), (1279, 4, "noise"), (1279, 17, "board"),
    (1280, 3, "board"), (1280, 33, "noise"), (1281, 2, "noise"), (1281, 247, "board"), (1921, 1, "noise"), (1921, 31, "board")]]
SIGMAS = [Case(f"s{s}-{w}x{h}", w, h, s, ("board" if (w + s) % 2 else "noise",)) for s in (2, 6, 8)
          for w, h in [(255, 40), (256, 17), (257, 9), (258, 33), (1025, 16), (1280, 47), (1921, 15)]]
TINY = [Case(f"tiny-s{s}-{w}x{h}", w, h, s, ("noise",)) for s in (4, 8) for w, h in [(2, 2), (5, 5), (14, 3), (15, 29), (29, 2), (1, 1)]]
BATCHES = [
    Case("batch-contiguous", 333, 247, 4, ("board", "noise", "flat", "range", "board")),          # 333 * 247 = 16 k + 11
    Case("batch-strided", 333, 247, 4, ("board", "noise", "flat", "range"), 352, 255),
    Case("batch-strided-band", 1280, 40, 4, ("noise", "board", "range"), 1296, 0),
    Case("batch-s8-contiguous", 257, 33, 8, ("noise", "flat", "board")),
    Case("batch-s2-strided", 513, 17, 2, ("board", "range", "noise"), 520, 255),
]
DENSE = [Case("dense-noise", 1280, 1080, 4, ("noise",)), Case("dense-checker", 1280, 1080, 4, ("checker",))]
BORDER = [Case("xcorners-border", 400, 300, 4, ("xcorners",))]
ARENA = [Case("arena-large", 1280, 1080, 4, ("board",)), Case("arena-small", 64, 48, 4, ("noise",)),
         Case("arena-large-again", 1279, 1001, 4, ("noise",))]
PADDING = [Case("padding-0", 333, 64, 4, ("range", "board", "range"), 344, 0),
           Case("padding-255", 333, 64, 4, ("range", "board", "range"), 344, 255)]
ALL_CASES = SHAPES + SIGMAS + TINY + BATCHES + DENSE + BORDER + ARENA + PADDING

_WORST = {k: (0.0, 0.0, "") for k in PLANES}          # plane -> (largest error / bound, that error, case)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in PLANES:
        r, e, name = _WORST[k]
        print(f"\n[corner planes] {k}: largest |gpu - reference| / bound = {r:.3g} (error {e:.3g}, case {name})")


def _scene():
    from tests.test_corners_oracle import _scene as sc
    if not hasattr(_scene, "img"):
        _scene.img = sc(3, 0)[0]
    return _scene.img


def _xcorners(w, h):
    """X-corners 9 to 17 px from each border: the orientation window is clipped and the radii that fit change"""
    img = np.full((h, w), 125, dtype=np.uint8)
    yy, xx = np.mgrid[-7:8, -7:8]
    patch = np.where((xx + 0.5) * (yy + 0.5) > 0, 205, 45).astype(np.uint8)
    centres = []
    for i, d in enumerate(range(9, 18)):
        centres += [(d, 40 + 25 * i), (w - 1 - d, 40 + 25 * i), (50 + 25 * i, d), (50 + 25 * i, h - 1 - d)]
    for cx, cy in centres:
        img[cy - 7:cy + 8, cx - 7:cx + 8] = patch
    return img


def _image(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    if kind == "flat":
        return np.full((h, w), 77, dtype=np.uint8)
    if kind == "range":                                         # grey values in [17, 230], both ends present
        g = rng.integers(17, 231, size=(h, w), dtype=np.uint8)
        g.flat[0], g.flat[-1] = 17, 230
        return g
    if kind == "checker":                                       # 6-pixel squares: ~37 k maxima at 1280 x 1080
        yy, xx = np.mgrid[0:h, 0:w]
        g = np.where(((yy // 6) + (xx // 6)) % 2 == 0, 40, 215) + rng.integers(-12, 13, size=(h, w))
        return np.clip(g, 0, 255).astype(np.uint8)
    if kind == "xcorners":
        return _xcorners(w, h)
    full = _scene()                                             # "board": a window on the rendered board, tiled if wider
    reps = (-(-(h + 300) // full.shape[0]), -(-(w + 380) // full.shape[1]))
    g = np.tile(full, reps)[300:300 + h, 380:380 + w].astype(int) + rng.integers(-6, 7, size=(h, w))
    return np.clip(g, 0, 255).astype(np.uint8)


def make_batch(case):
    """(contiguous images for the oracle and the reference, the views passed to the GPU)"""
    imgs = [_image(k, case.w, case.h, 1000 * case.w + 10 * case.h + i) for i, k in enumerate(case.kinds)]
    if case.stride is None:
        return imgs, imgs
    views = []
    for g in imgs:
        buf = np.full((case.h, case.stride), case.pad, dtype=np.uint8)
        buf[:, :case.w] = g
        views.append(buf[:, :case.w])
    return imgs, views


def _taps(sigma):
    from oracle import pyoracle as orc
    k = np.zeros(7 * sigma + 1)
    orc.lib().orc_gaussian_kernel(sigma, k.ctypes.data_as(C.POINTER(C.c_double)))
    return k


def _n_cells(w, h):
    sx, sy = w - 18, h - 18
    return ((sx + 4) // 5 if sx > 0 else 0) * ((sy + 4) // 5 if sy > 0 else 0)


def _where(mask):
    i, j = np.nonzero(mask)
    return (f"{i.size} pixels, rows {i.min()}..{i.max()} (row % 16 in {sorted(set((i % 16).tolist()))[:8]}), "
            f"cols {j.min()}..{j.max()} (col % 256 in {sorted(set((j % 256).tolist()))[:8]})")


def _same_bits(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def check_case(case, device):
    """Planes bit-identical to the oracle and within the reference's bound; candidates equal to the oracle's.
    Returns the GPU planes."""
    from oracle import pyoracle as orc
    from tscm_calib_amd import corners
    from tests.test_gpu_corners import _compare
    imgs, views = make_batch(case)
    P = corners.corner_planes(views, case.sigma, device, stride=case.stride)
    D = corners.detect_corners_batch(views, sigma=case.sigma, min_score=-1.0, device=device, stride=case.stride)
    taps = _taps(case.sigma)
    for b, img in enumerate(imgs):
        o = orc.corner_planes(img, case.sigma)
        ref = R.planes(img, case.sigma, taps)
        for k in PLANES:
            same = _same_bits(P[k][b], o[k])
            assert same.all(), f"{case.name} image {b} {k}: differs from the oracle at {_where(~same)}"
            err, ratio, bad = R.excess(P[k][b], ref[k])
            assert bad == 0, f"{case.name} image {b} {k}: {bad} pixels beyond the bound (largest error {err:.3g}, {ratio:.3g} x bound)"
            if ratio > _WORST[k][0]:
                _WORST[k] = (ratio, err, case.name)
        if img.min() == img.max():                              # 0 / 0 normalisation: NaN planes, for this image only
            assert all(np.isnan(P[k][b]).all() for k in PLANES)
        else:
            assert not any(np.isnan(P[k][b]).any() for k in PLANES), f"{case.name} image {b}: NaN outside the flat image"
        oc = orc.detect_corners(img, sigma=case.sigma, cap=max(_n_cells(case.w, case.h), 1))
        _compare(D[b], oc, min_score=-1.0)
    return P, D


@pytest.mark.parametrize("case", SHAPES + SIGMAS + TINY + BATCHES, ids=lambda c: c.name)
def test_planes_and_candidates(hip_device, case):
    check_case(case, hip_device)


@pytest.mark.parametrize("case", DENSE, ids=lambda c: c.name)
def test_dense_maxima(hip_device, case):
    _, D = check_case(case, hip_device)
    # every wave of k_nms_compact walks 3392 of the 53 k cells in 512-cell steps; the checkerboard goes beyond the
    # oracle's default cap of 8192 candidates
    assert D[0]["n_maxima"] > (8192 if case.kinds[0] == "checker" else 4096)


def test_clipped_windows_near_the_border(hip_device):
    case = BORDER[0]
    _, D = check_case(case, hip_device)
    x, y = D[0]["x"].astype(int), D[0]["y"].astype(int)
    d = np.minimum(np.minimum(x, case.w - 1 - x), np.minimum(y, case.h - 1 - y))      # fits(r) <=> d >= r
    assert (d < 10).any() and ((d >= 8) & (d < 12)).any() and ((d >= 12) & (d < 16)).any() and (d >= 16).any(), sorted(set(d.tolist()))


def test_padding_bytes_are_never_read(hip_device):
    p0, d0 = check_case(PADDING[0], hip_device)
    p1, d1 = check_case(PADDING[1], hip_device)
    for k in PLANES:
        assert _same_bits(p0[k], p1[k]).all(), k
    for a, b in zip(d0, d1):
        for k in ("x", "y", "v1", "v2", "score", "sub"):
            assert np.array_equal(a[k], b[k]), k


def test_arena_reuse(hip_device):
    """large, small, large: the grow-only arena is reused; every call's planes are checked"""
    for case in ARENA:
        check_case(case, hip_device)


def test_argument_checks(hip_device):
    from tscm_calib_amd import corners, lib
    img = np.zeros((32, 32), dtype=np.uint8)
    for kw, code in ((dict(sigma=3), -5), (dict(sigma=10), -5), (dict(device=99), -2)):
        with pytest.raises(lib.TscmError) as e:
            corners.corner_planes([img], **{"sigma": 4, **kw})
        assert e.value.code == code, kw
    with pytest.raises(ValueError):
        corners.corner_planes([img], stride=40)                       # a contiguous image has row stride 32
    f = lib.lib().tscm_corner_planes_batch
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
    ptrs = (C.c_void_p * 1)(img.ctypes.data)
    assert f(ptrs, 1, 32, 32, 31, 4, hip_device, None, None, None) == -1                  # stride < width
    assert f(None, 1, 32, 32, 32, 4, hip_device, None, None, None) == -1
    assert f(ptrs, 0, 32, 32, 32, 4, hip_device, None, None, None) == 0
    out = corners.corner_planes([img, img], planes=("metric",), device=hip_device)
    assert set(out) == {"metric"} and out["metric"].shape == (2, 32, 32)
