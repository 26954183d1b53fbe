"""GPU tests of the panorama composer (tscm_panorama_*): the output bytes, the coverage, every stage output and the overlap
sums equal the host restatement tests/pano_ref.py bit for bit (all of it is integer arithmetic).  Shapes are the smallest at
which each path can go wrong: a 72 x 24 panorama (no multiple of 64, 9 reduce columns of 8 at level 3, level widths 36, 18
and 9 that leave the 4-pixel vector path) and 64 x 32, 1..3 cameras, 1 and 3 channels.  LIMIT_CASES go to the ends of the
API's ranges, kPanoMaxCameras = 16 and kPanoMaxLevels = 6 (tscm_pano_kernels.h): 16 cameras set bit 15 of the uint16 coverage
mask, give label 15, fill the Gains struct and all 16 x 16 LDS slots of k_pano_overlap; 96 x 48 at L = 4 (the default level
count) has level widths 96, 48, 24, 12 and 6, the last off the vector path; 128 x 64 at L = 5 ends in a 4 x 2 level and
64 x 64 at L = 6 in a 1 x 1 level under a 2 x 2 one, all narrower than the 34 x 10 coarse halo of load_halo (kPanoHaloW,
kPanoHaloH) and than the kRedW = 32 outputs of a k_pano_reduce block, with col_index wrapping or clamping on W = 1; 12 cameras
at 64 x 32 leave 64 x 16 tiles (kPanoTileW, kPanoTileH) in which a camera's mask is zero and k_pano_lapblend skips it."""
import ctypes as C
import functools

import numpy as np
import pytest

from tscm_calib_amd import lib, panorama, synth
from tests import pano_ref as R

pytestmark = pytest.mark.gpu

SRC_W, SRC_H = 48, 40
MODES = [("seam", 0), ("feather", 0), ("multiband", 1), ("multiband", 2), ("multiband", 3)]
MODE_ID = {"seam": R.SEAM, "feather": R.FEATHER, "multiband": R.MULTIBAND}


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _tables(n, pw, ph):
    """Random sample positions, a fifth outside the image, a tenth (-1, -1), a tenth exactly on integer coordinates; every
    camera also gets a band of columns it does not see at all."""
    rng = np.random.default_rng(100 * n + pw)
    mx = rng.uniform(-0.5, SRC_W - 0.5, (n, ph, pw)).astype(np.float32)
    my = rng.uniform(-0.5, SRC_H - 0.5, (n, ph, pw)).astype(np.float32)
    pick = rng.uniform(size=(n, ph, pw))
    far = pick < 0.2
    mx[far] = rng.uniform(-40.0, SRC_W + 40.0, far.sum()).astype(np.float32)
    my[far] = rng.uniform(-40.0, SRC_H + 40.0, far.sum()).astype(np.float32)
    hole = (pick >= 0.2) & (pick < 0.3)
    mx[hole], my[hole] = -1.0, -1.0
    whole = (pick >= 0.3) & (pick < 0.4)
    mx[whole], my[whole] = np.rint(mx[whole]), np.rint(my[whole])
    for k in range(n):
        lo = (k * pw) // (n + 1)
        mx[k, :, lo:lo + pw // 6], my[k, :, lo:lo + pw // 6] = -1.0, -1.0
    mx.setflags(write=False)
    my.setflags(write=False)
    return mx, my


@functools.lru_cache(maxsize=None)
def _limit_tables(n, pw, ph):
    """The recipe of _tables for the LIMIT_CASES, with the unseen bands replaced: the columns are cut into n bands, and in band
    b only camera b samples the top quarter of the rows (label b occurs whatever the weights are) and the cameras below b
    sample nothing further down (coverage n - b at most, so band 0 is where all cameras meet); the odd cameras see nothing of
    the lower half, so that whole tiles of their masks are zero."""
    rng = np.random.default_rng(100 * n + pw + 7)
    mx = rng.uniform(-0.5, SRC_W - 0.5, (n, ph, pw)).astype(np.float32)
    my = rng.uniform(-0.5, SRC_H - 0.5, (n, ph, pw)).astype(np.float32)
    pick = rng.uniform(size=(n, ph, pw))
    far = pick < 0.2
    mx[far] = rng.uniform(-40.0, SRC_W + 40.0, far.sum()).astype(np.float32)
    my[far] = rng.uniform(-40.0, SRC_H + 40.0, far.sum()).astype(np.float32)
    hole = (pick >= 0.2) & (pick < 0.3)
    mx[hole], my[hole] = -1.0, -1.0
    whole = (pick >= 0.3) & (pick < 0.4)
    mx[whole], my[whole] = np.rint(mx[whole]), np.rint(my[whole])
    top = max(ph // 4, 1)
    for b in range(n):
        lo, hi = (b * pw) // n, ((b + 1) * pw) // n
        for k in range(n):
            if k != b:
                mx[k, :top, lo:hi], my[k, :top, lo:hi] = -1.0, -1.0
            if k < b:
                mx[k, top:, lo:hi], my[k, top:, lo:hi] = -1.0, -1.0
    mx[1::2, ph // 2:], my[1::2, ph // 2:] = -1.0, -1.0
    mx.setflags(write=False)
    my.setflags(write=False)
    return mx, my


@functools.lru_cache(maxsize=None)
def _images(n, ch, seed=0):
    rng = np.random.default_rng(7 + seed)
    out = tuple(rng.integers(0, 256, (SRC_H, SRC_W) if ch == 1 else (SRC_H, SRC_W, ch)).astype(np.uint8) for _ in range(n))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _weights(n):
    rng = np.random.default_rng(99)
    out = []
    for k in range(n):
        wgt = rng.integers(0, 256, (SRC_H, SRC_W)).astype(np.uint8)
        wgt[:, :8] = 0                                   # a_k = 0 where the image itself is not: v_k != 0 without coverage
        out.append(None if (n > 1 and k == 1) else wgt)  # a NULL entry among weight images
    return tuple(out)


# distinct, in 1..4095, both ends included; the first three are those of the 1..3 camera cases
GAINS = (200, 256, 700, 1, 4095, 64, 1024, 300, 128, 511, 2048, 90, 257, 255, 150, 3000)


def _options(index):
    """wrap_x, weight images and gains rotate through the cases so that every value of each meets every mode."""
    return bool(index & 1), bool(index & 2), bool(index & 4)


@functools.lru_cache(maxsize=None)
def _reference(n, ch, pw, ph, mode, levels, wrap, with_weights, with_gains, seed=0, limit=False):
    mx, my = (_limit_tables if limit else _tables)(n, pw, ph)
    gains = tuple(int(g) for g in GAINS[:n]) if with_gains else None
    return R.compose(list(_images(n, ch, seed)), list(_weights(n)) if with_weights else None, mx, my, MODE_ID[mode], levels, wrap, gains), gains


def _composer(n, ch, pw, ph, mode, levels, wrap, with_weights, device, limit=False):
    mx, my = (_limit_tables if limit else _tables)(n, pw, ph)
    return panorama.Composer.from_tables(mx, my, (SRC_W, SRC_H), channels=ch, mode=mode, levels=max(levels, 1), wrap_x=wrap,
                                         weights=list(_weights(n)) if with_weights else None, device=device)


def _squeeze(ref_out, ch):
    return ref_out[..., 0] if ch == 1 else ref_out


CASES = [(n, ch, pw, ph, mode, levels) for n in (1, 2, 3) for ch in (1, 3) for pw, ph in ((72, 24), (64, 32)) for mode, levels in MODES]


# n, channels, pano_w, pano_h, mode, levels: the ends of the API's ranges (the module docstring says what each one reaches)
LIMIT_CASES = [
    (5, 3, 96, 48, "multiband", 4),
    (9, 1, 128, 64, "multiband", 5),
    (16, 1, 64, 64, "multiband", 6),
    (16, 1, 64, 64, "multiband", 6),
    (16, 3, 72, 24, "seam", 0),
    (16, 3, 72, 24, "feather", 0),
    (12, 1, 64, 32, "multiband", 3),
]


def _limit_options(index):
    """_options one step on: the two L = 6 cases get wrap_x on with weight images and wrap_x off with gains, and the 16-camera
    FEATHER case weights and gains together."""
    return _options(index + 1)


def _check_compose_and_stages(device, case, options, limit):
    n, ch, pw, ph, mode, levels = case
    wrap, with_weights, with_gains = options
    ref, gains = _reference(n, ch, pw, ph, mode, levels, wrap, with_weights, with_gains, 0, limit)
    with _composer(n, ch, pw, ph, mode, levels, wrap, with_weights, device, limit) as c:
        out, cov = c.compose(_images(n, ch), gains=gains, with_coverage=True)
        st = c.stages(_images(n, ch), gains=gains)
    assert np.array_equal(st["alpha"], ref["alpha"])
    assert np.array_equal(st["label"], ref["label"])
    assert np.array_equal(cov, ref["coverage"])
    assert np.array_equal(st["sampled"], ref["sampled"])
    if mode == "multiband":
        assert np.array_equal(st["mask_pyramid"], R.flat(ref["mask"], 1))
        assert np.array_equal(st["lap_pyramid"], R.flat(ref["lap"], 2))
        assert np.array_equal(st["blend_pyramid"], R.flat(ref["blend"], 1))
    assert np.array_equal(out, _squeeze(ref["out"], ch))


@pytest.mark.parametrize("index,case", list(enumerate(CASES)), ids=["n%d-c%d-%dx%d-%s%d" % c for c in CASES])
def test_compose_and_stages_equal_the_restatement(hip_device, index, case):
    _check_compose_and_stages(hip_device, case, _options(index + index // 8), False)


@pytest.mark.parametrize("index,case", list(enumerate(LIMIT_CASES)),
                         ids=["n%d-c%d-%dx%d-%s%d" % c + "-w%d" % _limit_options(i)[0] for i, c in enumerate(LIMIT_CASES)])
def test_compose_and_stages_equal_the_restatement_at_the_limits(hip_device, index, case):
    _check_compose_and_stages(hip_device, case, _limit_options(index), True)


@pytest.mark.parametrize("mode,levels", [("feather", 0), ("multiband", 2)])
@pytest.mark.parametrize("ch", [1, 3])
def test_padded_strides_and_untouched_padding(hip_device, mode, levels, ch):
    n, pw, ph = 2, 72, 24
    ref, _ = _reference(n, ch, pw, ph, mode, levels, True, False, False)
    wide = [np.full((SRC_H, SRC_W + 5) if ch == 1 else (SRC_H, SRC_W + 5, ch), 77, np.uint8) for _ in range(n)]
    views = []
    for buf, img in zip(wide, _images(n, ch)):
        buf[:, :SRC_W] = img
        views.append(buf[:, :SRC_W])
    canvas = np.full((ph, pw + 3) if ch == 1 else (ph, pw + 3, ch), 201, np.uint8)
    with _composer(n, ch, pw, ph, mode, levels, True, False, hip_device) as c:
        c.compose(views, out=canvas[:, :pw])
    assert np.array_equal(canvas[:, :pw], _squeeze(ref["out"], ch))
    assert np.all(canvas[:, pw:] == 201)


@pytest.mark.parametrize("mode,levels", [("seam", 0), ("multiband", 3)])
def test_a_handle_is_reusable(hip_device, mode, levels):
    n, ch, pw, ph = 3, 3, 72, 24
    first, second = _images(n, ch, 0), _images(n, ch, 1)
    with _composer(n, ch, pw, ph, mode, levels, True, True, hip_device) as c:
        a1 = c.compose(first)
        b = c.compose(second)
        a2 = c.compose(first)
    with _composer(n, ch, pw, ph, mode, levels, True, True, hip_device) as fresh:
        b_fresh = fresh.compose(second)
    assert np.array_equal(b, b_fresh)
    assert np.array_equal(a1, a2)
    assert np.array_equal(b, _squeeze(_reference(n, ch, pw, ph, mode, levels, True, True, False, 1)[0]["out"], ch))
    assert not np.array_equal(a1, b)


@pytest.mark.parametrize("ch", [1, 3])
def test_overlap_sums(hip_device, ch):
    n, pw, ph = 3, 72, 24
    ref, _ = _reference(n, ch, pw, ph, "feather", 0, True, True, False)
    with _composer(n, ch, pw, ph, "feather", 0, True, True, hip_device) as c:
        count, total = c.overlap(_images(n, ch))
    assert np.array_equal(count, ref["count"]) and np.array_equal(total, ref["sum"])
    assert count[0, 1] > 0 and count[0, 0] > count[0, 1]


@pytest.mark.parametrize("ch", [1, 3])
def test_overlap_sums_of_sixteen_cameras(hip_device, ch):
    """Every one of the 16 x 16 LDS slots of k_pano_overlap (a * 16 + b) holds a pair that occurs."""
    n, pw, ph = 16, 72, 24
    ref, _ = _reference(n, ch, pw, ph, "feather", 0, True, True, False, 0, True)
    assert ref["count"].shape == (16, 16) and np.all(ref["count"] > 0)
    with _composer(n, ch, pw, ph, "feather", 0, True, True, hip_device, True) as c:
        count, total = c.overlap(_images(n, ch))
    assert np.array_equal(count, ref["count"]) and np.array_equal(total, ref["sum"])


def test_refusals_that_need_a_handle(hip_device):
    """stride, dst_stride, a gain out of range, a NULL image and a pyramid output outside MULTIBAND: TSCM_E_INVALID with a
    text that names the argument.  (They need a handle, so they cannot run without a device.)"""
    L = lib.lib()
    n, ch, pw, ph = 2, 1, 64, 32
    imgs = _images(n, ch)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in imgs])
    dst = np.zeros((ph, pw), np.uint8)
    ub = C.POINTER(C.c_ubyte)
    d = dst.ctypes.data_as(ub)
    with _composer(n, ch, pw, ph, "feather", 0, True, False, hip_device) as c:
        h = c._handle
        for gains, text, full in (((0, 256), b"gain_q8[0]", b"gain_q8[0] = 0 outside 1..4095"), ((256, 4096), b"gain_q8[1]", b"gain_q8[1] = 4096 outside 1..4095")):
            g = np.array(gains, np.uint16)
            assert L.tscm_panorama_compose(h, ptrs, SRC_W, lib.ushort_ptr(g), d, pw, None, None) == -1
            assert text in L.tscm_last_error()
            assert L.tscm_last_error() == full               # the sentences the sweep's composer shares: the whole text
        assert L.tscm_panorama_compose(h, ptrs, SRC_W - 1, None, d, pw, None, None) == -1 and b"stride" in L.tscm_last_error()
        assert L.tscm_last_error() == b"stride %d < width * channels = %d" % (SRC_W - 1, SRC_W)
        assert L.tscm_panorama_compose(h, ptrs, SRC_W, None, d, pw - 1, None, None) == -1 and b"dst_stride" in L.tscm_last_error()
        assert L.tscm_panorama_compose(h, ptrs, SRC_W, None, None, pw, None, None) == -1 and b"dst" in L.tscm_last_error()
        holed = (C.c_void_p * n)(imgs[0].ctypes.data, None)
        assert L.tscm_panorama_compose(h, holed, SRC_W, None, d, pw, None, None) == -1 and b"images[1]" in L.tscm_last_error()
        assert L.tscm_last_error() == b"images[1] is NULL"
        assert L.tscm_panorama_compose(h, None, SRC_W, None, d, pw, None, None) == -1 and L.tscm_last_error() == b"images is NULL"
        assert L.tscm_panorama_overlap(h, ptrs, SRC_W, None, None) == -1 and b"count" in L.tscm_last_error()
        pyr = np.zeros(8 * pw * ph, np.int16).ctypes.data_as(C.POINTER(C.c_short))
        assert L.tscm_panorama_stages(h, ptrs, SRC_W, None, None, None, None, None, None, pyr) == -1 and b"blend_pyramid" in L.tscm_last_error()
        assert L.tscm_panorama_stages(h, ptrs, SRC_W, None, None, None, None, d, None, None) == -1 and b"mask_pyramid" in L.tscm_last_error()
        assert np.all(dst == 0)


def _hash_noise(k, w, h):
    idx = np.arange(w * h, dtype=np.uint64) + np.uint64(k) * np.uint64(w * h)
    return (synth.splitmix64(idx) >> np.uint64(56)).astype(np.uint8).reshape(h, w)


def test_golden_rig_through_the_composer(hip_device):
    """The four-camera golden calibration, 256 x 128, L = 4, radial weights.  The device-built tables are an input to both
    sides, so the sincos of the table kernel does not enter."""
    w, h, pw, ph = int(synth.IMG_W), int(synth.IMG_H), 256, 128
    images = [_hash_noise(k, w, h) for k in range(4)]
    with panorama.Composer(synth.CALIB_INTR, synth.CALIB_TWC, (w, h), (pw, ph), channels=1, mode="multiband", levels=4, device=hip_device) as c:
        out, cov = c.compose(images, with_coverage=True)
        count, total = c.overlap(images)
        ref = R.compose(images, c.weights, c.mapx, c.mapy, R.MULTIBAND, 4, True)
    assert np.array_equal(cov, ref["coverage"])
    assert np.array_equal(out, ref["out"][..., 0])
    assert np.array_equal(count, ref["count"]) and np.array_equal(total, ref["sum"])
    assert cov[ph // 2].min() >= 1 and cov.max() >= 2       # the rig sees the whole horizon, neighbours overlap
    assert panorama.exposure_gains(count, total).shape == (4,)
