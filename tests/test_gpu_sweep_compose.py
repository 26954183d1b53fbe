"""GPU tests of the composer at the swept depth (tscm_sweep_compose, tscm_sweep_compose_stages): every stage output, the
panorama and the coverage equal the host restatement tests/sweep_compose_ref.py bit for bit (all of it is integer
arithmetic), a constant index map equals the static composer (tscm_panorama_compose) on that table, and the device chain
depth -> compose removes the parallax of the sphere scene of tests/test_gpu_sweep.py.  Shapes are those of that file, the
smallest at which each path can go wrong: 72 x 24 (no multiple of the 64 x 16 pyramid tile, two tiles per row and column),
64 x 32, 5 x 3 (an odd number of pixels: the last quad holds 3), 2..4 and 8 cameras, D = 16 and 80.  Three shapes take the
per-frame pyramids to the depths the static composer's LIMIT_CASES reach (kPanoMaxLevels = 6 of tscm_pano_kernels.h):
64 x 64 at L = 6 ends in a 2 x 2 level over a 1 x 1 top, where col_index wraps on W = 1; 96 x 48 at L = 4, the default level
count, has level widths 96 .. 6, the last off the 4-pixel vector path; 128 x 64 at L = 5 ends in 4 x 2.  Every one of these
levels is narrower than the 34 x 10 coarse halo of load_halo (kPanoHaloW, kPanoHaloH)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import sweep_compose_ref as CR
from tests import test_gpu_sweep as gs
from tests import test_sweep_compose_reference as ref_scene
from tscm_calib_amd import lib, panorama, sweep

pytestmark = pytest.mark.gpu

SRC_W, SRC_H = gs.SRC_W, gs.SRC_H
MODES = {CR.SEAM: "seam", CR.FEATHER: "feather", CR.MULTIBAND: "multiband"}


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _images(n, ch, seed=0):
    rng = np.random.default_rng(31 + 10 * seed + ch)
    out = tuple(rng.integers(0, 256, (SRC_H, SRC_W) if ch == 1 else (SRC_H, SRC_W, 3)).astype(np.uint8) for _ in range(n))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _index_map(pw, ph, D, seed=0):
    """Uniform in [-16, 16 D + 40), and in every run of 64 pixels one invalid and one over-range entry, so that both occur
    in every wave (a wave owns 256 consecutive pixels)."""
    rng = np.random.default_rng(500 + pw + D + seed)
    idx = rng.integers(-16, 16 * D + 40, ph * pw).astype(np.int16)
    for lo in range(0, ph * pw, 64):
        a, b = rng.choice(min(64, ph * pw - lo), 2, replace=False)
        idx[lo + a], idx[lo + b] = -16, 16 * D + 8 + rng.integers(0, 32)
    idx = idx.reshape(ph, pw)
    idx.setflags(write=False)
    return idx


def _gains(n, on):
    return [(200 + 37 * k) % 700 + 60 for k in range(n)] if on else None


# n, pw, ph, D, channels, mode, levels, wrap_x, weight images, gains, fallback at D - 1: the options rotate through the shapes
S_, F_, M_ = CR.SEAM, CR.FEATHER, CR.MULTIBAND
CASES = [
    (2, 72, 24, 16, 1, S_, 0, True, False, False, False),
    (3, 64, 32, 80, 3, F_, 0, False, True, True, True),
    (4, 72, 24, 80, 1, M_, 1, True, True, True, False),
    (8, 72, 24, 16, 3, M_, 2, False, False, True, True),
    (2, 64, 32, 16, 3, M_, 3, True, True, False, False),
    (3, 72, 24, 16, 1, M_, 3, False, True, True, True),
    (4, 64, 32, 80, 3, S_, 0, True, True, True, True),
    (8, 64, 32, 16, 1, F_, 0, True, True, True, False),
    (2, 5, 3, 16, 3, S_, 0, True, True, True, True),
    (3, 5, 3, 80, 1, F_, 0, False, False, False, False),
    (4, 5, 3, 16, 3, F_, 0, True, True, True, True),
    (8, 72, 24, 80, 1, S_, 0, False, True, False, True),
    (4, 64, 32, 16, 1, M_, 1, False, False, True, True),
    (3, 64, 32, 80, 3, M_, 2, True, True, True, False),
    (2, 72, 24, 80, 3, M_, 1, False, False, False, True),
    (8, 64, 32, 16, 3, M_, 3, True, True, False, False),
    (3, 72, 24, 80, 3, F_, 0, True, False, True, False),
    # the pyramid's depth: the 1 x 1 top of L = 6, the default L = 4 with a 6 x 3 top, the 4 x 2 top of L = 5
    (8, 64, 64, 16, 3, M_, 6, True, True, True, False),
    (5, 96, 48, 16, 1, M_, 4, False, True, False, True),
    (8, 128, 64, 16, 1, M_, 5, True, False, True, True),
]
IDS = ["n%d-%dx%d-D%d-c%d-%s%d-w%d-m%d-g%d-f%d" % (c[:5] + (MODES[c[5]],) + c[6:]) for c in CASES]


def _params(case):
    n, pw, ph, D, ch, mode, levels, wrap, with_weights, with_gains, last = case
    return dict(mode=mode, levels=max(levels, 1), wrap_x=int(wrap), fallback_index=D - 1 if last else 0)


def _weights(case):
    return list(gs._weights(case[0])) if case[8] else None


@functools.lru_cache(maxsize=None)
def _reference(case, seed=0, constant=None):
    n, pw, ph, D, ch, mode, levels, wrap = case[:8]
    mx, my = gs._tables(n, D, pw, ph)
    idx = _index_map(pw, ph, D, seed) if constant is None else np.full((ph, pw), constant, np.int16)
    p = _params(case)
    return CR.compose(list(_images(n, ch, seed)), _weights(case), mx, my, idx, mode=mode, levels=levels, wrap=wrap, gains=_gains(n, case[9]),
                      fallback_index=p["fallback_index"])


def _sweeper(case, device):
    n, pw, ph, D = case[:4]
    mx, my = gs._tables(n, D, pw, ph)
    return sweep.Sweeper.from_tables(mx, my, (SRC_W, SRC_H), weights=_weights(case), device=device)


def _check_stages(st, ref, mode):
    for name in ("hypothesis", "sampled", "alpha", "label"):
        assert np.array_equal(st[name], ref[name]), name
    if mode == CR.MULTIBAND:
        assert np.array_equal(st["mask_pyramid"], CR.pano_ref.flat(ref["mask"], 1)), "mask_pyramid"
        assert np.array_equal(st["lap_pyramid"], CR.pano_ref.flat(ref["lap"], 2)), "lap_pyramid"
        assert np.array_equal(st["blend_pyramid"], CR.pano_ref.flat(ref["blend"], 1)), "blend_pyramid"


# ------------------------------------------------------------------------------------------------ equality
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stages_and_output_equal_the_restatement(hip_device, case):
    n, pw, ph, D, ch, mode = case[:6]
    ref = _reference(case)
    imgs, idx, g, p = _images(n, ch), _index_map(pw, ph, D), _gains(n, case[9]), _params(case)
    with _sweeper(case, hip_device) as s:
        st = s.compose_stages(imgs, idx, gains=g, **p)
        out, cov = s.compose(imgs, idx, gains=g, with_coverage=True, **p)
    _check_stages(st, ref, mode)
    assert np.array_equal(out.reshape(ph, pw, ch), ref["out"])
    assert np.array_equal(cov, ref["coverage"])
    z = ref["hypothesis"]
    assert (idx < 0).any() and (idx >= 16 * D).any() and z.max() == D - 1 and len(np.unique(z)) > min(D, ph * pw) // 4
    if pw > 5:
        assert set(np.unique(ref["coverage"]).tolist()) >= {0, 1, 2}


@pytest.mark.parametrize("case", [CASES[k] for k in (0, 1, 5, 7, 10)], ids=[IDS[k] for k in (0, 1, 5, 7, 10)])
def test_a_constant_map_equals_the_restatement(hip_device, case):
    n, pw, ph, D, ch, mode = case[:6]
    z0 = D // 3
    ref = _reference(case, 0, 16 * z0 + 5)
    with _sweeper(case, hip_device) as s:
        out, cov = s.compose(_images(n, ch), np.full((ph, pw), 16 * z0 + 5, np.int16), gains=_gains(n, case[9]), with_coverage=True, **_params(case))
    assert np.all(ref["hypothesis"] == z0)
    assert np.array_equal(out.reshape(ph, pw, ch), ref["out"]) and np.array_equal(cov, ref["coverage"])


@pytest.mark.parametrize("mode", [S_, F_, M_], ids=["seam", "feather", "multiband"])
@pytest.mark.parametrize("ch", [1, 3])
def test_a_constant_map_equals_the_static_composer(hip_device, mode, ch):
    """16 z0 everywhere: tscm_panorama_compose on the tables (., z0), byte for byte; an all-invalid map with fallback 0: the
    composer on the tables (., 0), today's panorama at infinity when inv_distance[0] = 0."""
    n, pw, ph, D, levels = 4, 72, 24, 16, 3
    mx, my = gs._tables(n, D, pw, ph)
    wgt, g, imgs = list(gs._weights(n)), _gains(n, True), _images(n, ch)
    with sweep.Sweeper.from_tables(mx, my, (SRC_W, SRC_H), weights=wgt, device=hip_device) as s:
        for z0, idx in ((11, np.full((ph, pw), 16 * 11, np.int16)), (0, np.full((ph, pw), sweep.INVALID, np.int16))):
            got, gcov = s.compose(imgs, idx, gains=g, with_coverage=True, mode=mode, levels=levels, wrap_x=1, fallback_index=0)
            with panorama.Composer.from_tables(mx[:, z0], my[:, z0], (SRC_W, SRC_H), channels=ch, mode=MODES[mode], levels=levels, wrap_x=True, weights=wgt,
                                               device=hip_device) as c:
                want, wcov = c.compose(imgs, gains=g, with_coverage=True)
            assert np.array_equal(got, want) and np.array_equal(gcov, wcov)
            assert want.any()


# ------------------------------------------------------------------------------------------------ strides, handle paths
@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_row_padding_of_images_index_map_and_output_at_once(hip_device, case):
    n, pw, ph, D, ch = case[:5]
    ref = _reference(case)
    views = []
    for img in _images(n, ch):
        buf = np.full((SRC_H, SRC_W + 5) + img.shape[2:], 77, np.uint8)
        buf[:, :SRC_W] = img
        views.append(buf[:, :SRC_W])
    wide_idx = np.full((ph, pw + 3), -5000, np.int16)
    wide_idx[:, :pw] = _index_map(pw, ph, D)
    canvas = np.full((ph, pw + 7) + ((ch,) if ch > 1 else ()), 201, np.uint8)
    with _sweeper(case, hip_device) as s:
        s.compose(views, wide_idx[:, :pw], gains=_gains(n, case[9]), out=canvas[:, :pw], **_params(case))
    assert np.array_equal(canvas[:, :pw].reshape(ph, pw, ch), ref["out"])
    assert np.all(canvas[:, pw:] == 201)


def test_the_map_left_on_the_device_and_a_handle_that_changes_mode_and_channels(hip_device):
    """index16=None after depth() equals passing the downloaded map; depth, compose, depth, compose on one handle with another
    mode and channel count each time, and the first frame again: the same bits."""
    n, pw, ph, D = 3, 72, 24, 16
    mx, my = gs._tables(n, D, pw, ph)
    grey0, grey1 = gs._images(n, 0), gs._images(n, 1)
    col = _images(n, 3)
    with sweep.Sweeper.from_tables(mx, my, (SRC_W, SRC_H), device=hip_device, paths=4) as s:
        idx0 = s.depth(grey0)
        a_dev = s.compose(grey0, mode="feather")
        a_host = s.compose(grey0, idx0, mode="feather")
        idx1 = s.depth(grey1)
        b_dev = s.compose(col, mode="multiband", levels=2, fallback_index=5)
        b_host = s.compose(col, idx1, mode="multiband", levels=2, fallback_index=5)
        assert np.array_equal(s.depth(grey0), idx0)                   # the composer's buffers leave the depth pass alone
        a_again = s.compose(grey0, mode="feather")
        c_seam = s.compose(col, idx1, mode="seam", fallback_index=5)
    assert not np.array_equal(idx0, idx1) and (idx0 < 0).any() and (idx0 >= 0).any()
    assert np.array_equal(a_dev, a_host) and np.array_equal(a_dev, a_again)
    assert np.array_equal(b_dev, b_host)
    assert np.array_equal(a_dev[..., None], CR.compose(list(grey0), None, mx, my, idx0, mode=F_)["out"])
    assert np.array_equal(b_dev, CR.compose(list(col), None, mx, my, idx1, mode=M_, levels=2, fallback_index=5)["out"])
    assert np.array_equal(c_seam, CR.compose(list(col), None, mx, my, idx1, mode=S_, fallback_index=5)["out"])


def test_refusals_that_need_a_handle(hip_device):
    """Every refusal of tscm_sweep_compose / _stages behind the NULL handle: TSCM_E_INVALID with a text that names the argument."""
    L = lib.lib()
    n, pw, ph, D = 2, 72, 24, 16
    mx, my = gs._tables(n, D, pw, ph)
    imgs = _images(n, 1)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in imgs])
    out, idx = np.zeros((ph, pw * 3), np.uint8), np.zeros((ph, pw), np.int16)
    o, ix = out.ctypes.data_as(C.POINTER(C.c_ubyte)), idx.ctypes.data_as(C.POINTER(C.c_short))
    mk = lambda **kw: C.byref(sweep.compose_params(**dict(dict(mode="seam"), **kw)))

    def refused(word, images=ptrs, stride=SRC_W, ch=1, index=ix, istride=pw, params=None, gains=None, dst=o, dstride=pw, full=None):
        rc = L.tscm_sweep_compose(h, images, stride, ch, index, istride, params or mk(), gains, dst, dstride, None, None)
        assert rc == -1 and word in L.tscm_last_error(), (word, rc, L.tscm_last_error())
        assert full is None or L.tscm_last_error() == full, (full, L.tscm_last_error())      # the sentences shared with other entry points: the whole text

    with sweep.Sweeper.from_tables(mx, my, (SRC_W, SRC_H), device=hip_device) as s:
        h = s._handle
        refused(b"index16 is NULL", index=None, full=b"index16 is NULL and the handle has not run tscm_sweep_depth yet")       # no frame yet
        refused(b"images is NULL", images=None, full=b"images is NULL")
        refused(b"images[1]", images=(C.c_void_p * n)(imgs[0].ctypes.data, None), full=b"images[1] is NULL")
        refused(b"channels", ch=2)
        refused(b"channels", ch=4)
        refused(b"images is NULL", images=None, ch=2, full=b"images is NULL")          # two faults: the images come first, then channels, then stride
        refused(b"images[1]", images=(C.c_void_p * n)(imgs[0].ctypes.data, None), ch=2, full=b"images[1] is NULL")
        refused(b"channels", ch=2, stride=0, full=b"channels 2 is not 1 or 3")
        refused(b"stride", stride=SRC_W - 1, full=b"stride %d < width * channels = %d" % (SRC_W - 1, SRC_W))
        refused(b"stride", stride=3 * SRC_W - 1, ch=3, full=b"stride %d < width * channels = %d" % (3 * SRC_W - 1, 3 * SRC_W))
        assert L.tscm_sweep_compose(h, ptrs, SRC_W, 1, ix, pw, None, None, o, pw, None, None) == -1 and b"params is NULL" in L.tscm_last_error()
        bad = sweep.compose_params(mode="seam")
        bad.struct_size -= 4
        refused(b"struct_size", params=C.byref(bad), full=b"params: struct_size %d is not sizeof(tscm_sweep_compose_params) = %d"
                % (bad.struct_size, C.sizeof(lib.CSweepComposeParams)))
        refused(b"unknown mode", params=mk(mode=3))
        refused(b"levels", params=mk(mode="multiband", levels=0))
        refused(b"levels", params=mk(mode="multiband", levels=7))
        refused(b"pano_w", params=mk(mode="multiband", levels=4))      # 72 is no multiple of 16
        refused(b"fallback_index", params=mk(fallback_index=-1))
        refused(b"fallback_index", params=mk(fallback_index=D))
        refused(b"index_stride", istride=pw - 1, full=b"index_stride %d < pano_w %d" % (pw - 1, pw))
        refused(b"gain_q8[1]", gains=(C.c_ushort * n)(256, 0), full=b"gain_q8[1] = 0 outside 1..4095")
        refused(b"gain_q8[0]", gains=(C.c_ushort * n)(4096, 256), full=b"gain_q8[0] = 4096 outside 1..4095")
        refused(b"dst is NULL", dst=None)
        refused(b"dst_stride", dstride=pw - 1)
        refused(b"dst_stride", dstride=3 * pw - 1, ch=3, stride=3 * SRC_W)
        mask, lap = np.zeros(8, np.uint8), np.zeros(8, np.int16)
        mp, lp = mask.ctypes.data_as(C.POINTER(C.c_ubyte)), lap.ctypes.data_as(C.POINTER(C.c_short))
        for pyr, word in (((mp, None, None), b"mask_pyramid"), ((None, lp, None), b"lap_pyramid"), ((None, None, lp), b"blend_pyramid")):
            rc = L.tscm_sweep_compose_stages(h, ptrs, SRC_W, 1, ix, pw, mk(mode="feather"), None, None, None, None, None, *pyr)
            assert rc == -1 and word in L.tscm_last_error() and b"MULTIBAND" in L.tscm_last_error()
        assert L.tscm_sweep_compose_stages(h, ptrs, SRC_W - 1, 1, ix, pw, mk(), None, None, None, None, None, None, None, None) == -1 and b"stride" in L.tscm_last_error()
    assert not out.any()
    # pano_h: a handle whose width passes and whose height does not
    mx2, my2 = gs._tables(2, 16, 64, 32)
    with sweep.Sweeper.from_tables(mx2[:, :, :24], my2[:, :, :24], (SRC_W, SRC_H), device=hip_device) as s:
        idx2 = np.zeros((24, 64), np.int16)
        rc = L.tscm_sweep_compose(s._handle, ptrs, SRC_W, 1, idx2.ctypes.data_as(C.POINTER(C.c_short)), 64, mk(mode="multiband", levels=4), None, o, 64, None, None)
        assert rc == -1 and b"pano_h" in L.tscm_last_error()


# ------------------------------------------------------------------------------------------------ end to end
def test_rig_panorama_on_the_textured_sphere(hip_device):
    """The device chain depth -> compose and the restatement on the device-built tables give equal bytes, and the parallax
    goes: FEATHER against the texture seen from the rig origin stays within twice the CPU reference value (the project's
    allowance for the unpinned sincos of the table kernel) and within half of the error at infinity of the same run; SEAM
    and MULTIBAND beat their own error at infinity."""
    intr, T, imgs = gs.sphere_scene()
    pw, ph = gs.SCENE["pano_w"], gs.SCENE["pano_h"]
    inv = sweep.inverse_distances(gs.SCENE["near"], D=gs.SCENE["D"])
    truth = ref_scene.sphere_truth()
    far = np.full((ph, pw), sweep.INVALID, np.int16)
    swept, at_inf = {}, {}
    with sweep.Sweeper.from_rig(intr, T, (320, 270), pw, ph, inv, weights=None, device=hip_device, keep_tables=True, paths=gs.SCENE["paths"]) as s:
        idx = s.depth(imgs)
        for mode in (S_, F_, M_):
            swept[mode], cov = s.compose(imgs, with_coverage=True, mode=mode, levels=ref_scene.LEVELS)
            at_inf[mode] = s.compose(imgs, far, mode=mode, levels=ref_scene.LEVELS)
        mx, my = s.mapx, s.mapy
    # the device-built tables are an input to both sides, so the sincos of the table kernel does not enter
    for mode in (S_, F_, M_):
        host = CR.compose(imgs, None, mx, my, idx, mode=mode, levels=ref_scene.LEVELS)
        assert np.array_equal(swept[mode][..., None], host["out"]), MODES[mode]
        assert np.array_equal(cov, host["coverage"])
    err = {m: CR.mean_abs_error(swept[m], truth) for m in swept}
    err_inf = {m: CR.mean_abs_error(at_inf[m], truth) for m in at_inf}
    for m in (S_, F_, M_):
        print(f"{MODES[m]}: error against the texture {err[m]:.2f} at the swept depth, {err_inf[m]:.2f} at infinity "
              f"(CPU reference {ref_scene.SPHERE_TABLE['swept'][m]}, {ref_scene.SPHERE_TABLE['infinity'][m]})")
    assert ref_scene.SPHERE_RATIO_CPU < 0.5                       # a condition on the scene, not a tolerance
    assert err[F_] <= 2.0 * ref_scene.SPHERE_FEATHER_CPU
    assert err[F_] <= 0.5 * err_inf[F_]
    assert err[S_] < err_inf[S_] and err[M_] < err_inf[M_]


def test_rig_panorama_in_one_call(hip_device):
    """sweep.rig_panorama on colour images: the grey depth pass, the filter and the compose at the filtered map."""
    intr, T, imgs = gs.sphere_scene()
    col = [np.stack([g, g // 2, 255 - g], axis=-1) for g in imgs]
    pw, ph = gs.SCENE["pano_w"], gs.SCENE["pano_h"]
    post = dict(speckle_window_size=20, speckle_range=1, median=3)
    pano, idx, cov = sweep.rig_panorama(col, intr, T, pw, ph, near=gs.SCENE["near"], D=gs.SCENE["D"], weights=None, device=hip_device, post=post, mode="feather",
                                        paths=gs.SCENE["paths"])
    inv = sweep.inverse_distances(gs.SCENE["near"], D=gs.SCENE["D"])
    with sweep.Sweeper.from_rig(intr, T, (320, 270), pw, ph, inv, weights=None, device=hip_device, keep_tables=True, paths=gs.SCENE["paths"]) as s:
        raw = s.depth([sweep.bgr_to_gray(x) for x in col])
        mx, my = s.mapx, s.mapy
    from tscm_calib_amd import stereo
    assert np.array_equal(idx, stereo.filter(raw, min_disparity=0, device=hip_device, **post)) and not np.array_equal(idx, raw)
    host = CR.compose(col, None, mx, my, idx, mode=F_)
    assert pano.shape == (ph, pw, 3) and np.array_equal(pano, host["out"]) and np.array_equal(cov, host["coverage"])
