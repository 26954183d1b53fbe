"""GPU tests of the per-camera visibility at the swept depth (tscm_sweep_visibility, tscm_sweep_compose_visible and their
stages): use, state, the depth buffers, cells and the visible planes, and the output, coverage and stages of the composer under
visibility equal the host restatement tests/sweep_visibility_ref.py bit for bit (all of it is integer arithmetic); tolerance
255 and a constant map give the bytes of tscm_sweep_compose; and on the scene with an occluding ball of
tests/test_sweep_visibility_reference.py the device chain brings the frame nearer to the truth where it takes cameras away.
Tables, weights, images and index maps are those of tests/test_gpu_sweep.py and tests/test_gpu_sweep_compose.py, at their
shapes: 72 x 24, 64 x 32, 5 x 3 (the last quad holds 3 pixels), 2..4 and 8 cameras, D = 16 and 80; and 128 x 64 with 8 cameras
at L = 5, whose pyramid under the use planes ends in a 4 x 2 level, narrower than the 34 x 10 coarse halo of load_halo
(kPanoHaloW, kPanoHaloH of tscm_pano_kernels.h)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import sweep_compose_ref as CR
from tests import sweep_visibility_ref as V
from tests import test_gpu_sweep as gs
from tests import test_gpu_sweep_compose as gc
from tests import test_sweep_visibility_reference as ref_scene
from tscm_calib_amd import lib, sweep

pytestmark = pytest.mark.gpu

SRC_W, SRC_H = gs.SRC_W, gs.SRC_H
S_, F_, M_ = CR.SEAM, CR.FEATHER, CR.MULTIBAND
MODES = gc.MODES

# n, pw, ph, D, weight images, near_is_high
SHAPES = [
    (2, 72, 24, 16, False, 1),
    (3, 64, 32, 80, True, 1),
    (4, 72, 24, 80, False, 0),
    (8, 72, 24, 16, True, 1),
    (8, 64, 32, 16, True, 1),
    (4, 64, 32, 16, True, 0),
    (4, 5, 3, 16, True, 1),
    (3, 5, 3, 80, False, 0),
    (8, 128, 64, 16, True, 1),
]
LEVELS = {8: 5}               # shape index -> pyramid levels, where they do not rotate with the setting


def _settings(D):
    """cell_shift, tolerance, dilate"""
    return [(0, 0, 0), (0, D // 4, 0), (1, D // 2, 0), (0, D // 4, 1), (2, 3 * D // 4, 0)]


def _case(si, ti):
    """shape and setting, and the composer's options rotating through them: channels, mode, levels, wrap_x, gains, the
    fallback at D - 1.  5 x 3 has no pyramid level."""
    n, pw, ph, D, with_weights, high = SHAPES[si]
    shift, tol, dil = _settings(D)[ti]
    r = si + ti
    mode = (S_, F_, M_)[r % 3] if pw > 5 else (S_, F_)[r % 2]
    return dict(n=n, pw=pw, ph=ph, D=D, weights=with_weights, vp=dict(cell_shift=shift, tolerance=tol, dilate=dil, near_is_high=high), ch=(1, 3)[(r // 3) % 2],
                mode=mode, levels=LEVELS.get(si, 1 + ti % 3), wrap=bool(r % 2), gains=bool((r // 2) % 2), last=bool(si % 2))


CASES = [(si, ti) for si in range(8) for ti in range(5)] + [(8, 3)]           # (8, 3): MULTIBAND, 3 channels, wrap_x, gains, dilate 1
IDS = ["n%d-%dx%d-D%d-m%d-h%d-s%d-t%d-d%d" % (SHAPES[si] + _settings(SHAPES[si][3])[ti]) for si, ti in CASES]


def _weights(c):
    return list(gs._weights(c["n"])) if c["weights"] else None


def _compose_kw(c):
    return dict(mode=c["mode"], levels=c["levels"], wrap_x=int(c["wrap"]), fallback_index=c["D"] - 1 if c["last"] else 0)


@functools.lru_cache(maxsize=None)
def _vis_reference(si, ti):
    c = _case(si, ti)
    mx, my = gs._tables(c["n"], c["D"], c["pw"], c["ph"])
    return V.visibility(_weights(c), mx, my, gc._index_map(c["pw"], c["ph"], c["D"]), (SRC_W, SRC_H), **c["vp"])


@functools.lru_cache(maxsize=None)
def _compose_reference(si, ti):
    c = _case(si, ti)
    mx, my = gs._tables(c["n"], c["D"], c["pw"], c["ph"])
    return V.compose(list(gc._images(c["n"], c["ch"])), _weights(c), mx, my, gc._index_map(c["pw"], c["ph"], c["D"]), c["vp"], mode=c["mode"], levels=c["levels"],
                     wrap=c["wrap"], gains=gc._gains(c["n"], c["gains"]), fallback_index=c["D"] - 1 if c["last"] else 0)


def _sweeper(c, device):
    mx, my = gs._tables(c["n"], c["D"], c["pw"], c["ph"])
    return sweep.Sweeper.from_tables(mx, my, (SRC_W, SRC_H), weights=_weights(c), device=device)


# ------------------------------------------------------------------------------------------------ equality
@pytest.mark.parametrize("si,ti", CASES, ids=IDS)
def test_visibility_and_the_composer_under_it_equal_the_restatement(hip_device, si, ti):
    c = _case(si, ti)
    n, pw, ph, ch = c["n"], c["pw"], c["ph"], c["ch"]
    ref, cref = _vis_reference(si, ti), _compose_reference(si, ti)
    imgs, idx, g = gc._images(n, ch), gc._index_map(pw, ph, c["D"]), gc._gains(n, c["gains"])
    with _sweeper(c, hip_device) as s:
        st = s.visibility_stages(idx, **c["vp"])
        use, state = s.visibility(idx, with_state=True, **c["vp"])
        cst = s.compose_stages(imgs, idx, gains=g, visibility=c["vp"], **_compose_kw(c))
        out, cov = s.compose(imgs, idx, gains=g, with_coverage=True, visibility=c["vp"], **_compose_kw(c))
    for name in ("hypothesis", "depth_buffer", "cell", "visible", "use", "state"):
        assert st[name].dtype == ref[name].dtype and np.array_equal(st[name], ref[name]), name
    assert np.array_equal(use, ref["use"]) and np.array_equal(state, ref["state"])
    assert np.array_equal(cst["use"], ref["use"]) and np.array_equal(cst["state"], ref["state"])
    gc._check_stages(cst, cref, c["mode"])
    assert np.array_equal(out.reshape(ph, pw, ch), cref["out"])
    assert np.array_equal(cov, cref["coverage"])
    # a case proves nothing unless the states occur
    count = np.bincount(ref["state"].ravel(), minlength=5)
    seen = int((ref["cell"] >= 0).sum())
    print(f"states 0..4: {count.tolist()}, {seen - int(ref['visible'].sum())} of {seen} seen (pixel, camera) entries occluded")
    if pw >= 64:
        assert count[3] >= 10 and count[2] >= 3 and count[4] >= 3, count
        assert count[0] > 0 and count[1] > 0
        plain = CR.compose(list(imgs), _weights(c), *gs._tables(n, c["D"], pw, ph), idx, mode=S_, fallback_index=_compose_kw(c)["fallback_index"])
        assert not np.array_equal(cref["coverage"], plain["coverage"])


# ------------------------------------------------------------------------------------------------ against tscm_sweep_compose
@pytest.mark.parametrize("mode", [S_, F_, M_], ids=["seam", "feather", "multiband"])
def test_tolerance_255_and_a_constant_map_give_the_bytes_of_the_plain_composer(hip_device, mode):
    n, pw, ph, D, ch = 4, 72, 24, 16, (3, 1, 3)[mode]
    c = dict(n=n, pw=pw, ph=ph, D=D, weights=True)
    imgs, idx, g = gc._images(n, ch), gc._index_map(pw, ph, D), gc._gains(n, True)
    kw = dict(mode=mode, levels=2, wrap_x=1, fallback_index=3)
    with _sweeper(c, hip_device) as s:
        for index16, vp in ((idx, dict(cell_shift=0, tolerance=255, dilate=2)), (np.full((ph, pw), 16 * 5 + 5, np.int16), dict(cell_shift=3, tolerance=0, dilate=2))):
            want, wcov = s.compose(imgs, index16, gains=g, with_coverage=True, **kw)
            got, gcov = s.compose(imgs, index16, gains=g, with_coverage=True, visibility=vp, **kw)
            state = s.visibility(index16, with_state=True, **vp)[1]
            assert np.array_equal(got, want) and np.array_equal(gcov, wcov) and want.any()
            assert set(np.unique(state).tolist()) <= {0, 1, 2} and (state == 2).any()
        # the same frame under a test that bites differs: the equalities above are not vacuous
        bites = s.compose(imgs, idx, gains=g, visibility=dict(cell_shift=0, tolerance=0, dilate=2), **kw)
        assert not np.array_equal(bites, s.compose(imgs, idx, gains=g, **kw))


def test_two_calls_give_the_same_bytes(hip_device):
    """The atomic maximum does not depend on the order of its operands."""
    c = _case(4, 3)
    imgs, idx = gc._images(c["n"], 3), gc._index_map(c["pw"], c["ph"], c["D"])
    with _sweeper(c, hip_device) as s:
        a = s.visibility_stages(idx, **c["vp"])
        first = s.compose(imgs, idx, visibility=c["vp"], mode="feather")
        b = s.visibility_stages(idx, **c["vp"])
        second = s.compose(imgs, idx, visibility=c["vp"], mode="feather")
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(first, second) and (a["state"] == 3).sum() >= 10


# ------------------------------------------------------------------------------------------------ strides, handle paths
def test_the_map_left_on_the_device_and_a_handle_that_changes_mode_and_channels(hip_device):
    """depth -> compose -> compose under visibility -> compose -> another mode and channel count -> the first frame again,
    all with index16 = None: the plain composer is not disturbed by the pass, the pass not by the composer's buffers."""
    n, pw, ph, D = 3, 72, 24, 16
    mx, my = gs._tables(n, D, pw, ph)
    grey, col = gs._images(n, 0), gc._images(n, 3)
    vp = dict(cell_shift=0, tolerance=1, dilate=1)
    with sweep.Sweeper.from_tables(mx, my, (SRC_W, SRC_H), device=hip_device, paths=4) as s:
        idx = s.depth(grey)
        plain = s.compose(grey, mode="feather")
        vis = s.compose(grey, mode="feather", visibility=vp)
        use_dev = s.visibility(**vp)
        plain_again = s.compose(grey, mode="feather")
        other = s.compose(col, mode="multiband", levels=2, fallback_index=5, visibility=vp)
        other_host = s.compose(col, idx, mode="multiband", levels=2, fallback_index=5, visibility=vp)
        vis_again = s.compose(grey, mode="feather", visibility=vp)
    ref = V.compose(list(grey), None, mx, my, idx, vp, mode=F_)
    assert (idx < 0).any() and (ref["state"] == 3).sum() >= 10
    assert np.array_equal(plain, plain_again) and np.array_equal(plain[..., None], CR.compose(list(grey), None, mx, my, idx, mode=F_)["out"])
    assert np.array_equal(vis, vis_again) and np.array_equal(vis[..., None], ref["out"]) and not np.array_equal(vis, plain)
    assert np.array_equal(use_dev, ref["use"])
    assert np.array_equal(other, other_host)
    assert np.array_equal(other, V.compose(list(col), None, mx, my, idx, vp, mode=M_, levels=2, fallback_index=5)["out"])


def test_row_padding_of_images_index_map_and_output_at_once(hip_device):
    si, ti = 1, 0
    c = _case(si, ti)
    n, pw, ph, ch = c["n"], c["pw"], c["ph"], c["ch"]
    ref = _compose_reference(si, ti)
    views = []
    for img in gc._images(n, ch):
        buf = np.full((SRC_H, SRC_W + 5) + img.shape[2:], 77, np.uint8)
        buf[:, :SRC_W] = img
        views.append(buf[:, :SRC_W])
    wide_idx = np.full((ph, pw + 3), 16 * (c["D"] - 1), np.int16)         # padding that would occlude everything if it were read
    wide_idx[:, :pw] = gc._index_map(pw, ph, c["D"])
    canvas = np.full((ph, pw + 7) + ((ch,) if ch > 1 else ()), 201, np.uint8)
    with _sweeper(c, hip_device) as s:
        s.compose(views, wide_idx[:, :pw], gains=gc._gains(n, c["gains"]), out=canvas[:, :pw], visibility=c["vp"], **_compose_kw(c))
        use = s.visibility(wide_idx[:, :pw], **c["vp"])
    assert np.array_equal(canvas[:, :pw].reshape(ph, pw, ch), ref["out"])
    assert np.all(canvas[:, pw:] == 201)
    assert np.array_equal(use, ref["use"])


def test_refusals_that_need_a_handle(hip_device):
    """Every refusal of the four calls behind the NULL handle: TSCM_E_INVALID with a text that names the argument."""
    L = lib.lib()
    n, pw, ph, D = 2, 72, 24, 16
    mx, my = gs._tables(n, D, pw, ph)
    imgs = gc._images(n, 1)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in imgs])
    out, idx = np.zeros((ph, pw * 3), np.uint8), np.zeros((ph, pw), np.int16)
    use, state = np.zeros((n, ph, pw), np.uint8), np.zeros((ph, pw), np.uint8)
    ub = C.POINTER(C.c_ubyte)
    o, u, st, ix = out.ctypes.data_as(ub), use.ctypes.data_as(ub), state.ctypes.data_as(ub), idx.ctypes.data_as(C.POINTER(C.c_short))
    mk = lambda **kw: C.byref(sweep.compose_params(**dict(dict(mode="seam"), **kw)))
    mv = lambda **kw: C.byref(sweep.visibility_params(**kw))

    def refused(word, images=ptrs, stride=SRC_W, ch=1, index=ix, istride=pw, params=None, vparams=None, gains=None, dst=o, dstride=pw):
        rc = L.tscm_sweep_compose_visible(h, images, stride, ch, index, istride, params or mk(), vparams or mv(), gains, dst, dstride, None, None)
        assert rc == -1 and word in L.tscm_last_error(), (word, rc, L.tscm_last_error())

    def pass_refused(word, index=ix, istride=pw, vparams=None):
        for rc in (L.tscm_sweep_visibility(h, index, istride, vparams or mv(), u, st, None),
                   L.tscm_sweep_visibility_stages(h, index, istride, vparams or mv(), None, None, None, None, u, st)):
            assert rc == -1 and word in L.tscm_last_error(), (word, rc, L.tscm_last_error())

    with sweep.Sweeper.from_tables(mx, my, (SRC_W, SRC_H), device=hip_device) as s:
        h = s._handle
        bad = sweep.visibility_params()
        bad.struct_size += 4
        for check in (refused, pass_refused):
            check(b"index16 is NULL", index=None)                     # no frame yet
            check(b"index_stride", istride=pw - 1)
            assert L.tscm_last_error() == b"index_stride %d < pano_w %d" % (pw - 1, pw)           # shared sentences: the whole text
            check(b"struct_size", vparams=C.byref(bad))
            assert L.tscm_last_error() == b"vparams: struct_size %d is not sizeof(tscm_sweep_visibility_params) = %d" % (bad.struct_size, C.sizeof(lib.CSweepVisibilityParams))
            check(b"cell_shift", vparams=mv(cell_shift=-1))
            check(b"cell_shift", vparams=mv(cell_shift=9))
            check(b"tolerance", vparams=mv(tolerance=-1))
            check(b"tolerance", vparams=mv(tolerance=256))
            check(b"dilate", vparams=mv(dilate=-1))
            check(b"dilate", vparams=mv(dilate=3))
            check(b"near_is_high", vparams=mv(near_is_high=2))
            check(b"near_is_high", vparams=mv(near_is_high=-1))
        assert L.tscm_sweep_visibility(h, ix, pw, None, u, st, None) == -1 and b"vparams is NULL" in L.tscm_last_error()
        assert L.tscm_sweep_compose_visible(h, ptrs, SRC_W, 1, ix, pw, mk(), None, None, o, pw, None, None) == -1 and b"vparams is NULL" in L.tscm_last_error()
        # everything tscm_sweep_compose refuses
        refused(b"images is NULL", images=None)
        refused(b"images[1]", images=(C.c_void_p * n)(imgs[0].ctypes.data, None))
        refused(b"channels", ch=2)
        refused(b"stride", stride=SRC_W - 1)
        refused(b"stride", stride=3 * SRC_W - 1, ch=3)
        assert L.tscm_sweep_compose_visible(h, ptrs, SRC_W, 1, ix, pw, None, mv(), None, o, pw, None, None) == -1 and b"params is NULL" in L.tscm_last_error()
        wrong = sweep.compose_params(mode="seam")
        wrong.struct_size -= 4
        refused(b"struct_size", params=C.byref(wrong))
        refused(b"unknown mode", params=mk(mode=3))
        refused(b"levels", params=mk(mode="multiband", levels=0))
        refused(b"levels", params=mk(mode="multiband", levels=7))
        refused(b"pano_w", params=mk(mode="multiband", levels=4))      # 72 is no multiple of 16
        refused(b"fallback_index", params=mk(fallback_index=-1))
        refused(b"fallback_index", params=mk(fallback_index=D))
        refused(b"gain_q8[1]", gains=(C.c_ushort * n)(256, 0))
        refused(b"dst is NULL", dst=None)
        refused(b"dst_stride", dstride=pw - 1)
        refused(b"dst_stride", dstride=3 * pw - 1, ch=3, stride=3 * SRC_W)
        mask = np.zeros(8, np.uint8)
        rc = L.tscm_sweep_compose_visible_stages(h, ptrs, SRC_W, 1, ix, pw, mk(mode="feather"), mv(), None, None, None, None, None, mask.ctypes.data_as(ub), None, None, u, st)
        assert rc == -1 and b"mask_pyramid" in L.tscm_last_error() and b"MULTIBAND" in L.tscm_last_error()
        rc = L.tscm_sweep_compose_visible_stages(h, ptrs, SRC_W, 1, ix, pw, mk(), mv(dilate=3), None, None, None, None, None, None, None, None, u, st)
        assert rc == -1 and b"dilate" in L.tscm_last_error()
        # use and state may each be NULL
        assert L.tscm_sweep_visibility(h, ix, pw, mv(), None, None, None) == 0
    assert not out.any() and not use.any() and not state.any()


# ------------------------------------------------------------------------------------------------ end to end
def test_the_occluder_scene(hip_device):
    """Sweeper.from_rig on the scene with the ball, composed at the true index map with and without visibility: the device
    chain and the restatement on the device-built tables give equal bytes; over the pixels in state 3 the error against the
    truth with visibility stays within twice the CPU reference value (the allowance tests/test_gpu_sweep_compose.py grants its
    sphere figure for the unpinned sincos of the table kernel) and below the device's own error without visibility."""
    intr, T, imgs, truth, idx = ref_scene.ball_scene()
    pw, ph = gs.SCENE["pano_w"], gs.SCENE["pano_h"]
    inv = sweep.inverse_distances(gs.SCENE["near"], D=gs.SCENE["D"])
    vp = ref_scene.VISIBILITY
    got, plain = {}, {}
    with sweep.Sweeper.from_rig(intr, T, (320, 270), pw, ph, inv, weights=None, device=hip_device, keep_tables=True, paths=gs.SCENE["paths"]) as s:
        state = s.visibility(idx, with_state=True, **vp)[1]
        for mode in (S_, F_):
            got[mode] = s.compose(imgs, idx, mode=mode, visibility=vp)
            plain[mode] = s.compose(imgs, idx, mode=mode)
        mx, my = s.mapx, s.mapy
    # the device-built tables are an input to both sides, so the sincos of the table kernel does not enter
    for mode in (S_, F_):
        host = V.compose(imgs, None, mx, my, idx, vp, mode=mode)
        assert np.array_equal(got[mode][..., None], host["out"]), MODES[mode]
        assert np.array_equal(state, host["state"])
    assert (state == 3).sum() >= ref_scene.BALL_STATE3 // 2
    for k, mode in enumerate((S_, F_)):
        with_vis, without = ref_scene.state3_error(got[mode], truth, state), ref_scene.state3_error(plain[mode], truth, state)
        print(f"{MODES[mode]}: error over the {int((state == 3).sum())} pixels in state 3: {with_vis:.2f} with visibility, {without:.2f} without "
              f"(CPU reference {ref_scene.BALL_FIGURES['visible'][k]}, {ref_scene.BALL_FIGURES['plain'][k]})")
        assert with_vis <= 2.0 * ref_scene.BALL_FIGURES["visible"][k]
        assert with_vis < without


def test_rig_panorama_with_visibility(hip_device):
    """sweep.rig_panorama(..., visibility=...) composes at the map of its own depth pass under the pass."""
    intr, T, imgs, _, _ = ref_scene.ball_scene()
    pw, ph = gs.SCENE["pano_w"], gs.SCENE["pano_h"]
    vp = ref_scene.VISIBILITY
    pano, idx, cov = sweep.rig_panorama(imgs, intr, T, pw, ph, near=gs.SCENE["near"], D=gs.SCENE["D"], weights=None, device=hip_device, mode="feather",
                                        paths=gs.SCENE["paths"], visibility=vp)
    inv = sweep.inverse_distances(gs.SCENE["near"], D=gs.SCENE["D"])
    with sweep.Sweeper.from_rig(intr, T, (320, 270), pw, ph, inv, weights=None, device=hip_device, keep_tables=True, paths=gs.SCENE["paths"]) as s:
        mx, my = s.mapx, s.mapy
    host = V.compose(imgs, None, mx, my, idx, vp, mode=F_)
    assert np.array_equal(pano[..., None], host["out"]) and np.array_equal(cov, host["coverage"])
    assert (host["state"] == 3).sum() >= 10
