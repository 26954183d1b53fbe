"""The full text of tscm_last_error() for the refusals that several entry points word alike: a wrong struct_size of every
perception params struct, and each sentence of the block that the map stages (filter, fill, refine) share.  The other
refusal tests look for one word of the message; these compare all of it, so a sentence cannot change unnoticed.  Every
check here runs before a device is selected, so no GPU is needed."""
import ctypes as C

import numpy as np
import pytest

from tscm_calib_amd import lib

W, H = 24, 10
SP, UB = C.POINTER(C.c_short), C.POINTER(C.c_ubyte)


def _defaults(struct, fn):
    p = struct()
    getattr(lib.lib(), fn)(C.byref(p))
    return p


# ------------------------------------------------------------------------------------------------ the map stages
MAP_STAGES = {
    "filter": (lib.CStereoFilterParams, "tscm_stereo_filter_default_params", "tscm_stereo_filter_params"),
    "fill": (lib.CStereoFillParams, "tscm_stereo_fill_default_params", "tscm_stereo_fill_params"),
    "refine": (lib.CStereoRefineParams, "tscm_stereo_refine_default_params", "tscm_stereo_refine_params"),
}


def _call_map_stage(stage, disp=True, w=W, h=H, disp_stride=W, params=True, out=True, out_stride=W, guide=True, guide_stride=W, **fields):
    L = lib.lib()
    struct, fn, _ = MAP_STAGES[stage]
    d, o, g = np.zeros((H, W), np.int16), np.zeros((H, W), np.int16), np.zeros((H, W), np.uint8)
    p = _defaults(struct, fn)
    for k, v in fields.items():
        setattr(p, k, v)
    dp, op, pp = d.ctypes.data_as(SP) if disp else None, o.ctypes.data_as(SP) if out else None, C.byref(p) if params else None
    if stage == "filter":
        rc = L.tscm_stereo_filter(dp, w, h, disp_stride, pp, 0, op, out_stride, None)
    elif stage == "fill":
        rc = L.tscm_stereo_fill(dp, w, h, disp_stride, pp, 0, op, out_stride, None, None)
    else:
        rc = L.tscm_stereo_refine(dp, w, h, disp_stride, g.ctypes.data_as(UB) if guide else None, guide_stride, None, pp, 0, op, out_stride, None)
    return rc, L.tscm_last_error().decode()


SHARED_BLOCK = [
    (dict(disp=False), "disparity is NULL"),
    (dict(params=False), "params is NULL"),
    (dict(w=-1), "negative width or height"),
    (dict(h=-1), "negative width or height"),
    (dict(disp_stride=23), "disp_stride 23 < width 24"),
    (dict(min_disparity=-2048), "params: min_disparity -2048 outside -2047..2031, what the matcher accepts"),
    (dict(min_disparity=2032), "params: min_disparity 2032 outside -2047..2031, what the matcher accepts"),
    (dict(out=False), "out is NULL"),
    (dict(out_stride=23), "out_stride 23 < width 24"),
]


@pytest.mark.parametrize("stage", sorted(MAP_STAGES))
@pytest.mark.parametrize("args,text", SHARED_BLOCK, ids=[t.split(":")[-1].strip().replace(" ", "_")[:28] for _, t in SHARED_BLOCK])
def test_map_stages_word_their_shared_refusals_alike(stage, args, text):
    assert _call_map_stage(stage, **args) == (-1, text)


@pytest.mark.parametrize("stage", sorted(MAP_STAGES))
@pytest.mark.parametrize("delta", [-4, 4])
def test_map_stage_struct_size(stage, delta):
    struct, _, name = MAP_STAGES[stage]
    size = C.sizeof(struct)
    assert _call_map_stage(stage, struct_size=size + delta) == (-1, f"params: struct_size {size + delta} is not sizeof({name}) = {size}")


# with two faults in one call the first check in the stage's own order answers: the shared block is interleaved with the
# guide's checks in refine, and min_disparity comes behind the stage's own fields
TWO_FAULTS = [
    ("refine", dict(disp=False, guide=False), "disparity is NULL"),
    ("refine", dict(guide=False, params=False), "guide is NULL"),
    ("refine", dict(guide=False, w=-1), "guide is NULL"),
    ("refine", dict(disp_stride=23, guide_stride=23), "disp_stride 23 < width 24"),
    ("refine", dict(guide_stride=23, struct_size=4), "guide_stride 23 < width 24"),
    ("refine", dict(guide_stride=23, radius=0), "guide_stride 23 < width 24"),
    ("refine", dict(radius=0, min_disparity=2032), "params: radius 0 outside 1..7"),
    ("filter", dict(median=4, min_disparity=-2048), "params: median 4 is not 0, 3 or 5"),
    ("fill", dict(wrap_x=2, min_disparity=2032), "params: wrap_x 2 is not 0 or 1"),
    ("fill", dict(min_disparity=2032, out=False), "params: min_disparity 2032 outside -2047..2031, what the matcher accepts"),
]


@pytest.mark.parametrize("stage,args,text", TWO_FAULTS, ids=["%s-%s" % (s, "+".join(a)) for s, a, _ in TWO_FAULTS])
def test_the_order_of_the_checks(stage, args, text):
    assert _call_map_stage(stage, **args) == (-1, text)


# ------------------------------------------------------------------------------------------------ struct_size elsewhere
def _match(p):
    L = lib.lib()
    a, d = np.zeros((H, W), np.uint8), np.zeros((H, W), np.int16)
    return L.tscm_stereo_match(a.ctypes.data_as(UB), a.ctypes.data_as(UB), W, H, W, C.byref(p), 0, d.ctypes.data_as(SP), W, None)


def _sweep_create(p):
    tab = np.zeros(2 * 16 * 32 * 16, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    hdl = C.c_void_p()
    rc = lib.lib().tscm_sweep_create(2, 16, 12, None, tab, tab, 32, 16, C.byref(p), 0, C.byref(hdl))
    assert hdl.value is None
    return rc


def _panorama_create(p):
    tab = np.zeros(2 * 32 * 16, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    hdl = C.c_void_p()
    rc = lib.lib().tscm_panorama_create(2, 16, 12, 1, None, tab, tab, 32, 16, C.byref(p), 0, C.byref(hdl))
    assert hdl.value is None
    return rc


CREATORS = [
    (lib.CStereoParams, "tscm_stereo_default_params", "tscm_stereo_params", _match),
    (lib.CSweepParams, "tscm_sweep_default_params", "tscm_sweep_params", _sweep_create),
    (lib.CPanoramaParams, "tscm_panorama_default_params", "tscm_panorama_params", _panorama_create),
]


@pytest.mark.parametrize("struct,fn,name,call", CREATORS, ids=[c[2] for c in CREATORS])
@pytest.mark.parametrize("delta", [-4, 4])
def test_struct_size_of_the_matcher_and_the_handles(struct, fn, name, call, delta):
    p = _defaults(struct, fn)
    size = C.sizeof(struct)
    assert p.struct_size == size
    p.struct_size = size + delta
    assert call(p) == -1
    assert lib.lib().tscm_last_error().decode() == f"params: struct_size {size + delta} is not sizeof({name}) = {size}"
