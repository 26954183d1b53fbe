"""Stereo matching and depth on a rectified pair (tscm.h: tscm_stereo_*): census + semi-global matching on the device,
the post-filter of a disparity map (speckle removal, masked median), hole filling from the nearest valid values along the
path directions, the edge-aware weighted median guided by the image, the 3-D points of a disparity map, and pair_depth,
the chain from two fisheye images of a calibrated rig to points:
rectify_pair_descs -> build_maps -> remap -> match [-> filter] [-> fill] [-> refine] -> points."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib
from . import maps as _maps

PARAM_NAMES = ("min_disparity", "num_disparities", "p1", "p2", "paths", "uniqueness_ratio", "disp12_max_diff")
STAGE_NAMES = ("census", "cost", "aggregate", "right_winner", "winner")
FILTER_PARAM_NAMES = ("min_disparity", "speckle_window_size", "speckle_range", "median")
FILL_PARAM_NAMES = ("min_disparity", "rule", "paths", "max_distance", "min_directions", "wrap_x")
REFINE_PARAM_NAMES = ("min_disparity", "radius", "iterations", "fill_invalid", "wrap_x")
FILL_RULES = dict(lowest=_lib.FILL_LOWEST, second_lowest=_lib.FILL_SECOND_LOWEST, median=_lib.FILL_MEDIAN)


def params(**over) -> _lib.CStereoParams:
    """tscm_stereo_default_params with the given fields replaced."""
    return _lib._params_struct(_lib.CStereoParams, "tscm_stereo_default_params", PARAM_NAMES, "stereo", over)


def _gray(img) -> np.ndarray:
    a = np.asarray(img)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("stereo images are 2-D uint8 arrays")
    if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a)
    return a


def _pair(left, right):
    left, right = _gray(left), _gray(right)
    if left.shape != right.shape:
        raise ValueError("left and right images differ in shape")
    if left.strides[0] != right.strides[0]:
        left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    return left, right


def match(left, right, device: int = 0, out: np.ndarray | None = None, with_seconds: bool = False, **over):
    """tscm_stereo_match -> int16 [h, w]: 16 * disparity, invalid pixels 16 * (min_disparity - 1).  Rows of `left` / `right`
    may be padded (a view of a wider array); `out` may be such a view too, and its padding keeps its values."""
    left, right = _pair(left, right)
    h, w = left.shape
    p = params(**over)
    out = _out_map(out, h, w, "images'")
    ub = C.POINTER(C.c_ubyte)
    sec = C.c_double(0.0)
    _lib.check(_lib.lib().tscm_stereo_match(left.ctypes.data_as(ub), right.ctypes.data_as(ub), w, h, left.strides[0] if h else w, C.byref(p), device,
                                            out.ctypes.data_as(C.POINTER(C.c_short)), out.strides[0] // 2 if h else w, C.byref(sec)))
    return (out, sec.value) if with_seconds else out


def stages(left, right, device: int = 0, **over) -> dict:
    """tscm_stereo_stages -> census_left / census_right uint64 [h, w], cost uint8 [h, w, D], aggregated uint16 [h, w, D]."""
    left, right = _pair(left, right)
    h, w = left.shape
    p = params(**over)
    D = max(int(p.num_disparities), 0)
    cl, cr = np.zeros((h, w), dtype=np.uint64), np.zeros((h, w), dtype=np.uint64)
    cost, agg = np.zeros((h, w, D), dtype=np.uint8), np.zeros((h, w, D), dtype=np.uint16)
    ub, ull = C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong)
    _lib.check(_lib.lib().tscm_stereo_stages(left.ctypes.data_as(ub), right.ctypes.data_as(ub), w, h, left.strides[0] if h else w, C.byref(p), device,
                                             cl.ctypes.data_as(ull), cr.ctypes.data_as(ull), cost.ctypes.data_as(ub), _lib.ushort_ptr(agg)))
    return dict(census_left=cl, census_right=cr, cost=cost, aggregated=agg)


def stage_times() -> dict:
    """Device seconds of this thread's last match / stages call by stage (tscm_stereo_stage_times)."""
    t = np.zeros(5)
    _lib.check(_lib.lib().tscm_stereo_stage_times(_lib.dptr(t)))
    return dict(zip(STAGE_NAMES, t.tolist()))


def filter_params(**over) -> _lib.CStereoFilterParams:
    """tscm_stereo_filter_default_params with the given fields replaced."""
    return _lib._params_struct(_lib.CStereoFilterParams, "tscm_stereo_filter_default_params", FILTER_PARAM_NAMES, "stereo filter", over)


def _disparity_map(disp) -> np.ndarray:
    disp = np.asarray(disp)
    if disp.ndim != 2 or disp.dtype != np.int16:
        raise ValueError("a disparity map is a 2-D int16 array")
    if disp.strides[1] != 2 or disp.strides[0] % 2 or disp.strides[0] < 2 * disp.shape[1]:
        disp = np.ascontiguousarray(disp)
    return disp


def _out_map(out, h: int, w: int, whose: str = "map's") -> np.ndarray:
    """the caller's `out`, checked, or a new int16 [h, w] map"""
    if out is None:
        return np.zeros((h, w), dtype=np.int16)
    if out.dtype != np.int16 or out.shape != (h, w) or (w and out.strides[1] != 2) or out.strides[0] % 2:
        raise ValueError(f"out must be an int16 array (or row-padded view) of the {whose} shape")
    return out


def filter(disp, device: int = 0, out: np.ndarray | None = None, with_seconds: bool = False, **over):
    """tscm_stereo_filter: speckle removal and masked median of a disparity map -> int16 [h, w].  `disp` may be a
    row-padded view; `out` may be one too (its padding keeps its values) and may be `disp` itself."""
    disp = _disparity_map(disp)
    h, w = disp.shape
    p = filter_params(**over)
    out = _out_map(out, h, w)
    sp = C.POINTER(C.c_short)
    sec = C.c_double(0.0)
    _lib.check(_lib.lib().tscm_stereo_filter(disp.ctypes.data_as(sp), w, h, disp.strides[0] // 2 if h else w, C.byref(p), device,
                                             out.ctypes.data_as(sp), out.strides[0] // 2 if h else w, C.byref(sec)))
    return (out, sec.value) if with_seconds else out


def filter_stages(disp, device: int = 0, **over) -> dict:
    """tscm_stereo_filter_stages -> label int32 [h, w] (the smallest linear index of the pixel's component, -1 invalid),
    size int32 [h, w] (its pixel count, 0 invalid), despeckled int16 [h, w] (the map before the median)."""
    disp = _disparity_map(disp)
    h, w = disp.shape
    p = filter_params(**over)
    label, size, desp = np.zeros((h, w), dtype=np.int32), np.zeros((h, w), dtype=np.int32), np.zeros((h, w), dtype=np.int16)
    ip, sp = C.POINTER(C.c_int), C.POINTER(C.c_short)
    _lib.check(_lib.lib().tscm_stereo_filter_stages(disp.ctypes.data_as(sp), w, h, disp.strides[0] // 2 if h else w, C.byref(p), device,
                                                    label.ctypes.data_as(ip), size.ctypes.data_as(ip), desp.ctypes.data_as(sp)))
    return dict(label=label, size=size, despeckled=desp)


def fill_params(**over) -> _lib.CStereoFillParams:
    """tscm_stereo_fill_default_params with the given fields replaced; rule also as "lowest" | "second_lowest" | "median"."""
    return _lib._params_struct(_lib.CStereoFillParams, "tscm_stereo_fill_default_params", FILL_PARAM_NAMES, "stereo fill", over, {"rule": ("fill rule", FILL_RULES)})


def fill(disp, device: int = 0, out: np.ndarray | None = None, with_mask: bool = False, with_seconds: bool = False, **over):
    """tscm_stereo_fill: every invalid pixel of a disparity (or sweep index) map gets the lowest, second-lowest or median of
    the nearest valid values along the path directions -> int16 [h, w]; with_mask adds uint8 [h, w]: 0 valid on input,
    1 filled, 2 left invalid.  `disp` may be a row-padded view; `out` may be one too (its padding keeps its values) and may
    be `disp` itself."""
    disp = _disparity_map(disp)
    h, w = disp.shape
    p = fill_params(**over)
    out = _out_map(out, h, w)
    mask = np.zeros((h, w), dtype=np.uint8) if with_mask else None
    sp = C.POINTER(C.c_short)
    sec = C.c_double(0.0)
    _lib.check(_lib.lib().tscm_stereo_fill(disp.ctypes.data_as(sp), w, h, disp.strides[0] // 2 if h else w, C.byref(p), device,
                                           out.ctypes.data_as(sp), out.strides[0] // 2 if h else w,
                                           None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(sec)))
    res = (out,) + ((mask,) if with_mask else ()) + ((sec.value,) if with_seconds else ())
    return res[0] if len(res) == 1 else res


_fill = fill                # pair_depth has a keyword of that name


def fill_stages(disp, device: int = 0, **over) -> dict:
    """tscm_stereo_fill_stages -> value, distance int16 [paths, h, w]: per direction the nearest valid value and the steps
    to it (the invalid value and 0 without one), for every pixel."""
    disp = _disparity_map(disp)
    h, w = disp.shape
    p = fill_params(**over)
    value, distance = np.zeros((max(int(p.paths), 0), h, w), dtype=np.int16), np.zeros((max(int(p.paths), 0), h, w), dtype=np.int16)
    sp = C.POINTER(C.c_short)
    _lib.check(_lib.lib().tscm_stereo_fill_stages(disp.ctypes.data_as(sp), w, h, disp.strides[0] // 2 if h else w, C.byref(p), device,
                                                  value.ctypes.data_as(sp), distance.ctypes.data_as(sp)))
    return dict(value=value, distance=distance)


def refine_params(**over) -> _lib.CStereoRefineParams:
    """tscm_stereo_refine_default_params with the given fields replaced."""
    return _lib._params_struct(_lib.CStereoRefineParams, "tscm_stereo_refine_default_params", REFINE_PARAM_NAMES, "stereo refine", over)


def range_weights(sigma: float) -> np.ndarray:
    """tscm_stereo_refine_weights -> uint8 [256]: floor(255 exp(-k / sigma) + 0.5); 255, 0, 0, ... for a sigma that is not > 0."""
    t = np.zeros(256, dtype=np.uint8)
    _lib.lib().tscm_stereo_refine_weights(float(sigma), t.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return t


def _refine_args(disp, guide, weights, sigma):
    """-> (disp, guide, table or None): the guide as one grey channel of the map's shape, the table from weights or sigma"""
    disp = _disparity_map(disp)
    g = np.asarray(guide)
    if g.ndim == 3:
        from .sweep import bgr_to_gray
        g = bgr_to_gray(g)
    g = _gray(g)
    if g.shape != disp.shape:
        raise ValueError("the guide does not have the map's shape")
    if weights is not None and sigma is not None:
        raise TypeError("weights and sigma: give one of them")
    table = None
    if sigma is not None:
        table = range_weights(sigma)
    elif weights is not None:
        table = np.ascontiguousarray(weights)
        if table.dtype != np.uint8 or table.shape != (256,):
            raise ValueError("weights is a uint8 table of 256 entries")
    return disp, g, table


def refine(disp, guide, device: int = 0, out: np.ndarray | None = None, weights=None, sigma=None, with_seconds: bool = False, **over):
    """tscm_stereo_refine: every pixel of a disparity (or sweep index) map takes the lower weighted median of the valid
    pixels of its (2 radius + 1)^2 window, a neighbour weighted by weights[|guide(p) - guide(q)|] -> int16 [h, w].  guide:
    uint8 [h, w], or BGR [h, w, 3], which goes through sweep.bgr_to_gray.  weights: a uint8 table of 256 entries; sigma:
    short for range_weights(sigma); neither: every weight 255.  `disp` and `guide` may be row-padded views; `out` may be one
    too (its padding keeps its values) and may be `disp` itself."""
    disp, g, table = _refine_args(disp, guide, weights, sigma)
    h, w = disp.shape
    p = refine_params(**over)
    out = _out_map(out, h, w)
    sp, ub = C.POINTER(C.c_short), C.POINTER(C.c_ubyte)
    sec = C.c_double(0.0)
    _lib.check(_lib.lib().tscm_stereo_refine(disp.ctypes.data_as(sp), w, h, disp.strides[0] // 2 if h else w, g.ctypes.data_as(ub), g.strides[0] if h else w,
                                             None if table is None else table.ctypes.data_as(ub), C.byref(p), device,
                                             out.ctypes.data_as(sp), out.strides[0] // 2 if h else w, C.byref(sec)))
    return (out, sec.value) if with_seconds else out


_refine = refine            # pair_depth has a keyword of that name


def refine_stages(disp, guide, device: int = 0, weights=None, sigma=None, **over) -> dict:
    """tscm_stereo_refine_stages -> weight_sum int32 [h, w] and count uint8 [h, w] (the summed weights and the number of the
    participants of every pixel's window) and first_pass int16 [h, w], the map after one pass."""
    disp, g, table = _refine_args(disp, guide, weights, sigma)
    h, w = disp.shape
    p = refine_params(**over)
    res = dict(weight_sum=np.zeros((h, w), dtype=np.int32), count=np.zeros((h, w), dtype=np.uint8), first_pass=np.zeros((h, w), dtype=np.int16))
    sp, ub = C.POINTER(C.c_short), C.POINTER(C.c_ubyte)
    _lib.check(_lib.lib().tscm_stereo_refine_stages(disp.ctypes.data_as(sp), w, h, disp.strides[0] // 2 if h else w, g.ctypes.data_as(ub), g.strides[0] if h else w,
                                                    None if table is None else table.ctypes.data_as(ub), C.byref(p), device,
                                                    res["weight_sum"].ctypes.data_as(C.POINTER(C.c_int)), res["count"].ctypes.data_as(ub),
                                                    res["first_pass"].ctypes.data_as(sp)))
    return res


def _post_fill_refine(disp, post, fill, refine, min_disparity: int, wrap_x, guide, device: int) -> np.ndarray:
    """filter -> fill -> refine of a disparity or index map, each for a dict of its arguments that is not None.  wrap_x: None,
    or what fill and refine take where their dict does not say; guide(map) yields the guide of refine."""
    wrap = {} if wrap_x is None else {"wrap_x": wrap_x}
    if post is not None:
        disp = filter(disp, device=device, min_disparity=min_disparity, **post)
    if fill is not None:
        disp = _fill(disp, device=device, min_disparity=min_disparity, **{**wrap, **fill})
    if refine is not None:
        disp = _refine(disp, guide(disp), device=device, min_disparity=min_disparity, **{**wrap, **refine})
    return disp


def points(disp, desc, baseline: float, min_disparity: int = 0, device: int = 0):
    """tscm_stereo_points: the disparity map of the left image of a PERSPECTIVE or LONGLAT pair (desc = its MapDesc) ->
    (points [h, w, 3] fp64 in the pair frame of the left camera, valid [h, w] bool); invalid points are NaN."""
    disp = np.asarray(disp)
    if disp.ndim != 2 or disp.dtype != np.int16:
        raise ValueError("a disparity map is a 2-D int16 array")
    if disp.strides[1] != 2 or disp.strides[0] % 2 or disp.strides[0] < 2 * disp.shape[1]:
        disp = np.ascontiguousarray(disp)
    h, w = disp.shape
    pts, valid = np.zeros((h, w, 3)), np.zeros((h, w), dtype=np.uint8)
    _lib.check(_lib.lib().tscm_stereo_points(disp.ctypes.data_as(C.POINTER(C.c_short)), w, h, disp.strides[0] // 2 if h else w, int(min_disparity),
                                             _maps._c_descs([desc]), _maps.projection_kind(desc.projection), float(baseline), device, _lib.dptr(pts),
                                             valid.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return pts, valid.astype(bool)


def pair_depth(img_a, img_b, intr_a, Twc_a, intr_b, Twc_b, projection="longlat", width: int = 640, height: int = 320, fov_x: float = np.pi,
               fov_y: float = np.pi / 2, device: int = 0, matcher=None, post=None, fill=None, refine=None, **over):
    """Two grey fisheye images of cameras a and b of a calibrated rig -> (points [height, width, 3] in the pair frame of
    camera a, valid [height, width], R_pair).  R_pair = rectify_pair_rotation(t_a, t_b) turns pair-frame vectors into the
    rig frame: P_rig = R_pair @ P + t_a.  Camera a is the left image: b lies at +|t_b - t_a| on the pair frame's x-axis.
    `matcher` replaces match (same signature without device; for comparisons with a reference matcher).  `post`: a dict
    of filter parameters (speckle_window_size, speckle_range, median); the disparity map then passes through filter, with
    the matcher's min_disparity, before its points are taken.  None: no filter.  `fill`: a dict of fill parameters (rule,
    paths, max_distance, min_directions, wrap_x), applied after `post`, also with the matcher's min_disparity.  None: no
    filling.  `refine`: a dict of refine arguments (radius, iterations, fill_invalid, wrap_x, sigma or weights), applied after
    `fill` with the rectified left image as the guide and the matcher's min_disparity.  None: no refinement."""
    if post is not None and "min_disparity" in post:
        raise TypeError("post: min_disparity is the matcher's")
    if fill is not None and "min_disparity" in fill:
        raise TypeError("fill: min_disparity is the matcher's")
    if refine is not None and "min_disparity" in refine:
        raise TypeError("refine: min_disparity is the matcher's")
    kind = _maps.projection_kind(projection)
    if kind not in (_lib.PROJ_PERSPECTIVE, _lib.PROJ_LONGLAT):
        raise ValueError("pair_depth needs rows that are epipolar lines: 'longlat' or 'perspective'")
    if kind == _lib.PROJ_PERSPECTIVE and fov_x >= np.pi:
        fov_x = np.pi / 2
    descs = _maps.rectify_pair_descs(intr_a, Twc_a, intr_b, Twc_b, kind, width, height, fov_x, fov_y)
    rect = []
    for img, d in zip((img_a, img_b), descs):
        mx, my, _ = _maps.build_maps([d], device=device)
        rect.append(_maps.remap(_gray(img), mx.reshape(height, width), my.reshape(height, width), device=device))
    disp = matcher(rect[0], rect[1], **over) if matcher is not None else match(rect[0], rect[1], device=device, **over)
    disp = _post_fill_refine(disp, post, fill, refine, int(over.get("min_disparity", 0)), None, lambda d: rect[0], device)
    Ta, Tb = np.asarray(Twc_a, dtype=np.float64).reshape(3, 4), np.asarray(Twc_b, dtype=np.float64).reshape(3, 4)
    baseline = float(np.linalg.norm(Tb[:, 3] - Ta[:, 3]))
    pts, valid = points(disp, descs[0], baseline, min_disparity=int(over.get("min_disparity", 0)), device=device)
    return pts, valid, _maps.rectify_pair_rotation(Ta[:, 3], Tb[:, 3])
