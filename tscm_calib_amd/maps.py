"""Remap tables: host-side mirror of TripleSphereCamera::undistort (TS.cpp:284-306), the table of
undistort_chessboard (TS.cpp:308-330) and Remap::init_remap (EpipolarRectify/rectify.cpp:86-199),
all built by tscm_build_maps on the device; output images that are not pinholes (long-lat, cylindrical,
stereographic, equirect: tscm_build_maps_ex), the tables of a sphere sweep (tscm_build_sweep_maps) and the point direction
tscm_rectify_points."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import lib as _lib


@dataclass
class MapDesc:
    intr: np.ndarray            # [9] camera that is sampled
    R: np.ndarray               # [3,3]
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    offset_x: float = 0.0
    offset_y: float = 0.0
    out_offset: int = 0
    out_stride: int = 0         # 0 -> width
    check_w2: int = 0
    w2: float = 0.42399         # rectify.cpp:7
    projection: int | str = 0   # tscm.h TSCM_PROJ_*, or "perspective", "longlat", "cylindrical", "stereographic", "equirect"

    def __post_init__(self):
        if self.out_stride == 0:
            self.out_stride = self.width
        self.projection = projection_kind(self.projection)


def projection_kind(projection) -> int:
    """TSCM_PROJ_* of a kind name; integers pass (the C ABI refuses the ones it does not know)."""
    if isinstance(projection, str):
        if projection not in _lib.PROJ_KINDS:
            raise ValueError(f"unknown projection {projection!r}: one of {', '.join(_lib.PROJ_KINDS)}")
        return _lib.PROJ_KINDS[projection]
    return int(projection)


def undistort_desc(intr, fx, fy, cx, cy, width, height, **kw) -> MapDesc:
    """TripleSphereCamera::undistort(fx, fy, cx, cy, img_size, mapx, mapy)."""
    return MapDesc(np.asarray(intr, dtype=np.float64), np.eye(3), fx, fy, cx, cy, width, height, **kw)


def chessboard_desc(intr, Rt, chessboard_cols, chessboard_rows, chessboard_size, **kw) -> MapDesc:
    """The table of undistort_chessboard(src, index, chessboard, chessboard_size): Rt = Rt_[index];
    output (cols+1)*size x (rows+1)*size, P = Rt * (j - size, i - size, 1)."""
    w, h = int((chessboard_cols + 1) * chessboard_size), int((chessboard_rows + 1) * chessboard_size)
    return MapDesc(np.asarray(intr, dtype=np.float64), np.asarray(Rt, dtype=np.float64).reshape(3, 3), 1.0, 1.0,
                   float(chessboard_size), float(chessboard_size), w, h, **kw)


def rectify_pair_rotation(t1, t2) -> np.ndarray:
    """Remap::calc_R (rectify.cpp:234-248)."""
    x = np.asarray(t2, dtype=np.float64) - np.asarray(t1, dtype=np.float64)
    n = np.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
    if n != 0:
        x = x / n
    z = np.array([-x[2], 0.0, x[0]])
    n = np.sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2])
    if n != 0:
        z = z / n
    y = np.array([-z[2] * x[1] + z[1] * x[2], z[2] * x[0] - z[0] * x[2], -z[1] * x[0] + z[0] * x[1]])
    n = np.sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2])
    if n != 0:
        y = y / n
    return np.stack([x, y, z], axis=1)


def rectify_descs(intr4, Twc4, size=400, mosaic_w=1280.0, mosaic_h=1080.0):
    """The eight tables of Remap::init_remap for cameras (front, right, rear, left) = cam0..3 of the
    calibration file.  Returns (descs, n_elems): elements [0, 4*size*size) are left_map (400 x 1600),
    [4*size*size, 8*size*size) right_map, each four size x size blocks stacked vertically."""
    intr4 = np.asarray(intr4, dtype=np.float64).reshape(4, 9)
    Twc4 = np.asarray(Twc4, dtype=np.float64).reshape(4, 3, 4)
    Rc, tc = Twc4[:, :, :3], Twc4[:, :, 3]
    origin = [(0.0, 0.0), (mosaic_w, 0.0), (0.0, mosaic_h), (mosaic_w, mosaic_h)]   # front, right, rear, left in the mosaic
    block = size * size
    descs = []
    for k in range(4):                       # pairs (front,right), (right,rear), (rear,left), (left,front)
        a, b = k, (k + 1) % 4
        Rp = rectify_pair_rotation(tc[a], tc[b])
        for cam, side in ((a, 0), (b, 1)):   # side 0 -> left_map, 1 -> right_map   (rectify.cpp:95-118)
            descs.append(MapDesc(intr4[cam], Rc[cam].T @ Rp, size / 2.0, size / 2.0, size / 2.0, size / 2.0, size, size,
                                 offset_x=origin[cam][0], offset_y=origin[cam][1],
                                 out_offset=side * 4 * block + k * block, check_w2=1))
    return descs, 8 * block


def _pinhole_of(kind: int, width: int, height: int, fov_x: float, fov_y: float):
    """fx, fy, cx, cy of an output image of `kind` that spans fov_x by fov_y radians about its centre."""
    def scale(n, fov, how):
        if how == "angle":
            return n / fov
        if how == "tan":
            if not fov < np.pi:
                raise ValueError("a tangent axis cannot span 180 degrees or more")
            return 0.5 * n / np.tan(0.5 * fov)
        return 0.5 * n / (2.0 * np.tan(0.25 * fov))               # stereographic: 2 tan(theta / 2)
    how = {_lib.PROJ_PERSPECTIVE: ("tan", "tan"), _lib.PROJ_LONGLAT: ("angle", "angle"), _lib.PROJ_CYLINDRICAL: ("angle", "tan"),
           _lib.PROJ_STEREOGRAPHIC: ("stereo", "stereo"), _lib.PROJ_EQUIRECT: ("angle", "angle")}
    if kind not in how:
        raise ValueError(f"unknown projection kind {kind}")
    return scale(width, fov_x, how[kind][0]), scale(height, fov_y, how[kind][1]), width / 2.0, height / 2.0


def rectify_pair_descs(intr_a, Twc_a, intr_b, Twc_b, projection="longlat", width: int = 640, height: int = 320,
                       fov_x: float = np.pi, fov_y: float = np.pi / 2):
    """Two tables that rectify the camera pair (a, b): R = R_cam^T * rectify_pair_rotation(t_a, t_b), the x-axis of both
    output images along the baseline.  With "longlat" (and "perspective") a scene point lies on the same row of both; the
    long-lat image keeps that over the whole hemisphere (fov_x up to pi), where a pinhole cannot go."""
    kind = projection_kind(projection)
    fx, fy, cx, cy = _pinhole_of(kind, width, height, fov_x, fov_y)
    Ta, Tb = np.asarray(Twc_a, dtype=np.float64).reshape(3, 4), np.asarray(Twc_b, dtype=np.float64).reshape(3, 4)
    Rp = rectify_pair_rotation(Ta[:, 3], Tb[:, 3])
    return [MapDesc(np.asarray(intr, dtype=np.float64), T[:, :3].T @ Rp, fx, fy, cx, cy, width, height, check_w2=1, projection=kind)
            for intr, T in ((intr_a, Ta), (intr_b, Tb))]


def panorama_descs(intr, Twc, width: int, height: int, projection="equirect"):
    """One table per camera of the rig over the full 360 x 180 degrees in the rig frame (R = R_cam^T, check_w2 = 1):
    element (i, j) of every table looks along the same rig-frame ray.  "equirect", or "cylindrical" (rows at unit height
    per fx pixels).  No blending: the caller composes the tables' images."""
    kind = projection_kind(projection)
    if kind not in (_lib.PROJ_EQUIRECT, _lib.PROJ_CYLINDRICAL):
        raise ValueError("a panorama is equirect or cylindrical")
    fx = width / (2.0 * np.pi)
    fy = height / np.pi if kind == _lib.PROJ_EQUIRECT else fx
    intr = np.asarray(intr, dtype=np.float64).reshape(-1, 9)
    Twc = np.asarray(Twc, dtype=np.float64).reshape(-1, 3, 4)
    return [MapDesc(intr[k], Twc[k, :, :3].T.copy(), fx, fy, width / 2.0, height / 2.0, width, height, check_w2=1, projection=kind)
            for k in range(intr.shape[0])]


def _c_descs(descs):
    arr = (_lib.CMapDesc * len(descs))()
    for m, d in zip(arr, descs):
        m.intr[:] = list(np.asarray(d.intr, dtype=np.float64).ravel())
        m.R[:] = list(np.asarray(d.R, dtype=np.float64).ravel())
        for k in ("fx", "fy", "cx", "cy", "offset_x", "offset_y", "width", "height", "out_stride", "check_w2", "out_offset", "w2"):
            setattr(m, k, getattr(d, k))
    return arr


def build_maps(descs, n_elems: int | None = None, device: int = 0, exact: bool = True):
    """tscm_build_maps -> mapx, mapy (float32, flat), seconds_kernel"""
    if n_elems is None:
        n_elems = max((d.out_offset + (d.height - 1) * d.out_stride + d.width for d in descs if d.width and d.height), default=0)
    mapx, mapy = np.zeros(n_elems, dtype=np.float32), np.zeros(n_elems, dtype=np.float32)
    fp = C.POINTER(C.c_float)
    sec = C.c_double(0.0)
    arr = _c_descs(descs)
    kinds = [projection_kind(d.projection) for d in descs]
    if any(kinds):                       # some output image is not a pinhole
        _lib.check(_lib.lib().tscm_build_maps_ex(arr, (C.c_int * len(kinds))(*kinds), len(descs), device, 1 if exact else 0,
                                                  mapx.ctypes.data_as(fp), mapy.ctypes.data_as(fp), n_elems,
                                                  C.cast(C.byref(sec), C.POINTER(C.c_double))))
        return mapx, mapy, sec.value
    _lib.check(_lib.lib().tscm_build_maps(arr, len(descs), device, 1 if exact else 0, mapx.ctypes.data_as(fp),
                                           mapy.ctypes.data_as(fp), n_elems, C.cast(C.byref(sec), C.POINTER(C.c_double))))
    return mapx, mapy, sec.value


def build_sweep_maps(descs, centers, inv_distance, device: int = 0, exact: bool = True):
    """tscm_build_sweep_maps -> mapx, mapy (float32 [n, D, height, width]), seconds_kernel.  descs: one table per camera on
    one output grid (panorama_descs); centers [n, 3]: the camera centres in the output frame (Twc[:, :, 3]); inv_distance
    [D]: non-negative and strictly increasing, 0 = infinity."""
    centers = np.ascontiguousarray(centers, dtype=np.float64).reshape(-1, 3)
    inv = np.ascontiguousarray(inv_distance, dtype=np.float64).ravel()
    n, D = len(descs), inv.size
    if centers.shape[0] != n:
        raise ValueError(f"{n} tables need {n} centres")
    h, w = (descs[0].height, descs[0].width) if n else (0, 0)
    mapx, mapy = np.zeros((n, D, h, w), dtype=np.float32), np.zeros((n, D, h, w), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    sec = C.c_double(0.0)
    kinds = [projection_kind(d.projection) for d in descs]
    _lib.check(_lib.lib().tscm_build_sweep_maps(_c_descs(descs), (C.c_int * max(n, 1))(*kinds), n, _lib.dptr(centers), _lib.dptr(inv), D, device,
                                                 1 if exact else 0, mapx.ctypes.data_as(fp), mapy.ctypes.data_as(fp), mapx.size, C.byref(sec)))
    return mapx, mapy, sec.value


def rectify_points(desc: MapDesc, pixels, device: int = 0):
    """tscm_rectify_points: pixels [n, 2] of the sampled camera -> (xy [n, 2] in the output image of `desc`, valid [n] bool).
    desc.offset_x / offset_y do not enter (they belong to the sampled image); invalid points are NaN."""
    px = np.ascontiguousarray(pixels, dtype=np.float64).reshape(-1, 2)
    out, valid = np.zeros_like(px), np.zeros(px.shape[0], dtype=np.uint8)
    _lib.check(_lib.lib().tscm_rectify_points(_c_descs([desc]), projection_kind(desc.projection), _lib.dptr(px), px.shape[0], device,
                                               _lib.dptr(out), valid.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return out, valid.astype(bool)


def remap(src, mapx, mapy, to_gray: bool = False, device: int = 0) -> np.ndarray:
    """cv::remap(src, dst, mapx, mapy, INTER_LINEAR) on the GPU (TS.cpp:304, :329) for uint8 images (H, W) or
    (H, W, 3) and float32 tables of the output size; to_gray: BGR2GRAY of the result (findCorner.cpp:9-10)."""
    import ctypes as C
    from . import lib as _l
    src = np.ascontiguousarray(src, dtype=np.uint8)
    ch = 1 if src.ndim == 2 else src.shape[2]
    mapx, mapy = np.ascontiguousarray(mapx, dtype=np.float32), np.ascontiguousarray(mapy, dtype=np.float32)
    if mapx.shape != mapy.shape or mapx.ndim != 2:
        raise ValueError("mapx and mapy must be 2-D tables of the same shape")
    mh, mw = mapx.shape
    out_ch = 1 if (to_gray or ch == 1) else ch
    dst = np.zeros((mh, mw) if out_ch == 1 else (mh, mw, out_ch), dtype=np.uint8)
    f = _l.lib().tscm_remap
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    _l.check(f(src.ctypes.data, src.shape[1], src.shape[0], src.strides[0], ch, mapx.ctypes.data, mapy.ctypes.data, mw, mh, mw, int(bool(to_gray)), int(device),
               dst.ctypes.data, dst.strides[0] if mh else mw * out_ch))
    return dst
