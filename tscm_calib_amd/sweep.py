"""Sphere-sweep depth of a calibrated rig (tscm.h: tscm_sweep_*): Sweeper keeps the n x D packed sweep tables on the device
and gives one index map per frame -- 16 x the winning inverse-distance hypothesis of every panorama pixel -- and its 3-D
points in the rig frame; rig_depth does it in one call.  Sweeper.compose blends the frame at the swept depth -- the panorama
without the parallax of a composition at infinity -- and rig_panorama runs depth, the optional filter and compose in one call."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib
from . import maps as _maps

INVALID = -16


def _fields(struct) -> tuple:
    return tuple(k for k, _ in struct._fields_ if k != "struct_size")


def params(**over) -> _lib.CSweepParams:
    """tscm_sweep_default_params with fields replaced: num_hypotheses, p1, p2, paths, uniqueness_ratio, wrap_x."""
    return _lib._params_struct(_lib.CSweepParams, "tscm_sweep_default_params", _fields(_lib.CSweepParams), None, over)


def compose_params(**over) -> _lib.CSweepComposeParams:
    """tscm_sweep_compose_default_params with fields replaced: mode ("seam", "feather", "multiband" or TSCM_PANO_*), levels,
    wrap_x, fallback_index."""
    return _lib._params_struct(_lib.CSweepComposeParams, "tscm_sweep_compose_default_params", _fields(_lib.CSweepComposeParams), None, over,
                              {"mode": ("mode", _lib.PANO_MODES)})


def visibility_params(**over) -> _lib.CSweepVisibilityParams:
    """tscm_sweep_visibility_default_params with fields replaced: cell_shift, tolerance, dilate, near_is_high."""
    return _lib._params_struct(_lib.CSweepVisibilityParams, "tscm_sweep_visibility_default_params", _fields(_lib.CSweepVisibilityParams), None, over)


def _visibility_struct(visibility) -> _lib.CSweepVisibilityParams:
    return visibility if isinstance(visibility, _lib.CSweepVisibilityParams) else visibility_params(**visibility)


def bgr_to_gray(img) -> np.ndarray:
    """The composer's BGR2GRAY integers (tscm.h, overlap): (b 1868 + g 9617 + r 4899 + 2^13) >> 14; a grey image is returned
    as it is."""
    a = np.asarray(img)
    if a.ndim == 2:
        return a
    v = a.astype(np.int64)
    return ((v[..., 0] * 1868 + v[..., 1] * 9617 + v[..., 2] * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def inverse_distances(near: float, far: float = np.inf, D: int = 64) -> np.ndarray:
    """D hypotheses uniform in inverse distance, index 0 = far (inverse distance 0 for far = inf), index D - 1 = near."""
    if not (near > 0 and far > near):
        raise ValueError("0 < near < far")
    return np.linspace(0.0 if np.isinf(far) else 1.0 / far, 1.0 / near, int(D))


class Sweeper:
    """Context manager around a tscm_sweep handle: Sweeper.from_rig(intr, Twc, size, pano_w, pano_h, inv_distance, ...)
    builds the tables through maps.panorama_descs / maps.build_sweep_maps, Sweeper.from_tables(mapx, mapy, size, ...) takes
    tables [n, D, pano_h, pano_w] of the caller's.  size = (width, height) of the grey source images.  weights: None (all
    255), "radial" (from_rig: panorama.radial_weights per camera) or n arrays [height, width] uint8 (entries may be None)."""

    def __init__(self):
        raise TypeError("use Sweeper.from_rig or Sweeper.from_tables")

    @classmethod
    def from_tables(cls, mapx, mapy, size, weights=None, device: int = 0, pano_desc=None, inv_distance=None, **over):
        self = cls.__new__(cls)
        self._handle = None
        mapx, mapy = np.ascontiguousarray(mapx, dtype=np.float32), np.ascontiguousarray(mapy, dtype=np.float32)
        if mapx.ndim != 4 or mapx.shape != mapy.shape:
            raise ValueError("mapx and mapy are [n, D, pano_h, pano_w] tables of the same shape")
        self.n, self.D, self.pano_h, self.pano_w = mapx.shape
        self.width, self.height, self.device = int(size[0]), int(size[1]), int(device)
        self.params = params(num_hypotheses=self.D, **over)
        self.pano_desc = pano_desc
        self.inv_distance = None if inv_distance is None else np.ascontiguousarray(inv_distance, dtype=np.float64).ravel()
        if self.inv_distance is not None and self.inv_distance.size != self.D:
            raise ValueError(f"{self.D} tables per camera need {self.D} inverse distances")
        wptr = None
        self.weights = None
        if weights is not None:
            if len(weights) != self.n:
                raise ValueError(f"{self.n} cameras need {self.n} weight entries")
            self.weights = [None if x is None else np.ascontiguousarray(x, dtype=np.uint8) for x in weights]
            for x in self.weights:
                if x is not None and x.shape != (self.height, self.width):
                    raise ValueError("a weight image has the shape [height, width] of the source images")
            wptr = (C.c_void_p * self.n)(*[None if x is None else x.ctypes.data for x in self.weights])
        fp = C.POINTER(C.c_float)
        hdl = C.c_void_p()
        _lib.check(_lib.lib().tscm_sweep_create(self.n, self.width, self.height, wptr, mapx.ctypes.data_as(fp), mapy.ctypes.data_as(fp), self.pano_w, self.pano_h,
                                                C.byref(self.params), self.device, C.byref(hdl)))
        self._handle = hdl
        return self

    @classmethod
    def from_rig(cls, intr, Twc, size, pano_w: int, pano_h: int, inv_distance, weights=None, projection="equirect", device: int = 0, exact: bool = True,
                 max_theta: float = np.radians(100.0), keep_tables: bool = False, **over):
        intr = np.asarray(intr, dtype=np.float64).reshape(-1, 9)
        Twc = np.asarray(Twc, dtype=np.float64).reshape(-1, 3, 4)
        descs = _maps.panorama_descs(intr, Twc, int(pano_w), int(pano_h), projection)
        mapx, mapy, _ = _maps.build_sweep_maps(descs, Twc[:, :, 3], inv_distance, device=device, exact=exact)
        if isinstance(weights, str):
            if weights != "radial":
                raise ValueError("weights: 'radial', None or one array per camera")
            from . import panorama
            weights = [panorama.radial_weights(intr[k], int(size[0]), int(size[1]), max_theta, device=device) for k in range(len(descs))]
        over.setdefault("wrap_x", 1)
        self = cls.from_tables(mapx, mapy, size, weights=weights, device=device, pano_desc=descs[0], inv_distance=inv_distance, **over)
        if keep_tables:
            self.mapx, self.mapy = mapx, mapy
        return self

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if self._handle is not None:
            _lib.lib().tscm_sweep_destroy(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ frames
    def _frame(self, images):
        if self._handle is None:
            raise ValueError("the sweeper is closed")
        if len(images) != self.n:
            raise ValueError(f"{self.n} cameras need {self.n} images")
        imgs = []
        for x in images:
            a = np.asarray(x)
            if a.dtype != np.uint8 or a.shape != (self.height, self.width):
                raise ValueError(f"images are uint8 arrays of shape {(self.height, self.width)}")
            imgs.append(a if a.strides[1] == 1 and a.strides[0] >= self.width else np.ascontiguousarray(a))
        if len({a.strides[0] for a in imgs}) > 1:
            imgs = [np.ascontiguousarray(a) for a in imgs]
        return imgs, (C.c_void_p * self.n)(*[a.ctypes.data for a in imgs]), int(imgs[0].strides[0])

    def depth(self, images, out: np.ndarray | None = None, with_seconds: bool = False):
        """tscm_sweep_depth -> int16 [pano_h, pano_w]: 16 x the hypothesis index with its sub-index term, INVALID = -16.
        `out` may be a row-padded view, whose padding keeps its values."""
        imgs, ptrs, stride = self._frame(images)
        if out is None:
            out = np.zeros((self.pano_h, self.pano_w), dtype=np.int16)
        if out.dtype != np.int16 or out.shape != (self.pano_h, self.pano_w) or out.strides[1] != 2 or out.strides[0] % 2:
            raise ValueError("out must be an int16 array (or row-padded view) of the panorama's shape")
        sec = C.c_double(0.0)
        _lib.check(_lib.lib().tscm_sweep_depth(self._handle, ptrs, stride, out.ctypes.data_as(C.POINTER(C.c_short)), int(out.strides[0] // 2), C.byref(sec)))
        return (out, sec.value) if with_seconds else out

    def stages(self, images) -> dict:
        """tscm_sweep_stages -> sampled, alpha [n, D, ph, pw] uint8, census alike uint64, cost [ph, pw, D] uint8, aggregated
        alike uint16."""
        imgs, ptrs, stride = self._frame(images)
        n, D, ph, pw = self.n, self.D, self.pano_h, self.pano_w
        res = dict(sampled=np.zeros((n, D, ph, pw), np.uint8), alpha=np.zeros((n, D, ph, pw), np.uint8), census=np.zeros((n, D, ph, pw), np.uint64),
                   cost=np.zeros((ph, pw, D), np.uint8), aggregated=np.zeros((ph, pw, D), np.uint16))
        ub = C.POINTER(C.c_ubyte)
        _lib.check(_lib.lib().tscm_sweep_stages(self._handle, ptrs, stride, res["sampled"].ctypes.data_as(ub), res["alpha"].ctypes.data_as(ub),
                                                res["census"].ctypes.data_as(C.POINTER(C.c_ulonglong)), res["cost"].ctypes.data_as(ub),
                                                res["aggregated"].ctypes.data_as(C.POINTER(C.c_ushort))))
        return res

    def _colour_frame(self, images):
        """n images [height, width] or [height, width, 3] uint8, all alike -> (arrays, pointers, stride, channels)"""
        if self._handle is None:
            raise ValueError("the sweeper is closed")
        if len(images) != self.n:
            raise ValueError(f"{self.n} cameras need {self.n} images")
        first = np.asarray(images[0])
        ch = 1 if first.ndim == 2 else 3
        shape = (self.height, self.width) if ch == 1 else (self.height, self.width, 3)
        imgs = []
        for x in images:
            a = np.asarray(x)
            if a.dtype != np.uint8 or a.shape != shape:
                raise ValueError(f"images are uint8 arrays of shape {shape}")
            inner = a.strides[1:] == ((3, 1) if ch == 3 else (1,))
            imgs.append(a if inner and a.strides[0] >= self.width * ch else np.ascontiguousarray(a))
        if len({a.strides[0] for a in imgs}) > 1:
            imgs = [np.ascontiguousarray(a) for a in imgs]
        return imgs, (C.c_void_p * self.n)(*[a.ctypes.data for a in imgs]), int(imgs[0].strides[0]), ch

    def _compose_args(self, index16, gains, over):
        p = over if isinstance(over, _lib.CSweepComposeParams) else compose_params(**over)
        idx, iptr, istride = None, None, 0
        if index16 is not None:
            idx = np.asarray(index16)
            if idx.dtype != np.int16 or idx.shape != (self.pano_h, self.pano_w) or idx.strides[1] != 2 or idx.strides[0] % 2:
                raise ValueError("index16 is an int16 array (or row-padded view) of the panorama's shape")
            iptr, istride = idx.ctypes.data_as(C.POINTER(C.c_short)), int(idx.strides[0] // 2)
        g, gptr = None, None
        if gains is not None:
            g = np.ascontiguousarray(gains, dtype=np.uint16)
            if g.shape != (self.n,):
                raise ValueError(f"gains: {self.n} Q8 values")
            gptr = _lib.ushort_ptr(g)
        return p, (idx, iptr, istride), (g, gptr)

    def compose(self, images, index16=None, gains=None, out: np.ndarray | None = None, with_coverage: bool = False, with_seconds: bool = False, visibility=None,
                **params):
        """tscm_sweep_compose -> uint8 [pano_h, pano_w] or [pano_h, pano_w, 3]: the frame blended at the hypothesis that
        index16 names per pixel (None: the map of this sweeper's last depth(), still on the device).  images: grey or
        3-channel, they need not be those of the depth pass.  params: the fields of compose_params.  `out` may be a
        row-padded view, whose padding keeps its values.  visibility: None, or the fields of visibility_params as a dict (or
        the struct): tscm_sweep_compose_visible, which leaves out the cameras that do not see a pixel's point."""
        imgs, ptrs, stride, ch = self._colour_frame(images)
        p, (idx, iptr, istride), (g, gptr) = self._compose_args(index16, gains, params)
        shape = (self.pano_h, self.pano_w) if ch == 1 else (self.pano_h, self.pano_w, ch)
        if out is None:
            out = np.zeros(shape, dtype=np.uint8)
        inner = out.strides[1:] == ((ch, 1) if ch > 1 else (1,))
        if out.dtype != np.uint8 or out.shape != shape or not inner:
            raise ValueError("out must be a uint8 array (or row-padded view) of the panorama's shape")
        cov = np.zeros((self.pano_h, self.pano_w), dtype=np.uint8) if with_coverage else None
        ub = C.POINTER(C.c_ubyte)
        sec = C.c_double(0.0)
        tail = (gptr, out.ctypes.data_as(ub), int(out.strides[0]), None if cov is None else cov.ctypes.data_as(ub), C.byref(sec))
        if visibility is None:
            _lib.check(_lib.lib().tscm_sweep_compose(self._handle, ptrs, stride, ch, iptr, istride, C.byref(p), *tail))
        else:
            _lib.check(_lib.lib().tscm_sweep_compose_visible(self._handle, ptrs, stride, ch, iptr, istride, C.byref(p), C.byref(_visibility_struct(visibility)), *tail))
        res = (out,) + ((cov,) if with_coverage else ()) + ((sec.value,) if with_seconds else ())
        return res[0] if len(res) == 1 else res

    def compose_stages(self, images, index16=None, gains=None, visibility=None, **params) -> dict:
        """tscm_sweep_compose_stages -> hypothesis [ph, pw], sampled [n, ph, pw, C], alpha [n, ph, pw], label [ph, pw] and, in
        MULTIBAND mode, mask_pyramid [n, S], lap_pyramid [n, C, S], blend_pyramid [C, S] (levels 0..L one after the other).
        visibility (as for compose): tscm_sweep_compose_visible_stages, which adds use [n, ph, pw] and state [ph, pw]."""
        imgs, ptrs, stride, ch = self._colour_frame(images)
        p, (idx, iptr, istride), (g, gptr) = self._compose_args(index16, gains, params)
        n, ph, pw = self.n, self.pano_h, self.pano_w
        res = dict(hypothesis=np.zeros((ph, pw), np.uint8), sampled=np.zeros((n, ph, pw, ch), np.uint8), alpha=np.zeros((n, ph, pw), np.uint8),
                   label=np.zeros((ph, pw), np.uint8))
        ub, sh = C.POINTER(C.c_ubyte), C.POINTER(C.c_short)
        pyr = [None, None, None]
        if p.mode == _lib.PANO_MULTIBAND:
            S = sum((ph >> l) * (pw >> l) for l in range(max(int(p.levels), 0) + 1))
            res.update(mask_pyramid=np.zeros((n, S), np.uint8), lap_pyramid=np.zeros((n, ch, S), np.int16), blend_pyramid=np.zeros((ch, S), np.int16))
            pyr = [res["mask_pyramid"].ctypes.data_as(ub), res["lap_pyramid"].ctypes.data_as(sh), res["blend_pyramid"].ctypes.data_as(sh)]
        tail = (gptr, res["hypothesis"].ctypes.data_as(ub), res["sampled"].ctypes.data_as(ub), res["alpha"].ctypes.data_as(ub), res["label"].ctypes.data_as(ub), *pyr)
        if visibility is None:
            _lib.check(_lib.lib().tscm_sweep_compose_stages(self._handle, ptrs, stride, ch, iptr, istride, C.byref(p), *tail))
        else:
            res.update(use=np.zeros((n, ph, pw), np.uint8), state=np.zeros((ph, pw), np.uint8))
            _lib.check(_lib.lib().tscm_sweep_compose_visible_stages(self._handle, ptrs, stride, ch, iptr, istride, C.byref(p), C.byref(_visibility_struct(visibility)),
                                                                    *tail, res["use"].ctypes.data_as(ub), res["state"].ctypes.data_as(ub)))
        return res

    def visibility(self, index16=None, with_state: bool = False, with_seconds: bool = False, **params):
        """tscm_sweep_visibility -> use uint8 [n, pano_h, pano_w] (1: the composer takes camera k at that pixel) and, with_state,
        state uint8 [pano_h, pano_w] (0 no depth, 1 seen by nobody, 2 all visible, 3 some occluded, 4 all occluded and all
        kept).  index16: None for the map of the last depth().  params: the fields of visibility_params."""
        if self._handle is None:
            raise ValueError("the sweeper is closed")
        vp = visibility_params(**params)
        _, (idx, iptr, istride), _ = self._compose_args(index16, None, {})
        use, state = np.zeros((self.n, self.pano_h, self.pano_w), np.uint8), np.zeros((self.pano_h, self.pano_w), np.uint8)
        ub = C.POINTER(C.c_ubyte)
        sec = C.c_double(0.0)
        _lib.check(_lib.lib().tscm_sweep_visibility(self._handle, iptr, istride, C.byref(vp), use.ctypes.data_as(ub), state.ctypes.data_as(ub) if with_state else None,
                                                    C.byref(sec)))
        res = (use,) + ((state,) if with_state else ()) + ((sec.value,) if with_seconds else ())
        return res[0] if len(res) == 1 else res

    def visibility_stages(self, index16=None, **params) -> dict:
        """tscm_sweep_visibility_stages -> hypothesis [ph, pw] uint8, depth_buffer [n, ch, cw] uint16, cell [n, ph, pw] int32,
        visible [n, ph, pw], use [n, ph, pw], state [ph, pw] uint8."""
        if self._handle is None:
            raise ValueError("the sweeper is closed")
        vp = visibility_params(**params)
        _, (idx, iptr, istride), _ = self._compose_args(index16, None, {})
        n, ph, pw = self.n, self.pano_h, self.pano_w
        shift = min(max(vp.cell_shift, 0), 8)                        # outside 0..8: refused below
        cw, ch = ((self.width - 1) >> shift) + 1, ((self.height - 1) >> shift) + 1
        res = dict(hypothesis=np.zeros((ph, pw), np.uint8), depth_buffer=np.zeros((n, ch, cw), np.uint16), cell=np.zeros((n, ph, pw), np.int32),
                   visible=np.zeros((n, ph, pw), np.uint8), use=np.zeros((n, ph, pw), np.uint8), state=np.zeros((ph, pw), np.uint8))
        ub = C.POINTER(C.c_ubyte)
        _lib.check(_lib.lib().tscm_sweep_visibility_stages(self._handle, iptr, istride, C.byref(vp), res["hypothesis"].ctypes.data_as(ub),
                                                           res["depth_buffer"].ctypes.data_as(C.POINTER(C.c_ushort)), res["cell"].ctypes.data_as(C.POINTER(C.c_int)),
                                                           res["visible"].ctypes.data_as(ub), res["use"].ctypes.data_as(ub), res["state"].ctypes.data_as(ub)))
        return res

    def stage_times(self) -> np.ndarray:
        """Device seconds of the last depth / stages call: cost volume, aggregation, winner."""
        t = np.zeros(3)
        _lib.check(_lib.lib().tscm_sweep_stage_times(_lib.dptr(t)))
        return t

    def points(self, index16):
        """tscm_sweep_points with the panorama and the inverse distances the sweeper was built from (from_rig, or from_tables
        with pano_desc and inv_distance) -> (points [ph, pw, 3] in the rig frame, valid [ph, pw] bool)."""
        if self.pano_desc is None or self.inv_distance is None:
            raise ValueError("points need the panorama's descriptor and the inverse distances")
        return points(index16, self.pano_desc, self.inv_distance, device=self.device)


def points(index16, pano_desc, inv_distance, device: int = 0):
    """tscm_sweep_points -> (points [h, w, 3] float64 in the rig frame, NaN where invalid; valid [h, w] bool)."""
    idx = np.asarray(index16)
    if idx.dtype != np.int16 or idx.ndim != 2 or idx.strides[1] != 2 or idx.strides[0] % 2:
        raise ValueError("index16 is an int16 [h, w] array (or row-padded view)")
    h, w = idx.shape
    inv = np.ascontiguousarray(inv_distance, dtype=np.float64).ravel()
    pts, valid = np.zeros((h, w, 3)), np.zeros((h, w), dtype=np.uint8)
    _lib.check(_lib.lib().tscm_sweep_points(idx.ctypes.data_as(C.POINTER(C.c_short)), w, h, int(idx.strides[0] // 2) if h else w, _maps._c_descs([pano_desc]),
                                            _maps.projection_kind(pano_desc.projection), _lib.dptr(inv), inv.size, device, _lib.dptr(pts),
                                            valid.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return pts, valid.astype(bool)


def _check_fill(fill):
    if fill is not None and "min_disparity" in fill:
        raise TypeError("fill: min_disparity is 0 for an index map")


def _check_refine(refine):
    if refine is not None and "min_disparity" in refine:
        raise TypeError("refine: min_disparity is 0 for an index map")


def _post_fill_refine(s, grey, idx, post, fill, refine, fallback_index, device):
    """The chain of stereo on an index map: min_disparity 0, wrap_x = 1 unless a dict says otherwise, refine guided by the
    grey frame that the sweeper composes in SEAM mode at the map as it stands."""
    from . import stereo
    return stereo._post_fill_refine(idx, post or None, fill, refine, 0, 1, lambda m: s.compose(grey, index16=m, mode="seam", fallback_index=fallback_index), device)


def rig_depth(images, intr, Twc, pano_w: int = 1024, pano_h: int = 512, near: float = 500.0, far: float = np.inf, D: int = 64, weights="radial",
              projection="equirect", device: int = 0, post=None, fill=None, refine=None, **over):
    """One call from a calibration and a frame to (index16 [ph, pw], points [ph, pw, 3] in the rig frame, valid [ph, pw]).
    near / far in the units of Twc's translations.  post: keyword arguments of stereo.filter (speckle_window_size,
    speckle_range, median), applied to the index map before the points; an index map is a disparity map with
    min_disparity = 0.  fill: keyword arguments of stereo.fill (rule, paths, max_distance, min_directions, wrap_x; wrap_x
    defaults to 1 here), applied after post.  refine: keyword arguments of stereo.refine (radius, iterations, fill_invalid,
    wrap_x, sigma or weights; wrap_x defaults to 1 here), applied after fill; the guide is the frame composed in SEAM mode at
    the map as it stands, pixels without depth at hypothesis 0."""
    _check_fill(fill)
    _check_refine(refine)
    size = (np.asarray(images[0]).shape[1], np.asarray(images[0]).shape[0])
    inv = inverse_distances(near, far, D)
    with Sweeper.from_rig(intr, Twc, size, pano_w, pano_h, inv, weights=weights, projection=projection, device=device, **over) as s:
        idx = s.depth(images)
        idx = _post_fill_refine(s, images, idx, post, fill, refine, 0, device)
        pts, valid = s.points(idx)
    return idx, pts, valid


def rig_panorama(images, intr, Twc, pano_w: int = 1024, pano_h: int = 512, near: float = 500.0, far: float = np.inf, D: int = 64, weights="radial",
                 projection="equirect", device: int = 0, post=None, mode="multiband", levels: int = 4, gains=None, fallback_index: int = 0, fill=None,
                 refine=None, visibility=None, **over):
    """One call from a calibration and a frame to the parallax-free panorama: (panorama uint8 [ph, pw] or [ph, pw, 3],
    index16 [ph, pw], coverage [ph, pw]).  Colour images (BGR) go through bgr_to_gray for the depth pass and are blended in
    colour.  post: keyword arguments of stereo.filter for the index map, as in rig_depth; the filtered map is the one the
    frame is composed at and the one returned.  fill: keyword arguments of stereo.fill, as in rig_depth, applied after
    post; the frame is then composed at the filled map.  refine: keyword arguments of stereo.refine, as in rig_depth,
    applied after fill and guided by the grey frame composed in SEAM mode at the map as it stands (pixels without depth at
    fallback_index); the returned frame is composed at the refined map.  fallback_index: the hypothesis of a pixel without
    depth (0 = far).  visibility: None, or the fields of visibility_params as a dict: the returned frame leaves out, per pixel,
    the cameras that look at its point through something nearer (Sweeper.compose with visibility), judged at the map the
    frame is composed at."""
    _check_fill(fill)
    _check_refine(refine)
    size = (np.asarray(images[0]).shape[1], np.asarray(images[0]).shape[0])
    inv = inverse_distances(near, far, D)
    with Sweeper.from_rig(intr, Twc, size, pano_w, pano_h, inv, weights=weights, projection=projection, device=device, **over) as s:
        grey = [bgr_to_gray(x) for x in images]
        idx = s.depth(grey)
        idx = _post_fill_refine(s, grey, idx, post, fill, refine, fallback_index, device)
        pano, cov = s.compose(images, index16=idx if post or fill is not None or refine is not None else None, gains=gains, with_coverage=True, visibility=visibility, mode=mode, levels=levels, fallback_index=fallback_index)
    return pano, idx, cov
