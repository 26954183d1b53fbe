"""The panorama of a calibrated rig (tscm.h: tscm_panorama_*): Composer keeps the rig's tables, alphas, seam labels and mask
pyramids on the device and composes one frame per call by seam, feather or multi-band blending; radial_weights gives the
per-camera masks, exposure_gains the gain compensation from the overlap sums."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib
from . import maps as _maps


def params(mode="multiband", levels: int = 4, wrap_x: bool = True) -> _lib.CPanoramaParams:
    if isinstance(mode, str):
        if mode not in _lib.PANO_MODES:
            raise ValueError(f"unknown mode {mode!r}: one of {', '.join(_lib.PANO_MODES)}")
        mode = _lib.PANO_MODES[mode]
    p = _lib.CPanoramaParams()
    _lib.lib().tscm_panorama_default_params(C.byref(p))
    p.mode, p.levels, p.wrap_x = int(mode), int(levels), int(bool(wrap_x))
    return p


def weights_from_rays(rays, max_theta: float) -> np.ndarray:
    """255 cos^2(pi/2 theta/max_theta) of unit rays [..., 3] (theta = angle to the optical axis), rounded to uint8; 0 beyond
    max_theta and for rays outside the model's domain (NaN)."""
    rays = np.asarray(rays, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        theta = np.arctan2(np.hypot(rays[..., 0], rays[..., 1]), rays[..., 2])
        wgt = 255.0 * np.cos(0.5 * np.pi * theta / max_theta) ** 2
        ok = np.all(np.isfinite(rays), axis=-1) & (theta < max_theta)
    return np.where(ok, np.rint(np.where(ok, wgt, 0.0)), 0.0).astype(np.uint8)


def radial_weights(intr, width: int, height: int, max_theta: float = np.radians(100.0), device: int = 0) -> np.ndarray:
    """uint8 [height, width] mask of one camera: weights_from_rays of tscm_unproject_pixels at every pixel."""
    from . import api
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    rays = api.unproject(intr, np.stack([u.ravel(), v.ravel()], axis=-1), device=device)
    return weights_from_rays(rays, max_theta).reshape(height, width)


def exposure_gains(count, sum, sigma_n: float = 10.0, sigma_g: float = 0.1) -> np.ndarray:
    """Gain compensation of Brown & Lowe (OpenCV's GainCompensator) from the overlap sums: minimises
    sum_ij N_ij [(g_i I_ij - g_j I_ji)^2 / sigma_n^2 + (1 - g_i)^2 / sigma_g^2] with N = count and I = sum / count, an
    n x n linear system solved in fp64.  Returns round(256 g) clipped to 64..1024 as uint16 (the gain_q8 of compose)."""
    N = np.asarray(count, dtype=np.float64)
    n = N.shape[0]
    if N.shape != (n, n) or np.asarray(sum).shape != (n, n):
        raise ValueError("count and sum are [n, n] arrays")
    I = np.divide(np.asarray(sum, dtype=np.float64), N, out=np.zeros((n, n)), where=N > 0)
    if n == 1:
        return np.full(1, 256, dtype=np.uint16)
    alpha, beta = 1.0 / (sigma_n * sigma_n), 1.0 / (sigma_g * sigma_g)
    A, b = np.zeros((n, n)), np.zeros(n)
    for i in range(n):
        for j in range(n):
            b[i] += beta * N[i, j]
            A[i, i] += beta * N[i, j]
            if j == i:
                continue
            A[i, i] += 2.0 * alpha * I[i, j] * I[i, j] * N[i, j]
            A[i, j] -= 2.0 * alpha * I[i, j] * I[j, i] * N[i, j]
    for i in range(n):                       # a camera that covers nothing keeps gain 1
        if A[i, i] == 0.0:
            A[i, i], b[i] = 1.0, 1.0
    g = np.linalg.solve(A, b)
    return np.clip(np.rint(256.0 * g), 64, 1024).astype(np.uint16)


class Composer:
    """Context manager around a tscm_panorama handle.  Either from a calibration -- Composer(intr, Twc, image_size,
    pano_size, ...) builds the tables through maps.panorama_descs / maps.build_maps -- or from tables of the caller's:
    Composer.from_tables(mapx, mapy, image_size, channels, ...).  image_size = (width, height), pano_size = (pano_w, pano_h).
    weights: "radial" (radial_weights per camera), None (all 255), or n arrays [height, width] uint8 (entries may be None)."""

    def __init__(self, intr, Twc, image_size, pano_size, channels: int = 3, mode="multiband", levels: int = 4, weights="radial",
                 projection="equirect", device: int = 0, max_theta: float = np.radians(100.0)):
        w, h = int(image_size[0]), int(image_size[1])
        pw, ph = int(pano_size[0]), int(pano_size[1])
        intr = np.asarray(intr, dtype=np.float64).reshape(-1, 9)
        descs = _maps.panorama_descs(intr, Twc, pw, ph, projection)
        for k, d in enumerate(descs):
            d.out_offset = k * pw * ph
        mapx, mapy, _ = _maps.build_maps(descs, n_elems=len(descs) * pw * ph, device=device)
        if isinstance(weights, str):
            if weights != "radial":
                raise ValueError("weights: 'radial', None or one array per camera")
            weights = [radial_weights(intr[k], w, h, max_theta, device=device) for k in range(len(descs))]
        self._handle = None
        self._open(mapx.reshape(len(descs), ph, pw), mapy.reshape(len(descs), ph, pw), w, h, channels, mode, levels, True, weights, device)

    @classmethod
    def from_tables(cls, mapx, mapy, image_size, channels: int = 3, mode="multiband", levels: int = 4, wrap_x: bool = True, weights=None,
                    device: int = 0):
        self = cls.__new__(cls)
        self._handle = None
        self._open(mapx, mapy, int(image_size[0]), int(image_size[1]), channels, mode, levels, wrap_x, weights, device)
        return self

    def _open(self, mapx, mapy, w, h, channels, mode, levels, wrap_x, weights, device):
        mapx, mapy = np.ascontiguousarray(mapx, dtype=np.float32), np.ascontiguousarray(mapy, dtype=np.float32)
        if mapx.ndim != 3 or mapx.shape != mapy.shape:
            raise ValueError("mapx and mapy are [n, pano_h, pano_w] tables of the same shape")
        self.n, self.pano_h, self.pano_w = mapx.shape
        self.width, self.height, self.channels, self.device = w, h, int(channels), int(device)
        self.mapx, self.mapy = mapx, mapy
        self.params = params(mode, levels, wrap_x)
        self.levels = int(self.params.levels) if self.params.mode == _lib.PANO_MULTIBAND else 0
        wptr = None
        if weights is not None:
            if len(weights) != self.n:
                raise ValueError(f"{self.n} cameras need {self.n} weight entries")
            self.weights = [None if x is None else np.ascontiguousarray(x, dtype=np.uint8) for x in weights]
            for x in self.weights:
                if x is not None and x.shape != (h, w):
                    raise ValueError("a weight image has the shape [height, width] of the source images")
            wptr = (C.c_void_p * self.n)(*[None if x is None else x.ctypes.data for x in self.weights])
        else:
            self.weights = None
        fp = C.POINTER(C.c_float)
        hdl = C.c_void_p()
        _lib.check(_lib.lib().tscm_panorama_create(self.n, w, h, self.channels, wptr, mapx.ctypes.data_as(fp), mapy.ctypes.data_as(fp), self.pano_w, self.pano_h,
                                                   C.byref(self.params), self.device, C.byref(hdl)))
        self._handle = hdl

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if self._handle is not None:
            _lib.lib().tscm_panorama_destroy(self._handle)
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
            raise ValueError("the composer is closed")
        if len(images) != self.n:
            raise ValueError(f"{self.n} cameras need {self.n} images")
        shape = (self.height, self.width) if self.channels == 1 else (self.height, self.width, self.channels)
        imgs = []
        for x in images:
            a = np.asarray(x)
            if a.dtype != np.uint8 or a.shape != shape:
                raise ValueError(f"images are uint8 arrays of shape {shape}")
            inner = a.strides[1:] == (tuple([self.channels, 1]) if self.channels > 1 else (1,))
            imgs.append(a if inner and a.strides[0] >= self.width * self.channels else np.ascontiguousarray(a))
        if len({a.strides[0] for a in imgs}) > 1:
            imgs = [np.ascontiguousarray(a) for a in imgs]
        return imgs, (C.c_void_p * self.n)(*[a.ctypes.data for a in imgs]), int(imgs[0].strides[0])

    def _gains(self, gains):
        if gains is None:
            return None, None
        g = np.ascontiguousarray(gains, dtype=np.uint16)
        if g.shape != (self.n,):
            raise ValueError(f"gains: {self.n} Q8 values")
        return g, _lib.ushort_ptr(g)

    def compose(self, images, gains=None, out: np.ndarray | None = None, with_coverage: bool = False, with_seconds: bool = False):
        """tscm_panorama_compose -> uint8 [pano_h, pano_w] or [pano_h, pano_w, 3]; `out` may be a row-padded view, whose
        padding keeps its values.  gains: Q8 per camera (exposure_gains)."""
        imgs, ptrs, stride = self._frame(images)
        shape = (self.pano_h, self.pano_w) if self.channels == 1 else (self.pano_h, self.pano_w, self.channels)
        if out is None:
            out = np.zeros(shape, dtype=np.uint8)
        inner = out.strides[1:] == ((self.channels, 1) if self.channels > 1 else (1,))
        if out.dtype != np.uint8 or out.shape != shape or not inner:
            raise ValueError("out must be a uint8 array (or row-padded view) of the panorama's shape")
        cov = np.zeros((self.pano_h, self.pano_w), dtype=np.uint8) if with_coverage else None
        g, gptr = self._gains(gains)
        ub = C.POINTER(C.c_ubyte)
        sec = C.c_double(0.0)
        _lib.check(_lib.lib().tscm_panorama_compose(self._handle, ptrs, stride, gptr, out.ctypes.data_as(ub), int(out.strides[0]),
                                                    None if cov is None else cov.ctypes.data_as(ub), C.byref(sec)))
        res = (out,) + ((cov,) if with_coverage else ()) + ((sec.value,) if with_seconds else ())
        return res[0] if len(res) == 1 else res

    def level_shapes(self):
        return [(self.pano_h >> l, self.pano_w >> l) for l in range(self.levels + 1)]

    def stages(self, images, gains=None) -> dict:
        """tscm_panorama_stages -> sampled [n, ph, pw, C], alpha [n, ph, pw], label [ph, pw] and, in MULTIBAND mode,
        mask_pyramid [n, S], lap_pyramid [n, C, S], blend_pyramid [C, S] (levels 0..L one after the other)."""
        imgs, ptrs, stride = self._frame(images)
        n, ph, pw, ch = self.n, self.pano_h, self.pano_w, self.channels
        res = dict(sampled=np.zeros((n, ph, pw, ch), np.uint8), alpha=np.zeros((n, ph, pw), np.uint8), label=np.zeros((ph, pw), np.uint8))
        ub, sh = C.POINTER(C.c_ubyte), C.POINTER(C.c_short)
        pyr = [None, None, None]
        if self.params.mode == _lib.PANO_MULTIBAND:
            S = sum(a * b for a, b in self.level_shapes())
            res.update(mask_pyramid=np.zeros((n, S), np.uint8), lap_pyramid=np.zeros((n, ch, S), np.int16), blend_pyramid=np.zeros((ch, S), np.int16))
            pyr = [res["mask_pyramid"].ctypes.data_as(ub), res["lap_pyramid"].ctypes.data_as(sh), res["blend_pyramid"].ctypes.data_as(sh)]
        g, gptr = self._gains(gains)
        _lib.check(_lib.lib().tscm_panorama_stages(self._handle, ptrs, stride, gptr, res["sampled"].ctypes.data_as(ub), res["alpha"].ctypes.data_as(ub),
                                                   res["label"].ctypes.data_as(ub), *pyr))
        return res

    def overlap(self, images):
        """tscm_panorama_overlap -> count [n, n], sum [n, n] (int64): the inputs of exposure_gains."""
        imgs, ptrs, stride = self._frame(images)
        count, total = np.zeros((self.n, self.n), np.int64), np.zeros((self.n, self.n), np.int64)
        ll = C.POINTER(C.c_longlong)
        _lib.check(_lib.lib().tscm_panorama_overlap(self._handle, ptrs, stride, count.ctypes.data_as(ll), total.ctypes.data_as(ll)))
        return count, total
