"""Chessboard-corner candidates of a grey image on the GPU: host-side mirror of findCorner()'s first stage
(DetectCorner/findCorner.cpp:7-66 + :492-541) over tscm_detect_corners.  No CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _l


def detect_corners(gray, sigma: int = 4, min_score: float = 0.01, device: int = 0) -> dict:
    """gray: (H, W) uint8.  Returns the kept candidates in suppression order: x, y (pixel of the maximum), v1, v2
    (edge directions), score, sub (sub-pixel position), plus n_maxima and the device time in seconds."""
    g = np.asarray(gray)
    if g.ndim != 2 or g.dtype != np.uint8:
        raise ValueError("detect_corners expects a 2-D uint8 image (convert BGR to grey first, findCorner.cpp:9-10)")
    if g.strides[1] != 1 or g.strides[0] < g.shape[1]:          # rows must be contiguous; a row stride > width is passed through
        g = np.ascontiguousarray(g)
    h, w = g.shape
    out = _l.CCornerCandidates()
    f = _l.lib().tscm_detect_corners
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(_l.CCornerCandidates)]
    _l.check(f(g.ctypes.data, w, h, g.strides[0], int(sigma), float(min_score), int(device), C.byref(out)))
    try:
        n = out.n
        arr = lambda p, k: np.ctypeslib.as_array(p, shape=(n * k,)).copy().reshape(n, k) if n else np.zeros((0, k))
        return dict(n=n, n_maxima=out.n_maxima, x=arr(out.x, 1)[:, 0], y=arr(out.y, 1)[:, 0], v1=arr(out.v1, 2), v2=arr(out.v2, 2),
                    score=arr(out.score, 1)[:, 0], sub=arr(out.sub, 2), seconds=out.seconds)
    finally:
        fr = _l.lib().tscm_corner_candidates_free
        fr.restype = None
        fr.argtypes = [C.POINTER(_l.CCornerCandidates)]
        fr(C.byref(out))


def _unpack(out) -> dict:
    n = out.n
    arr = lambda p, k: np.ctypeslib.as_array(p, shape=(n * k,)).copy().reshape(n, k) if n else np.zeros((0, k))
    return dict(n=n, n_maxima=out.n_maxima, x=arr(out.x, 1)[:, 0], y=arr(out.y, 1)[:, 0], v1=arr(out.v1, 2), v2=arr(out.v2, 2),
                score=arr(out.score, 1)[:, 0], sub=arr(out.sub, 2), seconds=out.seconds)


def _batch(images, stride, what: str):
    """The images of a batch call as (arrays kept alive, pointer array, width, height, row stride).  stride None: each
    image is made contiguous; otherwise every image must be a view with that row stride (e.g. buf[:, :w] of an
    (H, stride) buffer), whose padding bytes are passed through untouched."""
    if stride is None:
        imgs = [np.ascontiguousarray(g) for g in images]
    else:
        imgs = [np.asarray(g) for g in images]
    if not imgs:
        return [], None, 0, 0, 0
    h, w = imgs[0].shape[:2]
    if any(g.ndim != 2 or g.dtype != np.uint8 or g.shape != (h, w) for g in imgs):
        raise ValueError(f"{what} expects 2-D uint8 images of one size")
    s = w if stride is None else int(stride)
    if stride is not None and (s < w or any(g.strides != (s, 1) for g in imgs)):
        raise ValueError(f"{what}: every image must have row stride {s} >= width {w} and contiguous rows")
    return imgs, (C.c_void_p * len(imgs))(*[g.ctypes.data for g in imgs]), w, h, s


def detect_corners_batch(images, sigma: int = 4, min_score: float = 0.01, device: int = 0, stride=None) -> list:
    """tscm_detect_corners_batch: a list of (H, W) uint8 images of one size -> list of candidate dicts, one pass of the
    kernels for all of them.  stride: see corner_planes."""
    imgs, ptrs, w, h, s = _batch(images, stride, "detect_corners_batch")
    if not imgs:
        return []
    n = len(imgs)
    outs = (_l.CCornerCandidates * n)()
    f = _l.lib().tscm_detect_corners_batch
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]
    _l.check(f(ptrs, n, w, h, s, int(sigma), float(min_score), int(device), outs))
    fr = _l.lib().tscm_corner_candidates_free
    fr.restype = None
    fr.argtypes = [C.POINTER(_l.CCornerCandidates)]
    try:
        return [_unpack(outs[i]) for i in range(n)]
    finally:
        for i in range(n):
            fr(C.byref(outs[i]))


def corner_planes(images, sigma: int = 4, device: int = 0, stride=None, planes=("ig", "metric", "ixy")) -> dict:
    """tscm_corner_planes_batch: the planes tscm_detect_corners_batch computes for a list of (H, W) uint8 images of one
    size (or one image) -- ig (normalised and blurred image), metric (cxy + c45) and ixy -- each (n, H, W) fp64, for the
    names in `planes`.  stride None: the images are made contiguous; otherwise every image must be a view with that row
    stride (e.g. buf[:, :w] of an (H, stride) buffer) and the batch is passed with it."""
    if isinstance(images, np.ndarray) and images.ndim == 2:
        images = [images]
    imgs, ptrs, w, h, s = _batch(images, stride, "corner_planes")
    n = len(imgs)
    out = {k: np.empty((n, h, w)) for k in planes}
    if not imgs:
        return out
    f = _l.lib().tscm_corner_planes_batch
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
    p = [out[k].ctypes.data if k in out else None for k in ("ig", "metric", "ixy")]
    _l.check(f(ptrs, n, w, h, s, int(sigma), int(device), *p))
    return out


def chessboards_from_corners(x, y, v1, v2) -> list:
    """chessboardsFromCorners (DetectCorner/chessboard.cpp:3-103): list of index matrices (rows x cols, cols >= rows)
    into the candidate list.  Host logic of the library (no device needed)."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    v1, v2 = np.ascontiguousarray(v1, dtype=np.float64), np.ascontiguousarray(v2, dtype=np.float64)
    out = _l.CChessboards()
    f = _l.lib().tscm_chessboards_from_corners
    f.restype = C.c_int
    f.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.POINTER(_l.CChessboards)]
    _l.check(f(int(x.shape[0]), x.ctypes.data, y.ctypes.data, v1.ctypes.data, v2.ctypes.data, C.byref(out)))
    try:
        res = []
        for q in range(out.n_boards):
            r, c, o = out.rows[q], out.cols[q], out.offset[q]
            res.append(np.array([out.cells[o + k] for k in range(r * c)], dtype=np.int32).reshape(r, c))
        return res
    finally:
        fr = _l.lib().tscm_chessboards_free
        fr.restype = None
        fr.argtypes = [C.POINTER(_l.CChessboards)]
        fr(C.byref(out))


_WHERE = {"host": _l.BOARDS_HOST, "device": _l.BOARDS_DEVICE}


def _candidate_records(cands):
    """Candidate dicts (or (x, y, v1, v2) tuples) as an array of tscm_corner_candidates; only n, x, y, v1, v2 are filled.
    Returns the arrays kept alive and the records."""
    keep, recs = [], (_l.CCornerCandidates * max(len(cands), 1))()
    dp = C.POINTER(C.c_double)
    for k, c in enumerate(cands):
        x, y, v1, v2 = (c["x"], c["y"], c["v1"], c["v2"]) if isinstance(c, dict) else c
        a = [np.ascontiguousarray(x, dtype=np.float64).ravel(), np.ascontiguousarray(y, dtype=np.float64).ravel(),
             np.ascontiguousarray(v1, dtype=np.float64).ravel(), np.ascontiguousarray(v2, dtype=np.float64).ravel()]
        n = a[0].shape[0]
        if a[1].shape[0] != n or a[2].shape[0] != 2 * n or a[3].shape[0] != 2 * n:
            raise ValueError(f"candidates {k}: x, y of n and v1, v2 of (n, 2) values expected")
        keep.append(a)
        recs[k].n = n
        recs[k].x, recs[k].y, recs[k].v1, recs[k].v2 = (q.ctypes.data_as(dp) for q in a)
    return keep, recs


def _where(where: str) -> int:
    if where not in _WHERE:
        raise ValueError(f"where = {where!r}: 'host' or 'device'")
    return _WHERE[where]


def chessboards_from_corners_batch(cands, where: str = "device", device: int = 0) -> list:
    """tscm_chessboards_from_corners_batch: the structure recovery of a list of candidate sets (the dicts of
    detect_corners_batch, or (x, y, v1, v2) tuples) in one call, one independent job per (image, seed) -- on the device
    (k_board_seeds) or, where="host", the same definition on the host.  Returns one list of index matrices per image.  The
    definition (tscm.h) differs from chessboards_from_corners in one documented step; the boards agree unless a winning
    proposal holds an exact tie of two distances."""
    cands = list(cands)
    keep, recs = _candidate_records(cands)
    outs = (_l.CChessboards * max(len(cands), 1))()
    f = _l.lib().tscm_chessboards_from_corners_batch
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    _l.check(f(len(cands), recs, _where(where), int(device), outs))
    fr = _l.lib().tscm_chessboards_free
    fr.restype = None
    fr.argtypes = [C.POINTER(_l.CChessboards)]
    res = []
    try:
        for k in range(len(cands)):
            o = outs[k]
            off = np.ctypeslib.as_array(o.offset, shape=(o.n_boards + 1,)) if o.n_boards else np.zeros(1, dtype=np.int32)
            cells = np.ctypeslib.as_array(o.cells, shape=(int(off[-1]),)).astype(np.int32) if o.n_boards else np.zeros(0, dtype=np.int32)
            res.append([cells[off[q]:off[q + 1]].reshape(o.rows[q], o.cols[q]).copy() for q in range(o.n_boards)])
    finally:
        for k in range(len(cands)):
            fr(C.byref(outs[k]))
    return res


def chessboards_batch_stages(cands, where: str = "device", device: int = 0) -> list:
    """tscm_chessboards_batch_stages: per image a dict of the seeds' records in seed order -- status (0 blank seed, 1 seed
    energy > 0, 2 grown but energy not < -10, 3 offered to the overlap resolution), rows, cols, steps, energy, offset
    (n + 1) and cells (the boards before the turn, row-major), plus on_device."""
    cands = list(cands)
    keep, recs = _candidate_records(cands)
    outs = (_l.CBoardSeedStages * max(len(cands), 1))()
    f = _l.lib().tscm_chessboards_batch_stages
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    _l.check(f(len(cands), recs, _where(where), int(device), outs))
    fr = _l.lib().tscm_board_seed_stages_free
    fr.restype = None
    fr.argtypes = [C.POINTER(_l.CBoardSeedStages)]
    res = []
    try:
        for k in range(len(cands)):
            o, n = outs[k], outs[k].n
            arr = lambda p, m, dt: np.ctypeslib.as_array(p, shape=(m,)).astype(dt) if m else np.zeros(0, dtype=dt)
            off = np.ctypeslib.as_array(o.offset, shape=(n + 1,)).astype(np.int32)
            res.append(dict(n=n, on_device=bool(o.on_device), status=arr(o.status, n, np.int32), rows=arr(o.rows, n, np.int32), cols=arr(o.cols, n, np.int32),
                            steps=arr(o.steps, n, np.int32), energy=arr(o.energy, n, np.float64), offset=off, cells=arr(o.cells, int(off[-1]), np.int32)))
    finally:
        for k in range(len(cands)):
            fr(C.byref(outs[k]))
    return res


def chessboards_batch_seconds() -> float:
    """Device time of k_board_seeds in this thread's last device call."""
    f = _l.lib().tscm_chessboards_batch_seconds
    f.restype = C.c_double
    f.argtypes = []
    return float(f())


_RECOVER = ("host", "device", "host-batch")


def _recovered(ds, recover: str, device: int) -> list:
    """The boards of every candidate dict of ds by the route `recover` names."""
    if recover not in _RECOVER:
        raise ValueError(f"recover = {recover!r}: one of {_RECOVER}")
    if recover == "host":
        return [chessboards_from_corners(d["x"], d["y"], d["v1"], d["v2"]) for d in ds]
    return chessboards_from_corners_batch(ds, where="device" if recover == "device" else "host", device=device)


def find_chessboard(gray, cols: int, rows: int, sigma: int = 4, device: int = 0, recover: str = "host"):
    """The acceptance test of main.cpp:32-46: corner candidates, structure recovery, and -- when exactly one board of
    cols x rows inner corners came out -- its sub-pixel corners as a (rows * cols, 2) array in board order; else None.
    recover: see find_chessboards."""
    d = detect_corners(gray, sigma=sigma, device=device)
    boards = _recovered([d], recover, device)[0]
    if len(boards) != 1 or boards[0].shape != (rows, cols):
        return None
    return d["sub"][boards[0].ravel()]


def find_chessboards(images, cols: int, rows: int, sigma: int = 4, device: int = 0, first_board_only: bool = False, recover: str = "host") -> list:
    """find_chessboard for a list of images of one size: ONE pass of the detection kernels for all of them
    (tscm_detect_corners_batch), then the structure recovery.  Entries are (rows * cols, 2) arrays or None.
    Acceptance: exactly one board of rows x cols corners (main.cpp:40-46, the input images); first_board_only: at least
    one board and board 0 has the right shape (main.cpp:67, the remapped chessboards of the refinement pass).
    recover: "host" = chessboards_from_corners per image (the default); "device" = one call of
    chessboards_from_corners_batch for all images on the device; "host-batch" = that definition on the host."""
    out = []
    ds = detect_corners_batch(images, sigma=sigma, device=device)
    for d, boards in zip(ds, _recovered(ds, recover, device)):
        ok = (len(boards) >= 1 if first_board_only else len(boards) == 1) and boards[0].shape == (rows, cols)
        out.append(d["sub"][boards[0].ravel()] if ok else None)
    return out
