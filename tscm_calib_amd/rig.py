"""Rig initialisation: host-side mirror of the constructor MultiCalib::MultiCalib(cameras, worlds)
(multi_calib.cpp:6-153), the step that produces the initial guess calibrate() starts from.

RigInput is what the constructor reads from the mono-calibrated cameras:
cameras_[m].intrinsic(), has_chessboard(j), Rt(j), pixels()[j] and the board points.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import lib as _lib
from .problem import Problem


@dataclass
class RigInput:
    worlds: np.ndarray      # [n,3]   board points (main.cpp:12-18)
    intr: np.ndarray        # [C,9]
    has: np.ndarray         # [C,B]   uint8
    Rt: np.ndarray          # [C,B,3,3]  [r1 r2 t] (TS.cpp:150-204 output, TS.h:33)
    pix_u: np.ndarray       # [C,B,n]
    pix_v: np.ndarray       # [C,B,n]
    meta: dict = field(default_factory=dict)

    @property
    def n_cameras(self) -> int:
        return self.intr.shape[0]

    @property
    def n_boards(self) -> int:
        return self.has.shape[1]

    @property
    def n_points(self) -> int:
        return self.worlds.shape[0]

    def normalised(self) -> "RigInput":
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        return RigInput(f(self.worlds), f(self.intr), np.ascontiguousarray(self.has, dtype=np.uint8), f(self.Rt),
                        f(self.pix_u), f(self.pix_v), self.meta)


def rig_init(inp: RigInput, device: int = 0) -> dict:
    """tscm_rig_init.  Returns cam_R/cam_t/cam_rt, board_R/board_t/board_rt, board_initial,
    cam_choice, cam_min_error and the device timings."""
    inp = inp.normalised()
    Cn, B, n = inp.n_cameras, inp.n_boards, inp.n_points
    if inp.has.shape != (Cn, B) or inp.Rt.shape != (Cn, B, 3, 3) or inp.pix_u.shape != (Cn, B, n) \
            or inp.pix_v.shape != (Cn, B, n) or inp.worlds.shape != (n, 3) or inp.intr.shape != (Cn, 9):
        raise ValueError("inconsistent RigInput shapes")
    q = _lib.CRigInput()
    q.n_cameras, q.n_boards, q.n_points = Cn, B, n
    for name in ("worlds", "intr", "has", "Rt", "pix_u", "pix_v"):
        setattr(q, name, getattr(inp, name).ctypes.data)
    out = dict(cam_R=np.zeros((Cn, 3, 3)), cam_t=np.zeros((Cn, 3)), cam_rt=np.zeros((Cn, 6)),
               board_R=np.zeros((B, 3, 3)), board_t=np.zeros((B, 3)), board_rt=np.zeros((B, 6)),
               board_initial=np.zeros(B, dtype=np.uint8), cam_choice=np.zeros(Cn, dtype=np.int32),
               cam_min_error=np.zeros(Cn))
    r = _lib.CRigResult()
    for name in ("cam_R", "cam_t", "cam_rt", "board_R", "board_t", "board_rt", "board_initial", "cam_choice",
                 "cam_min_error"):
        setattr(r, name, out[name].ctypes.data)
    _lib.check(_lib.lib().tscm_rig_init(C.byref(q), device, C.byref(r)))
    out.update(seconds_hypotheses=r.seconds_hypotheses, seconds_total=r.seconds_total,
               n_projections=r.n_projections)
    return out


def stage_errors(inp: RigInput, i: int, Rp, tp, ksplit: int = 0, device: int = 0) -> dict:
    """tscm_rig_stage_errors: stage i of the camera chaining (camera i against camera i-1 posed at Rp, tp) without
    the choice.  Returns the K hypotheses Rs [K,3,3] / ts [K,3], all K summed errors, and the partition the kernels
    ran: jgroups (hypothesis groups of 64), ksplit (board slices; 0 = the host's rule), skew (SKEW instantiation)."""
    inp = inp.normalised()
    Cn, B, n = inp.n_cameras, inp.n_boards, inp.n_points
    if inp.has.shape != (Cn, B) or inp.Rt.shape != (Cn, B, 3, 3) or inp.pix_u.shape != (Cn, B, n) \
            or inp.pix_v.shape != (Cn, B, n) or inp.worlds.shape != (n, 3) or inp.intr.shape != (Cn, 9):
        raise ValueError("inconsistent RigInput shapes")
    K = int(np.count_nonzero(inp.has[i - 1] & inp.has[i])) if 1 <= i < Cn else 0
    q = _lib.CRigInput()
    q.n_cameras, q.n_boards, q.n_points = Cn, B, n
    for name in ("worlds", "intr", "has", "Rt", "pix_u", "pix_v"):
        setattr(q, name, getattr(inp, name).ctypes.data)
    Rp = np.ascontiguousarray(Rp, dtype=np.float64).reshape(9)
    tp = np.ascontiguousarray(tp, dtype=np.float64).reshape(3)
    Rs, ts, err = np.zeros((max(K, 1), 3, 3)), np.zeros((max(K, 1), 3)), np.zeros(max(K, 1))
    info = np.zeros(4, dtype=np.int32)
    _lib.check(_lib.lib().tscm_rig_stage_errors(C.byref(q), int(i), _lib.dptr(Rp), _lib.dptr(tp), int(ksplit), device,
                                                _lib.dptr(Rs), _lib.dptr(ts), _lib.dptr(err),
                                                info.ctypes.data_as(C.POINTER(C.c_int))))
    assert info[0] == K
    return dict(Rs=Rs[:K], ts=ts[:K], err=err[:K], K=K, jgroups=int(info[1]), ksplit=int(info[2]), skew=bool(info[3]))


def problem_from_rig(inp: RigInput, init: dict) -> Problem:
    """The ceres::Problem MultiCalib::calibrate() builds from the constructor's result
    (multi_calib.cpp:157-207): one view per (camera, initialised board) with pixels."""
    Cn, B, n = inp.n_cameras, inp.n_boards, inp.n_points
    cams, boards = np.nonzero(inp.has.astype(bool) & init["board_initial"].astype(bool)[None, :])
    order = np.lexsort((cams, boards))       # board-major like the reference loop (:164-168)
    cams, boards = cams[order], boards[order]
    V = cams.shape[0]
    const = np.zeros(Cn, dtype=np.uint8)
    const[0] = 1
    p = Problem(Cn, B, inp.worlds[:, :2].copy(), cams.astype(np.int32), boards.astype(np.int32),
                (np.arange(V) * n).astype(np.int32), np.full(V, n, dtype=np.int32),
                inp.pix_u[cams, boards].ravel().copy(), inp.pix_v[cams, boards].ravel().copy(),
                init["cam_rt"].copy(), inp.intr.copy(), init["board_rt"].copy(), const, False, meta=dict(inp.meta))
    return p.normalised()


def estimate_focal(pix_u, pix_v, count, board_w: int, board_h: int, cx: float, cy: float, device: int = 0):
    """tscm_estimate_focal (TripleSphereCamera::estimate_focal, TS.cpp:110-168) -> focal, accepted rows."""
    pix_u = np.ascontiguousarray(pix_u, dtype=np.float64)
    pix_v = np.ascontiguousarray(pix_v, dtype=np.float64)
    count = np.ascontiguousarray(count, dtype=np.int32)
    if pix_u.size != count.shape[0] * board_w * board_h or pix_v.size != pix_u.size:
        raise ValueError("pix_u / pix_v must hold n_views * board_w * board_h values")
    focal, used = C.c_double(0.0), C.c_int(0)
    _lib.check(_lib.lib().tscm_estimate_focal(_lib.dptr(pix_u), _lib.dptr(pix_v), count.ctypes.data_as(C.POINTER(C.c_int)),
                                              count.shape[0], board_w, board_h, cx, cy, device,
                                              C.cast(C.byref(focal), C.POINTER(C.c_double)), C.byref(used)))
    return focal.value, used.value


def estimate_focal_rows(pix_u, pix_v, count, board_w: int, board_h: int, cx: float, cy: float, device: int = 0) -> np.ndarray:
    """tscm_estimate_focal_rows -> [n_views, board_h]: the row kernel's output, -1 (image without a board), -2 (row
    rejected) or the sample gamma.  estimate_focal returns the mean and number of the values that are not markers."""
    pix_u = np.ascontiguousarray(pix_u, dtype=np.float64)
    pix_v = np.ascontiguousarray(pix_v, dtype=np.float64)
    count = np.ascontiguousarray(count, dtype=np.int32)
    if pix_u.size != count.shape[0] * board_w * board_h or pix_v.size != pix_u.size:
        raise ValueError("pix_u / pix_v must hold n_views * board_w * board_h values")
    g = np.zeros((count.shape[0], max(board_h, 0)))
    _lib.check(_lib.lib().tscm_estimate_focal_rows(_lib.dptr(pix_u), _lib.dptr(pix_v), count.ctypes.data_as(C.POINTER(C.c_int)),
                                                   count.shape[0], board_w, board_h, cx, cy, device, _lib.dptr(g)))
    return g


def poses_from_Rt(Rt, has=None) -> np.ndarray:
    """tscm_poses_from_r1r2t (TS.cpp:62-74): [n,3,3] [r1 r2 t] -> [n,6] angle-axis + t (host-only)."""
    Rt = np.ascontiguousarray(Rt, dtype=np.float64).reshape(-1, 3, 3)
    rt = np.zeros((Rt.shape[0], 6))
    h = None if has is None else np.ascontiguousarray(has, dtype=np.uint8)
    _lib.check(_lib.lib().tscm_poses_from_r1r2t(_lib.dptr(Rt), None if h is None else h.ctypes.data, Rt.shape[0], _lib.dptr(rt)))
    return rt


def _extrinsic_args(intr, pix_u, pix_v, count, worlds, Rt_init):
    intr = np.ascontiguousarray(intr, dtype=np.float64).reshape(9)
    pix_u = np.ascontiguousarray(pix_u, dtype=np.float64)
    pix_v = np.ascontiguousarray(pix_v, dtype=np.float64)
    count = np.ascontiguousarray(count, dtype=np.int32)
    worlds = np.ascontiguousarray(worlds, dtype=np.float64).reshape(-1, 3)
    V, n = count.shape[0], worlds.shape[0]
    if pix_u.size != V * n or pix_v.size != V * n:
        raise ValueError("pix_u / pix_v must hold n_views * n_points values")
    Rt = np.zeros((V, 3, 3)) if Rt_init is None else np.array(Rt_init, dtype=np.float64).reshape(V, 3, 3)
    return intr, pix_u, pix_v, count, worlds, V, n, Rt


def estimate_extrinsic(intr, pix_u, pix_v, count, worlds, board_w: int, device: int = 0, Rt_init=None):
    """tscm_estimate_extrinsic (TripleSphereCamera::estimate_extrinsic, TS.cpp:170-203, with a deterministic
    planar PnP in place of cv::solvePnPRansac) -> Rt [V,3,3] = [r1 r2 t] per image, number of poses.
    Images without a pose keep Rt_init (a copy; zeros when None)."""
    intr, pix_u, pix_v, count, worlds, V, n, Rt = _extrinsic_args(intr, pix_u, pix_v, count, worlds, Rt_init)
    done = C.c_int(0)
    _lib.check(_lib.lib().tscm_estimate_extrinsic(_lib.dptr(intr), _lib.dptr(pix_u), _lib.dptr(pix_v),
                                                  count.ctypes.data_as(C.POINTER(C.c_int)), V, _lib.dptr(worlds), n, board_w,
                                                  device, _lib.dptr(Rt), C.byref(done)))
    return Rt, done.value


def estimate_extrinsic_stages(intr, pix_u, pix_v, count, worlds, board_w: int, device: int = 0, Rt_init=None) -> dict:
    """tscm_estimate_extrinsic_stages: the launch of estimate_extrinsic with every stage of every image.  Returns
    Rt [V,3,3] and n_estimated as estimate_extrinsic does, T [V,3,3] (look-at turn), H [V,3,3] (homography),
    rv0/t0 [V,3] (pose from the columns), rv/t [V,3] (after Gauss-Newton), steps [V] and code [V]
    (TSCM_EXTRINSIC_*: 1 no board, 2 degenerate board, 3 DLT failed, 4 zero column, 5 converged, 6 iteration
    cap, 7 Gauss-Newton Cholesky failure).  Stages an image does not reach are NaN (steps -1)."""
    intr, pix_u, pix_v, count, worlds, V, n, Rt = _extrinsic_args(intr, pix_u, pix_v, count, worlds, Rt_init)
    T, H, pose0, pose = np.zeros((V, 3, 3)), np.zeros((V, 3, 3)), np.zeros((V, 6)), np.zeros((V, 6))
    steps, code = np.zeros(V, dtype=np.int32), np.zeros(V, dtype=np.int32)
    done = C.c_int(0)
    ip = C.POINTER(C.c_int)
    _lib.check(_lib.lib().tscm_estimate_extrinsic_stages(_lib.dptr(intr), _lib.dptr(pix_u), _lib.dptr(pix_v),
                                                         count.ctypes.data_as(ip), V, _lib.dptr(worlds), n, board_w, device,
                                                         _lib.dptr(Rt), C.byref(done), _lib.dptr(T), _lib.dptr(H),
                                                         _lib.dptr(pose0), _lib.dptr(pose), steps.ctypes.data_as(ip),
                                                         code.ctypes.data_as(ip)))
    return dict(Rt=Rt, n_estimated=done.value, T=T, H=H, rv0=pose0[:, :3], t0=pose0[:, 3:], rv=pose[:, :3], t=pose[:, 3:],
                steps=steps, code=code)


def ransac_params(threshold_px=None, n_hypotheses=None, min_inliers=None, seed=None) -> _lib.CRansacParams:
    """tscm_ransac_params with the library's defaults (8.0 px, 256 hypotheses, min_inliers 0 = max(4, ceil(n / 2)),
    seed 0), the given fields replaced."""
    p = _lib.CRansacParams()
    _lib.lib().tscm_ransac_default_params(C.byref(p))
    if threshold_px is not None:
        p.threshold_px = float(threshold_px)
    if n_hypotheses is not None:
        p.n_hypotheses = int(n_hypotheses)
    if min_inliers is not None:
        p.min_inliers = int(min_inliers)
    if seed is not None:
        p.seed = int(seed)
    return p


def _ransac_call(stages: bool, intr, pix_u, pix_v, count, worlds, board_w, params, device, Rt_init):
    intr, pix_u, pix_v, count, worlds, V, n, Rt = _extrinsic_args(intr, pix_u, pix_v, count, worlds, Rt_init)
    params = ransac_params() if params is None else params
    inlier = np.zeros((V, n), dtype=np.uint8)
    n_inl, code = np.zeros(V, dtype=np.int32), np.zeros(V, dtype=np.int32)
    done, seconds = C.c_int(0), C.c_double(0.0)
    ip = C.POINTER(C.c_int)
    args = [_lib.dptr(intr), _lib.dptr(pix_u), _lib.dptr(pix_v), count.ctypes.data_as(ip), V, _lib.dptr(worlds), n, board_w,
            C.byref(params), device, _lib.dptr(Rt), inlier.ctypes.data_as(C.POINTER(C.c_ubyte)), n_inl.ctypes.data_as(ip),
            code.ctypes.data_as(ip), C.byref(done), C.byref(seconds)]
    out = dict(Rt=Rt, n_inliers=n_inl, code=code)
    if not stages:
        _lib.check(_lib.lib().tscm_estimate_extrinsic_ransac(*args))
    else:
        H = params.n_hypotheses
        samples, score = np.zeros((V, max(H, 0), 4), dtype=np.int32), np.zeros((V, max(H, 0)), dtype=np.int32)
        winner, steps = np.zeros(V, dtype=np.int32), np.zeros(V, dtype=np.int32)
        T, Hb, Hr, pose0, pose, rms = (np.zeros((V, 3, 3)), np.zeros((V, 3, 3)), np.zeros((V, 3, 3)), np.zeros((V, 6)),
                                       np.zeros((V, 6)), np.zeros(V))
        _lib.check(_lib.lib().tscm_estimate_extrinsic_ransac_stages(
            *args, samples.ctypes.data_as(ip), score.ctypes.data_as(ip), winner.ctypes.data_as(ip), _lib.dptr(T), _lib.dptr(Hb),
            _lib.dptr(Hr), _lib.dptr(pose0), _lib.dptr(pose), steps.ctypes.data_as(ip), _lib.dptr(rms)))
        out.update(samples=samples, score=score, winner=winner, T=T, H_best=Hb, H_refit=Hr, rv0=pose0[:, :3], t0=pose0[:, 3:],
                   rv=pose[:, :3], t=pose[:, 3:], steps=steps, rms_px=rms)
    out.update(inlier=inlier.astype(bool), n_estimated=done.value, seconds_kernel=seconds.value)
    return out


def estimate_extrinsic_ransac(intr, pix_u, pix_v, count, worlds, board_w: int, params=None, device: int = 0, Rt_init=None):
    """tscm_estimate_extrinsic_ransac: consensus search over 4-corner homographies and a refit on the winner's inliers
    (definition: tscm.h) -> Rt [V,3,3], inlier [V,n] bool, n_inliers [V], code [V] (TSCM_EXTRINSIC_*, 8 no hypothesis,
    9 few inliers), n_estimated.  A pose is written exactly where code is 5, 6 or 7; other views keep Rt_init (a copy;
    zeros when None).  params: ransac_params(...), None for the defaults."""
    r = _ransac_call(False, intr, pix_u, pix_v, count, worlds, board_w, params, device, Rt_init)
    return r["Rt"], r["inlier"], r["n_inliers"], r["code"], r["n_estimated"]


def estimate_extrinsic_ransac_stages(intr, pix_u, pix_v, count, worlds, board_w: int, params=None, device: int = 0, Rt_init=None) -> dict:
    """tscm_estimate_extrinsic_ransac_stages: the same launch with every stage of every view.  Returns what
    estimate_extrinsic_ransac returns under Rt, inlier, n_inliers, code, n_estimated, and samples [V,H,4] (-1 rejected),
    score [V,H], winner [V], T, H_best, H_refit [V,3,3], rv0/t0, rv/t [V,3], steps [V], rms_px [V], seconds_kernel.
    Stages a view does not reach are NaN (steps -1)."""
    return _ransac_call(True, intr, pix_u, pix_v, count, worlds, board_w, params, device, Rt_init)
