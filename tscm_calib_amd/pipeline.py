"""Image-level flow of the reference's main.cpp on top of the library: monocular_calib (main.cpp:8-130: corner
detection, TripleSphereCamera::calibrate, the refinement pass on the remapped chessboards with the flip rule, second
calibrate) and the rig calibration that follows it (MultiCalib constructor + calibrate, main.cpp:196-319).
Host orchestration only: every numeric step is a call into the C ABI (GPU), nothing is computed here."""
from __future__ import annotations

import numpy as np

from . import api, corners, maps, rig, synth
from . import lib as _l
from .problem import Problem


def board_points(cols: int, rows: int, pitch: float) -> np.ndarray:
    """main.cpp:12-18: (v * size, u * size, 0), v fastest."""
    v, u = np.meshgrid(np.arange(cols), np.arange(rows))
    return np.stack([v.ravel() * pitch, u.ravel() * pitch, np.zeros(cols * rows)], axis=1).astype(np.float64)


MODELS = {"ts": 0, "ds": _l.MODEL_DS, "ucm": _l.MODEL_UCM}


def _model_masks(model: str, fixed, n_cameras: int) -> np.ndarray:
    """[C] mask words of a model ("ts": Triple Sphere, "ds": lambda held at 0, "ucm": xi and lambda held at 0) and the
    caller's held intrinsics (fixed: as for api.calibrate)."""
    if model not in MODELS:
        raise ValueError(f"unknown camera model {model!r}: one of 'ts', 'ds', 'ucm'")
    return _l.fixed_masks(fixed, n_cameras) | np.uint16(MODELS[model])


def _start_in_model(intr: np.ndarray, model: str) -> None:
    """xi / lambda of [..., 9] intrinsics set to 0 where the model holds them there (in place)."""
    if model in ("ds", "ucm"):
        intr[..., 5] = 0.0
    if model == "ucm":
        intr[..., 4] = 0.0


def _prepare_camera(pu, pv, has, cols, rows, pitch, img_size, device=0, init_intr=None, model="ts", ransac=None):
    """calibrate_camera up to its refinement: the start intrinsics, the poses and the mono problem of the refinement.
    ransac: None, or rig.ransac_params(...): the start poses come from rig.estimate_extrinsic_ransac, and a view whose exit
    code is not 5..7 leaves the refinement (count 0).  Returns q, count, sel and None or dict(inlier [V,n], code [V], has [V])."""
    n = cols * rows
    W = board_points(cols, rows, pitch)
    count = (np.asarray(has, dtype=np.int32) * n).astype(np.int32)
    if init_intr is None:
        intr = np.array([0.0, 0.0, img_size[0] / 2 - 0.5, img_size[1] / 2 - 0.5, 0.0, 0.0, 0.5, 0.0, 0.0])
        intr[0] = intr[1] = rig.estimate_focal(pu, pv, count, cols, rows, intr[2], intr[3], device)[0]
    else:
        intr = np.array(init_intr, dtype=np.float64).reshape(9).copy()
    _start_in_model(intr, model)
    found = None
    if ransac is None:
        Rt0, _ = rig.estimate_extrinsic(intr, pu, pv, count, W, cols, device)
    else:
        Rt0, inlier, _, code, _ = rig.estimate_extrinsic_ransac(intr, pu, pv, count, W, cols, ransac, device)
        kept = (code >= 5) & (code <= 7)
        count = np.where(kept, count, 0).astype(np.int32)
        found = dict(inlier=inlier, code=code, has=kept.astype(np.uint8))
    sel = np.flatnonzero(count > 0)
    V = sel.shape[0]
    q = Problem(1, V, W[:, :2].copy(), np.zeros(V, dtype=np.int32), np.arange(V, dtype=np.int32), (np.arange(V) * n).astype(np.int32),
                np.full(V, n, dtype=np.int32), pu[sel].ravel().copy(), pv[sel].ravel().copy(), np.zeros((1, 6)), intr[None, :].copy(),
                rig.poses_from_Rt(Rt0[sel]), np.ones(1, dtype=np.uint8), True).normalised()
    return q, count, sel, found


def _inlier_weights(found, sel, mask_outliers):
    """The corner mask of a prepared camera's refinement: the RANSAC inlier mask of the kept views, or None."""
    if not mask_outliers or found is None:
        return None
    return np.asarray(found["inlier"], dtype=bool)[sel].ravel()


def _finish_camera(q, count, sel):
    """calibrate_camera behind its refinement (TS.cpp:88-102): intr[9] and Rt[V,3,3] = [r1 r2 t] from the refined problem."""
    R = synth.rodrigues(q.board_rt[:, :3])
    Rt = np.zeros((count.shape[0], 3, 3))
    Rt[sel] = np.stack([R[:, :, 0], R[:, :, 1], q.board_rt[:, 3:]], axis=2)
    return q.intr[0].copy(), Rt


def _priors_kw(problem, priors):
    """{} without priors (the calls of a run without them), or priors= for api.refinement / calibrate / covariance: priors is the
    keyword arguments of api.camera_priors (intr_sigma, cam_rt_sigma, pixel_sigma) -- Gaussian priors about the values the
    solve starts from."""
    if priors is None:
        return {}
    if "mean" in priors:
        raise ValueError("pipeline priors are about the start values: give sigmas (intr_sigma, cam_rt_sigma, pixel_sigma), no mean")
    return dict(priors=api.camera_priors(problem, **priors))


PRUNE_DEFAULTS = dict(k=3.0, floor=0.0, max_fraction=0.2, rounds=1, corner_threshold=None, grid=None, angle_bins=0)


def prune_solve(problem, solve, device=0, *, loss=None, weights=None, prune=None, image_size=None) -> dict:
    """Outlier pruning behind a solve of `problem`, `rounds` times: api.residual_report -> api.view_outliers (k,
    floor, max_fraction) and, with corner_threshold, api.corner_outliers -> api.prune_weights -> solve(weights), which solves
    again from the parameters the problem holds, through the weights= path of api.calibrate / api.refinement (a view whose
    weights are all 0 goes in with count 0).  A round that flags nothing ends the loop.  Then one more report, with grid /
    angle_bins if given (grid needs image_size).
    -> weights (None if no round flagged anything and none came in), residuals (the final report), pruned_views [V] bool,
    pruned_corners [N] bool (without the corners of pruned views), prune_rounds (solves made), summaries (theirs).
    There is no rig-connectivity logic: a pruned rig that falls apart shows in the covariance's min_pivot_ratio."""
    opt = dict(PRUNE_DEFAULTS)
    for k_, v in (prune or {}).items():
        if k_ not in opt:
            raise TypeError(f"unknown prune parameter {k_!r}: one of {', '.join(PRUNE_DEFAULTS)}")
        opt[k_] = v
    field = dict(grid=opt["grid"], image_size=image_size if opt["grid"] is not None else None, angle_bins=int(opt["angle_bins"]))
    w = weights
    views, corners, summaries = np.zeros(problem.n_views, dtype=bool), np.zeros(problem.n_corners, dtype=bool), []
    for _ in range(int(opt["rounds"])):
        rep = api.residual_report(problem, device, weights=w, loss=loss)
        fv = api.view_outliers(rep, problem, opt["k"], opt["floor"], opt["max_fraction"])
        fc = api.corner_outliers(rep, opt["corner_threshold"]) if opt["corner_threshold"] is not None else np.zeros(problem.n_corners, dtype=bool)
        fc &= ~np.repeat(fv, problem.view_count)
        if not fv.any() and not fc.any():
            break
        w = api.prune_weights(problem, w, views=fv, corners=fc)
        views |= fv
        corners |= fc
        summaries.append(solve(w))
    final = api.residual_report(problem, device, weights=w, loss=loss, **field)
    return dict(weights=w, residuals=final, pruned_views=views, pruned_corners=corners, prune_rounds=len(summaries), summaries=summaries)


def calibrate_camera(pu, pv, has, cols, rows, pitch, img_size, device=0, init_intr=None, loss=None, model="ts", fixed=None, ransac=None,
                     mask_outliers=False, priors=None, prune=None):
    """TripleSphereCamera::calibrate (TS.cpp:30-105).  Without an initial guess (has_init_guess_ false, :41-51):
    principal point at the image centre, xi = lambda = 0, alpha = 0.5, estimate_focal.  With init_intr (the member
    intrinsic_ after a converged earlier refinement set has_init_guess_, :78) those steps are skipped and only the
    extrinsics are re-estimated (:52).  Then estimate_extrinsic, refinement.
    loss: None (the reference's plain least squares) or (kind, scale) of the refinement, see api.calibrate.
    model: "ts" (Triple Sphere, the reference), "ds" (Double Sphere: lambda starts at 0 and is held there) or "ucm" (Unified
    Camera Model: xi and lambda); fixed: further held intrinsics, as for api.calibrate.
    ransac: None (the poses start from the least-squares fit of all corners), or rig.ransac_params(...): they start from
    rig.estimate_extrinsic_ransac, a view without a pose there (exit code outside 5..7) is left out of the refinement (its Rt
    stays 0), and summary["ransac"] = dict(inlier [V,n] bool, code [V], has [V]: the views that were kept).
    mask_outliers (with ransac): the RANSAC inlier mask of the kept views is the corner mask of the refinement
    (api.refinement(weights=inlier[has])): a corner the consensus set excludes is taken out instead of weighed down.  False: the
    calls of a run without it.
    priors: None, or dict(intr_sigma={"xi": 0.1, ...}[, pixel_sigma=...]): Gaussian priors on the intrinsics about the values the
    refinement starts from (api.camera_priors; the pose of a mono problem is not free, so cam_rt_sigma counts for nothing).
    prune: None (the calls of a run without it), or the parameters of prune_solve: behind the refinement, report -> flag ->
    refine again with the pruned weights; the summary is then the last refinement's and carries residuals, pruned_views,
    pruned_corners (over the kept views) and prune_rounds.
    Returns (intr[9], Rt[V,3,3] = [r1 r2 t], summary)."""
    w = _model_masks(model, fixed, 1)
    q, count, sel, found = _prepare_camera(pu, pv, has, cols, rows, pitch, img_size, device, init_intr, model, ransac)
    cw = _inlier_weights(found, sel, mask_outliers)
    if cw is not None:
        _, summary = api.refinement(q, device, loss=loss, fixed=w if w.any() else None, weights=cw, **_priors_kw(q, priors))
    else:
        _, summary = api.refinement(q, device, loss=loss, fixed=w if w.any() else None, **_priors_kw(q, priors))
    if prune is not None:
        pk = _priors_kw(q, priors)
        pr = prune_solve(q, lambda cw_: api.refinement(q, device, loss=loss, fixed=w if w.any() else None, weights=cw_, **pk)[1], device, loss=loss,
                         weights=cw, prune=prune, image_size=img_size)
        if pr["summaries"]:
            summary = pr["summaries"][-1]
        summary.update(residuals=pr["residuals"], pruned_views=pr["pruned_views"], pruned_corners=pr["pruned_corners"], prune_rounds=pr["prune_rounds"])
    intr, Rt = _finish_camera(q, count, sel)
    if found is not None:
        summary["ransac"] = found
    return intr, Rt, summary


def _calibrate_cameras_batched(pus, pvs, hases, cols, rows, pitch, img_sizes, device, init_intrs, loss, model, masks, ransac=None,
                               mask_outliers=False):
    """calibrate_camera for every camera, the refinements of all of them in ONE batch (api.refinement_batch): the same
    start, poses and post-processing per camera, each camera's refinement as refinement() would return it alone."""
    prep = [_prepare_camera(pu, pv, has, cols, rows, pitch, size, device, init, model, ransac)
            for pu, pv, has, size, init in zip(pus, pvs, hases, img_sizes, init_intrs)]
    cws = [_inlier_weights(p[3], p[2], mask_outliers) for p in prep]
    if any(cw is not None for cw in cws):
        res = api.refinement_batch([p[0] for p in prep], device, loss=loss, fixed=[int(w) for w in masks], weights=cws)
    else:
        res = api.refinement_batch([p[0] for p in prep], device, loss=loss, fixed=[int(w) for w in masks])
    out = []
    for (q, count, sel, found), (_, summary) in zip(prep, res):
        if found is not None:
            summary["ransac"] = found
        out.append(_finish_camera(q, count, sel) + (summary,))
    return out


def _top_left_is_bright(board_img, pitch):
    """main.cpp:76-85: grey values at the centres of the squares (0,0), (1,0), (1,1), (0,1) of the remapped board."""
    g = lambda x, y: int(board_img[int(y), int(x)])
    return g(pitch / 2, pitch / 2) + g(pitch * 3 / 2, pitch * 3 / 2) > g(pitch * 3 / 2, pitch / 2) + g(pitch / 2, pitch * 3 / 2)


def _detect(images, cols, rows, sigma, device, recover="host"):
    """main.cpp:24-50: the grey images, their size, has [V] and the detected corners pu / pv [V, n].  recover: the route of the
    structure recovery (corners.find_chessboards)."""
    n, V = cols * rows, len(images)
    grey = [im if im.ndim == 2 else maps.remap(im, *np.meshgrid(np.arange(im.shape[1], dtype=np.float32), np.arange(im.shape[0], dtype=np.float32)),
                                                to_gray=True, device=device) for im in images]
    img_size = (grey[0].shape[1], grey[0].shape[0])
    has = np.zeros(V, dtype=np.uint8)
    pu, pv = np.zeros((V, n)), np.zeros((V, n))
    for i, pts in enumerate(corners.find_chessboards(grey, cols, rows, sigma=sigma, device=device, recover=recover)):     # one batch
        if pts is not None:
            has[i], pu[i], pv[i] = 1, pts[:, 0], pts[:, 1]
    return img_size, has, pu, pv


def _refine_pixels(images, intr, Rt, has, pu, pv, cols, rows, pitch, sigma, device, recover="host"):
    """main.cpp:59-126, the refinement pass on the remapped chessboards with the flip rule (pu / pv in place)."""
    n = cols * rows
    seen = np.flatnonzero(has)
    board_imgs = []
    for i in seen:
        desc = maps.chessboard_desc(intr, Rt[i], cols, rows, pitch)
        mx, my, _ = maps.build_maps([desc], desc.width * desc.height, device)
        board_imgs.append(maps.remap(images[i], mx.reshape(desc.height, desc.width), my.reshape(desc.height, desc.width), to_gray=images[i].ndim == 3,
                                     device=device))
    # (main.cpp:67: the remapped board is rejected only if NO board came out or board 0 has the wrong shape)
    for i, board_img, pts in zip(seen, board_imgs, corners.find_chessboards(board_imgs, cols, rows, sigma=sigma, device=device, first_board_only=True,
                                                                        recover=recover)):
        if pts is not None:                                                   # :92-105 back through [r1 r2 t] and project()
            P = (Rt[i] @ np.concatenate([pts - pitch, np.ones((n, 1))], axis=1).T).T
            uv = api.project(intr, P, device)
            pu[i], pv[i] = uv[:, 0], uv[:, 1]
        if _top_left_is_bright(board_img, pitch):                             # :72-89 / :107-121 flip rule
            pu[i], pv[i] = pu[i][::-1].copy(), pv[i][::-1].copy()


def monocular_calib(images, cols: int, rows: int, pitch: float, sigma: int = 4, device: int = 0, loss=None, model="ts",
                    fixed=None, ransac=None, mask_outliers=False, priors=None, prune=None, recover="host") -> dict:
    """main.cpp:8-130 for one camera.  images: list of (H, W) uint8 (or (H, W, 3) BGR) arrays, one per frame.
    loss: the robust loss of both refinements (None: plain least squares, as the reference); model, fixed: the camera model
    and held intrinsics of both refinements (calibrate_camera).
    ransac: None, or rig.ransac_params(...) for the start poses of both calibrate() calls (calibrate_camera); a view either
    call drops leaves `has`, and the result carries ransac = the second call's dict(inlier, code, has).
    mask_outliers (with ransac): each of the two refinements takes its own call's inlier mask as its corner mask (calibrate_camera).
    priors: Gaussian priors of both refinements, each about its own start values (calibrate_camera).
    prune: outlier pruning behind the last refinement (calibrate_camera); second then carries residuals, pruned_views, ...
    recover: the structure recovery behind both detections -- "host" (the default: the sequential function per image), "device"
    (all images of a detection in one batch on the GPU) or "host-batch" (that definition on the host); corners.find_chessboards.
    Returns intr, Rt [V,3,3], has [V], pix_u / pix_v [V, n] (refined, flip rule applied), the two LM summaries."""
    img_size, has, pu, pv = _detect(images, cols, rows, sigma, device, recover)
    intr, Rt, first = calibrate_camera(pu, pv, has, cols, rows, pitch, img_size, device, loss=loss, model=model, fixed=fixed,
                                       ransac=ransac, mask_outliers=mask_outliers, priors=priors)                               # :57
    if ransac is not None:
        has = first["ransac"]["has"]
    _refine_pixels(images, intr, Rt, has, pu, pv, cols, rows, pitch, sigma, device, recover)
    # :127 -- the second calibrate() of the same object: a converged first refinement left has_init_guess_ set (TS.cpp:78),
    # so it starts from the first-pass intrinsics and only re-estimates the extrinsics
    warm = intr if first["termination_type"] == 0 else None
    intr, Rt, second = calibrate_camera(pu, pv, has, cols, rows, pitch, img_size, device, init_intr=warm, loss=loss, model=model,
                                        fixed=fixed, ransac=ransac, mask_outliers=mask_outliers, priors=priors, **({} if prune is None else dict(prune=prune)))
    out = dict(intr=intr, Rt=Rt, has=has, pix_u=pu, pix_v=pv, first=first, second=second)
    if ransac is not None:
        out.update(has=second["ransac"]["has"], ransac=second["ransac"])
    return out


def monocular_calib_batch(images_by_camera, cols: int, rows: int, pitch: float, sigma: int = 4, device: int = 0, loss=None,
                          model="ts", masks=None, ransac=None, mask_outliers=False, recover="host") -> list:
    """monocular_calib for every camera, stage by stage across the cameras: detection, the first calibrate, the refinement
    pass, the second calibrate -- each of the two refinements of all cameras in one batch (api.refinement_batch).
    masks: [C] mask words (model included); ransac, mask_outliers, recover: as for monocular_calib.  Returns monocular_calib's dict
    per camera."""
    n_cam = len(images_by_camera)
    masks = np.zeros(n_cam, dtype=np.uint16) if masks is None else masks
    det = [_detect(imgs, cols, rows, sigma, device, recover) for imgs in images_by_camera]
    sizes = [d[0] for d in det]
    has = [d[1] for d in det]
    pu = [d[2] for d in det]
    pv = [d[3] for d in det]
    first = _calibrate_cameras_batched(pu, pv, has, cols, rows, pitch, sizes, device, [None] * n_cam, loss, model, masks, ransac, mask_outliers)
    if ransac is not None:
        has = [f[2]["ransac"]["has"] for f in first]
    for m, imgs in enumerate(images_by_camera):
        _refine_pixels(imgs, first[m][0], first[m][1], has[m], pu[m], pv[m], cols, rows, pitch, sigma, device, recover)
    warm = [f[0] if f[2]["termination_type"] == 0 else None for f in first]
    second = _calibrate_cameras_batched(pu, pv, has, cols, rows, pitch, sizes, device, warm, loss, model, masks, ransac, mask_outliers)
    out = [dict(intr=second[m][0], Rt=second[m][1], has=has[m], pix_u=pu[m], pix_v=pv[m], first=first[m][2], second=second[m][2])
           for m in range(n_cam)]
    if ransac is not None:
        for o in out:
            o.update(has=o["second"]["ransac"]["has"], ransac=o["second"]["ransac"])
    return out


def calibrate_rig(images_by_camera, cols: int, rows: int, pitch: float, sigma: int = 4, device: int = 0, loss=None, model="ts",
                  fixed=None, batch_mono=False, ransac=None, covariance=False, uncertainty=None, mask_outliers=False, priors=None, suggest=None, prune=None,
                  recover="host") -> dict:
    """main.cpp:196-303: monocular_calib per camera, MultiCalib(cameras, worlds), calibrate().  images_by_camera[m][f] is
    the image of frame f in camera m.  Returns the joint problem (intr, cam_rt, board_rt), the per-camera results
    and the LM summary; write the YAML with calib_io.write_calib_yaml.  loss: the robust loss of every solve (None: as the reference).
    model ("ts" | "ds" | "ucm") and fixed (names or a [C] / [C, 9] mask, as for api.calibrate): held in every refinement and in
    the joint solve; the YAML keeps the 9-vector with lambda (and xi) = 0 (calib_io.to_double_sphere / to_ucm convert).
    batch_mono: the per-camera flow stage by stage across the cameras, each of its two refinement passes one batch call for
    all cameras (monocular_calib_batch); False (the default) runs monocular_calib camera after camera.
    ransac: None, or rig.ransac_params(...) for the start poses of every mono calibration (monocular_calib): the views it drops
    are out of `has` when the rig is initialised, and mono[m]["ransac"] holds each camera's masks and codes.
    mask_outliers (with ransac): the RANSAC inlier masks are the corner masks of every refinement that follows -- both mono
    refinements of every camera, the joint solve and the covariance (rig_corner_mask: each view's mask from its camera's second
    calibration; result["corner_mask"] holds the joint problem's).  False: the calls of a run without it.
    covariance: True adds result["covariance"] = api.covariance at the solved parameters, with the loss and masks of the joint
    solve (standard deviations, sigma2, min_pivot_ratio: how well the views determine each parameter).
    uncertainty: None, or dict(step=pixels between grid points, inv_distances=(...)) -- implies covariance and adds
    result["uncertainty"] = api.projection_uncertainty on the grid x, y = 0, step, 2 step, ... of the image, with one observe
    request per camera (at the first inverse distance) and one transfer request per ordered pair of adjacent cameras (m, m + 1
    and back; for three and more cameras also the last and the first) per inverse distance: how many pixels a transferred pixel
    -- and above all its component across the epipolar line -- is uncertain (uncertainty_requests lists them).
    priors: None, or dict(intr_sigma=..., cam_rt_sigma=...[, pixel_sigma=...]) as for api.camera_priors: Gaussian priors of every
    mono refinement (intrinsics), of the joint solve about the values it starts from -- the mono intrinsics and rig_init's poses --
    and, about those same values, of the covariance.  Not with batch_mono (the batched route has no priors): ValueError.
    suggest: None, or dict(n_views=5[, grid, distances, tilts_deg, rolls_deg, pairs, criterion, border, min_corners]) -- implies
    covariance and adds result["suggested_views"] = suggest_views(...): where to hold the board next, by the covariance each
    pose would remove (api.plan_views on the candidates of every camera and of every adjacent pair).
    prune: None (every function runs the calls it ran before), or dict(k=3.0, floor=0.0, max_fraction=0.2, rounds=1,
    corner_threshold=None, grid=None, angle_bins=0) -- behind the joint solve, `rounds` times: api.residual_report -> flag
    (api.view_outliers, api.corner_outliers) -> solve again from the solved parameters with the pruned weights (prune_solve); the
    result carries residuals (the final report, with the grid over the image and the angle bins if asked for), pruned_views,
    pruned_corners, prune_rounds and prune_summaries, summary is the last solve's, and a following covariance uses the pruned
    weights.  There is no rig-connectivity logic: a pruned rig that falls apart shows in the covariance's min_pivot_ratio.
    recover: the structure recovery of every detection of the mono calibrations ("host" | "device" | "host-batch", monocular_calib)."""
    if priors is not None and batch_mono:
        raise ValueError("batch_mono=True has no priors: the batched mono route does not take them")
    n_cam = len(images_by_camera)
    w = _model_masks(model, fixed, n_cam)
    if batch_mono:
        mono = monocular_calib_batch(images_by_camera, cols, rows, pitch, sigma, device, loss=loss, model=model, masks=w, ransac=ransac,
                                     mask_outliers=mask_outliers, recover=recover)
    else:
        mono = [monocular_calib(imgs, cols, rows, pitch, sigma, device, loss=loss, model=model, fixed=np.array([w[m]]), ransac=ransac,
                                mask_outliers=mask_outliers, priors=None if priors is None else {k: v for k, v in priors.items() if k != "cam_rt_sigma"},
                                recover=recover)
                for m, imgs in enumerate(images_by_camera)]
    W = board_points(cols, rows, pitch)
    inp = rig.RigInput(W, np.stack([m["intr"] for m in mono]), np.stack([m["has"] for m in mono]), np.stack([m["Rt"] for m in mono]),
                       np.stack([m["pix_u"] for m in mono]), np.stack([m["pix_v"] for m in mono])).normalised()
    g = rig.rig_init(inp, device)
    problem = rig.problem_from_rig(inp, g)
    _start_in_model(problem.intr, model)
    cw = rig_corner_mask(problem, mono) if mask_outliers and ransac is not None else None
    pk = _priors_kw(problem, priors)        # (about the start values: built before the solve moves them)
    if cw is not None:
        summary = api.calibrate(problem, device, loss=loss, fixed=w if w.any() else None, weights=cw, **pk)
    else:
        summary = api.calibrate(problem, device, loss=loss, fixed=w if w.any() else None, **pk)
    out = dict(problem=problem, mono=mono, rig_init=g, summary=summary)
    if pk:
        out["priors"] = pk["priors"]
    if cw is not None:
        out["corner_mask"] = cw
    if prune is not None:
        img = images_by_camera[0][0]
        pr = prune_solve(problem, lambda cw_: api.calibrate(problem, device, loss=loss, fixed=w if w.any() else None, weights=cw_, **pk), device, loss=loss,
                         weights=cw, prune=prune, image_size=(img.shape[1], img.shape[0]))
        if pr["summaries"]:
            out["summary"] = pr["summaries"][-1]
            cw = pr["weights"]
        out.update(residuals=pr["residuals"], pruned_views=pr["pruned_views"], pruned_corners=pr["pruned_corners"], prune_rounds=pr["prune_rounds"],
                   prune_summaries=pr["summaries"])
    if covariance or uncertainty is not None or suggest is not None:
        if cw is not None:
            out["covariance"] = api.covariance(problem, device, loss=loss, fixed=w if w.any() else None, weights=cw, **pk)
        else:
            out["covariance"] = api.covariance(problem, device, loss=loss, fixed=w if w.any() else None, **pk)
    if uncertainty is not None:
        step = float(uncertainty["step"])
        img_w, img_h = images_by_camera[0][0].shape[1], images_by_camera[0][0].shape[0]
        grid = api.uncertainty_grid(int((img_w - 1) // step) + 1, int((img_h - 1) // step) + 1, 0.0, 0.0, step, step, img_w, img_h)
        out["uncertainty"] = api.projection_uncertainty(problem.cam_rt, problem.intr, out["covariance"], uncertainty_requests(n_cam, uncertainty["inv_distances"]),
                                                        grid, device)
    if suggest is not None:
        img_w, img_h = images_by_camera[0][0].shape[1], images_by_camera[0][0].shape[0]
        out["suggested_views"] = suggest_views(problem, out["covariance"], (img_w, img_h), device=device, **suggest)
    return out


def suggest_views(problem: Problem, cov: dict, image_size, n_views: int = 5, grid=(6, 4), distances=None, tilts_deg=(0.0, 25.0, -25.0), rolls_deg=(0.0,),
                  pairs=True, criterion: str = "gain_logdet", border: float = 0.0, min_corners: int = 8, device: int = 0) -> list:
    """Greedy next-best views of a calibrated rig (api.plan_views): the candidates are api.view_candidates of every camera
    alone and, with pairs, of every camera together with the next one (for three and more cameras also the last with the
    first).  distances: None takes 5 and 10 board diagonals.  -> a list of dict(camera_a, camera_b, board_rt, pixel, distance,
    tilt_x, tilt_y, roll, gain_logdet, gain_trace, n_visible, flags), one per chosen view, in the order they were chosen."""
    xy = np.asarray(problem.board_xy, dtype=np.float64)
    if distances is None:
        diag = float(np.sqrt(np.sum((xy.max(axis=0) - xy.min(axis=0)) ** 2)))
        distances = (5.0 * diag, 10.0 * diag)
    C = problem.n_cameras
    cands, info = [], []
    for m in range(C):
        partners = [None] + ([(m + 1) % C] if pairs and C > 1 and (m + 1 < C or C > 2) else [])
        for b in partners:
            c, i = api.view_candidates(problem.cam_rt, problem.intr, m, image_size, xy, grid, distances, tilts_deg, rolls_deg, pair=b)
            cands += c
            info += i
    steps = api.plan_views(problem.cam_rt, problem.intr, cov, xy, image_size, cands, n_views=n_views, criterion=criterion, border=border,
                           min_corners=min_corners, device=device)
    return [dict(info[s["index"]], camera_a=s["candidate"][0], camera_b=s["candidate"][1], board_rt=s["candidate"][2], gain_logdet=s["gain_logdet"],
                 gain_trace=s["gain_trace"], n_visible=s["n_visible"], flags=s["flags"]) for s in steps]


def rig_corner_mask(problem: Problem, mono) -> np.ndarray:
    """The corner mask of the joint problem (rig.problem_from_rig) from the per-camera results of monocular_calib with ransac:
    view (camera m, board i) takes mono[m]["ransac"]["inlier"][i], in the problem's corner order."""
    return np.concatenate([np.asarray(mono[m]["ransac"]["inlier"], dtype=bool)[i][:c]
                           for m, i, c in zip(problem.view_camera, problem.view_board, problem.view_count)]) if problem.n_views else np.zeros(0, dtype=bool)


def uncertainty_requests(n_cameras: int, inv_distances) -> list:
    """The requests of calibrate_rig(uncertainty=...): an observe request per camera, then per inverse distance a transfer
    request per ordered adjacent pair."""
    inv = [float(i) for i in inv_distances]
    pairs = [(m, m + 1) for m in range(n_cameras - 1)] + ([(n_cameras - 1, 0)] if n_cameras > 2 else [])
    req = [(m, m, inv[0]) for m in range(n_cameras)]
    for i in inv:
        for a, b in pairs:
            req += [(a, b, i), (b, a, i)]
    return req
