"""Host-side mirror of the reference's interface for the LM hot path, on top of the C ABI.

Reference                                              here
---------------------------------------------------    -----------------------------------------
TripleSphereCamera::refinement (TS.cpp:247-282)        refinement(problem)  -> bool, summary
MultiCalib::calibrate (multi_calib.cpp:155-232)        calibrate(problem)   -> summary
ReprojectionError functors via AutoDiffCostFunction    evaluate_functor(problem)
(TS.h:93-134, multi_calib.h:138-199)
TripleSphereCamera::project (TS.cpp:332-344)           project(intr, points)
get_unit_sphere_coordinate (TS.h:39-57)                unproject(intr, pixels)
error report (multi_calib.cpp:233-283)                 reprojection_error(problem)
AddResidualBlock(..., new ceres::HuberLoss(a), ...)    loss=("huber", a); Solver.set_loss("huber", a)
SetManifold(intrinsic_, new SubsetManifold(9, {..}))   fixed=("cx", "cy"); Solver.set_fixed_intrinsics(...)
AddResidualBlock(new NormalPrior(A, mean), NULL, x)    priors=camera_priors(problem, intr_sigma={"xi": 0.1})

Everything computes on the GPU through libtscm_hip.so; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _l
from .problem import Problem


class Solver:
    """RAII wrapper of tscm_solver (problem uploaded once, parameters in/out per solve)."""

    def __init__(self, problem: Problem, device: int = 0, rank: int = 0, world: int = 1, *, weights=None, priors=None):
        """rank / world: frame-sharded solve -- every rank passes the same WHOLE problem and keeps the boards it owns
        (tscm_solver_create_sharded); attach a communicator with set_comm() before solving.
        weights (default: problem.weights): corner weights as for set_corner_weights(); a view whose weights are all 0 is
        created with view_count 0.
        priors: camera priors as for set_camera_priors()."""
        self.problem = problem.normalised() if not _is_normalised(problem) else problem
        self.problem.validate()
        self._built, w = _l.corner_weights(self.problem, weights)
        self._cp = _l.c_problem(self._built)
        self._h = C.c_void_p()
        self.rank, self.world = rank, world
        _l.check(_l.lib().tscm_solver_create_sharded(C.byref(self._cp), device, rank, world, C.byref(self._h)))
        self._comm = None
        if w is not None:
            _l.check(_l.lib().tscm_solver_set_corner_weights(self._h, _l.dptr(w)))
        if priors is not None:
            self.set_camera_priors(priors)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _l.lib().tscm_solver_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_comm(self, comm: "Comm | None"):
        self._comm = comm
        _l.check(_l.lib().tscm_solver_set_comm(self._h, comm._h if comm else None))

    def set_loss(self, kind, scale: float = 1.0):
        """The robust loss of every later solve / solve_resident (tscm_solver_set_loss): kind "huber" | "soft_l1" |
        "cauchy" with its scale in pixels -- Ceres' HuberLoss(scale) etc. on every corner -- or None for plain least squares."""
        k, a = _l.loss_args(None if kind is None else (kind, scale))
        _l.check(_l.lib().tscm_solver_set_loss(self._h, k, a))

    def set_corner_weights(self, weights):
        """The corner weights of every later solve / solve_resident (tscm_solver_set_corner_weights): [n_corners] of the
        problem in corner order -- views in order, the corners of a view in order -- a bool mask meaning 0 / 1, or None for
        none.  Ceres' ScaledLoss per residual block; weight 0 takes the corner out, and its observation may hold anything.
        A view whose weights are all 0 must have been created with view_count 0 (pass weights= to the constructor): ValueError
        otherwise.  The solver keeps the views it was created with: on one created without some views, later weights for them
        are not used, and None is the solve without weights of the views it has, not of the whole problem."""
        if weights is None:
            _l.check(_l.lib().tscm_solver_set_corner_weights(self._h, None))
            return
        _, w = _l.corner_weights(self.problem, weights, self._built.view_count)
        _l.check(_l.lib().tscm_solver_set_corner_weights(self._h, _l.dptr(w)))

    def set_fixed_intrinsics(self, fixed):
        """The held intrinsics of every later solve / solve_resident (tscm_solver_set_fixed_intrinsics): None, names such as
        ("cx", "cy") for every camera, a [C] int array of TSCM_FIX_* words or a [C, 9] bool array (lib.fixed_masks)."""
        w = _l.fixed_masks(fixed, self.problem.n_cameras)
        _l.check(_l.lib().tscm_solver_set_fixed_intrinsics(self._h, _l.ushort_ptr(w)))

    def set_camera_priors(self, priors):
        """The Gaussian priors of every later solve / solve_resident (tscm_solver_set_camera_priors): a lib.CameraPriors
        (camera_priors() builds one) or None for none.  Ceres' NormalPrior per coordinate: the objective gains
        1/2 sum w (x - mean)^2; a weight on a coordinate that is not free (held, constant, b, c) counts as 0.  The library
        copies the arrays.  Not served on a sharded solver (world > 1)."""
        ptr, keep = _l.priors_ptr(priors, self.problem.n_cameras)
        _l.check(_l.lib().tscm_solver_set_camera_priors(self._h, ptr))
        del keep

    def debug_withhold_handoff(self, on=True):
        """Tests only: one producer of the device-side hand-off of the NEXT solve never reports in (tscm_solver_debug_withhold_handoff);
        on = 2: ... and the library must not run that solve again on separate launches; on = 3: like 1 for a reduction that rides in
        the Schur-complement launch."""
        _l.check(_l.lib().tscm_solver_debug_withhold_handoff(self._h, int(on)))

    def debug_schur_rot(self, rot=0):
        """Tests only: every Schur-complement workgroup of the later solves starts its deal of board groups at wave 0 or 2
        (tscm_solver_debug_schur_rot; 0 is the default).  The bits must not depend on it."""
        _l.check(_l.lib().tscm_solver_debug_schur_rot(self._h, int(rot)))

    def debug_reduced_backsub(self, on=True):
        """Tests and A/B runs only: the later solves of a rig of up to four cameras back-substitute behind the reduced system's
        factorisation instead of taking the step out of it (tscm_solver_debug_reduced_backsub; off is the default)."""
        _l.check(_l.lib().tscm_solver_debug_reduced_backsub(self._h, int(bool(on))))

    def reruns(self) -> int:
        """Solves of this solver that were run again on separate launches after a late device-side hand-off."""
        n = _l.lib().tscm_solver_reruns(self._h)
        if n < 0:
            _l.check(n)
        return n

    def solve(self, **options) -> dict:
        """ceres::Solve equivalent: in/out through problem.cam_rt / intr / board_rt."""
        o = _l.default_options(self.problem.mono, **options)
        s = _l.CSummary()
        _l.check(_l.lib().tscm_solver_solve(self._h, C.byref(o), C.byref(s)))
        return _l.summary_dict(s)

    def upload_params(self, cam_rt=None, intr=None, board_rt=None):
        p = self.problem
        cam_rt = p.cam_rt if cam_rt is None else np.ascontiguousarray(cam_rt, dtype=np.float64)
        intr = p.intr if intr is None else np.ascontiguousarray(intr, dtype=np.float64)
        board_rt = p.board_rt if board_rt is None else np.ascontiguousarray(board_rt, dtype=np.float64)
        _l.check(_l.lib().tscm_solver_upload_params(self._h, _l.dptr(cam_rt), _l.dptr(intr), _l.dptr(board_rt)))

    def solve_resident(self, reset: bool = True, **options) -> dict:
        o = _l.default_options(self.problem.mono, **options)
        s = _l.CSummary()
        _l.check(_l.lib().tscm_solver_solve_resident(self._h, C.byref(o), C.byref(s), 1 if reset else 0))
        return _l.summary_dict(s)

    def download_params(self):
        p = self.problem
        cam, intr, board = np.zeros_like(p.cam_rt), np.zeros_like(p.intr), np.zeros_like(p.board_rt)
        if p.mono:
            cam[:] = p.cam_rt
        _l.check(_l.lib().tscm_solver_download_params(self._h, _l.dptr(cam), _l.dptr(intr), _l.dptr(board)))
        return cam, intr, board

    def gather_boards(self):
        """Complete board_rt on every rank after a sharded solve_resident (tscm_solver_gather_boards)."""
        board = self.problem.board_rt.copy()
        _l.check(_l.lib().tscm_solver_gather_boards(self._h, _l.dptr(board)))
        return board

    def kernel_time(self, enable=True):
        """(timed launches, total_ms) of the dominant kernel since the last call; (re)arms the HIP-event timers:
        enable = False / 0 off, True / 1 every launch, n every n-th launch."""
        n, ms = C.c_int(0), C.c_double(0.0)
        _l.check(_l.lib().tscm_solver_kernel_time(self._h, int(enable), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def exchange_time(self):
        """((timed, total_ms) of the all-reduce of T, (timed, total_ms) of the all-reduce of H_stage) since the last call;
        sampled at kernel_time()'s rate.  Zeros without a communicator."""
        nt, nh, mt, mh = C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        _l.check(_l.lib().tscm_solver_exchange_time(self._h, C.byref(nt), C.byref(mt), C.byref(nh), C.byref(mh)))
        return (nt.value, mt.value), (nh.value, mh.value)


class Comm:
    """Communicator of a frame-sharded solve: RCCL (one process per GPU: the constructor), the in-process group
    (`local_group`), or the IPC back-end (`ipc`: one process per rank, ranks may share a device)."""

    def __init__(self, unique_id: bytes | None, rank: int, world: int, device: int, _handle=None):
        self._h = C.c_void_p()
        self.rank, self.world = rank, world
        if _handle is not None:
            self._h = _handle
            return
        buf = (C.c_ubyte * _l.UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        _l.check(_l.lib().tscm_comm_create(buf, rank, world, device, C.byref(self._h)))

    @staticmethod
    def local_group(world: int, device: int = 0) -> "list[Comm]":
        """The communicators of an in-process group on one device (tscm_comm_create_local)."""
        hs = (C.c_void_p * world)()
        _l.check(_l.lib().tscm_comm_create_local(world, device, hs))
        return [Comm(None, r, world, device, _handle=C.c_void_p(hs[r])) for r in range(world)]

    @staticmethod
    def ipc(rank: int, world: int, device: int, allgather, n_cameras: int = 32) -> "Comm":
        """Communicator of the IPC back-end (tscm_comm_ipc_open / _connect): one process per rank, the ranks may
        share a device.  `allgather(bytes) -> list[bytes]` is the caller's side channel (every rank calls it once, with
        its TSCM_IPC_HANDLE_BYTES-byte handle; it returns all ranks' handles in rank order).  `n_cameras`: upper bound of the rigs this
        communicator will serve (sizes the exchange slots: 256 doubles per camera-pair block)."""
        h = C.c_void_p()
        mine = (C.c_ubyte * _l.IPC_HANDLE_BYTES)()
        max_doubles = 256 * max(n_cameras * (n_cameras + 1) // 2, n_cameras) + 8 + world
        _l.check(_l.lib().tscm_comm_ipc_open(rank, world, device, max_doubles, C.byref(h), mine))
        note = _l.lib().tscm_last_error().decode(errors="replace")      # (which kind of memory the exchange buffer got)
        c = Comm(None, rank, world, device, _handle=h)
        c.note = note
        handles = allgather(bytes(mine))
        if len(handles) != world or any(len(x) != _l.IPC_HANDLE_BYTES for x in handles):
            raise RuntimeError(f"allgather must return one {_l.IPC_HANDLE_BYTES}-byte handle per rank")
        buf = (C.c_ubyte * (_l.IPC_HANDLE_BYTES * world)).from_buffer_copy(b"".join(handles))
        _l.check(_l.lib().tscm_comm_ipc_connect(c._h, buf))
        return c

    def backend_ranks(self) -> int:
        """Number of ranks the exchange back-end itself reports (ncclCommCount for RCCL)."""
        n = C.c_int(0)
        _l.check(_l.lib().tscm_comm_info(self._h, None, None, C.byref(n)))
        return n.value

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_ubyte * _l.UNIQUE_ID_BYTES)()
        _l.check(_l.lib().tscm_comm_unique_id(buf))
        return bytes(buf)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _l.lib().tscm_comm_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


class Group:
    """`world` shards of one problem on ONE device, solved in lock step with the in-process exchange
    (tscm_comm_create_local + tscm_solver_solve_group): the frame-sharded solver without RCCL, e.g. on a one-GPU box."""

    def __init__(self, problem: Problem, world: int, device: int = 0, *, loss=None, fixed=None, weights=None):
        """loss: None, or (kind, scale) as for calibrate(); every shard carries it (Solver.set_loss).
        fixed: held intrinsics as for calibrate(); every shard holds them (Solver.set_fixed_intrinsics).
        weights (default: problem.weights): corner weights as for calibrate(); every shard takes the whole array and keeps
        its own views' part."""
        self.problem = problem.normalised() if not _is_normalised(problem) else problem
        self.world = world
        self.comms = Comm.local_group(world, device)
        self.solvers = [Solver(self.problem, device, r, world, weights=weights) for r in range(world)]
        for s, c in zip(self.solvers, self.comms):
            s.set_comm(c)
        if loss is not None:
            k, a = _l.loss_args(loss)
            for s in self.solvers:
                _l.check(_l.lib().tscm_solver_set_loss(s._h, k, a))
        if fixed is not None:
            for s in self.solvers:
                s.set_fixed_intrinsics(fixed)

    def solve(self, **options) -> "list[dict]":
        """In/out through the problem's arrays, like Solver.solve; returns one summary per rank."""
        for s in self.solvers:
            s.upload_params()
        out = self.solve_resident(reset=True, **options)
        p = self.problem
        cam, intr, _ = self.solvers[0].download_params()
        if not p.mono:
            p.cam_rt[:] = cam
        p.intr[:] = intr
        for s in self.solvers:                                  # every rank writes the boards it owns
            _l.check(_l.lib().tscm_solver_download_params(s._h, None, None, _l.dptr(p.board_rt)))
        return out

    def solve_resident(self, reset: bool = True, **options) -> "list[dict]":
        o = _l.default_options(self.problem.mono, **options)
        hs = (C.c_void_p * self.world)(*[s._h for s in self.solvers])
        sums = (_l.CSummary * self.world)()
        _l.check(_l.lib().tscm_solver_solve_group(hs, self.world, C.byref(o), sums, 1 if reset else 0))
        return [_l.summary_dict(sums[r]) for r in range(self.world)]

    def close(self):
        for s in self.solvers:
            s.close()
        for c in self.comms:
            c.close()
        self.solvers, self.comms = [], []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def debug_reduced_backsub_default(on=True):
    """Tests and A/B runs only: Solver.debug_reduced_backsub for every solver created from now on, those of the one-shot
    entry points (calibrate, step, ...) among them.  Set it back to off afterwards."""
    _l.check(_l.lib().tscm_solver_debug_reduced_backsub(None, int(bool(on))))


def _is_normalised(p: Problem) -> bool:
    ok = lambda a, dt: isinstance(a, np.ndarray) and a.dtype == dt and a.flags["C_CONTIGUOUS"]
    return (all(ok(getattr(p, n), np.float64) for n in ("board_xy", "obs_u", "obs_v", "cam_rt", "intr", "board_rt"))
            and all(ok(getattr(p, n), np.int32) for n in ("view_camera", "view_board", "view_offset", "view_count"))
            and ok(p.cam_pose_constant, np.uint8)
            and (p.board_pose_constant is None or ok(p.board_pose_constant, np.uint8)))


def camera_priors(problem: Problem, intr_sigma=None, cam_rt_sigma=None, mean=None, pixel_sigma: float = 1.0) -> "_l.CameraPriors":
    """Priors "about this value, give or take sigma" for calibrate(), refinement(), Solver, ... (priors=).
    intr_sigma: {intrinsic name: sigma} for every camera (lib.INTRINSIC_NAMES: fx fy cx cy xi lambda alpha), or a [C, 9] array
    of sigmas with 0, inf or NaN for "no prior"; cam_rt_sigma: a scalar for all six pose coordinates of every camera, a [6] or
    a [C, 6] array, same convention.  Weight = (pixel_sigma / sigma)^2: with pixel_sigma the standard deviation of a corner in
    pixels the prior and the corners are weighted as their variances ask.  mean: None for the problem's current values, or a
    dict with "intr" [C, 9] and / or "cam_rt" [C, 6]."""
    Cn = problem.n_cameras
    mean = mean or {}

    def weights(sig, per):
        s = np.broadcast_to(np.asarray(sig, dtype=np.float64), (Cn, per)).copy()
        if np.any(s < 0.0):
            raise ValueError("a prior's sigma must not be negative")
        w = np.zeros((Cn, per))
        ok = np.isfinite(s) & (s > 0.0)
        w[ok] = (float(pixel_sigma) / s[ok]) ** 2
        return w

    iw = cw = im = cm = None
    if intr_sigma is not None:
        if isinstance(intr_sigma, dict):
            sig = np.zeros((Cn, 9))
            for name, v in intr_sigma.items():
                if name not in _l.INTRINSIC_NAMES:
                    raise ValueError(f"unknown intrinsic {name!r}: one of {', '.join(_l.INTRINSIC_NAMES)}")
                sig[:, _l.INTRINSIC_NAMES.index(name)] = float(v)
            intr_sigma = sig
        iw = weights(intr_sigma, 9)
        im = np.array(mean.get("intr", problem.intr), dtype=np.float64).reshape(Cn, 9)
    if cam_rt_sigma is not None:
        cw = weights(cam_rt_sigma, 6)
        cm = np.array(mean.get("cam_rt", problem.cam_rt), dtype=np.float64).reshape(Cn, 6)
    return _l.CameraPriors(cm, cw, im, iw)


def calibrate(problem: Problem, device: int = 0, *, loss=None, fixed=None, weights=None, priors=None, **options) -> dict:
    """The Ceres block of MultiCalib::calibrate() (multi_calib.cpp:157-218): joint LM over
    camera poses, board poses and intrinsics, in place on `problem`.  Like the reference,
    the outcome is not turned into an error -- inspect summary['termination'].
    loss: None (the reference's NULL loss), or (kind, scale) with kind "huber" | "soft_l1" | "cauchy"
    and scale in pixels: Ceres' HuberLoss(scale) etc. on every corner (tscm_solve_robust).
    fixed: intrinsics held at their start values (tscm_solve_fixed) -- None, names such as ("cx", "cy") for every
    camera, a [C] int array of TSCM_FIX_* words (lib.FIX, lib.MODEL_DS, ...) or a [C, 9] bool array.
    weights (default: problem.weights): [n_corners] corner weights in corner order, a bool mask meaning 0 / 1 -- Ceres'
    ScaledLoss per residual block; weight 0 takes the corner out, whatever its observation holds (tscm_solve_weighted).
    A view whose weights are all 0 goes in with view_count 0.
    priors: None, or Gaussian priors on camera parameters (camera_priors(), tscm_solve_prior)."""
    if problem.mono:
        raise ValueError("calibrate() is the multi-camera solve; use refinement() for a mono problem")
    assert _is_normalised(problem), "use Problem.normalised()"
    o = _l.default_options(False, **options)
    s = _l.CSummary()
    q, w = _l.corner_weights(problem, weights)
    cp = _l.c_problem(q)
    _select(device)
    _solve_one_shot(cp, o, s, loss, fixed, problem.n_cameras, w, priors)
    return _l.summary_dict(s)


def refinement(problem: Problem, device: int = 0, *, loss=None, fixed=None, weights=None, priors=None, **options):
    """TripleSphereCamera::refinement (TS.cpp:247-282): returns (converged, summary) where
    converged == (termination_type == CONVERGENCE), the reference's return value (:281).
    loss, fixed, weights, priors: as for calibrate()."""
    if not problem.mono:
        raise ValueError("refinement() is the mono solve")
    assert _is_normalised(problem), "use Problem.normalised()"
    o = _l.default_options(True, **options)
    s = _l.CSummary()
    q, w = _l.corner_weights(problem, weights)
    cp = _l.c_problem(q)
    _select(device)
    _solve_one_shot(cp, o, s, loss, fixed, problem.n_cameras, w, priors)
    d = _l.summary_dict(s)
    return d["termination_type"] == 0, d


def refinement_batch(problems, device: int = 0, *, loss=None, fixed=None, weights=None, priors=None, **options):
    """n TripleSphereCamera::refinement solves (TS.cpp:247-282) in one batch on one device (tscm_solve_mono_batch):
    returns [(converged, summary), ...] in problem order, each as refinement() would return it for that problem alone.
    Parameters are updated in place.  loss: shared, as for refinement(); fixed: None, or one mask per problem (anything
    fixed_masks takes for one camera: an int, names, a [9] bool array, or None); weights: None (then each problem's own
    .weights), or one entry per problem, each as for refinement() or None (tscm_solve_mono_batch_weighted).
    priors: the batched route has none (tscm_solve_mono_batch* takes no priors argument) -- anything but None raises ValueError
    here, in the Python layer; solve such problems one by one with refinement()."""
    if priors is not None:
        raise ValueError("refinement_batch: the batched mono route has no camera priors (use refinement() per problem)")
    problems = list(problems)
    if not problems:
        raise ValueError("refinement_batch() needs at least one problem")
    for p in problems:
        if not p.mono:
            raise ValueError("refinement_batch() takes mono problems only")
        assert _is_normalised(p), "use Problem.normalised()"
    n = len(problems)
    o = _l.default_options(True, **options)
    if weights is not None and len(weights) != n:
        raise ValueError("weights: one entry per problem")
    built = [_l.corner_weights(p, None if weights is None else weights[i]) for i, p in enumerate(problems)]
    ws = [w for _, w in built]
    cps = (_l.CProblem * n)(*[_l.c_problem(q) for q, _ in built])
    sums = (_l.CSummary * n)()
    if fixed is None:
        w = None
    else:
        if len(fixed) != n:
            raise ValueError("fixed: one mask per problem")
        w = np.array([_l.fixed_masks(f, 1)[0] for f in fixed], dtype=np.uint16)
    k, a = _l.loss_args(loss)
    dp = C.POINTER(C.c_double)
    wp = (dp * n)(*[_l.dptr(x) if x is not None else dp() for x in ws])
    _l.check(_l.lib().tscm_solve_mono_batch_weighted(cps, n, device, C.byref(o), None if w is None else _l.ushort_ptr(w), wp, k, a, sums))
    out = []
    for i in range(n):
        d = _l.summary_dict(sums[i])
        out.append((d["termination_type"] == 0, d))
    return out


def _solve_one_shot(cp, o, s, loss, fixed, n_cameras, weights=None, priors=None):
    # the most general export; None where nothing is set (tscm_solve_multi / _mono / _robust / _fixed / _weighted wrap the same path)
    w = None if fixed is None else _l.fixed_masks(fixed, n_cameras)
    k, a = _l.loss_args(loss)
    pr, keep = _l.priors_ptr(priors, n_cameras)
    _l.check(_l.lib().tscm_solve_prior(C.byref(cp), C.byref(o), _l.dptr(weights), None if w is None else _l.ushort_ptr(w), k, a, pr, C.byref(s)))
    del keep


def _select(device: int):
    # the one-shot entry points run on the calling thread's current HIP device (device 0 unless
    # the host program selected another one); use Solver(problem, device) to pick a device.
    if device != 0:
        raise ValueError("one-shot calibrate()/refinement() use the current device; use Solver(problem, device)")


def evaluate_functor(problem: Problem, device: int = 0, jacobians: bool = True):
    """-> cost, residuals [N,2], (J_cam [N,2,6], J_board [N,2,6], J_intr [N,2,9])."""
    assert _is_normalised(problem)
    N = problem.n_corners
    res = np.zeros((N, 2))
    cost = C.c_double(0.0)
    cp = _l.c_problem(problem)
    if jacobians:
        Jc, Jb, Ji = np.zeros((N, 2, 6)), np.zeros((N, 2, 6)), np.zeros((N, 2, 9))
        _l.check(_l.lib().tscm_eval_functor(C.byref(cp), device, _l.dptr(res), _l.dptr(Jc), _l.dptr(Jb), _l.dptr(Ji), C.byref(cost)))
        return cost.value, res, Jc, Jb, Ji
    _l.check(_l.lib().tscm_eval_functor(C.byref(cp), device, _l.dptr(res), None, None, None, C.byref(cost)))
    return cost.value, res


def normal_equations(problem: Problem, device: int = 0, *, jacobian_fp32: int = 0, exec_flags: int = 0, loss=None,
                     as_solved: bool = False, weights=None, priors=None) -> dict:
    """Schur-form normal equations (unscaled) from the Gram kernel a solve with these options runs:
    k_eval_gram4 by default, k_eval_gram_f32 with jacobian_fp32=1, k_eval_gram with exec_flags=EXEC_GRAM_16X16.
    loss (as for calibrate()): the corrected equations of a robust solve, cost = sum rho / 2.
    as_solved: the evaluation launch exactly as a solve makes it, on a fresh solver (tscm_solver_eval_normal_equations):
    k_eval_gram4 forms no rotation columns for a camera whose pose block is constant, and those entries are 0.
    weights (default: problem.weights): corner weights as for calibrate() -- the equations of the rows scaled by
    sqrt(omega rho'), cost = sum omega rho / 2 (tscm_eval_normal_equations_weighted).
    priors: camera priors as for calibrate() -- w on the diagonal of cam_gram, w (x - mean) in cam_grad, 1/2 w (x - mean)^2 in
    the cost, on every column that can be free (tscm_eval_normal_equations_prior); the board blocks do not change."""
    assert _is_normalised(problem)
    q, w = _l.corner_weights(problem, weights)
    Cn, B, V = problem.n_cameras, problem.n_boards, problem.n_views
    out = dict(board_gram=np.zeros((B, 6, 6)), board_grad=np.zeros((B, 6)), view_cross=np.zeros((V, 6, 15)),
               cam_gram=np.zeros((Cn, 15, 15)), cam_grad=np.zeros((Cn, 15)))
    cost = C.c_double(0.0)
    cp = _l.c_problem(q)
    o = _l.default_options(problem.mono, jacobian_fp32=jacobian_fp32, exec_flags=exec_flags)
    outs = (_l.dptr(out["board_gram"]), _l.dptr(out["board_grad"]), _l.dptr(out["view_cross"]),
            _l.dptr(out["cam_gram"]), _l.dptr(out["cam_grad"]), C.byref(cost))
    if as_solved:
        with Solver(problem, device, weights=weights, priors=priors) as s:
            if loss is not None:
                s.set_loss(*((loss,) if isinstance(loss, str) else loss))
            _l.check(_l.lib().tscm_solver_eval_normal_equations(s._h, C.byref(o), 1, *outs))
    else:
        k, a = _l.loss_args(loss)
        pr, keep = _l.priors_ptr(priors, Cn)
        _l.check(_l.lib().tscm_eval_normal_equations_prior(C.byref(cp), device, C.byref(o), _l.dptr(w), k, a, pr, *outs))
        del keep
    out["cost"] = cost.value
    return out


def step(problem: Problem, device: int = 0, *, loss=None, fixed=None, weights=None, priors=None, **options) -> dict:
    """The candidate point of the first trust-region step a solve with these options takes (tscm_eval_step_ex), at the
    problem's parameters, which stay as they are: cam_rt, intr, board_rt (x + delta as that solve evaluates it), valid
    (False: the linear solve failed) and the one-iteration summary.  loss: as for calibrate() (tscm_eval_step_robust);
    fixed: held intrinsics as for calibrate() (tscm_eval_step_fixed); weights: corner weights as for calibrate()
    (tscm_eval_step_weighted); priors: camera priors as for calibrate() (tscm_eval_step_prior)."""
    assert _is_normalised(problem)
    q, cw = _l.corner_weights(problem, weights)
    cam, intr, board = np.zeros_like(problem.cam_rt), np.zeros_like(problem.intr), np.zeros_like(problem.board_rt)
    valid = C.c_int(0)
    s = _l.CSummary()
    cp = _l.c_problem(q)
    o = _l.default_options(problem.mono, **options)
    outs = (_l.dptr(cam), _l.dptr(intr), _l.dptr(board), C.byref(valid), C.byref(s))
    w = None if fixed is None else _l.fixed_masks(fixed, problem.n_cameras)
    k, a = _l.loss_args(loss)
    pr, keep = _l.priors_ptr(priors, problem.n_cameras)
    _l.check(_l.lib().tscm_eval_step_prior(C.byref(cp), device, C.byref(o), _l.dptr(cw), None if w is None else _l.ushort_ptr(w), k, a, pr, *outs))
    del keep
    return dict(cam_rt=cam, intr=intr, board_rt=board, valid=bool(valid.value), summary=_l.summary_dict(s))


def project(intr, points, device: int = 0) -> np.ndarray:
    intr = np.ascontiguousarray(intr, dtype=np.float64).reshape(9)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((pts.shape[0], 2))
    _l.check(_l.lib().tscm_project_points(_l.dptr(intr), _l.dptr(pts), pts.shape[0], device, _l.dptr(out)))
    return out


def unproject(intr, pixels, device: int = 0) -> np.ndarray:
    intr = np.ascontiguousarray(intr, dtype=np.float64).reshape(9)
    px = np.ascontiguousarray(pixels, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((px.shape[0], 3))
    _l.check(_l.lib().tscm_unproject_pixels(_l.dptr(intr), _l.dptr(px), px.shape[0], device, _l.dptr(out)))
    return out


def reprojection_error(problem: Problem, device: int = 0):
    """-> (per-camera mean pixel error [C], global mean, rmse)  (multi_calib.cpp:233-283)."""
    assert _is_normalised(problem)
    per = np.zeros(problem.n_cameras)
    g, r = C.c_double(0.0), C.c_double(0.0)
    cp = _l.c_problem(problem)
    _l.check(_l.lib().tscm_reprojection_error(C.byref(cp), device, _l.dptr(per), C.byref(g), C.byref(r)))
    return per, g.value, r.value


def shard_owner(problem: Problem, world: int) -> np.ndarray:
    assert _is_normalised(problem)
    owner = np.zeros(problem.n_boards, dtype=np.int32)
    cp = _l.c_problem(problem)
    _l.check(_l.lib().tscm_shard_frames(C.byref(cp), world, owner.ctypes.data_as(C.POINTER(C.c_int))))
    return owner


def _covariance_dict(info, Cn: int, B: int, cam_cov, board_cov) -> dict:
    dof = int(info.n_residuals) - int(info.n_free)
    return dict(status=info.status, where=info.where, n_free=info.n_free, dof=dof, sigma2=info.sigma2, cost=info.cost,
                n_residuals=int(info.n_residuals), min_pivot_ratio=info.min_pivot_ratio, cam_cov=cam_cov.reshape(Cn, 15, Cn, 15), board_cov=board_cov.reshape(B, 6, 6),
                seconds_kernel=tuple(info.seconds_kernel))


def covariance(problem: Problem, device: int = 0, *, loss=None, fixed=None, weights=None, priors=None) -> dict:
    """What ceres::Covariance gives a Ceres user, at the problem's parameters (tscm_covariance): (J^T J)^-1 over the free
    columns in Ceres' convention (not multiplied by sigma2), sigma2 = 2 cost / dof and the standard deviations
    sqrt(sigma2 * diagonal).  loss, fixed, weights: as for calibrate() -- pass what the solve had (with weights:
    tscm_covariance_weighted, the residuals are the corners with a weight > 0; with priors: tscm_covariance_prior, every prior
    on a free column is one more residual, in the blocks, the cost and dof).
    -> status (0 ok, 1 singular board block, 2 singular reduced system: every array is then NaN), where, n_free, dof, sigma2,
    cost, min_pivot_ratio (near 0: gauge freedom or an unobservable parameter), cam_cov [C,15,C,15] and board_cov [B,6,6]
    (zero where not free), cam_rt_std [C,6], intr_std [C,9], board_rt_std [B,6] (0 where not free), seconds_kernel (board
    factor, Schur complement, reduced inverse, board marginals)."""
    assert _is_normalised(problem), "use Problem.normalised()"
    Cn, B = problem.n_cameras, problem.n_boards
    cam_cov, board_cov = np.zeros((Cn * 15, Cn * 15)), np.zeros((B, 6, 6))
    cam_std, intr_std, board_std = np.zeros((Cn, 6)), np.zeros((Cn, 9)), np.zeros((B, 6))
    info = _l.CCovarianceInfo(struct_size=C.sizeof(_l.CCovarianceInfo))
    q, cw = _l.corner_weights(problem, weights)
    cp = _l.c_problem(q)
    w = None if fixed is None else _l.fixed_masks(fixed, Cn)
    k, a = _l.loss_args(loss)
    outs = (_l.dptr(cam_cov), _l.dptr(board_cov), _l.dptr(cam_std), _l.dptr(intr_std), _l.dptr(board_std), C.byref(info))
    pr, keep = _l.priors_ptr(priors, Cn)
    _l.check(_l.lib().tscm_covariance_prior(C.byref(cp), device, None if w is None else _l.ushort_ptr(w), _l.dptr(cw), k, a, pr, *outs))
    del keep
    out = _covariance_dict(info, Cn, B, cam_cov, board_cov)
    out.update(cam_rt_std=cam_std, intr_std=intr_std, board_rt_std=board_std)
    return out


def covariance_from_normal_equations(view_camera, view_board, board_gram, view_cross, cam_gram, cam_free, board_free, device: int = 0) -> dict:
    """The covariance kernels on blocks the caller gives (tscm_covariance_from_normal_equations): board_gram [B,6,6],
    view_cross [V,6,15], cam_gram [C,15,15] in the layout of normal_equations(), cam_free [C,15] and board_free [B] (true =
    free).  -> the dict of covariance() without the standard deviations; cost, sigma2 and dof carry nothing."""
    vc, vb = np.ascontiguousarray(view_camera, dtype=np.int32), np.ascontiguousarray(view_board, dtype=np.int32)
    bg, vx, cg = (np.ascontiguousarray(x, dtype=np.float64) for x in (board_gram, view_cross, cam_gram))
    cf, bf = np.ascontiguousarray(cam_free, dtype=np.uint8), np.ascontiguousarray(board_free, dtype=np.uint8)
    Cn, B, V = cg.shape[0], bf.size, vc.size
    if cg.shape != (Cn, 15, 15) or bg.shape != (B, 6, 6) or vx.shape != (V, 6, 15) or cf.size != Cn * 15 or vb.size != V:
        raise ValueError("shapes: board_gram [B,6,6], view_cross [V,6,15], cam_gram [C,15,15], cam_free [C,15], board_free [B], view_* [V]")
    cam_cov, board_cov = np.zeros((Cn * 15, Cn * 15)), np.zeros((B, 6, 6))
    info = _l.CCovarianceInfo(struct_size=C.sizeof(_l.CCovarianceInfo))
    ip, ubp = C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    _l.check(_l.lib().tscm_covariance_from_normal_equations(Cn, B, V, vc.ctypes.data_as(ip), vb.ctypes.data_as(ip), _l.dptr(bg), _l.dptr(vx), _l.dptr(cg),
                                                            cf.ctypes.data_as(ubp), bf.ctypes.data_as(ubp), device, _l.dptr(cam_cov), _l.dptr(board_cov),
                                                            C.byref(info)))
    return _covariance_dict(info, Cn, B, cam_cov, board_cov)


RESIDUAL_CORNER = ("r_u", "r_v", "r_rad", "r_tan", "angle", "rho1")
RESIDUAL_VIEW = ("n_used", "sum_w", "rms", "mean_err", "max_err", "bias_u", "bias_v", "mean_rad")
RESIDUAL_CAMERA = ("n_used", "sum_w", "rms", "mean_err", "max_err", "worst_view", "n_views_used")


def residual_report(problem: Problem, device: int = 0, *, weights=None, loss=None, grid=None, image_size=None, angle_bins: int = 0,
                    max_angle=None, clamp: float = 64.0) -> dict:
    """Which views and corners are bad, and does the model fit the lens (tscm_residual_report), at the problem's parameters.
    weights (default: problem.weights): corner weights as for calibrate(), except that a view whose weights are all 0 is
    accepted -- it is unused -- so a pruned weights array can be reported on.  loss: as for calibrate(); it sets rho1 and cost.
    grid=(grid_w, grid_h) with image_size=(width, height): the residual field over the image, by the cell of the OBSERVED
    pixel.  angle_bins with max_angle (default pi / 2): the field over the incidence angle.  clamp: pixels, in (0, 64].
    -> corner [N, 6] (RESIDUAL_CORNER; rows of corners with weight 0 are 0) and corner_views (the same rows split per view),
    view [V, 8] (RESIDUAL_VIEW), view_worst [V] (-1: unused view), camera [C, 8] (RESIDUAL_CAMERA, then 0), cost, rmse, n_used,
    n_views_used, sum_w, seconds_kernel; with a grid grid_count [C, gh, gw, 2] (count, n_clamped), grid [C, gh, gw, 3] (mean_u,
    mean_v, rms) and grid_outside [C]; with bins angle_count [C, K, 2], angle [C, K, 4] (mean_rad, mean_tan, rms, mean_angle)
    and angle_outside [C]."""
    assert _is_normalised(problem), "use Problem.normalised()"
    Cn, V, N = problem.n_cameras, problem.n_views, problem.n_corners
    w = problem.weights if weights is None else weights
    if w is not None:
        w = np.ascontiguousarray(np.asarray(w), dtype=np.float64).ravel()
        if w.size != N:
            raise ValueError(f"weights: {w.size} entries for {N} corners (one per corner, views in order)")
    q = _l.CResidualParams()
    _l.lib().tscm_residual_default_params(C.byref(q))
    q.loss_kind, q.loss_scale = _l.loss_args(loss)
    gw = gh = 0
    if grid is not None:
        if image_size is None:
            raise ValueError("grid needs image_size=(width, height)")
        gw, gh = int(grid[0]), int(grid[1])
        q.grid_w, q.grid_h, q.image_width, q.image_height = gw, gh, int(image_size[0]), int(image_size[1])
    K = int(angle_bins)
    q.n_angle_bins = K
    if max_angle is not None:
        q.max_angle = float(max_angle)
    q.clamp = float(clamp)
    corner, view, worst, camera = np.zeros((N, 6)), np.zeros((V, 8)), np.zeros(V, dtype=np.int32), np.zeros((Cn, 8))
    grid_count, grid_mean = np.zeros((Cn, gh, gw, 2), dtype=np.int64), np.zeros((Cn, gh, gw, 3))
    angle_count, angle_mean = np.zeros((Cn, K, 2), dtype=np.int64), np.zeros((Cn, K, 4))
    info = _l.CResidualInfo(struct_size=C.sizeof(_l.CResidualInfo))
    llp = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
    cp = _l.c_problem(problem)
    _l.check(_l.lib().tscm_residual_report(C.byref(cp), device, _l.dptr(w), C.byref(q), _l.dptr(corner), _l.dptr(view),
                                          worst.ctypes.data_as(C.POINTER(C.c_int)), _l.dptr(camera), llp(grid_count) if gw else None,
                                          _l.dptr(grid_mean) if gw else None, llp(angle_count) if K else None, _l.dptr(angle_mean) if K else None,
                                          C.byref(info)))
    first = np.cumsum(problem.view_count) - problem.view_count
    out = dict(corner=corner, corner_views=[corner[f:f + n] for f, n in zip(first, problem.view_count)], view=view, view_worst=worst,
               camera=camera, cost=info.cost, rmse=info.rmse, n_used=int(info.n_used), n_views_used=int(info.n_views_used), sum_w=info.sum_w,
               seconds_kernel=tuple(info.seconds_kernel))
    if gw:
        out.update(grid_count=grid_count, grid=grid_mean, grid_outside=np.array(info.grid_outside[:Cn], dtype=np.int64))
    if K:
        out.update(angle_count=angle_count, angle=angle_mean, angle_outside=np.array(info.angle_outside[:Cn], dtype=np.int64))
    return out


def view_outliers(report: dict, problem: Problem, k: float = 3.0, floor: float = 0.0, max_fraction: float = 0.2) -> np.ndarray:
    """bool [V]: the views of a residual_report() whose rms stands out in their camera.  Per camera, over its views with
    n_used > 0: view v is flagged when rms_v > median + k * 1.4826 * MAD of those rms values and rms_v > floor; at most
    floor(max_fraction * those views) are flagged per camera, the worst first, ties to the lower view.  Host code."""
    rms, used = np.asarray(report["view"])[:, 2], np.asarray(report["view"])[:, 0] > 0
    cam = np.asarray(problem.view_camera)
    out = np.zeros(cam.size, dtype=bool)
    for m in range(problem.n_cameras):
        views = np.nonzero((cam == m) & used)[0]
        if views.size == 0:
            continue
        x = rms[views]
        med = np.median(x)
        mad = np.median(np.abs(x - med))
        hit = views[(x > med + k * 1.4826 * mad) & (x > floor)]
        cap = int(np.floor(max_fraction * views.size))
        order = np.lexsort((hit, -rms[hit]))                 # the worst first, then the lower view
        out[hit[order[:cap]]] = True
    return out


def corner_outliers(report: dict, threshold: float) -> np.ndarray:
    """bool [N]: the corners of a residual_report() with |r| > threshold (pixels)."""
    c = np.asarray(report["corner"])
    return np.hypot(c[:, 0], c[:, 1]) > threshold


def prune_weights(problem: Problem, weights=None, views=None, corners=None) -> np.ndarray:
    """float64 [N]: `weights` (None: problem.weights, or all 1) with the corners of the views in `views` (bool [V] or indices)
    and the corners in `corners` (bool [N] or indices) set to 0."""
    N = problem.n_corners
    w = problem.weights if weights is None else weights
    w = np.ones(N) if w is None else np.array(w, dtype=np.float64).ravel()
    if w.size != N:
        raise ValueError(f"weights: {w.size} entries for {N} corners")
    if views is not None:
        flag = np.zeros(problem.n_views, dtype=bool)
        flag[_index(views)] = True
        w[np.repeat(flag, problem.view_count)] = 0.0
    if corners is not None:
        w[_index(corners)] = 0.0
    return w


def _index(sel) -> np.ndarray:
    """a bool mask as it is, anything else (an empty list included) as integer indices"""
    sel = np.asarray(sel)
    return sel if sel.dtype == np.bool_ else sel.astype(np.int64)


UNCERTAINTY_PLANES = ("u_b", "v_b", "c_uu", "c_uv", "c_vv", "sd_worst", "sd_across")


def uncertainty_grid(nx: int, ny: int, x0: float = 0.0, y0: float = 0.0, dx: float = 1.0, dy: float = 1.0, width_b: int = 0, height_b: int = 0) -> dict:
    """The pixel grid of projection_uncertainty: pixel (col, row) is (x0 + col dx, y0 + row dy) in camera a; width_b x height_b
    is the target cameras' image for the `inside` flag (0: not asked)."""
    return dict(nx=int(nx), ny=int(ny), x0=float(x0), y0=float(y0), dx=float(dx), dy=float(dy), width_b=int(width_b), height_b=int(height_b))


def projection_uncertainty(cam_rt, intr, cov: dict, requests, grid: dict, device: int = 0) -> dict:
    """Projection uncertainty maps (tscm_projection_uncertainty): the 2 x 2 covariance of a pixel of camera a transferred to
    camera b at inverse distance i (a == b: of a fixed rig-frame point observed in its own camera) under the joint parameter
    covariance.  cam_rt [C,6], intr [C,9]: the calibration; cov: the dict of covariance() (cam_cov and sigma2 are used);
    requests: (camera_a, camera_b, inv_distance) triples; grid: uncertainty_grid(...).
    -> planes [R,7,ny,nx] and its views u_b, v_b, c_uu, c_uv, c_vv, sd_worst, sd_across [R,ny,nx] (NaN where the pixel does
    not unproject or its point does not project; sd_across also in observe mode), flags [R,ny,nx] uint8 (bit 0 unprojects,
    1 projects, 2 inside camera b's image), max_sd and n_valid [R], seconds_kernel."""
    rt, I = np.ascontiguousarray(cam_rt, dtype=np.float64), np.ascontiguousarray(intr, dtype=np.float64)
    Cn = rt.shape[0]
    cc = np.ascontiguousarray(cov["cam_cov"], dtype=np.float64)
    if rt.shape != (Cn, 6) or I.shape != (Cn, 9) or cc.size != (15 * Cn) ** 2:
        raise ValueError("shapes: cam_rt [C,6], intr [C,9], cov['cam_cov'] [C,15,C,15]")
    req = (_l.CUncertaintyRequest * max(len(requests), 1))(*[_l.CUncertaintyRequest(int(a), int(b), float(i)) for a, b, i in requests])
    g = _l.CUncertaintyGrid(struct_size=C.sizeof(_l.CUncertaintyGrid), **grid)
    R, ny, nx = len(requests), max(g.ny, 0), max(g.nx, 0)
    planes, flags = np.zeros((R, 7, ny, nx)), np.zeros((R, ny, nx), dtype=np.uint8)
    max_sd, n_valid = np.zeros(R), np.zeros(R, dtype=np.int64)
    _l.check(_l.lib().tscm_projection_uncertainty(Cn, _l.dptr(rt), _l.dptr(I), _l.dptr(cc), float(cov["sigma2"]), C.byref(g), req, R, device, _l.dptr(planes),
                                                  flags.ctypes.data_as(C.POINTER(C.c_ubyte)), _l.dptr(max_sd), n_valid.ctypes.data_as(C.POINTER(C.c_longlong))))
    out = dict(planes=planes, flags=flags, max_sd=max_sd, n_valid=n_valid, requests=[(int(a), int(b), float(i)) for a, b, i in requests], grid=dict(grid),
               seconds_kernel=float(_l.lib().tscm_projection_uncertainty_seconds()))
    out.update({name: planes[:, k] for k, name in enumerate(UNCERTAINTY_PLANES)})
    return out


# ----------------------------------------------------------------------------- next-best view (tscm_view_gain)
VIEW_GAIN_FLAGS = dict(a_contributes=1, b_contributes=2, numbers=4, pivot=8)


def _view_gain_args(cam_rt, intr, cov, board_xy, image_size, candidates, weights, border, min_corners):
    rt, I = np.ascontiguousarray(cam_rt, dtype=np.float64), np.ascontiguousarray(intr, dtype=np.float64)
    Cn = rt.shape[0]
    cc = np.ascontiguousarray(cov["cam_cov"] if isinstance(cov, dict) else cov, dtype=np.float64)
    xy = np.ascontiguousarray(board_xy, dtype=np.float64)
    size = np.ascontiguousarray(image_size, dtype=np.int32)
    if size.size == 2:
        size = np.ascontiguousarray(np.tile(size.reshape(1, 2), (Cn, 1)))
    if rt.shape != (Cn, 6) or I.shape != (Cn, 9) or cc.size != (15 * Cn) ** 2 or xy.ndim != 2 or xy.shape[1] != 2 or size.shape != (Cn, 2):
        raise ValueError("shapes: cam_rt [C,6], intr [C,9], cam_cov [C,15,C,15], board_xy [P,2], image_size (w, h) or [C,2]")
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w is not None and w.size != 15 * Cn:
        raise ValueError("weights: [C,15]")
    cands = [(int(a), int(b), [float(x) for x in np.asarray(r, dtype=np.float64).reshape(6)]) for a, b, r in candidates]
    arr = (_l.CViewCandidate * max(len(cands), 1))()
    for k, (a, b, r) in enumerate(cands):
        arr[k].camera_a, arr[k].camera_b = a, b
        arr[k].board_rt[:] = r
    prm = _l.CViewGainParams(struct_size=C.sizeof(_l.CViewGainParams), min_corners=int(min_corners), border=float(border))
    keep = (rt, I, cc, xy, size, w, arr, prm)
    head = (Cn, _l.dptr(rt), _l.dptr(I), _l.dptr(cc), None if w is None else _l.dptr(w), xy.shape[0], _l.dptr(xy), size.ctypes.data_as(C.POINTER(C.c_int)),
            C.byref(prm), arr)
    return head, len(cands), Cn, keep


def view_gain(cam_rt, intr, cov, board_xy, image_size, candidates, weights=None, border: float = 0.0, min_corners: int = 8, device: int = 0) -> dict:
    """Next-best view (tscm_view_gain): what a hypothetical view of the board at each candidate pose would remove from the
    camera covariance.  cam_rt [C,6], intr [C,9]: the calibration; cov: the dict of covariance() or its cam_cov; board_xy
    [P,2]; image_size (width, height) or [C,2]; candidates: (camera_a, camera_b, board_rt[6]) triples, board_rt in the rig
    frame (camera_a == camera_b: one camera sees the board); weights [C,15] of gain_trace or None (1 / variance).
    -> gain_logdet, gain_trace [R], n_visible [R,2], flags [R] (VIEW_GAIN_FLAGS), seconds_kernel."""
    head, R, _, keep = _view_gain_args(cam_rt, intr, cov, board_xy, image_size, candidates, weights, border, min_corners)
    ld, tr = np.zeros(R), np.zeros(R)
    nv, fl = np.zeros((R, 2), dtype=np.int32), np.zeros(R, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    _l.check(_l.lib().tscm_view_gain(*head, R, device, _l.dptr(ld), _l.dptr(tr), nv.ctypes.data_as(ip), fl.ctypes.data_as(ip)))
    del keep
    return dict(gain_logdet=ld, gain_trace=tr, n_visible=nv, flags=fl, seconds_kernel=float(_l.lib().tscm_view_gain_seconds()))


def view_gain_apply(cam_rt, intr, cov, board_xy, image_size, candidate, weights=None, border: float = 0.0, min_corners: int = 8, device: int = 0) -> dict:
    """One candidate applied (tscm_view_gain_apply): its outputs as view_gain gives them (scalars, n_visible [2]) and cam_cov
    [C,15,C,15], the camera covariance after the view -- what the next view_gain call takes for greedy planning."""
    head, _, Cn, keep = _view_gain_args(cam_rt, intr, cov, board_xy, image_size, [candidate], weights, border, min_corners)
    ld, tr = C.c_double(0.0), C.c_double(0.0)
    nv, fl = np.zeros(2, dtype=np.int32), C.c_int(0)
    out = np.zeros((15 * Cn, 15 * Cn))
    _l.check(_l.lib().tscm_view_gain_apply(*head, device, C.byref(ld), C.byref(tr), nv.ctypes.data_as(C.POINTER(C.c_int)), C.byref(fl), _l.dptr(out)))
    del keep
    return dict(gain_logdet=ld.value, gain_trace=tr.value, n_visible=nv, flags=fl.value, cam_cov=out.reshape(Cn, 15, Cn, 15),
                seconds_kernel=float(_l.lib().tscm_view_gain_seconds()))


def _rotation_matrix(w) -> np.ndarray:
    w = np.asarray(w, dtype=np.float64)
    th = float(np.sqrt(w @ w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th * th <= np.finfo(np.float64).eps:
        return np.eye(3) + K
    K = K / th
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _angle_axis(R) -> np.ndarray:
    """The angle-axis vector of a rotation matrix (angle in [0, pi])."""
    R = np.asarray(R, dtype=np.float64)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * float(np.sqrt(v @ v)), 0.5 * (np.trace(R) - 1.0)
    th = float(np.arctan2(s, c))
    if s > 1e-8:
        return v * (th / (2.0 * s))
    if c > 0:
        return 0.5 * v
    S = 0.5 * (R + np.eye(3))                                   # angle pi: R = 2 k k^T - I
    k = np.sqrt(np.maximum(np.diag(S), 0.0))
    i = int(np.argmax(k))
    k = np.where(S[i] < 0, -k, k)
    k[i] = abs(k[i])
    return th * k / np.sqrt(k @ k)


def board_pose_facing(cam_rt_m, ray, distance: float, board_xy, tilt_x_deg: float = 0.0, tilt_y_deg: float = 0.0, roll_deg: float = 0.0) -> np.ndarray:
    """board_rt [6] in the rig frame of a board whose centre (the mean of board_xy) lies at `distance` along the camera-frame
    direction `ray` of the camera with pose cam_rt_m, its normal along the ray (it faces the camera), its x axis the
    camera's x axis made orthogonal to the ray; then turned about its own x, y (tilts) and z (roll) axes through the centre."""
    z = np.asarray(ray, dtype=np.float64)
    z = z / np.sqrt(z @ z)
    ex = np.array([1.0, 0.0, 0.0]) if abs(z[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = ex - (ex @ z) * z
    x = x / np.sqrt(x @ x)
    Rcb = np.stack([x, np.cross(z, x), z], axis=1)
    tx, ty, rz = np.deg2rad([tilt_x_deg, tilt_y_deg, roll_deg])
    Rcb = Rcb @ _rotation_matrix([tx, 0, 0]) @ _rotation_matrix([0, ty, 0]) @ _rotation_matrix([0, 0, rz])
    centre = np.append(np.asarray(board_xy, dtype=np.float64).mean(axis=0), 0.0)
    tcb = float(distance) * z - Rcb @ centre
    rt = np.asarray(cam_rt_m, dtype=np.float64)
    Rm = _rotation_matrix(rt[:3])
    return np.concatenate([_angle_axis(Rm.T @ Rcb), Rm.T @ (tcb - rt[3:])])


def _unit_rays(intr_m, px) -> np.ndarray:
    """get_unit_sphere_coordinate with b = c = 0 on pixels px [P,2] in float64 numpy: rays [P,3], NaN where a pixel does not unproject."""
    fx, fy, cx, cy, xi, lam, al = (float(x) for x in np.asarray(intr_m, dtype=np.float64)[:7])
    mx, my = (px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy
    ks = al / (1 - al)
    r2 = mx * mx + my * my
    with np.errstate(invalid="ignore"):
        gamma = (ks + np.sqrt(1 + (1 - ks * ks) * r2)) / (r2 + 1)
        gk = gamma - ks
        yita = lam * gk + np.sqrt((gk * gk - 1) * lam * lam + 1)
        ml = yita * gk - lam
        mu = xi * ml + np.sqrt(xi * xi * (ml * ml - 1) + 1)
    return np.stack([mu * yita * gamma * mx, mu * yita * gamma * my, mu * ml - xi], axis=1)


def view_candidates(cam_rt, intr, camera: int, image_size, board_xy, grid=(6, 4), distances=(400.0, 800.0), tilts_deg=(0.0, 25.0, -25.0), rolls_deg=(0.0,),
                    pair=None):
    """A deterministic candidate set for view_gain: the board centre on the ray of each pixel of a grid[0] x grid[1] grid of
    camera `camera`'s image (cell centres) at each distance, facing the camera, then tilted about its x axis and about its y
    axis by each non-zero tilt and rolled (board_pose_facing).  pair: the second camera of every candidate (None: the camera
    alone).  -> (candidates, info): (camera_a, camera_b, board_rt) triples and per candidate dict(camera, pixel, distance,
    tilt_x, tilt_y, roll).  Pixels that do not unproject are left out."""
    rt, I = np.asarray(cam_rt, dtype=np.float64), np.asarray(intr, dtype=np.float64)
    w, h = (int(x) for x in np.asarray(image_size).reshape(-1, 2)[camera if np.asarray(image_size).size > 2 else 0])
    gx, gy = int(grid[0]), int(grid[1])
    px = np.array([[(i + 0.5) * w / gx - 0.5, (j + 0.5) * h / gy - 0.5] for j in range(gy) for i in range(gx)])
    rays = _unit_rays(I[camera], px)
    tilts = [(0.0, 0.0)] + [(t, 0.0) for t in tilts_deg if t != 0] + [(0.0, t) for t in tilts_deg if t != 0]
    b = camera if pair is None else int(pair)
    cands, info = [], []
    for q, ray in zip(px, rays):
        if not np.all(np.isfinite(ray)):
            continue
        for d in distances:
            for tx, ty in tilts:
                for roll in rolls_deg:
                    cands.append((int(camera), b, board_pose_facing(rt[camera], ray, d, board_xy, tx, ty, roll)))
                    info.append(dict(camera=int(camera), pixel=(float(q[0]), float(q[1])), distance=float(d), tilt_x=float(tx), tilt_y=float(ty), roll=float(roll)))
    return cands, info


def plan_views(cam_rt, intr, cov, board_xy, image_size, candidates, n_views: int = 5, criterion: str = "gain_logdet", weights=None, border: float = 0.0,
               min_corners: int = 8, device: int = 0) -> list:
    """Greedy next-best views: score every candidate (view_gain), take the first arg-max of `criterion` (gain_logdet or
    gain_trace), apply it (view_gain_apply) and repeat on the covariance it leaves, n_views times.  -> a list of dict(index,
    candidate, gain_logdet, gain_trace, n_visible, flags, scores (the step's view_gain), cam_cov (after the step)).  Stops early
    when no candidate has a positive, finite score."""
    if criterion not in ("gain_logdet", "gain_trace"):
        raise ValueError("criterion: gain_logdet or gain_trace")
    cc = np.array(cov["cam_cov"] if isinstance(cov, dict) else cov, dtype=np.float64)
    kw = dict(weights=weights, border=border, min_corners=min_corners, device=device)
    steps = []
    for _ in range(int(n_views)):
        scores = view_gain(cam_rt, intr, cc, board_xy, image_size, candidates, **kw)
        s = np.where((scores["flags"] & 4) != 0, scores[criterion], -np.inf)
        best = int(np.argmax(s))
        if not s[best] > 0:
            break
        ap = view_gain_apply(cam_rt, intr, cc, board_xy, image_size, candidates[best], **kw)
        cc = ap["cam_cov"]
        steps.append(dict(index=best, candidate=candidates[best], gain_logdet=ap["gain_logdet"], gain_trace=ap["gain_trace"], n_visible=ap["n_visible"],
                          flags=ap["flags"], scores=scores, cam_cov=cc))
    return steps
