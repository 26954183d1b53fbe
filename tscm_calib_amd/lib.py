"""ctypes binding of the C ABI in include/tscm/tscm.h (libtscm_hip.so).

There is no CPU fallback: if the shared library is missing, or no HIP device is
present, compute calls raise.  (The CPU oracle under oracle/ is test infrastructure
and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libtscm_hip.so")
UNIQUE_ID_BYTES = 128
IPC_HANDLE_BYTES = 80
MAX_ITERATIONS = 255
# tscm_options.exec_flags (tscm.h)
EXEC_SEPARATE_T_REDUCE = 1
EXEC_KEEP_SINGLE_RANK_COMM = 2
EXEC_GRAM_16X16 = 4
EXEC_SEPARATE_BACKSUB = 8
EXEC_SEPARATE_CONTROL = 16
EXEC_DENSE_REDUCED_ORDER = 32
EXEC_GRAPH_REDUCED_ORDER = 64
EXEC_SEPARATE_STATS = 128
# robust losses (tscm.h: TSCM_LOSS_*), by the names the Python layer takes
LOSS_NONE, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY = 0, 1, 2, 3
LOSS_KINDS = {None: LOSS_NONE, "none": LOSS_NONE, "huber": LOSS_HUBER, "soft_l1": LOSS_SOFT_L1, "cauchy": LOSS_CAUCHY}
# output-image kinds of the remap tables (tscm.h: TSCM_PROJ_*)
PROJ_PERSPECTIVE, PROJ_LONGLAT, PROJ_CYLINDRICAL, PROJ_STEREOGRAPHIC, PROJ_EQUIRECT = 0, 1, 2, 3, 4
PROJ_KINDS = {"perspective": PROJ_PERSPECTIVE, "longlat": PROJ_LONGLAT, "cylindrical": PROJ_CYLINDRICAL,
              "stereographic": PROJ_STEREOGRAPHIC, "equirect": PROJ_EQUIRECT}
# panorama blend modes (tscm.h: TSCM_PANO_*)
PANO_SEAM, PANO_FEATHER, PANO_MULTIBAND = 0, 1, 2
FILL_LOWEST, FILL_SECOND_LOWEST, FILL_MEDIAN = 0, 1, 2
PANO_MODES = {"seam": PANO_SEAM, "feather": PANO_FEATHER, "multiband": PANO_MULTIBAND}
# held intrinsics (tscm.h: TSCM_FIX_*): bit k holds intrinsic k of the 9-vector
INTRINSIC_NAMES = ("fx", "fy", "cx", "cy", "xi", "lambda", "alpha", "b", "c")
FIX = {name: 1 << k for k, name in enumerate(INTRINSIC_NAMES)}
FIX_INTRINSICS, FIX_ALL = 127, 511
MODEL_DS = FIX["lambda"]
MODEL_UCM = FIX["xi"] | FIX["lambda"]

E_NAMES = {0: "TSCM_OK", -1: "TSCM_E_INVALID", -2: "TSCM_E_NO_DEVICE", -3: "TSCM_E_HIP",
           -4: "TSCM_E_RCCL", -5: "TSCM_E_UNSUPPORTED", -6: "TSCM_E_NOMEM", -7: "TSCM_E_PEER"}
TERMINATION = {0: "CONVERGENCE", 1: "NO_CONVERGENCE", 2: "FAILURE"}


class TscmError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{E_NAMES.get(code, code)}: {message}")
        self.code = code


class CProblem(C.Structure):
    _fields_ = [
        ("n_cameras", C.c_int), ("n_boards", C.c_int), ("n_points", C.c_int), ("n_views", C.c_int),
        ("board_xy", C.c_void_p), ("view_camera", C.c_void_p), ("view_board", C.c_void_p),
        ("view_offset", C.c_void_p), ("view_count", C.c_void_p), ("obs_u", C.c_void_p), ("obs_v", C.c_void_p),
        ("cam_rt", C.c_void_p), ("intr", C.c_void_p), ("board_rt", C.c_void_p),
        ("cam_pose_constant", C.c_void_p), ("mono", C.c_int), ("board_pose_constant", C.c_void_p),
    ]


class COptions(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t), ("max_num_iterations", C.c_int), ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
        ("max_num_consecutive_invalid_steps", C.c_int), ("jacobi_scaling", C.c_int), ("check_every", C.c_int),
        ("jacobian_fp32", C.c_int), ("exec_flags", C.c_int),
    ]


class CIteration(C.Structure):
    _fields_ = [
        ("iteration", C.c_int), ("step_is_valid", C.c_int), ("step_is_successful", C.c_int),
        ("cost", C.c_double), ("cost_change", C.c_double), ("gradient_max_norm", C.c_double),
        ("gradient_norm", C.c_double), ("step_norm", C.c_double), ("relative_decrease", C.c_double),
        ("trust_region_radius", C.c_double),
    ]


class CSummary(C.Structure):
    _fields_ = [
        ("termination_type", C.c_int), ("num_iterations", C.c_int), ("num_successful_steps", C.c_int),
        ("num_unsuccessful_steps", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("n_residual_blocks", C.c_int), ("lm_iterations", C.c_int),
        ("iterations", CIteration * (MAX_ITERATIONS + 1)), ("message", C.c_char * 128),
        ("seconds_solve", C.c_double), ("seconds_total", C.c_double), ("rmse", C.c_double),
    ]


class CRigInput(C.Structure):
    _fields_ = [
        ("n_cameras", C.c_int), ("n_boards", C.c_int), ("n_points", C.c_int),
        ("worlds", C.c_void_p), ("intr", C.c_void_p), ("has", C.c_void_p), ("Rt", C.c_void_p),
        ("pix_u", C.c_void_p), ("pix_v", C.c_void_p),
    ]


class CRigResult(C.Structure):
    _fields_ = [
        ("cam_R", C.c_void_p), ("cam_t", C.c_void_p), ("cam_rt", C.c_void_p),
        ("board_R", C.c_void_p), ("board_t", C.c_void_p), ("board_rt", C.c_void_p),
        ("board_initial", C.c_void_p), ("cam_choice", C.c_void_p), ("cam_min_error", C.c_void_p),
        ("seconds_hypotheses", C.c_double), ("seconds_total", C.c_double), ("n_projections", C.c_longlong),
    ]


class CMapDesc(C.Structure):
    _fields_ = [
        ("intr", C.c_double * 9), ("R", C.c_double * 9), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
        ("cy", C.c_double), ("offset_x", C.c_double), ("offset_y", C.c_double), ("width", C.c_int), ("height", C.c_int),
        ("out_stride", C.c_int), ("check_w2", C.c_int), ("out_offset", C.c_longlong), ("w2", C.c_double),
    ]


class CStereoParams(C.Structure):
    """tscm_stereo_params (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("min_disparity", C.c_int), ("num_disparities", C.c_int), ("p1", C.c_int), ("p2", C.c_int),
                ("paths", C.c_int), ("uniqueness_ratio", C.c_int), ("disp12_max_diff", C.c_int)]


class CStereoFilterParams(C.Structure):
    """tscm_stereo_filter_params (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("min_disparity", C.c_int), ("speckle_window_size", C.c_int), ("speckle_range", C.c_int),
                ("median", C.c_int)]


class CStereoFillParams(C.Structure):
    """tscm_stereo_fill_params (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("min_disparity", C.c_int), ("rule", C.c_int), ("paths", C.c_int), ("max_distance", C.c_int),
                ("min_directions", C.c_int), ("wrap_x", C.c_int)]


class CStereoRefineParams(C.Structure):
    """tscm_stereo_refine_params (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("min_disparity", C.c_int), ("radius", C.c_int), ("iterations", C.c_int), ("fill_invalid", C.c_int),
                ("wrap_x", C.c_int)]


class CPanoramaParams(C.Structure):
    """tscm_panorama_params (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("mode", C.c_int), ("levels", C.c_int), ("wrap_x", C.c_int)]


class CSweepParams(C.Structure):
    """tscm_sweep_params (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("num_hypotheses", C.c_int), ("p1", C.c_int), ("p2", C.c_int), ("paths", C.c_int),
                ("uniqueness_ratio", C.c_int), ("wrap_x", C.c_int)]


class CSweepComposeParams(C.Structure):
    """tscm_sweep_compose_params (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("mode", C.c_int), ("levels", C.c_int), ("wrap_x", C.c_int), ("fallback_index", C.c_int)]


class CSweepVisibilityParams(C.Structure):
    """tscm_sweep_visibility_params (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("cell_shift", C.c_int), ("tolerance", C.c_int), ("dilate", C.c_int), ("near_is_high", C.c_int)]


class CRansacParams(C.Structure):
    """tscm_ransac_params (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("threshold_px", C.c_double), ("n_hypotheses", C.c_int), ("min_inliers", C.c_int),
                ("seed", C.c_uint)]


class CCovarianceInfo(C.Structure):
    """tscm_covariance_info (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("status", C.c_int), ("where", C.c_int), ("n_free", C.c_int), ("n_residuals", C.c_longlong),
                ("cost", C.c_double), ("sigma2", C.c_double), ("min_pivot_ratio", C.c_double), ("seconds_kernel", C.c_double * 4)]


class CCameraPriors(C.Structure):
    """tscm_camera_priors (tscm.h)"""
    _fields_ = [("struct_size", C.c_size_t), ("cam_rt_mean", C.c_void_p), ("cam_rt_weight", C.c_void_p), ("intr_mean", C.c_void_p),
                ("intr_weight", C.c_void_p)]


class CUncertaintyGrid(C.Structure):
    """tscm_uncertainty_grid (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("width_b", C.c_int), ("height_b", C.c_int),
                ("x0", C.c_double), ("y0", C.c_double), ("dx", C.c_double), ("dy", C.c_double)]


class CUncertaintyRequest(C.Structure):
    """tscm_uncertainty_request (tscm.h)"""
    _fields_ = [("camera_a", C.c_int), ("camera_b", C.c_int), ("inv_distance", C.c_double)]


class CViewGainParams(C.Structure):
    """tscm_view_gain_params (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("min_corners", C.c_int), ("border", C.c_double)]


class CViewCandidate(C.Structure):
    """tscm_view_candidate (tscm.h)"""
    _fields_ = [("camera_a", C.c_int), ("camera_b", C.c_int), ("board_rt", C.c_double * 6)]


class CResidualParams(C.Structure):
    """tscm_residual_params (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("loss_kind", C.c_int), ("loss_scale", C.c_double), ("grid_w", C.c_int), ("grid_h", C.c_int),
                ("image_width", C.c_int), ("image_height", C.c_int), ("n_angle_bins", C.c_int), ("pad", C.c_int), ("max_angle", C.c_double),
                ("clamp", C.c_double)]


class CResidualInfo(C.Structure):
    """tscm_residual_info (tscm.h)"""
    _fields_ = [("struct_size", C.c_int), ("n_views_used", C.c_int), ("n_used", C.c_longlong), ("sum_w", C.c_double), ("cost", C.c_double),
                ("rmse", C.c_double), ("grid_outside", C.c_longlong * 32), ("angle_outside", C.c_longlong * 32), ("seconds_kernel", C.c_double * 4)]


class CCornerSet(C.Structure):
    _fields_ = [
        ("n_cameras", C.c_int), ("n_boards", C.c_int), ("board_cols", C.c_int), ("board_rows", C.c_int), ("pitch", C.c_double),
        ("image_width", C.c_int), ("image_height", C.c_int), ("has", C.c_void_p), ("pix_u", C.c_void_p), ("pix_v", C.c_void_p),
    ]


# every symbol include/tscm/tscm.h declares
EXPORTS = [
    "tscm_abi_version", "tscm_last_error", "tscm_device_count", "tscm_device_synchronize", "tscm_device_peak_fp64", "tscm_device_peak_fp64_ex", "tscm_device_peak_fp32_mfma", "tscm_default_options",
    "tscm_solver_create", "tscm_solver_set_comm", "tscm_solver_debug_withhold_handoff", "tscm_solver_debug_schur_rot", "tscm_solver_debug_reduced_backsub", "tscm_solver_reruns", "tscm_solver_solve", "tscm_solver_upload_params",
    "tscm_solver_solve_resident", "tscm_solver_download_params", "tscm_solver_destroy",
    "tscm_solver_kernel_time", "tscm_solver_exchange_time", "tscm_solve_multi", "tscm_solve_mono", "tscm_eval_functor",
    "tscm_eval_normal_equations", "tscm_eval_normal_equations_ex", "tscm_eval_step_ex", "tscm_project_points", "tscm_unproject_pixels",
    "tscm_reprojection_error", "tscm_comm_unique_id", "tscm_comm_create", "tscm_comm_destroy",
    "tscm_shard_frames", "tscm_solver_create_sharded", "tscm_comm_create_local", "tscm_comm_ipc_open", "tscm_comm_ipc_connect", "tscm_solver_solve_group",
    "tscm_solver_gather_boards", "tscm_comm_info", "tscm_rig_init", "tscm_rig_stage_errors", "tscm_yaml_format", "tscm_yaml_write", "tscm_yaml_parse",
    "tscm_yaml_read", "tscm_build_maps", "tscm_estimate_focal", "tscm_poses_from_r1r2t",
    "tscm_estimate_extrinsic", "tscm_estimate_focal_rows", "tscm_estimate_extrinsic_stages", "tscm_corners_write", "tscm_corners_read", "tscm_corners_free",
    "tscm_detect_corners", "tscm_detect_corners_batch", "tscm_corner_planes_batch", "tscm_corner_candidates_free", "tscm_chessboards_from_corners", "tscm_chessboards_free", "tscm_remap",
    "tscm_solver_set_loss", "tscm_solve_robust", "tscm_eval_normal_equations_robust", "tscm_eval_step_robust",
    "tscm_solver_eval_normal_equations",
    "tscm_solver_set_fixed_intrinsics", "tscm_solve_fixed", "tscm_eval_step_fixed", "tscm_solve_mono_batch",
    "tscm_covariance", "tscm_covariance_from_normal_equations",
    "tscm_solver_set_corner_weights", "tscm_solve_weighted", "tscm_eval_normal_equations_weighted", "tscm_eval_step_weighted",
    "tscm_solve_mono_batch_weighted", "tscm_covariance_weighted",
    "tscm_solver_set_camera_priors", "tscm_solve_prior", "tscm_eval_normal_equations_prior", "tscm_eval_step_prior", "tscm_covariance_prior",
    "tscm_projection_uncertainty", "tscm_projection_uncertainty_seconds",
    "tscm_view_gain", "tscm_view_gain_apply", "tscm_view_gain_seconds",
    "tscm_residual_default_params", "tscm_residual_report", "tscm_residual_debug_chunk_target",
    "tscm_build_maps_ex", "tscm_rectify_points",
    "tscm_stereo_default_params", "tscm_stereo_match", "tscm_stereo_stages", "tscm_stereo_stage_times", "tscm_stereo_points",
    "tscm_stereo_filter_default_params", "tscm_stereo_filter", "tscm_stereo_filter_stages",
    "tscm_stereo_fill_default_params", "tscm_stereo_fill", "tscm_stereo_fill_stages",
    "tscm_stereo_refine_default_params", "tscm_stereo_refine_weights", "tscm_stereo_refine", "tscm_stereo_refine_stages",
    "tscm_panorama_default_params", "tscm_panorama_create", "tscm_panorama_compose", "tscm_panorama_stages", "tscm_panorama_overlap", "tscm_panorama_destroy",
    "tscm_build_sweep_maps",
    "tscm_sweep_default_params", "tscm_sweep_create", "tscm_sweep_depth", "tscm_sweep_stages", "tscm_sweep_stage_times", "tscm_sweep_points", "tscm_sweep_destroy",
    "tscm_sweep_compose_default_params", "tscm_sweep_compose", "tscm_sweep_compose_stages",
    "tscm_sweep_visibility_default_params", "tscm_sweep_visibility", "tscm_sweep_visibility_stages", "tscm_sweep_compose_visible", "tscm_sweep_compose_visible_stages",
    "tscm_ransac_default_params", "tscm_estimate_extrinsic_ransac", "tscm_estimate_extrinsic_ransac_stages",
    "tscm_chessboards_from_corners_batch", "tscm_chessboards_batch_stages", "tscm_board_seed_stages_free", "tscm_chessboards_batch_seconds",
]


def build(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 build of csrc/ (cross-compiles without a GPU)."""
    import glob
    srcs = [f for pat in ("*.hip", "*.cpp", "*.h") for f in glob.glob(os.path.join(CSRC, pat))]     # same list as the Makefile
    srcs.append(os.path.join(_HERE, "..", "include", "tscm", "tscm.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(f) > os.path.getmtime(LIB_PATH) for f in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC] + (["-B"] if force else []))
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TscmError(-2, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    L.tscm_abi_version.restype = C.c_int
    L.tscm_last_error.restype = C.c_char_p
    L.tscm_device_count.restype = C.c_int
    L.tscm_device_synchronize.argtypes = [C.c_int]
    L.tscm_device_peak_fp64.argtypes = [C.c_int, dp, dp]
    L.tscm_device_peak_fp64_ex.argtypes = [C.c_int, dp]
    L.tscm_device_peak_fp32_mfma.argtypes = [C.c_int, dp]
    L.tscm_default_options.argtypes = [C.POINTER(COptions), C.c_int]
    L.tscm_default_options.restype = None
    L.tscm_solver_create.argtypes = [C.POINTER(CProblem), C.c_int, C.POINTER(vp)]
    L.tscm_solver_create_sharded.argtypes = [C.POINTER(CProblem), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.tscm_comm_create_local.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    L.tscm_comm_ipc_open.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_ubyte)]
    L.tscm_comm_ipc_connect.argtypes = [vp, C.POINTER(C.c_ubyte)]
    L.tscm_solver_solve_group.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(COptions), C.POINTER(CSummary), C.c_int]
    L.tscm_solver_gather_boards.argtypes = [vp, dp]
    L.tscm_comm_info.argtypes = [vp, ip, ip, ip]
    L.tscm_solver_set_comm.argtypes = [vp, vp]
    L.tscm_solver_debug_withhold_handoff.argtypes = [vp, C.c_int]
    L.tscm_solver_debug_schur_rot.argtypes = [vp, C.c_int]
    L.tscm_solver_debug_reduced_backsub.argtypes = [vp, C.c_int]
    L.tscm_solver_reruns.argtypes = [vp]
    L.tscm_solver_solve.argtypes = [vp, C.POINTER(COptions), C.POINTER(CSummary)]
    L.tscm_solver_upload_params.argtypes = [vp, dp, dp, dp]
    L.tscm_solver_solve_resident.argtypes = [vp, C.POINTER(COptions), C.POINTER(CSummary), C.c_int]
    L.tscm_solver_download_params.argtypes = [vp, dp, dp, dp]
    L.tscm_solver_destroy.argtypes = [vp]
    L.tscm_solver_destroy.restype = None
    L.tscm_solver_kernel_time.argtypes = [vp, C.c_int, ip, dp]
    L.tscm_solver_exchange_time.argtypes = [vp, ip, dp, ip, dp]
    L.tscm_solve_multi.argtypes = [C.POINTER(CProblem), C.POINTER(COptions), C.POINTER(CSummary)]
    L.tscm_solve_mono.argtypes = [C.POINTER(CProblem), C.POINTER(COptions), C.POINTER(CSummary)]
    L.tscm_eval_functor.argtypes = [C.POINTER(CProblem), C.c_int, dp, dp, dp, dp, dp]
    L.tscm_eval_normal_equations.argtypes = [C.POINTER(CProblem), C.c_int, dp, dp, dp, dp, dp, dp]
    L.tscm_eval_normal_equations_ex.argtypes = [C.POINTER(CProblem), C.c_int, C.POINTER(COptions), dp, dp, dp, dp, dp, dp]
    L.tscm_eval_step_ex.argtypes = [C.POINTER(CProblem), C.c_int, C.POINTER(COptions), dp, dp, dp, ip, C.POINTER(CSummary)]
    L.tscm_solver_set_loss.argtypes = [vp, C.c_int, C.c_double]
    L.tscm_solve_robust.argtypes = [C.POINTER(CProblem), C.POINTER(COptions), C.c_int, C.c_double, C.POINTER(CSummary)]
    L.tscm_eval_normal_equations_robust.argtypes = [C.POINTER(CProblem), C.c_int, C.POINTER(COptions), C.c_int, C.c_double, dp, dp, dp, dp, dp, dp]
    L.tscm_eval_step_robust.argtypes = [C.POINTER(CProblem), C.c_int, C.POINTER(COptions), C.c_int, C.c_double, dp, dp, dp, ip, C.POINTER(CSummary)]
    L.tscm_solver_eval_normal_equations.argtypes = [vp, C.POINTER(COptions), C.c_int, dp, dp, dp, dp, dp, dp]
    usp = C.POINTER(C.c_ushort)
    L.tscm_solver_set_fixed_intrinsics.argtypes = [vp, usp]
    L.tscm_solve_fixed.argtypes = [C.POINTER(CProblem), C.POINTER(COptions), usp, C.c_int, C.c_double, C.POINTER(CSummary)]
    L.tscm_solve_mono_batch.argtypes = [C.POINTER(CProblem), C.c_int, C.c_int, C.POINTER(COptions), usp, C.c_int, C.c_double,
                                        C.POINTER(CSummary)]
    L.tscm_eval_step_fixed.argtypes = [C.POINTER(CProblem), C.c_int, C.POINTER(COptions), usp, C.c_int, C.c_double, dp, dp, dp, ip, C.POINTER(CSummary)]
    cip = C.POINTER(CCovarianceInfo)
    L.tscm_covariance.argtypes = [C.POINTER(CProblem), C.c_int, usp, C.c_int, C.c_double, dp, dp, dp, dp, dp, cip]
    L.tscm_covariance_from_normal_equations.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, dp, dp, dp, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), C.c_int,
                                                        dp, dp, cip]
    L.tscm_solver_set_corner_weights.argtypes = [vp, dp]
    L.tscm_solve_weighted.argtypes = [C.POINTER(CProblem), C.POINTER(COptions), dp, usp, C.c_int, C.c_double, C.POINTER(CSummary)]
    L.tscm_eval_normal_equations_weighted.argtypes = [C.POINTER(CProblem), C.c_int, C.POINTER(COptions), dp, C.c_int, C.c_double, dp, dp, dp, dp, dp, dp]
    L.tscm_eval_step_weighted.argtypes = [C.POINTER(CProblem), C.c_int, C.POINTER(COptions), dp, usp, C.c_int, C.c_double, dp, dp, dp, ip, C.POINTER(CSummary)]
    L.tscm_solve_mono_batch_weighted.argtypes = [C.POINTER(CProblem), C.c_int, C.c_int, C.POINTER(COptions), usp, C.POINTER(dp), C.c_int, C.c_double,
                                                 C.POINTER(CSummary)]
    L.tscm_covariance_weighted.argtypes = [C.POINTER(CProblem), C.c_int, usp, dp, C.c_int, C.c_double, dp, dp, dp, dp, dp, cip]
    pp = C.POINTER(CCameraPriors)
    L.tscm_solver_set_camera_priors.argtypes = [vp, pp]
    L.tscm_solve_prior.argtypes = [C.POINTER(CProblem), C.POINTER(COptions), dp, usp, C.c_int, C.c_double, pp, C.POINTER(CSummary)]
    L.tscm_eval_normal_equations_prior.argtypes = [C.POINTER(CProblem), C.c_int, C.POINTER(COptions), dp, C.c_int, C.c_double, pp, dp, dp, dp, dp, dp, dp]
    L.tscm_eval_step_prior.argtypes = [C.POINTER(CProblem), C.c_int, C.POINTER(COptions), dp, usp, C.c_int, C.c_double, pp, dp, dp, dp, ip, C.POINTER(CSummary)]
    L.tscm_covariance_prior.argtypes = [C.POINTER(CProblem), C.c_int, usp, dp, C.c_int, C.c_double, pp, dp, dp, dp, dp, dp, cip]
    L.tscm_projection_uncertainty.argtypes = [C.c_int, dp, dp, dp, C.c_double, C.POINTER(CUncertaintyGrid), C.POINTER(CUncertaintyRequest), C.c_int, C.c_int,
                                              dp, C.POINTER(C.c_ubyte), dp, C.POINTER(C.c_longlong)]
    L.tscm_projection_uncertainty_seconds.argtypes = []
    L.tscm_projection_uncertainty_seconds.restype = C.c_double
    vg = [C.c_int, dp, dp, dp, dp, C.c_int, dp, ip, C.POINTER(CViewGainParams), C.POINTER(CViewCandidate)]
    L.tscm_view_gain.argtypes = vg + [C.c_int, C.c_int, dp, dp, ip, ip]
    L.tscm_view_gain_apply.argtypes = vg + [C.c_int, dp, dp, ip, ip, dp]
    L.tscm_view_gain_seconds.argtypes = []
    L.tscm_view_gain_seconds.restype = C.c_double
    llp_ = C.POINTER(C.c_longlong)
    L.tscm_residual_default_params.argtypes = [C.POINTER(CResidualParams)]
    L.tscm_residual_default_params.restype = None
    L.tscm_residual_report.argtypes = [C.POINTER(CProblem), C.c_int, dp, C.POINTER(CResidualParams), dp, dp, ip, dp, llp_, dp, llp_, dp,
                                       C.POINTER(CResidualInfo)]
    L.tscm_residual_debug_chunk_target.argtypes = [C.c_int]
    L.tscm_residual_debug_chunk_target.restype = None
    L.tscm_project_points.argtypes = [dp, dp, C.c_int, C.c_int, dp]
    L.tscm_unproject_pixels.argtypes = [dp, dp, C.c_int, C.c_int, dp]
    L.tscm_reprojection_error.argtypes = [C.POINTER(CProblem), C.c_int, dp, dp, dp]
    L.tscm_comm_unique_id.argtypes = [C.POINTER(C.c_ubyte)]
    L.tscm_comm_create.argtypes = [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.tscm_comm_destroy.argtypes = [vp]
    L.tscm_comm_destroy.restype = None
    L.tscm_shard_frames.argtypes = [C.POINTER(CProblem), C.c_int, ip]
    L.tscm_rig_init.argtypes = [C.POINTER(CRigInput), C.c_int, C.POINTER(CRigResult)]
    L.tscm_rig_stage_errors.argtypes = [C.POINTER(CRigInput), C.c_int, dp, dp, C.c_int, C.c_int, dp, dp, dp, ip]
    L.tscm_build_maps.argtypes = [C.POINTER(CMapDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                  C.c_size_t, dp]
    L.tscm_build_maps_ex.argtypes = [C.POINTER(CMapDesc), ip, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.c_size_t, dp]
    L.tscm_rectify_points.argtypes = [C.POINTER(CMapDesc), C.c_int, dp, C.c_int, C.c_int, dp, C.POINTER(C.c_ubyte)]
    ubp = C.POINTER(C.c_ubyte)
    L.tscm_stereo_default_params.argtypes = [C.POINTER(CStereoParams)]
    L.tscm_stereo_default_params.restype = None
    L.tscm_stereo_match.argtypes = [ubp, ubp, C.c_int, C.c_int, C.c_int, C.POINTER(CStereoParams), C.c_int, C.POINTER(C.c_short), C.c_int, dp]
    L.tscm_stereo_stages.argtypes = [ubp, ubp, C.c_int, C.c_int, C.c_int, C.POINTER(CStereoParams), C.c_int, C.POINTER(C.c_ulonglong),
                                     C.POINTER(C.c_ulonglong), ubp, usp]
    L.tscm_stereo_stage_times.argtypes = [dp]
    L.tscm_stereo_points.argtypes = [C.POINTER(C.c_short), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(CMapDesc), C.c_int, C.c_double, C.c_int,
                                     dp, ubp]
    L.tscm_stereo_filter_default_params.argtypes = [C.POINTER(CStereoFilterParams)]
    L.tscm_stereo_filter_default_params.restype = None
    L.tscm_stereo_filter.argtypes = [C.POINTER(C.c_short), C.c_int, C.c_int, C.c_int, C.POINTER(CStereoFilterParams), C.c_int, C.POINTER(C.c_short), C.c_int, dp]
    L.tscm_stereo_filter_stages.argtypes = [C.POINTER(C.c_short), C.c_int, C.c_int, C.c_int, C.POINTER(CStereoFilterParams), C.c_int, C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), C.POINTER(C.c_short)]
    L.tscm_stereo_fill_default_params.argtypes = [C.POINTER(CStereoFillParams)]
    L.tscm_stereo_fill_default_params.restype = None
    L.tscm_stereo_fill.argtypes = [C.POINTER(C.c_short), C.c_int, C.c_int, C.c_int, C.POINTER(CStereoFillParams), C.c_int, C.POINTER(C.c_short), C.c_int, ubp, dp]
    L.tscm_stereo_fill_stages.argtypes = [C.POINTER(C.c_short), C.c_int, C.c_int, C.c_int, C.POINTER(CStereoFillParams), C.c_int, C.POINTER(C.c_short),
                                          C.POINTER(C.c_short)]
    L.tscm_stereo_refine_default_params.argtypes = [C.POINTER(CStereoRefineParams)]
    L.tscm_stereo_refine_default_params.restype = None
    L.tscm_stereo_refine_weights.argtypes = [C.c_double, ubp]
    L.tscm_stereo_refine_weights.restype = None
    L.tscm_stereo_refine.argtypes = [C.POINTER(C.c_short), C.c_int, C.c_int, C.c_int, ubp, C.c_int, ubp, C.POINTER(CStereoRefineParams), C.c_int,
                                     C.POINTER(C.c_short), C.c_int, dp]
    L.tscm_stereo_refine_stages.argtypes = [C.POINTER(C.c_short), C.c_int, C.c_int, C.c_int, ubp, C.c_int, ubp, C.POINTER(CStereoRefineParams), C.c_int,
                                            C.POINTER(C.c_int), ubp, C.POINTER(C.c_short)]
    fp, shp, llp, vpp = C.POINTER(C.c_float), C.POINTER(C.c_short), C.POINTER(C.c_longlong), C.POINTER(vp)
    L.tscm_panorama_default_params.argtypes = [C.POINTER(CPanoramaParams)]
    L.tscm_panorama_default_params.restype = None
    L.tscm_panorama_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vpp, fp, fp, C.c_int, C.c_int, C.POINTER(CPanoramaParams), C.c_int, vpp]
    L.tscm_panorama_compose.argtypes = [vp, vpp, C.c_int, usp, ubp, C.c_int, ubp, dp]
    L.tscm_panorama_stages.argtypes = [vp, vpp, C.c_int, usp, ubp, ubp, ubp, ubp, shp, shp]
    L.tscm_panorama_overlap.argtypes = [vp, vpp, C.c_int, llp, llp]
    L.tscm_panorama_destroy.argtypes = [vp]
    L.tscm_panorama_destroy.restype = None
    L.tscm_build_sweep_maps.argtypes = [C.POINTER(CMapDesc), ip, C.c_int, dp, dp, C.c_int, C.c_int, C.c_int, fp, fp, C.c_size_t, dp]
    L.tscm_sweep_default_params.argtypes = [C.POINTER(CSweepParams)]
    L.tscm_sweep_default_params.restype = None
    L.tscm_sweep_create.argtypes = [C.c_int, C.c_int, C.c_int, vpp, fp, fp, C.c_int, C.c_int, C.POINTER(CSweepParams), C.c_int, vpp]
    L.tscm_sweep_depth.argtypes = [vp, vpp, C.c_int, shp, C.c_int, dp]
    L.tscm_sweep_stages.argtypes = [vp, vpp, C.c_int, ubp, ubp, C.POINTER(C.c_ulonglong), ubp, usp]
    L.tscm_sweep_stage_times.argtypes = [dp]
    L.tscm_sweep_points.argtypes = [shp, C.c_int, C.c_int, C.c_int, C.POINTER(CMapDesc), C.c_int, dp, C.c_int, C.c_int, dp, ubp]
    L.tscm_sweep_compose_default_params.argtypes = [C.POINTER(CSweepComposeParams)]
    L.tscm_sweep_compose_default_params.restype = None
    L.tscm_sweep_compose.argtypes = [vp, vpp, C.c_int, C.c_int, shp, C.c_int, C.POINTER(CSweepComposeParams), usp, ubp, C.c_int, ubp, dp]
    L.tscm_sweep_compose_stages.argtypes = [vp, vpp, C.c_int, C.c_int, shp, C.c_int, C.POINTER(CSweepComposeParams), usp, ubp, ubp, ubp, ubp, ubp, shp, shp]
    vis = C.POINTER(CSweepVisibilityParams)
    L.tscm_sweep_visibility_default_params.argtypes = [vis]
    L.tscm_sweep_visibility_default_params.restype = None
    L.tscm_sweep_visibility.argtypes = [vp, shp, C.c_int, vis, ubp, ubp, dp]
    L.tscm_sweep_visibility_stages.argtypes = [vp, shp, C.c_int, vis, ubp, usp, ip, ubp, ubp, ubp]
    L.tscm_sweep_compose_visible.argtypes = [vp, vpp, C.c_int, C.c_int, shp, C.c_int, C.POINTER(CSweepComposeParams), vis, usp, ubp, C.c_int, ubp, dp]
    L.tscm_sweep_compose_visible_stages.argtypes = [vp, vpp, C.c_int, C.c_int, shp, C.c_int, C.POINTER(CSweepComposeParams), vis, usp, ubp, ubp, ubp, ubp, ubp, shp, shp,
                                                    ubp, ubp]
    L.tscm_sweep_destroy.argtypes = [vp]
    L.tscm_sweep_destroy.restype = None
    L.tscm_estimate_focal.argtypes = [dp, dp, ip, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, dp, ip]
    L.tscm_poses_from_r1r2t.argtypes = [dp, C.c_void_p, C.c_int, dp]
    L.tscm_estimate_extrinsic.argtypes = [dp, dp, dp, ip, C.c_int, dp, C.c_int, C.c_int, C.c_int, dp, ip]
    L.tscm_estimate_focal_rows.argtypes = [dp, dp, ip, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, dp]
    L.tscm_estimate_extrinsic_stages.argtypes = [dp, dp, dp, ip, C.c_int, dp, C.c_int, C.c_int, C.c_int, dp, ip, dp, dp, dp, dp, ip, ip]
    rp = C.POINTER(CRansacParams)
    L.tscm_ransac_default_params.argtypes = [rp]
    L.tscm_ransac_default_params.restype = None
    ransac = [dp, dp, dp, ip, C.c_int, dp, C.c_int, C.c_int, rp, C.c_int, dp, ubp, ip, ip, ip, dp]
    L.tscm_estimate_extrinsic_ransac.argtypes = ransac
    L.tscm_estimate_extrinsic_ransac_stages.argtypes = ransac + [ip, ip, ip, dp, dp, dp, dp, dp, ip, dp]
    L.tscm_corners_write.argtypes = [C.c_char_p, C.POINTER(CCornerSet)]
    L.tscm_corners_read.argtypes = [C.c_char_p, C.POINTER(CCornerSet)]
    L.tscm_corners_free.argtypes = [C.POINTER(CCornerSet)]
    L.tscm_corners_free.restype = None
    L.tscm_yaml_format.argtypes = [C.c_int, dp, dp, dp, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tscm_yaml_write.argtypes = [C.c_char_p, C.c_int, dp, dp, dp]
    L.tscm_yaml_parse.argtypes = [C.c_char_p, C.c_int, ip, dp, dp]
    L.tscm_yaml_read.argtypes = [C.c_char_p, C.c_int, ip, dp, dp]
    _lib = L
    return L


def _params_struct(struct, default_fn: str, names, what, over: dict, enums=None):
    """`struct` filled by the library's `default_fn`, then the fields in `over` replaced.  names: the fields a caller may
    set; another one raises TypeError naming `what`, or AttributeError where `what` is None.  enums: {field: (kind, {string:
    value})} for the fields that also take a string."""
    p = struct()
    getattr(lib(), default_fn)(C.byref(p))
    for k, v in over.items():
        if k not in names:                  # the sweep's builders have always raised AttributeError, the stereo ones TypeError with a text
            raise AttributeError(k) if what is None else TypeError(f"unknown {what} parameter {k!r}: one of {', '.join(names)}")
        if enums and k in enums and isinstance(v, str):
            kind, table = enums[k]
            if v not in table:
                raise ValueError(f"unknown {kind} {v!r}: one of {', '.join(table)}")
            v = table[v]
        setattr(p, k, int(v))
    return p


def loss_args(loss) -> tuple:
    """(kind, scale) of the C ABI from None, a kind name, or a (kind name, scale in pixels) pair."""
    if loss is None:
        return LOSS_NONE, 0.0
    if isinstance(loss, str):
        kind, scale = loss, 1.0
    else:
        kind, scale = loss
    if kind not in LOSS_KINDS:
        raise ValueError(f"unknown loss {kind!r}: one of 'huber', 'soft_l1', 'cauchy' or None")
    return LOSS_KINDS[kind], float(scale)


def fixed_masks(fixed, n_cameras: int) -> np.ndarray:
    """The [C] uint16 mask words of the C ABI (TSCM_FIX_*) from
      - None: nothing held (all zero);
      - an int: the same word for every camera;
      - names, e.g. ("cx", "cy") or "lambda": those intrinsics of every camera (INTRINSIC_NAMES);
      - a [C] integer array: one word per camera;
      - a [C, 9] bool array: True = held.
    Unknown names, other shapes and bits above 8 raise ValueError."""
    C_ = int(n_cameras)
    if fixed is None:
        return np.zeros(C_, np.uint16)
    if isinstance(fixed, str):
        fixed = (fixed,)
    if isinstance(fixed, (int, np.integer)) and not isinstance(fixed, bool):
        words = np.full(C_, int(fixed), np.int64)
    elif isinstance(fixed, (tuple, list)) and all(isinstance(x, str) for x in fixed):
        w = 0
        for name in fixed:
            if name not in FIX:
                raise ValueError(f"unknown intrinsic {name!r}: one of {', '.join(INTRINSIC_NAMES)}")
            w |= FIX[name]
        words = np.full(C_, w, np.int64)
    else:
        a = np.asarray(fixed)
        if a.dtype == np.bool_:
            if a.shape != (C_, 9):
                raise ValueError(f"a bool mask has shape [{C_}, 9], not {list(a.shape)}")
            words = (a.astype(np.int64) << np.arange(9, dtype=np.int64)).sum(axis=1)
        elif np.issubdtype(a.dtype, np.integer):
            if a.shape != (C_,):
                raise ValueError(f"an integer mask has shape [{C_}], not {list(a.shape)}")
            words = a.astype(np.int64)
        else:
            raise ValueError(f"fixed must be None, names, a [C] int array or a [C, 9] bool array, not {a.dtype}")
    if np.any(words < 0) or np.any(words & ~FIX_ALL):
        raise ValueError("unknown bits in a fixed-intrinsics mask (bits 0-8: fx fy cx cy xi lambda alpha b c)")
    return words.astype(np.uint16)


def corner_weights(problem, weights=None, built_count=None):
    """The corner weights of a call, and the problem it is made on: -> (problem', w).
    weights: None (then problem.weights), or [n_corners] in corner order -- views in order, the corners of a view in order; a
    bool mask means 0 / 1.  w: C-contiguous float64, or None without weights (problem' is problem then).
    A view whose weights are all 0 goes in with view_count 0, as the C ABI asks: problem' is then a copy of the description
    that shares every array with `problem` but view_count, and w has that view's entries removed.
    built_count (Solver.set_corner_weights): the view_count a solver of `problem` was created with.  The views it was created
    without (count 0 there) stay out whatever their weights are now; any other view whose weights are all 0 raises ValueError."""
    import dataclasses
    w = problem.weights if weights is None else weights
    if w is None:
        return problem, None
    w = np.ascontiguousarray(np.asarray(w), dtype=np.float64).ravel()
    if w.size != problem.n_corners:
        raise ValueError(f"weights: {w.size} entries for {problem.n_corners} corners (one per corner, views in order)")
    cnt = np.asarray(problem.view_count)
    view_of = np.repeat(np.arange(cnt.size), cnt)
    live = np.zeros(cnt.size, dtype=bool)
    live[view_of[w != 0.0]] = True              # (NaN counts as live: the library refuses it by name)
    dead = (cnt > 0) & ~live
    if built_count is not None:
        gone = (cnt > 0) & (np.asarray(built_count) == 0)
        if np.any(dead & ~gone):
            raise ValueError("a view's weights are all 0: create the Solver with weights= so that the view goes in with view_count 0")
        dead = gone
    if not dead.any():
        return problem, w
    q = dataclasses.replace(problem, view_count=np.where(dead, 0, cnt).astype(np.int32), weights=None)
    return q, np.ascontiguousarray(w[~dead[view_of]])


class CameraPriors:
    """Gaussian priors on camera-side coordinates (tscm.h: tscm_camera_priors) -- Ceres' NormalPrior on single coordinates:
    residual sqrt(weight) * (x - mean) per coordinate with a weight > 0.  cam_rt_mean / cam_rt_weight [C, 6] on the raw pose
    vectors, intr_mean / intr_weight [C, 9] on fx fy cx cy xi lambda alpha b c; either pair may be None.  The library checks the
    values; a weight on a coordinate that is not free in a solve counts as 0 there.  api.camera_priors() builds one from sigmas."""

    def __init__(self, cam_rt_mean=None, cam_rt_weight=None, intr_mean=None, intr_weight=None):
        as_array = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        self.cam_rt_mean, self.cam_rt_weight = as_array(cam_rt_mean), as_array(cam_rt_weight)
        self.intr_mean, self.intr_weight = as_array(intr_mean), as_array(intr_weight)

    def c_struct(self, n_cameras: int) -> CCameraPriors:
        """The struct of the C ABI; it references this object's arrays: keep the object alive."""
        q = CCameraPriors(struct_size=C.sizeof(CCameraPriors))
        for name, per in (("cam_rt_mean", 6), ("cam_rt_weight", 6), ("intr_mean", 9), ("intr_weight", 9)):
            a = getattr(self, name)
            if a is not None:
                if a.size != per * n_cameras:
                    raise ValueError(f"priors.{name}: {a.size} entries for {n_cameras} cameras ([C, {per}])")
                setattr(q, name, a.ctypes.data)
        return q


def priors_ptr(priors, n_cameras: int):
    """(pointer argument of the C ABI, what to keep alive) for None or a CameraPriors"""
    if priors is None:
        return None, None
    if not isinstance(priors, CameraPriors):
        raise TypeError("priors must be None or a lib.CameraPriors (api.camera_priors builds one)")
    q = priors.c_struct(n_cameras)
    return C.byref(q), (q, priors)


def ushort_ptr(a: np.ndarray):
    assert a.dtype == np.uint16 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_ushort))


def check(rc: int) -> None:
    if rc != 0:
        raise TscmError(rc, lib().tscm_last_error().decode(errors="replace"))


def dptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def c_problem(p) -> CProblem:
    """Wrap a normalised Problem. Arrays are referenced, not copied: keep `p` alive."""
    q = CProblem()
    q.n_cameras, q.n_boards, q.n_points, q.n_views = p.n_cameras, p.n_boards, p.n_points, p.n_views
    for name in ("board_xy", "view_camera", "view_board", "view_offset", "view_count", "obs_u", "obs_v",
                 "cam_rt", "intr", "board_rt", "cam_pose_constant"):
        arr = getattr(p, name)
        if not arr.flags["C_CONTIGUOUS"]:
            raise ValueError(f"{name} must be C-contiguous (use Problem.normalised())")
        setattr(q, name, arr.ctypes.data)
    q.mono = 1 if p.mono else 0
    bpc = getattr(p, "board_pose_constant", None)
    if bpc is not None:
        if bpc.dtype != np.uint8 or not bpc.flags["C_CONTIGUOUS"]:
            raise ValueError("board_pose_constant must be C-contiguous uint8 (use Problem.normalised())")
        q.board_pose_constant = bpc.ctypes.data
    return q


def default_options(mono: bool, **over) -> COptions:
    o = COptions()
    lib().tscm_default_options(C.byref(o), 1 if mono else 0)
    for k, v in over.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def summary_dict(s: CSummary) -> dict:
    its = []
    for i in range(min(s.num_iterations, MAX_ITERATIONS + 1)):
        it = s.iterations[i]
        its.append({k: getattr(it, k) for k, _ in CIteration._fields_})
    return dict(termination_type=s.termination_type, termination=TERMINATION.get(s.termination_type, "?"),
                num_iterations=s.num_iterations, num_successful_steps=s.num_successful_steps,
                num_unsuccessful_steps=s.num_unsuccessful_steps, initial_cost=s.initial_cost,
                final_cost=s.final_cost, n_residual_blocks=s.n_residual_blocks, lm_iterations=s.lm_iterations,
                iterations=its, message=s.message.decode(), seconds_solve=s.seconds_solve,
                seconds_total=s.seconds_total, rmse=s.rmse)


class CCornerCandidates(C.Structure):
    """tscm_corner_candidates (tscm.h)"""
    _fields_ = [("n", C.c_int), ("n_maxima", C.c_int),
                ("x", C.POINTER(C.c_double)), ("y", C.POINTER(C.c_double)),
                ("v1", C.POINTER(C.c_double)), ("v2", C.POINTER(C.c_double)),
                ("score", C.POINTER(C.c_double)), ("sub", C.POINTER(C.c_double)),
                ("seconds", C.c_double)]


class CBoardSeedStages(C.Structure):
    """tscm_board_seed_stages (tscm.h)"""
    _fields_ = [("n", C.c_int), ("on_device", C.c_int), ("status", C.POINTER(C.c_int)), ("rows", C.POINTER(C.c_int)), ("cols", C.POINTER(C.c_int)),
                ("steps", C.POINTER(C.c_int)), ("energy", C.POINTER(C.c_double)), ("offset", C.POINTER(C.c_int)), ("cells", C.POINTER(C.c_int))]


BOARDS_HOST, BOARDS_DEVICE, BOARDS_MAX_DEVICE_CANDIDATES = 0, 1, 1024


class CChessboards(C.Structure):
    """tscm_chessboards (tscm.h)"""
    _fields_ = [("n_boards", C.c_int), ("rows", C.POINTER(C.c_int)), ("cols", C.POINTER(C.c_int)),
                ("offset", C.POINTER(C.c_int)), ("cells", C.POINTER(C.c_int))]
