/*
 * tscm.h -- C ABI of the MI355X-native Triple-Sphere reprojection-error LM solver.
 *
 * Drop-in boundary for the hot path of imuncle/TSCM_Calib:
 * plain pointers and sizes, caller-owned parameter arrays updated in place -- the same
 * contract the reference has with Ceres, which identifies parameter blocks by pointer
 * (`intrinsic_.data()`, `rt_[i].data()`: TS.cpp:266-267, multi_calib.cpp:182-184).
 * Every entry point names the reference interface it replaces.  INTEGRATION.md shows
 * the reference-side binding (the body of MultiCalib::calibrate() /
 * TripleSphereCamera::refinement() rewritten onto these calls).
 *
 * All entry points return 0 on success or a negative TSCM_E_* code;
 * tscm_last_error() returns a thread-local description of the last failure.
 * The library never falls back to a CPU path: without a usable HIP device every
 * compute entry point fails with TSCM_E_NO_DEVICE.
 */
#ifndef TSCM_H
#define TSCM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSCM_ABI_VERSION 6   /* 2: tscm_problem.board_pose_constant; 3: tscm_options.exec_flags (both appended;  */
                             /*    zero-initialised structs keep their meaning); 4: unknown exec_flags bits are  */
                             /*    refused, TSCM_EXEC_DENSE_REDUCED_ORDER, the fault injection of the tests is   */
                             /*    an entry point of its own (tscm_solver_debug_withhold_handoff), no option;    */
                             /* 5: tscm_comm_ipc_open / tscm_comm_ipc_connect, tscm_device_peak_fp32_mfma,       */
                             /*    TSCM_EXEC_GRAPH_REDUCED_ORDER (no struct changed);                            */
                             /* 6: tscm_options starts with struct_size (the third appended field in four rounds */
                             /*    was the moment): the library reads only as many bytes as the caller's struct  */
                             /*    has and refuses a size it does not know -- an options struct of ABI <= 5 is   */
                             /*    refused instead of misread; TSCM_E_PEER; a late device-side hand-off re-runs  */
                             /*    the solve on separate launches before it is an error; TSCM_EXEC_SEPARATE_STATS */
                             /*    (no struct changed; a library without the bit refuses it)                     */

enum {
    TSCM_OK = 0,
    TSCM_E_INVALID = -1,      /* bad argument / inconsistent problem description      */
    TSCM_E_NO_DEVICE = -2,    /* no HIP device, or hipSetDevice failed                */
    TSCM_E_HIP = -3,          /* a HIP runtime call failed                            */
    TSCM_E_RCCL = -4,         /* an RCCL call failed (the communicator is aborted)    */
    TSCM_E_UNSUPPORTED = -5,  /* problem shape outside what the kernels support       */
    TSCM_E_NOMEM = -6,
    TSCM_E_PEER = -7          /* the IPC exchange back-end: a peer rank did not arrive within its time bound, or its */
                              /* memory could not be mapped (the communicator is unusable afterwards, like an        */
                              /* aborted RCCL communicator)                                                          */
};

/* ceres::TerminationType values the reference looks at (TS.cpp:281). */
enum { TSCM_CONVERGENCE = 0, TSCM_NO_CONVERGENCE = 1, TSCM_FAILURE = 2 };

#define TSCM_MAX_ITERATIONS 255

/*
 * Problem = what multi_calib.cpp:157-207 / TS.cpp:249-269 feed to ceres::Problem.
 *
 * A "view" is one (camera m, board i) pair with detected corners, i.e. a non-empty
 * cameras_[m].pixels()[i] with chessboards_[i].is_initial() (multi_calib.cpp:164-169);
 * corner j of the view is paired with board point worlds_[j] (:176).  Mono: a view is
 * an image with has_chessboard_[i] (TS.cpp:253), camera index 0, board index = image.
 *
 * Parameter layout is the reference's: intrinsics `fx fy cx cy xi lambda alpha b c`
 * (TS.h:105, multi_calib.h:22), poses = angle-axis (rad) then translation in board
 * units (TS.cpp:72, multi_calib.h:17).  b and c are inert (their terms are commented
 * out in both functors: TS.h:122-123, multi_calib.h:175-176) and are returned unchanged.
 */
typedef struct tscm_problem {
    int n_cameras;                 /* C                                                */
    int n_boards;                  /* B  (mono: number of images)                      */
    int n_points;                  /* board corners, e.g. 54 or 88                     */
    int n_views;
    const double *board_xy;        /* [n_points*2]  worlds_[j].x, .y (z forced to 0:   */
                                   /*   TS.h:107-109, multi_calib.h:154-156)           */
    const int *view_camera;        /* [n_views]                                        */
    const int *view_board;         /* [n_views]                                        */
    const int *view_offset;        /* [n_views] first corner of the view in obs_u/v    */
    const int *view_count;         /* [n_views] pixels[i].size()  (0..n_points)        */
    const double *obs_u;           /* [N] observed pixel x, SoA                        */
    const double *obs_v;           /* [N] observed pixel y                             */
    double *cam_rt;                /* [C*6] cameras_[m].rt_        in/out (host)       */
    double *intr;                  /* [C*9] cameras_[m].intrinsic_ in/out (host)       */
    double *board_rt;              /* [B*6] chessboards_[i].rt_ / rt_[i]  in/out (host)*/
    const unsigned char *cam_pose_constant; /* [C] SetParameterBlockConstant           */
                                   /*   (multi_calib.cpp:186: camera 0); NULL = none   */
    int mono;                      /* 1: TS.h functor -- no camera pose block at all   */
    const unsigned char *board_pose_constant; /* [B] 1 = the board's pose block is held    */
                                   /*   constant (problem.SetParameterBlockConstant on */
                                   /*   chessboards_[i].rt_ / rt_[i]); NULL = none.    */
                                   /*   The reference never does this; it is the       */
                                   /*   "intrinsics-only" form of BASELINE config 2    */
                                   /*   (all views fixed: 7 free intrinsics remain).   */
} tscm_problem;

/* ceres::Solver::Options fields the path depends on, Ceres defaults
 * (TS.cpp:271-274, multi_calib.cpp:209-212; linear solver is always DENSE_SCHUR). */
typedef struct tscm_options {
    size_t struct_size;                  /* sizeof(tscm_options) of the CALLER's header */
                                         /* (tscm_default_options sets it).  Fields     */
                                         /* behind it that the caller's struct does not */
                                         /* have take their defaults; 0 or an unknown   */
                                         /* size: TSCM_E_INVALID                        */
    int max_num_iterations;              /* 100 mono (TS.cpp:274) / 50 multi           */
    double function_tolerance;           /* 1e-6                                       */
    double gradient_tolerance;           /* 1e-10                                      */
    double parameter_tolerance;          /* 1e-8                                       */
    double initial_trust_region_radius;  /* 1e4                                        */
    double max_trust_region_radius;      /* 1e16                                       */
    double min_trust_region_radius;      /* 1e-32                                      */
    double min_relative_decrease;        /* 1e-3                                       */
    double min_lm_diagonal;              /* 1e-6.  As in Ceres, 0 (or a value that     */
                                         /* underflows over the radius) makes every    */
                                         /* step invalid while an intrinsic without a  */
                                         /* Jacobian column (b, c) is not held: its    */
                                         /* damped pivot is 0                          */
    double max_lm_diagonal;              /* 1e32                                       */
    int max_num_consecutive_invalid_steps; /* 5                                        */
    int jacobi_scaling;                  /* 1                                          */
    int check_every;                     /* host polls the device-resident LM loop     */
                                         /* every this many iterations (default 4)     */
    int jacobian_fp32;                   /* 0 (default): everything fp64, 1e-6 tier.   */
                                         /* 1: derivatives and the J^T J contraction in */
                                         /* fp32 (packed VALU + fp32 MFMA), projection, */
                                         /* residuals, cost and the whole linear solve  */
                                         /* stay fp64: north_star's 1e-3 tier          */
    int exec_flags;                      /* 0 (default).  Execution variants that do   */
                                         /* not change the mathematics (TSCM_EXEC_*)   */
} tscm_options;

/* tscm_options.exec_flags.  They select code paths for A/B runs and for tests that a one-GPU box would otherwise never
 * run; none of them changes the mathematics, all but the last two give the same bits.  Bits outside TSCM_EXEC_ALL are
 * refused with TSCM_E_INVALID (a caller built against an options struct without the field passes garbage here). */
enum {
    TSCM_EXEC_SEPARATE_T_REDUCE = 1,       /* keep the Schur-complement tile reduction a launch of its own instead of   */
                                           /* riding in the reduced solve's launch (what every communicator run does)   */
    TSCM_EXEC_KEEP_SINGLE_RANK_COMM = 2,   /* run the communicator code path (two all-reduces, separate control step)   */
                                           /* even when the attached communicator has one rank                          */
    TSCM_EXEC_GRAM_16X16 = 4,              /* the Gram contraction of the dominant kernel on v_mfma_f64_16x16x4 (one tile,  */
                                           /* rounds 1-3a) instead of three v_mfma_f64_4x4x4_4b per four rows (A/B runs)   */
    TSCM_EXEC_SEPARATE_BACKSUB = 8,        /* keep the back-substitution a launch of its own instead of workgroups that   */
                                           /* wait for the camera step inside the reduced solve's launch (one GPU)        */
    TSCM_EXEC_SEPARATE_CONTROL = 16,       /* take the LM control step in the reductions' launch (k_reduce_control) instead  */
                                           /* of in the head of the next Schur-complement kernel (one GPU)                    */
    TSCM_EXEC_DENSE_REDUCED_ORDER = 32,    /* k_solve_nd (rigs of 5-8 cameras) factors the reduced camera system as ONE dense  */
                                           /* block instead of along the camera-pair graph (same solution to rounding)       */
    TSCM_EXEC_GRAPH_REDUCED_ORDER = 64,    /* rigs of up to 4 cameras: k_solve_nd along the camera-pair graph instead of the  */
                                           /* dense k_solve_reduced (which is faster there: tests and A/B runs)               */
    TSCM_EXEC_SEPARATE_STATS = 128,        /* keep the reductions behind a candidate's evaluation (k_reduce_stats) a launch of  */
                                           /* their own instead of the first workgroups of the next Schur-complement launch    */
    TSCM_EXEC_ALL = 255
};

/* ceres::IterationSummary subset */
typedef struct tscm_iteration {
    int iteration;
    int step_is_valid;
    int step_is_successful;
    double cost;
    double cost_change;
    double gradient_max_norm;
    double gradient_norm;
    double step_norm;
    double relative_decrease;
    double trust_region_radius;
} tscm_iteration;

/* ceres::Solver::Summary subset (what BriefReport prints: TS.cpp:280, multi_calib.cpp:218)
 * plus the error report of multi_calib.cpp:233-283. */
typedef struct tscm_summary {
    int termination_type;          /* TSCM_CONVERGENCE / NO_CONVERGENCE / FAILURE      */
    int num_iterations;            /* entries in iterations[] (iteration 0 included)   */
    int num_successful_steps;
    int num_unsuccessful_steps;
    double initial_cost;
    double final_cost;
    int n_residual_blocks;         /* corners in the program                           */
    int lm_iterations;             /* LM iterations executed (incl. a final one that   */
                                   /*   ended on a tolerance test)                     */
    tscm_iteration iterations[TSCM_MAX_ITERATIONS + 1];
    char message[128];
    double seconds_solve;          /* minimiser loop on the device: first to last kernel */
    double seconds_total;          /* wall time of the call (tscm_solve_*: incl. upload/download) */
    double rmse;                   /* sqrt(2*final_cost/N); with a robust loss (below) */
                                   /*   the plain pixel RMSE at the final parameters,  */
                                   /*   what tscm_reprojection_error returns           */
} tscm_summary;

typedef struct tscm_solver tscm_solver;   /* opaque: device buffers, stream, layouts  */
typedef struct tscm_comm tscm_comm;       /* opaque: RCCL communicator                */

int tscm_abi_version(void);
const char *tscm_last_error(void);
int tscm_device_count(void);
/* hipSetDevice(device) + hipDeviceSynchronize(): lets a host (e.g. the multi-process benchmark) fence the
 * GPU without loading a second HIP runtime of its own. */
int tscm_device_synchronize(int device);
/* Measured fp64 ceilings of the device, every CU busy: v_mfma_f64_16x16x4_f64 and v_fma_f64 throughput in TFLOP/s
 * (a few milliseconds of micro-kernels; benchmark / roofline reporting only, not on any solver path). */
int tscm_device_peak_fp64(int device, double *mfma_tflops, double *valu_tflops);
/* ... with the two fp64 matrix instructions apart: peaks[0] = v_mfma_f64_16x16x4_f64 (the instruction of rounds 1-3a: about
 * half the datasheet rate on gfx950), peaks[1] = v_mfma_f64_4x4x4_4b_f64 (the one the dominant kernel uses since round 3:
 * the datasheet rate), peaks[2] = v_fma_f64; TFLOP/s. */
int tscm_device_peak_fp64_ex(int device, double peaks[3]);
/* ... and of v_mfma_f32_16x16x4_f32, the contraction of the fp32-Jacobian tier (tscm_options.jacobian_fp32), TFLOP/s */
int tscm_device_peak_fp32_mfma(int device, double *tflops);

void tscm_default_options(tscm_options *opt, int mono);

/* ------------------------------------------------------------------ solver handle
 * tscm_solver_create  uploads observations and builds the device layout once
 *                     (replaces the per-corner `new ReprojectionError` +
 *                     AddResidualBlock loops: TS.cpp:251-269, multi_calib.cpp:162-207).
 * tscm_solver_solve   = ceres::Solve(options, &problem, &summary)
 *                     (TS.cpp:278, multi_calib.cpp:216).  Reads the initial parameters
 *                     from the problem's cam_rt / intr / board_rt host arrays and
 *                     overwrites them with the result, like Ceres does.
 * Shapes served (anything else: TSCM_E_UNSUPPORTED, nothing is approximated): up to 32 cameras (1..8: reduced
 * system solved in registers/LDS, 9..32: blocked factorisation in global memory), any board shape whose corner
 * list fits the 160 KiB LDS tile (several thousand corners), up to 3.7 M views / 536 M corners per GPU.
 */
int tscm_solver_create(const tscm_problem *problem, int device, tscm_solver **out);
int tscm_solver_set_comm(tscm_solver *s, tscm_comm *comm);   /* frame-sharded multi-GPU, see below */
/* A hand-off between workgroups of one launch (evaluation's reductions -> control step; Schur-complement tiles -> reduced
 * solve -> back-substitution) that does not
 * come within its time bound (0.5 s: a debugger, a co-tenant, a context switch -- or a fault) stops the solve on the
 * device; the library then runs THAT solve again from its start point on the launches that hand nothing over inside a
 * launch (TSCM_EXEC_SEPARATE_T_REDUCE | _BACKSUB | _CONTROL, which implies _STATS: same mathematics, same bits) and returns its result;
 * tscm_last_error() carries a note, tscm_solver_reruns() counts them.  TSCM_E_HIP only if the re-run fails too -- or
 * with a communicator of several ranks, which would have to agree on it.
 * TESTS ONLY: tscm_solver_debug_withhold_handoff(s, 1): in the next solve of `s` one producer of the hand-off never
 * reports in (the solve must come back re-run, within seconds); (s, 2): ... and the re-run is forbidden: that solve
 * must end with TSCM_E_HIP within the time bound, the caller's parameters untouched, the solver usable afterwards;
 * (s, 3): like 1 for the other hand-off of an iteration -- one of the reductions behind the evaluation that ride in
 * the Schur-complement launch never counts itself in. */
int tscm_solver_debug_withhold_handoff(tscm_solver *s, int on);
/* TESTS ONLY: which wave of a Schur-complement workgroup contracts which boards of its chunk does not change a bit of a
 * solve.  rot = 0 (the default) or 2: every workgroup of every later solve of `s` starts its deal at wave 0 / wave 2. */
int tscm_solver_debug_schur_rot(tscm_solver *s, int rot);
/* TESTS AND A/B RUNS ONLY: rigs of up to four cameras take their camera step out of the reduced system's factorisation
 * where the column plan allows it; on = 1 makes every later solve of `s` back-substitute behind the factorisation
 * instead (what a plan that does not fit does anyway), 0 is the default.  s NULL: the default of the solvers this
 * process creates from now on, those of the one-shot entry points among them.  Same mathematics, last bits differ. */
int tscm_solver_debug_reduced_backsub(tscm_solver *s, int on);
int tscm_solver_reruns(const tscm_solver *s);                /* solves of `s` that were run again so far (>= 0) */
int tscm_solver_solve(tscm_solver *s, const tscm_options *opt, tscm_summary *summary);
/* Same as _solve but parameters start from / are left in device memory (used by the
 * benchmark to time the minimiser loop with inputs resident in HBM). reset=1 reloads
 * the parameters that were uploaded by the last tscm_solver_upload_params. */
int tscm_solver_upload_params(tscm_solver *s, const double *cam_rt, const double *intr, const double *board_rt);
int tscm_solver_solve_resident(tscm_solver *s, const tscm_options *opt, tscm_summary *summary, int reset);
int tscm_solver_download_params(tscm_solver *s, double *cam_rt, double *intr, double *board_rt);
void tscm_solver_destroy(tscm_solver *s);
/* timing of the dominant kernel (k_eval_gram) by HIP events on the solver's own stream, accumulated since the last
 * call: returns the number of timed launches and their total milliseconds, and (re)arms the timers --
 * enable = 0: off; n >= 1: bracket every n-th launch (an event pair delays the stream by a few microseconds, so a
 * benchmark samples instead of timing every launch). */
int tscm_solver_kernel_time(tscm_solver *s, int enable, int *launches, double *total_ms);
/* ... and of the two per-iteration exchanges of a sharded solve (the all-reduce of the Schur-complement tiles T and of
 * the staged camera tiles H_stage; the reference has no counterpart -- SURVEY 5: "measure it separately from compute"),
 * sampled at the same rate while tscm_solver_kernel_time has the timers armed: number of timed collectives and their
 * total milliseconds since the last call.  Zeros without a communicator. */
int tscm_solver_exchange_time(tscm_solver *s, int *n_T, double *ms_T, int *n_H, double *ms_H);

/* Refusal order of the one-shot entry points ------------------------------------
 * tscm_solve_*, tscm_eval_step_* and tscm_eval_normal_equations_* are each one path behind
 * several spellings: an export without a loss, a mask, weights or priors is the most general
 * one of its family (_prior) called with TSCM_LOSS_NONE and NULLs, bit for bit.  All of them
 * refuse, before any device is touched and in this order:
 *   1. the loss: an unknown kind, a scale that is not finite and > 0;
 *   2. NULL arguments (tscm_solve_multi / _mono: their mono / multi guard);
 *   3. the mask: bits 9 and up;
 *   4. the options struct: a struct_size this library does not know;
 *   5. the option values: max_num_iterations, unknown exec_flags bits, TSCM_EXEC_GRAM_16X16
 *      with a loss or with weights (TSCM_E_UNSUPPORTED);
 *   6. the problem, then the weights, then the camera priors.
 * All TSCM_E_INVALID unless said otherwise.  The device index (TSCM_E_NO_DEVICE) and what the
 * device cannot hold (TSCM_E_UNSUPPORTED) follow.  tscm_solve_mono_batch* and tscm_covariance*
 * state their own order below.
 *
 * One-shot drop-ins ------------------------------------------------------------
 * tscm_solve_multi replaces the Ceres block of MultiCalib::calibrate()
 *                  (multi_calib.cpp:157-218); the caller then runs update_param()
 *                  (multi_calib.cpp:221-232) on its own objects.
 * tscm_solve_mono  replaces TripleSphereCamera::refinement (TS.cpp:247-282); the
 *                  reference's `return summary.termination_type == CONVERGENCE`
 *                  is `summary->termination_type == TSCM_CONVERGENCE`.             */
int tscm_solve_multi(const tscm_problem *problem, const tscm_options *opt, tscm_summary *summary);
int tscm_solve_mono(const tscm_problem *problem, const tscm_options *opt, tscm_summary *summary);

/* ------------------------------------------------------------------ operator level
 * Batched cost-functor evaluation = ceres::CostFunction::Evaluate of
 * AutoDiffCostFunction<ReprojectionError,2,6,6,9> (multi_calib.h:138-199) /
 * <...,2,9,6> (TS.h:93-134) for every corner of the problem, on the GPU, with the
 * analytic Jacobian.  Corner order = views in problem order, corners in order.
 * residuals [N*2]; J_cam [N*2*6], J_board [N*2*6], J_intr [N*2*9] row-major per corner
 * (any of the three may be NULL).  cost = 0.5*sum r^2.  Host pointers.            */
int tscm_eval_functor(const tscm_problem *problem, int device, double *residuals,
                      double *J_cam, double *J_board, double *J_intr, double *cost);

/* Schur-form normal equations at the problem's current parameters (the quantities
 * Ceres' SchurEliminator forms from the Jacobian), for parity tests.  Outputs (host,
 * any may be NULL):  board_gram [B*36] = sum E^T E ; board_grad [B*6] = E^T r ;
 * view_cross [n_views*6*15] = E^T [F_campose(6) F_intr(9)] per view ;
 * cam_gram [C*15*15] = F^T F per camera ; cam_grad [C*15] = F^T r ; cost.
 * All UNSCALED (no Jacobi scaling, no damping).                                    */
int tscm_eval_normal_equations(const tscm_problem *problem, int device, double *board_gram,
                               double *board_grad, double *view_cross, double *cam_gram,
                               double *cam_grad, double *cost);

/* The same, formed by the Gram kernel a solve with `opt` runs (NULL = defaults, which
 * is tscm_eval_normal_equations): opt->jacobian_fp32 selects the fp32-Jacobian tier,
 * opt->exec_flags & TSCM_EXEC_GRAM_16X16 the 16x16-tile kernel; the other flags do not
 * change the evaluation and are ignored.                                            */
int tscm_eval_normal_equations_ex(const tscm_problem *problem, int device, const tscm_options *opt,
                                  double *board_gram, double *board_grad, double *view_cross,
                                  double *cam_gram, double *cam_grad, double *cost);

/* At the problem's parameters: the candidate point of the first trust-region step that
 * a solve with `opt` takes (NULL = defaults).  The radius is
 * opt->initial_trust_region_radius; the step also follows opt's LM diagonal clamps,
 * jacobi_scaling, jacobian_fp32 and exec_flags.  Termination tolerances are ignored.
 * cam_rt [C*6] (may be NULL for a mono problem), intr [C*9], board_rt [B*6] receive
 * x + delta exactly as that solve evaluates it; constant blocks come back as their input.
 * *valid = 0 if the step is invalid (the linear solve failed: no candidate).  summary
 * (may be NULL) = the one-iteration summary.  For parity tests.                      */
int tscm_eval_step_ex(const tscm_problem *problem, int device, const tscm_options *opt,
                      double *cam_rt, double *intr, double *board_rt, int *valid,
                      tscm_summary *summary);

/* ------------------------------------------------------------------ robust losses
 * The loss function of ceres::Problem::AddResidualBlock, for every residual block (one corner,
 * r = (r_u, r_v), s = |r|^2) of the problem.  Ceres' own HuberLoss(a), SoftLOneLoss(a) and
 * CauchyLoss(a) with scale a > 0 in pixels (b = a^2):
 *   HUBER    rho = s (s <= b), 2 a sqrt(s) - b (s > b)
 *   SOFT_L1  rho = 2 b (sqrt(1 + s / b) - 1)
 *   CAUCHY   rho = b log(1 + s / b)
 * The cost of a block is rho(s) / 2: initial_cost, final_cost, the iteration costs, cost_change and
 * relative_decrease all use it; the gradient, the normal equations and the tolerance tests use the
 * Jacobian and residual scaled by sqrt(rho'(s)) (Ceres' Corrector: rho'' <= 0 for all three losses,
 * so no rank-one term).  TSCM_LOSS_NONE is the plain least-squares solve, bit for bit.
 * An unknown kind, or a scale that is not finite or <= 0: TSCM_E_INVALID.  A loss with
 * TSCM_EXEC_GRAM_16X16: TSCM_E_UNSUPPORTED.
 *   new ceres::HuberLoss(1.0)  ->  tscm_solver_set_loss(s, TSCM_LOSS_HUBER, 1.0)              */
enum { TSCM_LOSS_NONE = 0, TSCM_LOSS_HUBER = 1, TSCM_LOSS_SOFT_L1 = 2, TSCM_LOSS_CAUCHY = 3 };
/* the loss of every later solve / solve_resident of s (scale ignored for TSCM_LOSS_NONE).  The shards
 * of a local group must carry the same loss (tscm_solver_solve_group: TSCM_E_INVALID otherwise); with
 * an RCCL or IPC communicator every rank must set the same loss -- this is not checked.            */
int tscm_solver_set_loss(tscm_solver *s, int kind, double scale);
/* tscm_solve_mono or tscm_solve_multi (by problem->mono) with a loss                               */
int tscm_solve_robust(const tscm_problem *problem, const tscm_options *opt, int kind, double scale, tscm_summary *summary);
/* tscm_eval_normal_equations_ex / tscm_eval_step_ex with a loss: the outputs are the corrected
 * (sqrt(rho')-scaled) normal equations, *cost = sum rho / 2                                        */
int tscm_eval_normal_equations_robust(const tscm_problem *problem, int device, const tscm_options *opt, int kind, double scale,
                                      double *board_gram, double *board_grad, double *view_cross,
                                      double *cam_gram, double *cam_grad, double *cost);
int tscm_eval_step_robust(const tscm_problem *problem, int device, const tscm_options *opt, int kind, double scale,
                          double *cam_rt, double *intr, double *board_rt, int *valid, tscm_summary *summary);
/* The outputs of tscm_eval_normal_equations_ex at the problem's parameters, from a solver (one rank;
 * a sharded one: TSCM_E_UNSUPPORTED) and with its loss (tscm_solver_set_loss).  as_solved != 0: from
 * the evaluation launch exactly as a solve makes it -- the default Gram kernel forms no rotation
 * columns for a camera whose pose block is constant (cam_pose_constant, every camera of a mono
 * problem): the reduced system has no column for them.  Those rows and columns of cam_gram /
 * cam_grad and columns 0-2 of such a view's view_cross are exactly 0 on a solver that has evaluated
 * nothing else; every other entry has the bits of as_solved == 0.  With jacobian_fp32 or
 * TSCM_EXEC_GRAM_16X16 both give the same.  The solver's next solve starts afresh.               */
int tscm_solver_eval_normal_equations(tscm_solver *s, const tscm_options *opt, int as_solved,
                                      double *board_gram, double *board_grad, double *view_cross,
                                      double *cam_gram, double *cam_grad, double *cost);

/* ------------------------------------------------------------------ held intrinsics
 * A mask word per camera: bit k holds intrinsic k of fx fy cx cy xi lambda alpha b c (the 9-vector of
 * tscm_problem.intr) at the value it has when the solve starts.  Ceres' semantics:
 *   - some of bits 0-6: SubsetManifold on the camera's intrinsic block.  Held coordinates leave the
 *     tangent space -- no column of the reduced system, no Jacobi scale, no LM diagonal, nothing in
 *     the gradient norms (|x - Plus(x, -g)| is 0 there), the step or the step norm -- but their values
 *     still count in x_norm (Ceres' ambient state), as b and c do.  Held values come back bit-identical.
 *   - all of bits 0-6: SetParameterBlockConstant on the block, which leaves the program and x_norm like
 *     a constant camera pose (tscm_problem.cam_pose_constant).
 *   - bits 7-8 (b, c): b and c are inert in the model -- no Jacobian column, never moved -- and holding them changes no
 *     step.  As in Ceres they count as columns of the program while their block is in it and they are not held: their LM
 *     diagonal is clamp(0, min_lm_diagonal, max_lm_diagonal) / radius, and where that is not > 0 (min_lm_diagonal = 0) the
 *     factorisation fails and every step is invalid.  Holding both, or all of bits 0-6, takes them out.
 *   - bits 9 and up: TSCM_E_INVALID.
 *   - mask 0 for every camera (or fixed = NULL) is the solve without held intrinsics, bit for bit.
 * Lambda = 0 makes the Triple Sphere model the Double Sphere model, xi = lambda = 0 the Unified Camera
 * Model: TSCM_MODEL_DS / TSCM_MODEL_UCM with lambda (and xi) at 0 calibrate those models.
 *   SetManifold(intrinsic_.data(), new SubsetManifold(9, {2, 3}))  ->  fixed[m] = TSCM_FIX_CX | TSCM_FIX_CY */
enum {
    TSCM_FIX_FX = 1, TSCM_FIX_FY = 2, TSCM_FIX_CX = 4, TSCM_FIX_CY = 8, TSCM_FIX_XI = 16, TSCM_FIX_LAMBDA = 32,
    TSCM_FIX_ALPHA = 64, TSCM_FIX_B = 128, TSCM_FIX_C = 256,
    TSCM_FIX_INTRINSICS = 127, TSCM_FIX_ALL = 511,
    TSCM_MODEL_DS = TSCM_FIX_LAMBDA, TSCM_MODEL_UCM = TSCM_FIX_XI | TSCM_FIX_LAMBDA
};
/* the held intrinsics of every later solve / solve_resident of s: fixed[n_cameras], or NULL for none.
 * May be called between solves.  The shards of a local group must hold the same intrinsics
 * (tscm_solver_solve_group: TSCM_E_INVALID otherwise); with an RCCL or IPC communicator every rank
 * must set the same masks -- this is not checked.                                                   */
int tscm_solver_set_fixed_intrinsics(tscm_solver *s, const unsigned short *fixed);
/* tscm_solve_robust with held intrinsics (kind TSCM_LOSS_NONE: no loss)                              */
int tscm_solve_fixed(const tscm_problem *problem, const tscm_options *opt, const unsigned short *fixed, int kind, double scale,
                     tscm_summary *summary);
/* tscm_eval_step_robust with held intrinsics                                                         */
int tscm_eval_step_fixed(const tscm_problem *problem, int device, const tscm_options *opt, const unsigned short *fixed, int kind,
                         double scale, double *cam_rt, double *intr, double *board_rt, int *valid, tscm_summary *summary);

/* n independent TripleSphereCamera::refinement problems (TS.cpp:247-282) solved together on one device -- main.cpp's
 * per-camera monocular_calib refinements in one call.  Every problem is solved exactly as
 * tscm_solve_fixed(problems[k], opt, fixed ? fixed + k : NULL, kind, scale) would solve it alone: its own trust region,
 * its own termination, its own summary (to rounding: the batched route has its own kernels).  Parameters are updated in
 * place in each problem's arrays; a problem that has terminated is frozen while the others go on.
 *   - opt and the loss are shared; fixed[k] (or NULL) is problem k's mask (TSCM_FIX_*, TSCM_MODEL_DS / _UCM).
 *   - every problem: mono, n_cameras == 1, the same n_points and board_xy (else TSCM_E_UNSUPPORTED), at most 256 corners.
 *   - refused before any device is touched: n_problems <= 0, bad masks, losses or options (the codes of tscm_solve_fixed);
 *     jacobian_fp32 or any exec_flags bit (TSCM_E_UNSUPPORTED).
 *   - a problem without a single corner comes back as tscm_solve_fixed returns it alone.
 *   - summaries[k].seconds_solve / seconds_total are the batch's times (the same in every summary); rmse and
 *     n_residual_blocks are the problem's own. */
int tscm_solve_mono_batch(const tscm_problem *problems, int n_problems, int device, const tscm_options *opt,
                          const unsigned short *fixed /* [n_problems] or NULL */, int loss_kind, double loss_scale,
                          tscm_summary *summaries /* [n_problems] */);

/* ------------------------------------------------------------------ parameter covariance
 * What ceres::Covariance gives a Ceres user: Sigma = (J^T J)^-1 over the free columns of the problem at its current
 * parameters, NOT multiplied by sigma^2 (Ceres' convention), plus sigma^2 and the standard deviations that follow.  A
 * stand-alone stage behind a solve; it runs no kernel of the LM iteration.
 *
 * Free columns.  A camera's 15 columns are (pose 6, fx fy cx cy xi lambda alpha b c).
 *   - pose columns are free unless the problem is mono, cam_pose_constant[m] is set, or the camera has no view with corners;
 *   - intrinsic k < 7 is free unless it is held (bit k of fixed[m], TSCM_FIX_*) or the camera has no view with corners;
 *   - b and c are never free;
 *   - a board's 6 columns are free if the board has a view with corners and board_pose_constant[i] is not set;
 *   - n_free = free camera columns + 6 * free boards.
 * Jacobian.  J is the Jacobian at the problem's parameters, corrected by the loss as a robust solve corrects it
 * (sqrt(rho') on a corner's rows): the blocks are board_gram, view_cross, cam_gram and cost of
 * tscm_eval_normal_equations_robust with default options (the fp64 Gram kernel).
 * Covariance.  With B_i = board_gram[i], W_v = view_cross[v] restricted to the free camera columns, C =
 * blockdiag(cam_gram) and Z_v = B_i^-1 W_v:
 *   S        = C - sum over free boards i, over the views v, v' of board i, of W_v^T Z_v'   (free camera columns, dense)
 *   Sigma_cc = S^-1
 *   Sigma_bb,i = B_i^-1 + sum over the views v, v' of board i of Z_v Sigma_cc[m_v, m_v'] Z_v'^T
 * Board-camera cross blocks are not formed.  S is scaled to unit diagonal, factored by Cholesky, inverted from the factor
 * and scaled back; every B_i by a 6 x 6 Cholesky.
 * Scale.  sigma2 = 2 cost / (n_residuals - n_free), n_residuals = 2 * corners; NaN when that difference is <= 0.  The
 * standard deviations are sqrt(sigma2 * diagonal), and exactly 0 for columns that are not free.
 * Singularity.  A Cholesky pivot that is not > 0 (NaN included) ends the call with TSCM_OK, every element of the five output
 * arrays NaN and info->status = 1 (a board block; where = the lowest such board) or 2 (the reduced system; where = camera *
 * 15 + column of the first such pivot); info keeps n_free, n_residuals, cost and sigma2.  min_pivot_ratio is the smallest
 * pivot of the scaled reduced system, whose diagonal is 1 before the factorisation (the failing pivot with status 2, NaN
 * with status 1, 1 when no camera column is free): near 0 for a rig without a constant camera pose (gauge freedom) or an
 * unobservable parameter.  The library applies no threshold of its own.
 * Two calls on the same input give the same bytes (no floating-point atomics, every sum in a fixed order).
 *
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: a NULL problem, info or required
 * block; info->struct_size other than sizeof(tscm_covariance_info); mask bits 9 and up; an unknown loss kind, or a scale that
 * is not finite and > 0; a view_camera or view_board out of range; n_cameras outside 1..32; cam_free set for b or c.
 * device_index: as `device` elsewhere, TSCM_E_NO_DEVICE outside [0, tscm_device_count()), after the argument checks. */
typedef struct tscm_covariance_info {
    int struct_size;               /* sizeof(tscm_covariance_info), set by the caller                                 */
    int status;                    /* 0 ok, 1 singular board block, 2 singular reduced system                          */
    int where;                     /* status 1: board; status 2: camera * 15 + column; else -1                         */
    int n_free;
    long long n_residuals;         /* 2 * corners (tscm_covariance only, else 0)                                       */
    double cost, sigma2;           /* tscm_covariance only; else 0 and NaN                                             */
    double min_pivot_ratio;
    double seconds_kernel[4];      /* device seconds: board factor, Schur complement, reduced inverse, board marginals */
} tscm_covariance_info;

/* cam_cov [C*15][C*15] and board_cov [B][6][6]: zero rows / columns / blocks where not free; either may be NULL, as may
 * cam_rt_std [C*6], intr_std [C*9] and board_rt_std [B*6].  fixed: [C] mask words or NULL.  Host pointers. */
int tscm_covariance(const tscm_problem *problem, int device_index, const unsigned short *fixed, int loss_kind, double loss_scale,
                    double *cam_cov, double *board_cov, double *cam_rt_std, double *intr_std, double *board_rt_std,
                    tscm_covariance_info *info);

/* The same kernels on blocks the caller gives (the host layout of tscm_eval_normal_equations; board_grad, cam_grad and the
 * cost are not needed) and the caller's masks cam_free [C*15], board_free [B]; every view counts.  For parity tests and
 * crafted inputs.  cost, sigma2 and n_residuals stay 0 / NaN / 0. */
int tscm_covariance_from_normal_equations(int n_cameras, int n_boards, int n_views, const int *view_camera, const int *view_board,
                                          const double *board_gram, const double *view_cross, const double *cam_gram,
                                          const unsigned char *cam_free, const unsigned char *board_free, int device_index,
                                          double *cam_cov, double *board_cov, tscm_covariance_info *info);

/* ------------------------------------------------------------------ corner weights and corner masks
 * Ceres' ScaledLoss on every residual block -- new ScaledLoss(loss, w, TAKE_OWNERSHIP) -- or, with weight 0, the corner's
 * AddResidualBlock left out.
 *   - Every corner i has a weight omega_i >= 0, with s_i = r_u^2 + r_v^2.
 *   - Loss rho of kind TSCM_LOSS_NONE is rho(s) = s, rho' = 1.
 *   - Block cost is omega_i rho(s_i) / 2.
 *   - Residual and Jacobian rows are scaled by w_i = sqrt(omega_i rho'(s_i)).  rho' is clamped at DBL_MIN as for a loss, before
 *     the multiplication by omega, so omega_i = 0 gives w_i = 0 exactly.
 *   - Every reported cost, gradient, LM diagonal and tolerance test follows from these, exactly as for a loss.
 * Masked corners.  omega_i = 0 takes the corner out.  The observation of a masked corner may hold anything, NaN and
 * infinities included: this is how a partial board with a missing interior corner is expressed.  The device copy of a masked
 * observation is written as 0.0, 0.0 at upload, so no NaN reaches arithmetic.
 * Counts and RMSE.  summary.n_residual_blocks counts the corners with omega_i > 0; summary.rmse = sqrt(sum omega_i s_i /
 * sum omega_i) at the accepted point -- for a 0/1 mask the pixel RMSE over the kept corners.  tscm_reprojection_error knows
 * no weights.
 * Refused with TSCM_E_INVALID, the text naming the corner or view: a weight that is negative, NaN or infinite; a view with view_count > 0 whose weights are all 0 (pass view_count = 0 for it).  Weights with
 * TSCM_EXEC_GRAM_16X16: TSCM_E_UNSUPPORTED, as for a loss.
 * weights = NULL is the solve without weights, bit for bit, on a fresh solver and after weights were set and cleared.
 *
 * weights: [N] in the problem's corner order -- views in problem order, the corners of a view in order (N = sum of view_count;
 * view_offset plays no part) -- or NULL for none.  May be called between solves.  A sharded solver takes the full [N] array
 * and keeps its own views' part.  The shards of a local group must all have weights or all have none
 * (tscm_solver_solve_group: TSCM_E_INVALID otherwise); across processes this is not checked.
 * tscm_solver_eval_normal_equations uses the solver's weights.                                                              */
int tscm_solver_set_corner_weights(tscm_solver *s, const double *weights);
/* tscm_solve_fixed, tscm_eval_normal_equations_robust and tscm_eval_step_fixed with corner weights (device_index: as `device`
 * of those) */
int tscm_solve_weighted(const tscm_problem *problem, const tscm_options *opt, const double *weights, const unsigned short *fixed, int kind,
                        double scale, tscm_summary *summary);
int tscm_eval_normal_equations_weighted(const tscm_problem *problem, int device_index, const tscm_options *opt, const double *weights, int kind,
                                        double scale, double *board_gram, double *board_grad, double *view_cross, double *cam_gram,
                                        double *cam_grad, double *cost);
int tscm_eval_step_weighted(const tscm_problem *problem, int device_index, const tscm_options *opt, const double *weights,
                            const unsigned short *fixed, int kind, double scale, double *cam_rt, double *intr, double *board_rt,
                            int *valid, tscm_summary *summary);
/* tscm_solve_mono_batch with weights[k] (or NULL) the corner weights of problem k; weights = NULL: none */
int tscm_solve_mono_batch_weighted(const tscm_problem *problems, int n_problems, int device_index, const tscm_options *opt,
                                   const unsigned short *fixed /* [n_problems] or NULL */,
                                   const double *const *weights /* [n_problems] pointers, entries may be NULL */, int loss_kind,
                                   double loss_scale, tscm_summary *summaries /* [n_problems] */);
/* tscm_covariance on the blocks of the weighted normal equations; n_residuals = 2 * #{omega_i > 0} */
int tscm_covariance_weighted(const tscm_problem *problem, int device_index, const unsigned short *fixed, const double *weights,
                             int loss_kind, double loss_scale, double *cam_cov, double *board_cov, double *cam_rt_std,
                             double *intr_std, double *board_rt_std, tscm_covariance_info *info);

/* ------------------------------------------------------------------ Gaussian priors on camera parameters
 * Ceres' NormalPrior on single coordinates of a camera's pose or intrinsic block: one more residual sqrt(w_k) (x_k - mean_k)
 * per coordinate k with a weight w_k > 0 -- "about this value, give or take sigma", w = (sigma_pixel / sigma)^2.
 *   - Objective.  The solve's objective (loss and corner weights included) plus 1/2 sum_k w_k (x_k - mean_k)^2 over the
 *     camera-side coordinates.  Every prior is a residual block of its own with Jacobian sqrt(w_k) and no loss.
 *   - Where it counts.  In everything a Jacobian row takes part in: the column norms behind the Jacobi scaling, the LM
 *     diagonal, the gradient and its norms, the cost and the model cost change, tscm_eval_normal_equations* (the diagonal of
 *     cam_gram, cam_grad, cost) and tscm_eval_step*.  Board blocks and view_cross do not change by a bit.
 *   - Pose.  The pose prior is on the raw 6-vector (angle-axis and translation differences as stored): a NormalPrior on rt_.
 *   - Coordinates that are not free.  A weight is taken as 0 (no cost, no gradient) on a coordinate that is not a free column of
 *     the solve: a held intrinsic, b, c, the pose of a mono problem or of a cam_pose_constant camera, a camera without corners.
 *     tscm_solver_set_fixed_intrinsics re-derives the effective weights.  tscm_eval_normal_equations* takes no mask: there
 *     every column that can be free counts.
 *   - Summary.  n_residual_blocks stays the corner count; with an effective prior, rmse is the plain pixel RMSE at the final
 *     parameters (sqrt(sum omega s / sum omega) with corner weights), not sqrt(2 final_cost / N): final_cost holds the prior.
 *   - Covariance.  n_residuals = 2 N + P with P the effective prior rows, sigma2 = 2 cost / (n_residuals - n_free) with the cost
 *     including the prior, and the blocks include it: a parameter that only the prior determines has a finite variance.
 *   - No floating-point atomics: two calls give the same bytes.  priors = NULL, or every effective weight 0, is the solve
 *     without priors: the same launches, summaries and parameters bit for bit.
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: a struct_size other than
 * sizeof(tscm_camera_priors); a mean given without its weight or the reverse; a weight that is negative, NaN or infinite; a
 * mean that is not finite where its weight is > 0.  In the refusal order of the one-shot entry points the priors follow the
 * corner weights.  Not served: a sharded solver (tscm_solver_create_sharded with world > 1: TSCM_E_UNSUPPORTED); and
 * tscm_solve_mono_batch* takes no priors argument.
 *   problem.AddResidualBlock(new NormalPrior(A, mean), nullptr, intrinsic)  with A = diag(sqrt(w))                          */
typedef struct tscm_camera_priors {
    size_t struct_size;                          /* sizeof(tscm_camera_priors), set by the caller                            */
    const double *cam_rt_mean, *cam_rt_weight;   /* [C*6] in the order of tscm_problem.cam_rt, or both NULL                  */
    const double *intr_mean,   *intr_weight;     /* [C*9] in the order of tscm_problem.intr,   or both NULL                  */
} tscm_camera_priors;
/* the priors of every later solve / solve_resident / tscm_solver_eval_normal_equations of s; the arrays are copied.  May be
 * called between solves; NULL clears.                                                                                       */
int tscm_solver_set_camera_priors(tscm_solver *s, const tscm_camera_priors *priors);
/* tscm_solve_weighted, tscm_eval_normal_equations_weighted, tscm_eval_step_weighted and tscm_covariance_weighted with priors */
int tscm_solve_prior(const tscm_problem *problem, const tscm_options *opt, const double *weights, const unsigned short *fixed, int kind,
                     double scale, const tscm_camera_priors *priors, tscm_summary *summary);
int tscm_eval_normal_equations_prior(const tscm_problem *problem, int device_index, const tscm_options *opt, const double *weights, int kind,
                                     double scale, const tscm_camera_priors *priors, double *board_gram, double *board_grad,
                                     double *view_cross, double *cam_gram, double *cam_grad, double *cost);
int tscm_eval_step_prior(const tscm_problem *problem, int device_index, const tscm_options *opt, const double *weights,
                         const unsigned short *fixed, int kind, double scale, const tscm_camera_priors *priors, double *cam_rt,
                         double *intr, double *board_rt, int *valid, tscm_summary *summary);
int tscm_covariance_prior(const tscm_problem *problem, int device_index, const unsigned short *fixed, const double *weights,
                          int loss_kind, double loss_scale, const tscm_camera_priors *priors, double *cam_cov, double *board_cov,
                          double *cam_rt_std, double *intr_std, double *board_rt_std, tscm_covariance_info *info);

/* ------------------------------------------------------------------ projection uncertainty maps
 * The covariance of a projected pixel under the joint parameter covariance of tscm_covariance: what a standard deviation
 * on xi or lambda means in pixels.  A stage of its own behind tscm_covariance; it runs no other kernel of the library.
 *
 * Model.  The functor's (multi_calib.h:146-195): b and c are inert in both directions, P_c = R_c P_rig + t_c, angle-axis
 * rotations with both branches of ceres::AngleAxisRotatePoint.  I = (fx fy cx cy xi lambda alpha) below.
 * Request (camera_a, camera_b, inv_distance i >= 0), for the grid pixel q = (x0 + col * dx, y0 + row * dy) of camera a:
 *   r   = get_unit_sphere_coordinate(I_a, q) with b = c = 0                       (TS.h:39-57), a unit ray
 *   s   = r - i t_a,   D = R_a^T s        the point at distance 1 / i from a's centre, scaled by i, in the rig frame
 *   p_b = R_b D + i t_b
 *   rho2 = X^2 + Y^2, d1 = sqrt(rho2 + Z^2), z1 = Z + xi d1, d2 = sqrt(rho2 + z1^2), z2 = z1 + lambda d2,
 *   d3 = sqrt(rho2 + z2^2), beta = alpha / (1 - alpha), k = z2 + beta d3          at (X, Y, Z) = p_b with I_b
 *   q_b = (fx X / k + cx, fy Y / k + cy)
 * The projection does not change under a positive scale of p_b, so i = 0 is the point at infinity without a special case
 * (the convention of tscm_build_sweep_maps).
 * Derivatives of the projection at a point p = (X, Y, Z) with intrinsics I, as the functor's Jacobian has them:
 *   c1 = 1 + xi Z / d1, c2 = 1 + lambda z1 / d2, c3 = 1 + beta z2 / d3, g = beta / d3 + c3 (lambda / d2 + c2 xi / d1),
 *   kz = c1 c2 c3, mx = X / k, my = Y / k
 *   A(p, I) = d(u, v) / dp = [ fx/k (1 - X mx g)   -fx/k mx Y g        -fx/k mx kz ]
 *                            [ -fy/k my X g        fy/k (1 - Y my g)   -fy/k my kz ]        (its rows are orthogonal to p)
 *   G(p, I) = d(u, v) / dI = [ mx 0 1 0 -hu c3 c2 d1  -hu c3 d2  -hu d3 / (1 - alpha)^2 ]   hu = fx/k mx
 *                            [ 0 my 0 1 -hv c3 c2 d1  -hv c3 d2  -hv d3 / (1 - alpha)^2 ]   hv = fy/k my
 * Transfer (a != b): theta = (w_a, t_a, I_a, w_b, t_b, I_b), 26 columns, J = d q_b / d theta with q and i held.  With
 * A_b = A(p_b, I_b), AR = A_b R_b, M = AR R_a^T, A_a = A(r, I_a), G_a = G(r, I_a) and dR_k = dR / dw_k:
 *   columns w_a,k :  AR (dR_a,k)^T s
 *   columns t_a   :  -i M
 *   columns I_a   :  -(M A_a^T) (A_a A_a^T)^-1 G_a     (pi(I_a, r) = q for every I_a gives dr = -A_a^T (A_a A_a^T)^-1 G_a dI_a)
 *   columns w_b,k :  A_b dR_b,k D
 *   columns t_b   :  i A_b
 *   columns I_b   :  G(p_b, I_b)
 * Observe (a == b == m): D is held, theta = (w_m, t_m, I_m), 13 columns: the three column groups of camera b above -- the
 * functor's negated camera-side Jacobian with D in the place of the rig point, the translation columns times i because D is
 * the point times i.  p_b is r up to rounding and q_b is q: how far the image of a fixed rig-frame point moves in camera m.
 * Covariance.  Sigma_theta [n][n] (n = 26 or 13) is gathered from cam_cov as tscm_covariance lays it out: theta column c
 * of camera m is row 15 m + c, c = 0..12 (b and c skipped); the lower triangle is read.  Rows that are not free are zero
 * there.  With row i of Sigma taken in order i = 0..n-1 and s_x = sum_{j<i} Sigma_ij J_xj (j ascending):
 *   c_uu += J_ui (Sigma_ii J_ui + 2 s_u),  c_vv += J_vi (Sigma_ii J_vi + 2 s_v),  c_uv += J_ui (Sigma_ii J_vi + s_v) + J_vi s_u
 *   Cov(q_b) = sigma2 * (c_uu c_uv; c_uv c_vv)
 * Outputs per request, planes [ny][nx] in this order: u_b, v_b, c_uu, c_uv, c_vv (sigma2 applied),
 *   sd_worst  = sqrt((c_uu + c_vv + sqrt((c_uu - c_vv)^2 + 4 c_uv^2)) / 2)        the larger eigenvalue's root
 *   sd_across = sqrt((e_v^2 c_uu - 2 e_u e_v c_uv + e_u^2 c_vv) / (e_u^2 + e_v^2)),  e = d q_b / d i = A_b t_b - M t_a, the
 *               epipolar direction at q_b: the deviation across the epipolar line.  NaN in observe mode and where e = 0.
 * flags, a byte per pixel: bit 0 the pixel unprojects (every square-root argument of the unprojection is > 0); bit 1 p_b
 * projects (k > 0; only with bit 0); bit 2 q_b is inside camera b's image, 0 <= u_b <= width_b - 1 and 0 <= v_b <=
 * height_b - 1 (only with bits 0 and 1, and only when width_b > 0 and height_b > 0).  Without bits 0 and 1 all seven doubles
 * of the pixel are NaN.
 * Summary per request: n_valid = pixels with bits 0 and 1; max_sd = the largest sd_worst among them (0 without any; a NaN
 * sd_worst is passed over), taken by an integer maximum of the bit patterns of the non-negative doubles.
 * Two calls on the same input give the same bytes (no floating-point atomics, every sum in a fixed order).  All requests
 * of a call run in one launch.
 *
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: cam_rt, intr, cam_cov, grid,
 * requests, planes or flags NULL; grid->struct_size other than sizeof(tscm_uncertainty_grid); nx, ny or n_requests <= 0
 * (or nx * ny above 2^30, n_requests above 65535); camera_a or camera_b outside [0, n_cameras); inv_distance negative or not
 * finite; sigma2 negative or NaN; x0, y0, dx or dy not finite; n_cameras outside 1..32.  device_index as elsewhere, after
 * the argument checks. */
typedef struct tscm_uncertainty_grid {
    int struct_size;               /* sizeof(tscm_uncertainty_grid), set by the caller                                 */
    int nx, ny;                    /* grid columns and rows                                                            */
    int width_b, height_b;         /* image size of the target cameras for flag bit 2; 0: the bit stays 0              */
    double x0, y0, dx, dy;         /* pixel (col, row) of the grid is (x0 + col * dx, y0 + row * dy) in camera a       */
} tscm_uncertainty_grid;

typedef struct tscm_uncertainty_request {
    int camera_a, camera_b;        /* equal: observe mode                                                              */
    double inv_distance;           /* 1 / distance from camera a's centre, in 1 / the unit of the translations; 0: infinity */
} tscm_uncertainty_request;

/* cam_rt [C*6], intr [C*9] (b and c are not read), cam_cov [C*15][C*15] and sigma2 as tscm_covariance returned them;
 * planes [n_requests][7][ny][nx], flags [n_requests][ny][nx]; max_sd and n_valid [n_requests] or NULL.  Host pointers. */
int tscm_projection_uncertainty(int n_cameras, const double *cam_rt, const double *intr, const double *cam_cov, double sigma2,
                                const tscm_uncertainty_grid *grid, const tscm_uncertainty_request *requests, int n_requests,
                                int device_index, double *planes, unsigned char *flags, double *max_sd, long long *n_valid);
/* device seconds of the kernel of this thread's last tscm_projection_uncertainty call (HIP events around its one launch;
 * uploads and read-back are outside); 0 after a call that was refused or failed */
double tscm_projection_uncertainty_seconds(void);

/* ------------------------------------------------------------------ next-best view
 * Where should the board go next?  A hypothetical view's Jacobian depends on the current parameters only, not on any
 * observation, so what the view would do to the camera covariance of tscm_covariance is known before the image is taken: a
 * low-rank update of the camera block (Peng and Sturm, Calibration Wizard, ICCV 2019).  This stage scores many candidate
 * board poses by the covariance they would remove and can apply one of them, which makes greedy planning possible without a
 * re-solve.  A stage of its own behind tscm_covariance; it runs no other kernel of the library.
 *
 * Inputs.  n_cameras (1..32); cam_rt [C*6], intr [C*9] (b and c are not read); cam_cov [C*15][C*15] as tscm_covariance
 * returns it (unscaled, zero rows and columns where a column is not free; the lower triangle is read); weights [C*15] or
 * NULL; the board, n_points (1..1024) and board_xy [n_points*2]; image_size [C*2] (width, height of each camera, > 0);
 * params (border >= 0 pixels, min_corners >= 4); candidates {camera_a, camera_b, board_rt[6]}, board_rt the board's pose in
 * the rig frame as tscm_problem.board_rt.  camera_a == camera_b: one camera sees the board; otherwise both cameras see the
 * same board instance.
 * A corner in a camera m.  For corner j of the board, with the functor's chain (multi_calib.h:146-195):
 *   P = R_board (x_j, y_j, 0) + t_board,   p = R_m P + t_m,   the projection of p with I_m, its k, A(p, I_m) and G(p, I_m) as
 *   the projection uncertainty stage above defines them.
 * The corner is visible iff k > 0, border <= u <= width_m - 1 - border and border <= v <= height_m - 1 - border.  Its rows:
 *   E = A R_m [dR_board,k (x, y, 0) (k = 0..2) | I3]       2 x 6, the board side
 *   F = [A dR_m,k P (k = 0..2) | A | G]                    2 x 13, the camera side: columns w_m, t_m, I_m
 * (only Gram products are used, so the sign does not matter; both branches of AngleAxisRotatePoint and its derivatives).
 * A camera of the candidate contributes iff its visible count is >= min_corners.  Invisible corners, and all corners of a
 * camera that does not contribute, add nothing.
 * Blocks.  theta = (w_a, t_a, I_a [, w_b, t_b, I_b]), n = 13 or 26 columns whether the cameras contribute or not; theta
 * column c of camera m is row 15 m + c of cam_cov.  Summed over the contributing cameras' visible corners, in corner order
 * (a corner's u row, then its v row) and camera order a then b:
 *   B' = sum E^T E (6 x 6),  W' = sum E^T F (6 x n, into the camera's column group),  C' = sum F^T F (n x n, block diagonal)
 *   Delta S = C' - W'^T B'^-1 W' = C' - Z^T Z,  B' = Lb Lb^T (6 x 6 Cholesky),  Z = Lb^-1 W'
 * Delta S is the information about the camera-side parameters the view carries once its own unknown pose is eliminated.
 * The update.  Sigma_tt [n][n] is gathered from cam_cov; d_k = sqrt(Sigma_tt,kk); Sigma_tt = D G~ G~^T D with G~ the lower
 * Cholesky factor of the unit-diagonal matrix Sigma_tt,ij / (d_i d_j) (columns with Sigma_tt,kk == 0, not free, are skipped
 * and give a zero column and row); G = D G~.
 *   M = I + G^T Delta S G = L L^T  (symmetric, eigenvalues >= 1; the lower triangle of the computed M is factored),
 *   Y = L^-1 G^T Delta S,   K = Delta S - Y^T Y   (= (Delta S^-1 + Sigma_tt)^-1 wherever that exists)
 *   Sigma' = Sigma - Sigma[:, theta] K Sigma[theta, :]                 the covariance after the view
 * Outputs per candidate:
 *   gain_logdet = 2 sum_k log L_kk = log det Sigma_free - log det Sigma'_free, in nats; scale-free (sigma2 cancels)
 *   gain_trace  = sum_k w_k (Sigma_kk - Sigma'_kk) = tr(K Q_tt),  Q = Sigma diag(w) Sigma over all 15 C columns, k ascending.
 *                 weights == NULL: w_k = 1 / Sigma_kk where Sigma_kk > 0, else 0 -- the sum of relative variance reductions.
 *                 The trace is summed column by column of K Q (row index ascending within a column, then columns ascending).
 *   n_visible [2] (the second is 0 when camera_a == camera_b)
 *   flags: bit 0 camera a contributes; bit 1 camera b contributes (only when a != b); bit 2 both gains are numbers; bit 3 a
 *          pivot of B', of the scaled Sigma_tt or of M was not > 0.
 * Without a contributing camera nothing behind the blocks is evaluated: the gains are exactly 0, bit 2 is set and bit 3 is
 * not.  With bit 3 both gains are NaN.
 * Apply: the same inputs and ONE candidate; that candidate's outputs and cam_cov_out [C*15][C*15] = Sigma'.  Each element
 * of the lower triangle is Sigma_rc - sum_i Sigma_r,theta_i (sum_j K_ij Sigma_theta_j,c), i and j ascending, and is written to
 * its mirror too, so the result is symmetric; rows that were zero stay zero.  A copy of cam_cov when no camera contributes;
 * all NaN with bit 3.
 * Two calls on the same input give the same bytes, and a candidate's outputs do not depend on its place in the batch (no
 * floating-point atomics, every sum in a fixed order).
 *
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: a required pointer that is NULL
 * (all but weights); params->struct_size other than sizeof(tscm_view_gain_params); n_cameras outside 1..32; n_points
 * outside 1..1024; n_candidates <= 0 or above 2^24; camera_a or camera_b outside [0, n_cameras); a board_rt, board_xy,
 * cam_rt or intr (its first seven per camera) that is not finite; border negative or not finite; min_corners < 4; an image
 * size that is not positive; a weight that is negative or not finite.  device_index as elsewhere, after the argument
 * checks. */
typedef struct tscm_view_gain_params {
    int struct_size;               /* sizeof(tscm_view_gain_params), set by the caller                                 */
    int min_corners;               /* a camera contributes with at least this many visible corners; >= 4               */
    double border;                 /* pixels a visible corner keeps from the image's edge; >= 0                        */
} tscm_view_gain_params;

typedef struct tscm_view_candidate {
    int camera_a, camera_b;        /* equal: one camera sees the board                                                 */
    double board_rt[6];            /* the board's pose in the rig frame: angle-axis, translation                       */
} tscm_view_candidate;

/* gain_logdet, gain_trace, flags [n_candidates], n_visible [n_candidates*2].  Host pointers. */
int tscm_view_gain(int n_cameras, const double *cam_rt, const double *intr, const double *cam_cov, const double *weights,
                   int n_points, const double *board_xy, const int *image_size, const tscm_view_gain_params *params,
                   const tscm_view_candidate *candidates, int n_candidates, int device_index, double *gain_logdet,
                   double *gain_trace, int *n_visible, int *flags);
/* one candidate: gain_logdet, gain_trace, flags [1], n_visible [2], cam_cov_out [C*15][C*15] (must not alias cam_cov) */
int tscm_view_gain_apply(int n_cameras, const double *cam_rt, const double *intr, const double *cam_cov, const double *weights,
                         int n_points, const double *board_xy, const int *image_size, const tscm_view_gain_params *params,
                         const tscm_view_candidate *candidate, int device_index, double *gain_logdet, double *gain_trace,
                         int *n_visible, int *flags, double *cam_cov_out);
/* device seconds of the launches of this thread's last tscm_view_gain or tscm_view_gain_apply call (HIP events around them;
 * uploads and read-back are outside); 0 after a call that was refused or failed */
double tscm_view_gain_seconds(void);

/* ------------------------------------------------------------------ residual report
 * Which views and corners of a calibration are bad, and does the model fit the lens: every corner's residual at the
 * problem's parameters, statistics per view and per camera, and optional field statistics per camera (an image grid and
 * bins over the incidence angle).  A stage of its own: no kernel of the LM iteration runs.
 *
 * Corner order is the order of the corner weights: views in problem order, the corners of a view in order; N = sum of
 * view_count.  The residual is the functor form's (no skew terms, both branches of AngleAxisRotatePoint), from the device
 * function tscm_eval_functor evaluates.
 * Per corner i of view (camera m, board b), with omega_i its weight (weights == NULL: 1):
 *   r = observed - projected,  s = r_u^2 + r_v^2,  p = observed - r the projected pixel,  c = (cx, cy) of camera m
 *   e = (p - c) / |p - c|, or (1, 0) where |p - c| = 0;   r_rad = r . e;   r_tan = e_x r_v - e_y r_u
 *   angle = atan2(sqrt(X^2 + Y^2), Z) of the camera-frame point (X, Y, Z)
 *   rho1 = rho'(s) of the loss, clamped as the solver clamps it; 1 for TSCM_LOSS_NONE
 * A corner with omega_i = 0: its observation may hold anything, NaN included, and is read as (0, 0) as at solver upload;
 * all six of its outputs are exactly 0 and it takes part in no statistic.
 * Per view, over its corners with omega > 0 (a view without one: zeros and worst = -1):
 *   n_used, sum_w = sum omega, rms = sqrt(sum omega s / sum_w), mean_err = sum omega |r| / sum_w, max_err = max |r|,
 *   worst = index within the view of max_err (lowest on ties), bias_u, bias_v, mean_rad = weighted means of r_u, r_v, r_rad.
 * Per camera, the same formulas over all its used corners: n_used, sum_w, rms, mean_err, max_err, worst_view (the view of
 * max_err, lowest on ties, -1 without a used corner), n_views_used.
 * Per call (info): cost = sum omega rho(s) / 2, rmse = sqrt(sum omega s / sum omega), the used corners and views.
 *
 * Field statistics, per camera, over the corners with omega > 0 ("weights only gate": every such corner counts once).  A
 * corner with max(|r_u|, |r_v|) > clamp (pixels, in (0, 64]) is counted in n_clamped of its cell / bin and in no sum.
 *   Image grid (grid_w > 0): grid_w x grid_h cells over image_width x image_height.  A corner goes to the cell of its
 *   OBSERVED pixel, ix = floor(obs_u * grid_w / image_width), iy likewise -- a function of the inputs alone; outside the
 *   image it is counted in info->grid_outside[camera].  Per cell: count, n_clamped, and mean_u, mean_v, rms.
 *   Angle bins (n_angle_bins > 0): uniform over [0, max_angle], bin = floor(angle * n_angle_bins / max_angle), the angle
 *   max_angle itself in the last bin; a larger angle is counted in info->angle_outside[camera].  Per bin: count, n_clamped,
 *   and mean_rad, mean_tan, rms, mean_angle.
 * Field accumulation is exact: every addend is llrint(x * 2^24), summed in 64-bit integers; a mean is (double)sum * 2^-24 /
 * count and rms the square root of that for s.  |r_u|, |r_v| <= 64 gives s <= 2^13 = 2^37 quanta, so 2^26 used corners of
 * one camera cannot overflow; a camera with more and a field requested is refused with TSCM_E_UNSUPPORTED.
 * Two calls on the same input give the same bytes in every output: no floating-point atomics, a view's sums by a fixed lane
 * assignment and butterfly, a camera's sums over its views in problem order by a fixed tree, the field in integers.  A
 * view's rows do not depend on its place in the problem.
 *
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: a NULL problem, params or info;
 * a struct_size other than the struct's sizeof; an unknown loss kind, or a scale that is not finite and > 0; grid_w or
 * grid_h outside 0..64 or only one of them 0; a non-positive image size with a grid; n_angle_bins outside 0..64; max_angle
 * not in (0, pi] with bins; clamp not in (0, 64]; a field requested without its two output arrays; a problem tscm_solver_create
 * refuses; weights that are negative, NaN or infinite.  Unlike a solve, a view whose weights are all 0 is accepted: it is
 * unused.  device_index as elsewhere, TSCM_E_NO_DEVICE after the argument checks. */
typedef struct tscm_residual_params {
    int struct_size;               /* sizeof(tscm_residual_params), set by tscm_residual_default_params                */
    int loss_kind;                 /* TSCM_LOSS_*; default TSCM_LOSS_NONE                                              */
    double loss_scale;             /* pixels                                                                           */
    int grid_w, grid_h;            /* 1..64 each, or both 0: no image grid (default)                                   */
    int image_width, image_height; /* pixels; > 0 with a grid                                                          */
    int n_angle_bins;              /* 1..64, or 0: no angle bins (default)                                             */
    int pad;
    double max_angle;              /* radians, in (0, pi]; default pi / 2                                              */
    double clamp;                  /* pixels, in (0, 64]; default 64                                                   */
} tscm_residual_params;

typedef struct tscm_residual_info {
    int struct_size;               /* sizeof(tscm_residual_info), set by the caller                                    */
    int n_views_used;              /* views with a used corner                                                         */
    long long n_used;              /* corners with omega > 0                                                           */
    double sum_w;
    double cost;                   /* sum omega rho(s) / 2                                                             */
    double rmse;                   /* sqrt(sum omega s / sum omega); 0 without a used corner                           */
    long long grid_outside[32];    /* per camera: used corners observed outside the image (grid requested)             */
    long long angle_outside[32];   /* per camera: used corners with angle > max_angle (bins requested)                 */
    double seconds_kernel[4];      /* device seconds: views, cameras, field accumulation, field means                  */
} tscm_residual_info;

void tscm_residual_default_params(tscm_residual_params *params);

/* Every output may be NULL; grid_count and grid are required with a grid, angle_count and angle with bins.  Host pointers.
 *   corner      [N][6]  r_u r_v r_rad r_tan angle rho1
 *   view        [V][8]  n_used sum_w rms mean_err max_err bias_u bias_v mean_rad
 *   view_worst  [V]
 *   camera      [C][8]  n_used sum_w rms mean_err max_err worst_view n_views_used 0
 *   grid_count  [C][grid_h][grid_w][2]  count n_clamped      grid  [C][grid_h][grid_w][3]  mean_u mean_v rms
 *   angle_count [C][K][2]               count n_clamped      angle [C][K][4]  mean_rad mean_tan rms mean_angle */
int tscm_residual_report(const tscm_problem *problem, int device_index, const double *weights,
                         const tscm_residual_params *params, double *corner, double *view, int *view_worst, double *camera,
                         long long *grid_count, double *grid, long long *angle_count, double *angle,
                         tscm_residual_info *info);

/* Tests only: the corner count at which the field kernel's chunk lists are cut for this thread's next calls (0: the
 * default).  Cutting them differently changes no output byte. */
void tscm_residual_debug_chunk_target(int corners);

/* ------------------------------------------------------------------ projection family
 * tscm_project_points   = TripleSphereCamera::project (TS.cpp:332-344), skew terms
 *                         included, n camera-frame points [n*3] -> pixels [n*2].
 * tscm_unproject_pixels = get_unit_sphere_coordinate (TS.h:39-57) with
 *                         transform = identity, pixels [n*2] -> unit rays [n*3].
 * tscm_reprojection_error = the report of multi_calib.cpp:233-283 / main.cpp:245-288:
 *                         per-camera mean Euclidean pixel error [C] (may be NULL),
 *                         global mean, and RMSE over all corners.                  */
int tscm_project_points(const double *intr9, const double *points, int n, int device, double *pixels);
int tscm_unproject_pixels(const double *intr9, const double *pixels, int n, int device, double *rays);
int tscm_reprojection_error(const tscm_problem *problem, int device, double *per_camera_mean,
                            double *global_mean, double *rmse);

/* ------------------------------------------------------------------ multi-GPU (frame sharding)
 * The reference has no counterpart (multi_calib.cpp:209-212 never sets num_threads); this is north_star's
 * "observations shard by image across the GPUs of one node with an RCCL all-reduce of J^T J / J^T r".
 *
 * Every rank passes the SAME whole problem to tscm_solver_create_sharded(problem, device, rank, world): the library
 * assigns contiguous, corner-balanced ranges of boards (frames) to the ranks (tscm_shard_frames) and keeps on each
 * GPU only the observations, Schur records and pose blocks of the boards that rank owns, so every board's 6x6 block
 * is rank-local; camera poses and intrinsics are replicated.  What all ranks must agree on -- which cameras have
 * views, which camera pairs share a board, the total corner count -- is derived from the whole problem.
 * Per LM iteration the ranks exchange exactly two buffers with a sum all-reduce: the Schur-complement tiles
 * (256 doubles per camera pair that shares a board) and the camera tiles + scalars (256 C + 8 + world doubles);
 * every rank then solves the reduced camera system redundantly and takes identical accept / reject decisions.
 *
 * Two exchange back-ends:
 *   RCCL   one process per GPU (the production path).  Rank 0 calls tscm_comm_unique_id and distributes the 128
 *          bytes (a socket, a file, MPI ...); every rank calls tscm_comm_create, tscm_solver_set_comm, and then
 *          tscm_solver_solve / _solve_resident like on one GPU.
 *   LOCAL  all ranks in ONE process on ONE device (tscm_comm_create_local + tscm_solver_solve_group): the shards
 *          run in lock step on one stream and the all-reduce is a kernel.  RCCL refuses two ranks on one device,
 *          so this is how the sharded solver is exercised on a single-GPU machine; results are those of the RCCL
 *          path with the same world size (same shards, same summation order: rank order).
 * tscm_solver_download_params writes only the owned boards into board_rt; tscm_solver_gather_boards completes the
 * caller's full-length array on every rank (tscm_solver_solve does both).                                        */
#define TSCM_UNIQUE_ID_BYTES 128
int tscm_solver_create_sharded(const tscm_problem *problem, int device, int rank, int world, tscm_solver **out);
int tscm_comm_unique_id(unsigned char id[TSCM_UNIQUE_ID_BYTES]);
int tscm_comm_create(const unsigned char id[TSCM_UNIQUE_ID_BYTES], int rank, int world, int device, tscm_comm **out);
int tscm_comm_create_local(int world, int device, tscm_comm **out /* [world] */);
/* IPC  one process per rank like RCCL; the exchange is the library's own one-shot all-reduce over buffers the ranks map
 *      from each other (hipIpcMemHandle).  Ranks MAY share a device (RCCL refuses that): the multi-process path on a
 *      one-GPU box.  Every rank calls tscm_comm_ipc_open (max_doubles >= 256 * max(camera-pair blocks, cameras) + 8 +
 *      world: api.Comm.ipc computes it), the handles (TSCM_IPC_HANDLE_BYTES each) are all-gathered by the caller (socket, file, MPI ...),
 *      every rank calls tscm_comm_ipc_connect with all of them in rank order; then tscm_solver_set_comm as with RCCL.
 *      Exercised between processes on one device; RCCL is the production path across devices. */
#define TSCM_IPC_HANDLE_BYTES 80      /* (64 until ABI 5) the HIP handle, then the device's PCI address and the buffer's kind */
int tscm_comm_ipc_open(int rank, int world, int device, size_t max_doubles, tscm_comm **out, unsigned char handle[TSCM_IPC_HANDLE_BYTES]);
int tscm_comm_ipc_connect(tscm_comm *c, const unsigned char *handles /* [world][TSCM_IPC_HANDLE_BYTES] */);
void tscm_comm_destroy(tscm_comm *c);
/* rank / world the communicator was created with and the number of ranks the back-end itself reports
 * (ncclCommCount for RCCL, the group size for LOCAL); any output may be NULL. */
int tscm_comm_info(const tscm_comm *c, int *rank, int *world, int *backend_ranks);
/* solvers[r] = shard r of n with the r-th communicator of one tscm_comm_create_local call; summaries [n]. */
int tscm_solver_solve_group(tscm_solver **solvers, int n, const tscm_options *opt, tscm_summary *summaries, int reset);
int tscm_solver_gather_boards(tscm_solver *s, double *board_rt);
/* owner[b] = rank owning board b: contiguous ranges balanced by corner count.       */
int tscm_shard_frames(const tscm_problem *problem, int world, int *owner);


/* ------------------------------------------------------------------ rig initialisation
 * tscm_rig_init = the constructor MultiCalib::MultiCalib(cameras, worlds) (multi_calib.cpp:6-153),
 * the step right before calibrate(): camera i is chained to camera i-1 through every board both
 * see; each common board gives a pose hypothesis and the one with the smallest summed reprojection
 * error over ALL common boards and both cameras wins (:50-85 -- quadratic in the number of common
 * boards, 2.7e9 projections per camera pair at 10k views/camera: the GPU part); every board pose is
 * then chosen the same way among the cameras that see it (:90-151).  Semantics kept: Rt_to_R_t
 * builds R from float32 copies of r1, r2 and their float cross product (multi_calib.h:130-137),
 * TripleSphereCamera::ReprojectError is the SUM of pixel errors with the skew projection
 * (TS.h:58-69), strict `<` keeps the first minimum, rt_ = [cv::Rodrigues(R), t]
 * (multi_calib.h:16-18, 94-96).  The error sums are reduced in a different (tree) order than the
 * reference's sequential loop, so exact ties / 1-ulp near-ties may pick another hypothesis.
 * Adjacent cameras without a common board (undefined behaviour in the reference, :51/:86) ->
 * TSCM_E_INVALID.                                                                             */
typedef struct tscm_rig_input {
    int n_cameras, n_boards, n_points;
    const double *worlds;          /* [n_points*3] board points x, y, z                          */
    const double *intr;            /* [C*9]                                                      */
    const unsigned char *has;      /* [C*B] has_chessboard(j) of camera m                        */
    const double *Rt;              /* [C*B*9] row-major 3x3 [r1 r2 t] = TripleSphereCamera::Rt(j) */
    const double *pix_u, *pix_v;   /* [C*B*n_points] pixels()[j] (read only where has)           */
} tscm_rig_input;

typedef struct tscm_rig_result {
    double *cam_R, *cam_t, *cam_rt;        /* [C*9] row-major, [C*3], [C*6]  (host, caller-owned) */
    double *board_R, *board_t, *board_rt;  /* [B*9], [B*3], [B*6]                                 */
    unsigned char *board_initial;          /* [B] is_initial()                                     */
    int *cam_choice;                       /* [C] winning hypothesis (index among the common boards) or NULL */
    double *cam_min_error;                 /* [C] its summed error, or NULL                        */
    double seconds_hypotheses;             /* device time of the camera-chaining kernels           */
    double seconds_total;
    long long n_projections;               /* point projections evaluated on the device            */
} tscm_rig_result;

int tscm_rig_init(const tscm_rig_input *in, int device, tscm_rig_result *out);
/* One stage of the camera chaining without the choice: camera i (1 .. C-1) against camera i-1 posed at
 * (Rp [9] row-major, tp [3]).  K = the number of boards both cameras see (has[i-1][j] && has[i][j]);
 * Rs_out [K*9] / ts_out [K*3] receive the K pose hypotheses (multi_calib.cpp:29-48), err_out [K] the
 * summed reprojection error of each (:50-78) as tscm_rig_init computes it.  ksplit = 0 slices the common
 * boards by the host's rule, 1 .. K forces that many slices, anything else is TSCM_E_INVALID (checked
 * before the device is touched).  info_out [4] (or NULL) = K, hypothesis groups of 64, slices, and
 * 1 if the skew instantiation (b or c != 0 in either camera) ran.  For tests and diagnostics.   */
int tscm_rig_stage_errors(const tscm_rig_input *in, int i, const double *Rp, const double *tp, int ksplit, int device,
                          double *Rs_out, double *ts_out, double *err_out, int *info_out);


/* ------------------------------------------------------------------ result I/O
 * The YAML main.cpp:305-319 writes through cv::FileStorage -- "cam{i}": 1x9 intrinsic_matrix_,
 * "Twc{i}": 3x4 [R | t] -- and EpipolarRectify/rectify.cpp:262-270 reads.  Host-only (no device).
 * tscm_yaml_format   renders the file into buf (NULL buf: only *needed, incl. the final NUL).
 * tscm_yaml_write    = FileStorage(path, WRITE) + the loop of main.cpp:306-318.
 * tscm_yaml_parse / tscm_yaml_read  = FileStorage(path, READ)["cam{i}"], ["Twc{i}"]: fills
 *                    intr [max_cameras*9] and Twc [max_cameras*12, row-major 3x4] (either may be
 *                    NULL) and returns the number of cameras found in *n_cameras.             */
int tscm_yaml_format(int n_cameras, const double *intr, const double *cam_R, const double *cam_t,
                     char *buf, size_t buf_size, size_t *needed);
int tscm_yaml_write(const char *path, int n_cameras, const double *intr, const double *cam_R,
                    const double *cam_t);
int tscm_yaml_parse(const char *text, int max_cameras, int *n_cameras, double *intr, double *Twc);
int tscm_yaml_read(const char *path, int max_cameras, int *n_cameras, double *intr, double *Twc);


/* ------------------------------------------------------------------ remap tables
 * The per-pixel map builders TripleSphereCamera::undistort (TS.cpp:284-306), the map part of
 * undistort_chessboard (TS.cpp:308-330, before cv::remap) and the eight 400x400 tables of
 * EpipolarRectify/rectify.cpp:86-199 are one loop:
 *     ray = R * ((j - cx)/fx, (i - cy)/fy, 1);  (u, v) = project(ray)  [TS.cpp:332-344, skew terms]
 *     mapx(i, j) = (float)(u + offset_x);  mapy(i, j) = (float)(v + offset_y)
 *   undistort:             R = I, (fx, fy, cx, cy) = the pinhole arguments
 *   undistort_chessboard:  R = Rt_[index] (3x3 [r1 r2 t]), fx = fy = 1, cx = cy = chessboard_size
 *   rectify init_remap:    R = R_cam^T * R_pair, fx = fy = cx = cy = 200, offsets = the mosaic
 *                          origin of the sampled camera (0 | 1280, 0 | 1080); its TScamera::project
 *                          returns (-1, -1) when Z <= -w2 * d1, w2 = 0.42399 (rectify.cpp:7,27):
 *                          check_w2 = 1
 * A batch of maps is one launch; map m writes rows of `out_stride` floats starting at element
 * `out_offset` of mapx / mapy (so the 400x1600 left/right tables of rectify.cpp are 4 maps each).
 * exact != 0: IEEE sqrt / divide and unfused multiply-add in the reference's operation order
 * (bit-identical floats); exact == 0: hardware reciprocal / rsqrt seeds with one correction step
 * (fp64 values within ~2 ulp, i.e. identical floats except when within 1e-15 relative of a
 * float32 rounding boundary).                                                                */
typedef struct tscm_map_desc {
    double intr[9];              /* fx fy cx cy xi lambda alpha b c of the camera that is sampled */
    double R[9];                 /* row-major 3x3                                                  */
    double fx, fy, cx, cy;       /* pinhole of the output image                                    */
    double offset_x, offset_y;
    int width, height;           /* output size: j < width, i < height                             */
    int out_stride;              /* floats per output row (>= width)                               */
    int check_w2;                /* 1: (u, v) = (-1, -1) when Z <= -w2 * d1 (rectify.cpp:27)       */
    long long out_offset;        /* first element of this map inside mapx / mapy                   */
    double w2;
} tscm_map_desc;

/* mapx / mapy: host arrays of n_elems floats (caller-owned); seconds_kernel (may be NULL) returns
 * the device time of the map kernel alone (HIP events), without the copy back to the host.     */
int tscm_build_maps(const tscm_map_desc *maps, int n_maps, int device, int exact, float *mapx,
                    float *mapy, size_t n_elems, double *seconds_kernel);

/* Output images that are not pinholes.  A pinhole image cannot reach 90 degrees off axis; the Triple Sphere model is for
 * lenses of 180 degrees and more, and the overlap of two adjacent cameras of a rig lies near the edge of both images.
 * The projection kind of map m travels beside its descriptor (tscm_map_desc is frozen).  With a = (j - cx)/fx and
 * b = (i - cy)/fy the ray before R is
 *   PERSPECTIVE    (a, b, 1)                                        fx, fy: pixels per unit tangent (tscm_build_maps)
 *   LONGLAT        (sin a, cos a sin b, cos a cos b)                pixels per radian; rows are planes through the x-axis,
 *                                                                   so with R = R_cam^T * R_pair rows are epipolar lines
 *   CYLINDRICAL    (sin a, b, cos a)                                fx: pixels per radian about y, fy: per unit height
 *   STEREOGRAPHIC  (a, b, 1 - r2/4) / (1 + r2/4), r2 = a^2 + b^2    pixels per unit of 2 tan(theta/2)
 *   EQUIRECT       (cos b sin a, sin b, cos b cos a)                pixels per radian: longitude about y, latitude
 * All send the centre pixel to (0, 0, 1) and agree with the pinhole to first order there.  Everything after the ray -- R,
 * the projection with its skew terms, check_w2, the offsets, out_stride / out_offset, untouched gaps, the refusals -- is
 * tscm_build_maps.  An unknown kind is TSCM_E_INVALID (before any device is touched; the text names the map).
 * projection == NULL or all PERSPECTIVE: the kernel of tscm_build_maps, the same bits.  PERSPECTIVE maps of a mixed
 * batch keep those bits too.  For the other kinds `exact` selects the exact-order arithmetic of the part AFTER the ray;
 * the ray itself comes from the device's fp64 sincos, which is accurate but not correctly rounded, so no bit-for-bit
 * promise is made for them.                                                                                          */
enum { TSCM_PROJ_PERSPECTIVE = 0, TSCM_PROJ_LONGLAT = 1, TSCM_PROJ_CYLINDRICAL = 2,
       TSCM_PROJ_STEREOGRAPHIC = 3, TSCM_PROJ_EQUIRECT = 4 };

int tscm_build_maps_ex(const tscm_map_desc *maps, const int *projection /* [n_maps], NULL = all perspective */,
                       int n_maps, int device, int exact, float *mapx, float *mapy, size_t n_elems,
                       double *seconds_kernel);

/* Tables of a sphere sweep (tscm_sweep_* below): n_cameras x D tables on one output grid.  maps[k] is camera k's table as
 * panorama_descs gives it (R = R_cam^T, all of one width x height), centers[k] the camera centre in the output frame (the
 * translation column of Twc), inv_distance[z] the inverse distance of hypothesis z.  Table (k, z) uses the ray
 *     dir(i, j) - inv_distance[z] * centers[k]
 * in front of R, dir being the ray of the map's projection kind exactly as tscm_build_maps_ex forms it: the point
 * dir / inv seen from camera k, scaled by inv.  The projection ignores the scale, so inv = 0 (infinity) needs no special
 * case and gives the table of tscm_build_maps_ex, bit for bit.  Everything after the ray is tscm_build_maps_ex: R, the
 * projection with its skew terms, check_w2, the offsets, `exact`.  The hypothesis surface is dir / inv: a sphere for
 * EQUIRECT, LONGLAT and STEREOGRAPHIC, a cylinder about y for CYLINDRICAL.  The output is dense: plane (k, z) starts at
 * element (k * D + z) * height * width of mapx / mapy.
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: a NULL pointer, n_cameras < 1,
 * D < 1, descriptors whose width / height differ from each other, out_stride != width or out_offset != 0, n_elems below
 * n_cameras * D * height * width, an inv_distance that is negative, not finite or not strictly increasing, a centre that is
 * not finite, an unknown projection kind.  TSCM_PROJ_PERSPECTIVE (plane sweep) is TSCM_E_UNSUPPORTED, as are more than
 * 65535 tables in one call.  device_index: as `device` of tscm_build_maps_ex, TSCM_E_NO_DEVICE outside
 * [0, tscm_device_count()), after the argument checks. */
int tscm_build_sweep_maps(const tscm_map_desc *maps /* [n_cameras] */, const int *projection /* [n_cameras] */, int n_cameras,
                          const double *centers /* [n_cameras][3] */, const double *inv_distance /* [D] */, int D,
                          int device_index, int exact, float *mapx, float *mapy /* [n_cameras][D][height][width] */,
                          size_t n_elems, double *seconds_kernel);

/* The inverse direction for single points: pixel of the sampled camera -> get_unit_sphere_coordinate -> R^T -> the
 * inverse of the table above (x/z, y/z | atan2(x, hypot(y, z)), atan2(y, z) | atan2(x, z), y/hypot(x, z) |
 * 2(x, y)/(1 + z) | atan2(x, z), atan2(y, hypot(x, z))) -> out = (a fx + cx, b fy + cy), a position in the OUTPUT image.
 * offset_x / offset_y do not enter: they belong to the sampled image (subtract them from the pixels first if the table
 * carries them).  valid[k] = 0 and out = NaN when the pixel is outside the model's domain, when the ray is outside the
 * projection's (PERSPECTIVE z <= 0, CYLINDRICAL x = z = 0, STEREOGRAPHIC z = -1), or when check_w2 is set and the ray
 * fails the w2 rule.  n == 0 returns 0 without touching a device.                                                     */
int tscm_rectify_points(const tscm_map_desc *map, int projection, const double *pixels /* [n*2] in the sampled camera */,
                        int n, int device, double *out /* [n*2] (x, y) in the output image */, unsigned char *valid /* [n] */);


/* ------------------------------------------------------------------ mono initialisation pieces
 * tscm_estimate_focal = TripleSphereCamera::estimate_focal (TS.cpp:110-168): one circle fit
 *   (cv::SVD::solveZ of a board_w x 4 matrix) per board row of every image with a board; *focal is
 *   the mean of the accepted samples, *n_used their number (0: "focal estimation failed", fx_ = 0).
 *   pix_u / pix_v: [n_views][board_w * board_h] host arrays, count[k] = pixels[k].size() (0 = no
 *   board in image k); (cx, cy) = the principal point guess of TS.cpp:43-44.
 * tscm_poses_from_r1r2t = the loop TS.cpp:62-74: Rt_[i] (row-major 3x3 [r1 r2 t]) -> rt_[i] =
 *   [cv::Rodrigues(R), t] with R built from float32 r1, r2 and their float cross product
 *   (has[i] == 0: rt left untouched).  Host-only.
 * tscm_estimate_extrinsic = TripleSphereCamera::estimate_extrinsic (TS.cpp:170-203): per image the
 *   "look at the board" rotation (:175-187), the corners un-projected onto that plane (:188-191) and a
 *   planar PnP.  The reference calls cv::solvePnPRansac there (external OpenCV routine, randomised);
 *   this entry point runs the deterministic equivalent for an all-inlier detection -- DLT homography,
 *   pose from its columns, polar orthonormalisation, Gauss-Newton on the 6 pose parameters -- so its
 *   result is NOT comparable bit-wise with OpenCV's, only as an initial guess of the same quality.
 *   Rt: [n_views*9] row-major 3x3 [r1 r2 t] = Rt_[k]; images with count[k] == 0 or a degenerate
 *   configuration keep the caller's values; *n_estimated = number of poses written.            */
int tscm_estimate_focal(const double *pix_u, const double *pix_v, const int *count, int n_views,
                        int board_w, int board_h, double cx, double cy, int device, double *focal,
                        int *n_used);
int tscm_poses_from_r1r2t(const double *Rt, const unsigned char *has, int n, double *rt);
int tscm_estimate_extrinsic(const double *intr9, const double *pix_u, const double *pix_v, const int *count,
                            int n_views, const double *worlds, int n_points, int board_w, int device,
                            double *Rt, int *n_estimated);
/* Stage outputs of the same two launches, for tests and diagnostics.
 * tscm_estimate_focal_rows: the arguments of tscm_estimate_focal, and gamma [n_views*board_h] receives
 *   what the row kernel wrote for row i of image k at k*board_h + i: -1 for an image without a board,
 *   -2 for a rejected row (t < 0 or nx^2 + ny^2 > 0.95, TS.cpp:149, :153), otherwise the sample (NaN
 *   where the row holds a NaN: neither rejection test fires on it).  Both entry points run one host
 *   helper, so tscm_estimate_focal's *focal / *n_used are the mean / number of the values >= 0 or NaN
 *   here, summed in (image, row) order.
 * tscm_estimate_extrinsic_stages: the arguments of tscm_estimate_extrinsic (Rt and *n_estimated as
 *   there), and per image k: T [9k..] the look-at turn R2*R1 (:175-187), H [9k..] the de-normalised
 *   homography (h33 = 1 before de-normalisation), pose0 [6k..] = (rv0, t0) from the columns of H after
 *   the polar factor, pose [6k..] = (rv, t) after Gauss-Newton, steps[k] = Gauss-Newton updates applied
 *   (0 .. 10), exit_code[k] = one of TSCM_EXTRINSIC_*.  Stage values an image does not reach are NaN
 *   (steps -1).  A pose is written to Rt exactly when exit_code >= TSCM_EXTRINSIC_CONVERGED.  A NaN
 *   pixel, or a reference corner outside the model's domain (alpha > 0.5 and a ray past the sphere),
 *   reaches the DLT as NaN and ends there with TSCM_EXTRINSIC_DLT_FAILED.                          */
#define TSCM_EXTRINSIC_NO_BOARD 1           /* count[k] == 0                                        */
#define TSCM_EXTRINSIC_DEGENERATE_BOARD 2   /* mean distance of the board points to their centre == 0 (or NaN) */
#define TSCM_EXTRINSIC_DLT_FAILED 3         /* the 8x8 normal equations are not positive definite  */
#define TSCM_EXTRINSIC_ZERO_COLUMN 4        /* a column of H has norm 0 (or NaN)                   */
#define TSCM_EXTRINSIC_CONVERGED 5          /* the Gauss-Newton step met the stopping rule         */
#define TSCM_EXTRINSIC_ITERATION_CAP 6      /* 10 Gauss-Newton updates without meeting it          */
#define TSCM_EXTRINSIC_GN_CHOLESKY 7        /* J^T J not positive definite: the last iterate is kept */
int tscm_estimate_focal_rows(const double *pix_u, const double *pix_v, const int *count, int n_views,
                             int board_w, int board_h, double cx, double cy, int device, double *gamma);
int tscm_estimate_extrinsic_stages(const double *intr9, const double *pix_u, const double *pix_v,
                                   const int *count, int n_views, const double *worlds, int n_points,
                                   int board_w, int device, double *Rt, int *n_estimated, double *T,
                                   double *H, double *pose0, double *pose, int *steps, int *exit_code);

/* ------------------------------------------------------------------ outlier-tolerant pose initialisation
 * tscm_estimate_extrinsic_ransac: the consensus search that cv::solvePnPRansac runs at the end of
 * TripleSphereCamera::estimate_extrinsic (TS.cpp:170-203), as a defined, repeatable procedure: a start pose that ignores
 * mislabelled or displaced corners, and a per-corner verdict.  tscm_estimate_extrinsic is not changed by it.
 * Per view k with count[k] != 0 (full boards only, corner i paired with board point worlds[i]):
 *   Turn      T = the look-at turn of tscm_estimate_extrinsic (same reference corner n_points/2 - board_w/2 - 1), and
 *             (x_i, y_i) = (X/Z, Y/Z) of the turned unit ray T ray(u_i, v_i).  Corner i is USABLE when u_i, v_i, x_i, y_i
 *             are finite and the turned Z > 0.
 *   Samples   hypothesis h = 0 .. n_hypotheses-1 draws 4 distinct corner indices by a partial Fisher-Yates shuffle of
 *             0 .. n_points-1: for draw d = 0..3 the word r = mix(mix(mix(mix(seed + 0x9e3779b9) + k) + h) + d) picks
 *             position j = d + ((uint64(r) * (n_points - d)) >> 32), the draw is the element there, and positions d and j
 *             are swapped.  mix = MurmurHash3's 32-bit finaliser fmix32 (h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13;
 *             h *= 0xc2b2ae35; h ^= h >> 16), all arithmetic modulo 2^32.  A sample is REJECTED when it holds a corner
 *             that is not usable, or when three of its corners are collinear on the integer lattice
 *             (i mod board_w, i div board_w).  A rejected sample is not redrawn: its hypothesis scores -1.
 *   H_h       the exact homography through the 4 pairs, by two projective bases: with p_j = (X, Y, 1) of sampled board
 *             point j = 1..4, c_1 = p_2 x p_3, c_2 = p_3 x p_1, c_3 = p_1 x p_2, lam_j = c_j . p_4, and the same on the
 *             image side (q_j = (x, y, 1), d_j, mu_j):  H_h = sum_{j=1..3} mu_j lam_{j+1} lam_{j+2} q_j c_j^T (indices
 *             cyclic), negated when its third row times p_1 is negative.
 *   Score     (a, b, w) = H_h (X_i, Y_i, 1) for every corner i of the view.  Corner i is an inlier when it is usable,
 *             w > 0, and du^2 + dv^2 <= threshold_px^2, (du, dv) = (u_i, v_i) - the Triple Sphere projection
 *             (tscm_project_points' arithmetic, skew terms included) of the ray T^T (a/w, b/w, 1).  Comparisons with NaN
 *             are false.  The score is the number of inliers.  threshold_px is in pixels of the camera.
 *   Winner    the highest score, ties to the lowest h.  No hypothesis with a score >= 0: TSCM_EXTRINSIC_NO_HYPOTHESIS.
 *             Winner's score < min_inliers (0 means max(4, ceil(n_points / 2))): TSCM_EXTRINSIC_FEW_INLIERS.  In both
 *             cases Rt keeps the caller's values, inlier is all 0 and n_inliers 0.
 *   Mask      inlier[k*n_points + i] = 1 for the winner's inliers, n_inliers[k] their number.
 *   Refit     tscm_estimate_extrinsic's steps on the masked corners: Hartley normalisation over the masked board points,
 *             DLT with h33 = 1, pose from the columns, polar factor, up to 10 Gauss-Newton updates with the same stopping
 *             rule; exit codes 2..7 keep their meaning on the masked set (the mask stays the winner's for 2..4), and
 *             Rt = T^T [r1 r2 t].
 * A pose is written to Rt exactly when the exit code is TSCM_EXTRINSIC_CONVERGED, _ITERATION_CAP or _GN_CHOLESKY (5..7);
 * the rule "exit_code >= TSCM_EXTRINSIC_CONVERGED" of tscm_estimate_extrinsic_stages does NOT carry over, because the two
 * codes below are larger.  *n_estimated counts the views with 5..7.  The sums of the refit are taken over the wave in a
 * fixed order: two calls give the same bytes.
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: a NULL pointer (n_inliers,
 * exit_code and seconds_kernel may be NULL; the per-view arrays may be NULL when n_views == 0), a struct_size that is not
 * sizeof(tscm_ransac_params), a threshold_px that is not > 0 (NaN included), n_hypotheses outside 1..4096, min_inliers
 * outside 0..n_points or in 1..3, n_points < 4, a board_w that tscm_estimate_extrinsic refuses.  n_points > 1024:
 * TSCM_E_UNSUPPORTED.  n_views == 0 returns 0 without touching a device.  device_index: as `device` elsewhere,
 * TSCM_E_NO_DEVICE outside [0, tscm_device_count()), after the argument checks.
 * tscm_estimate_extrinsic_ransac_stages: the same launch, and per view samples [k][h][4] (-1 where rejected),
 * score [k][h], winner [k] (-1: none), T, H_best (the winner's H_h at unit Frobenius norm), H_refit (the refit's
 * de-normalised homography), pose0 = (rv0, t0), pose = (rv, t), steps and rms_px [k]: the RMS over the masked corners of
 * the pixel residual at the refit pose, through the full model.  Stage values a view does not reach are NaN (steps -1),
 * samples and score of a view without a board -1.                                                                     */
#define TSCM_EXTRINSIC_NO_HYPOTHESIS 8      /* every sample was rejected                             */
#define TSCM_EXTRINSIC_FEW_INLIERS 9        /* the winner's score is below min_inliers               */
typedef struct tscm_ransac_params {
    int struct_size;                        /* sizeof(tscm_ransac_params)                            */
    double threshold_px;                    /* inlier distance in pixels, default 8.0                */
    int n_hypotheses;                       /* 1 .. 4096, default 256                                */
    int min_inliers;                        /* 0 = max(4, ceil(n_points / 2)), else 4 .. n_points    */
    unsigned seed;                          /* default 0                                             */
} tscm_ransac_params;
void tscm_ransac_default_params(tscm_ransac_params *p);
int tscm_estimate_extrinsic_ransac(const double *intr9, const double *pix_u, const double *pix_v, const int *count,
                                   int n_views, const double *worlds, int n_points, int board_w,
                                   const tscm_ransac_params *params, int device_index, double *Rt /* [V*9] */,
                                   unsigned char *inlier /* [V*n_points] */, int *n_inliers /* [V], may be NULL */,
                                   int *exit_code /* [V], may be NULL */, int *n_estimated,
                                   double *seconds_kernel /* may be NULL */);
int tscm_estimate_extrinsic_ransac_stages(const double *intr9, const double *pix_u, const double *pix_v, const int *count,
                                          int n_views, const double *worlds, int n_points, int board_w,
                                          const tscm_ransac_params *params, int device_index, double *Rt,
                                          unsigned char *inlier, int *n_inliers, int *exit_code, int *n_estimated,
                                          double *seconds_kernel, int *samples /* [V][H][4] */, int *score /* [V][H] */,
                                          int *winner /* [V] */, double *T, double *H_best, double *H_refit, double *pose0,
                                          double *pose, int *steps, double *rms_px);


/* ------------------------------------------------------------------ corner lists
 * The reference has no on-disk form of its input: corners go straight from findCorner() into
 * TripleSphereCamera::calibrate (main.cpp:40-49, 196-222).  This is the library's own, minimal text
 * format for them (fixtures, hand-over between a detector and the calibration), dense like the
 * reference's vectors: pixels()[board] per camera, empty where the board was not detected.
 *
 *   TSCM-CORNERS 1
 *   cameras <C> boards <B> cols <W> rows <H> pitch <mm> image <width> <height>
 *   view <camera> <board>            -- followed by W*H lines "<u> <v>" (%.17g: exact round trip)
 *   ...
 * Board point j = (v*pitch, u*pitch, 0), j = u*W + v (main.cpp:12-18).
 * tscm_corners_read allocates has / pix_u / pix_v (release with tscm_corners_free).  Host-only.  */
typedef struct tscm_corner_set {
    int n_cameras, n_boards, board_cols, board_rows;
    double pitch;
    int image_width, image_height;
    unsigned char *has;            /* [C*B]                                   */
    double *pix_u, *pix_v;         /* [C*B*cols*rows], zero where !has        */
} tscm_corner_set;

int tscm_corners_write(const char *path, const tscm_corner_set *set);
int tscm_corners_read(const char *path, tscm_corner_set *set);
void tscm_corners_free(tscm_corner_set *set);

/* ------------------------------------------------------------------ application of remap tables
 * tscm_remap = cv::remap(src, dst, mapx, mapy, cv::INTER_LINEAR) with the defaulted border (constant 0) as
 * TripleSphereCamera::undistort / undistort_chessboard call it (TS.cpp:304, :329) for 8-bit images of 1 or 3
 * interleaved channels; to_gray != 0 (3 channels): the result is converted like cv::cvtColor(BGR2GRAY)
 * (findCorner.cpp:9-10 on the remapped chessboard, main.cpp:71) and dst has one channel.  OpenCV's fixed-point
 * interpolation (coordinates to 1/32 pixel, 15-bit weights).  dst: map_height rows of dst_stride bytes.
 */
int tscm_remap(const unsigned char *src, int width, int height, int stride, int channels, const float *mapx, const float *mapy, int map_width,
               int map_height, int map_stride, int to_gray, int device, unsigned char *dst, int dst_stride);

/* ------------------------------------------------------------------ corner candidates (first stage)
 * tscm_detect_corners  = findCorner() up to and including its score filter (DetectCorner/findCorner.cpp:7-66:
 *                        gradient angle / weight, secondDerivCornerMetric :103-142, nonMaximumSuppression(cxy + c45,
 *                        4, 0.07, 5) :144-193, getOrientations(r = 10) :200-349, scoreCorners(radii 8, 12, 16)
 *                        :391-490, removal of candidates with score < min_score (0.01 in the reference)), plus the
 *                        quadratic sub-pixel fit of subPixelLocation (:492-541) for EVERY kept candidate (the
 *                        reference applies it to the candidates the structure recovery assigned to a board; the fit
 *                        of a candidate does not depend on that assignment).
 * Input: 8-bit grey image (the reference converts BGR with cv::cvtColor first), `stride` bytes per row; sigma as in
 * findCorner(img, sigma): even (cv::GaussianBlur needs the odd kernel size 7 sigma + 1), main.cpp:32 passes 4.
 * Output order = the order the suppression finds the maxima (columns of cells left to right, cells top to bottom).
 * The chessboard structure recovery (chessboardsFromCorners, DetectCorner/chessboard.cpp) consumes this list.
 */
typedef struct tscm_corner_candidates {
    int n;                  /* candidates kept                                                     */
    int n_maxima;           /* maxima of the corner metric before the score filter                 */
    double *x, *y;          /* [n] pixel of the maximum (integral values; x = column, y = row)     */
    double *v1, *v2;        /* [2n] the two edge directions (unit vectors; (0,0) if none found)    */
    double *score;          /* [n]                                                                 */
    double *sub;            /* [2n] sub-pixel position (x, y)                                      */
    double seconds;         /* device time of the kernels                                          */
} tscm_corner_candidates;

int tscm_detect_corners(const unsigned char *gray, int width, int height, int stride, int sigma, double min_score, int device,
                        tscm_corner_candidates *out);
/* The same for n_images images of one size in ONE pass of the kernels (a calibration run detects on every image of
 * every camera: main.cpp:24-50): out[n_images], each freed with tscm_corner_candidates_free; out[i].seconds is the
 * image's share of the batch's device time.  Results are identical to n_images single calls. */
int tscm_detect_corners_batch(const unsigned char *const *images, int n_images, int width, int height, int stride, int sigma, double min_score,
                              int device, tscm_corner_candidates *out);
void tscm_corner_candidates_free(tscm_corner_candidates *c);
/* The image planes of tscm_detect_corners_batch, from the same launches: ig = the normalised and blurred image
 * (findCorner.cpp:30-34, :106), metric = cxy + c45 (the input of the suppression) and ixy = Ixy (the input of the
 * sub-pixel fit), each [n_images][height][width] fp64; any of the three may be NULL.  Arguments are checked as in
 * tscm_detect_corners_batch.  For parity tests. */
int tscm_corner_planes_batch(const unsigned char *const *images, int n_images, int width, int height, int stride, int sigma, int device,
                             double *ig, double *metric, double *ixy);

/* ------------------------------------------------------------------ chessboard structure (second stage)
 * tscm_chessboards_from_corners = chessboardsFromCorners (DetectCorner/chessboard.cpp:3-103): 3x3 seeds around every
 * candidate, energy-driven growth on the four sides, overlap resolution by energy, boards turned so that
 * cols >= rows.  Host logic (sequential, a few hundred candidates), input = the lists of tscm_detect_corners
 * (x, y = pixel of the maximum; v1, v2 = [2n] edge directions).  Board q is the rows[q] x cols[q] row-major matrix of
 * candidate indices cells[offset[q] .. offset[q + 1]).  findCorner (:67-95) then reads the sub-pixel position of
 * every board member; main.cpp:33 accepts an image when exactly one board of the expected size came out.
 */
typedef struct tscm_chessboards {
    int n_boards;
    int *rows, *cols;       /* [n_boards]                         */
    int *offset;            /* [n_boards + 1] start of each board */
    int *cells;             /* candidate indices                  */
} tscm_chessboards;

int tscm_chessboards_from_corners(int n, const double *x, const double *y, const double *v1, const double *v2, tscm_chessboards *out);
void tscm_chessboards_free(tscm_chessboards *b);

/* The structure recovery for a batch of images, one independent job per (image, seed candidate), from ONE definition
 * for host and device (tscm_boards_core.h).  That definition is the function above operation by
 * operation except for the extrapolation of three corners p1, p2, p3, which it states without atan2 / cos / sin so that
 * host and device agree on every bit: a = p2 - p1, b = p3 - p2, (c1, s1) = a / |a|, (c2, s2) = b / |b| (each (1, 0) for
 * a zero vector), cc = c2 c2 - s2 s2, ss = 2 c2 s2, cos a3 = cc c1 + ss s1, sin a3 = ss c1 - cc s1,
 * pred = p3 + 0.75 (2 |b| - |a|) (cos a3, sin a3); no fused multiply-add, IEEE sqrt and division.  The final boards are
 * those of the function above unless two candidates lie at exactly the same distance from a prediction of a winning
 * proposal.  where = TSCM_BOARDS_HOST runs the serial instantiation and needs no device; TSCM_BOARDS_DEVICE runs the
 * kernel k_board_seeds, and passes an image of more than TSCM_BOARDS_MAX_DEVICE_CANDIDATES candidates through the host
 * instantiation (the same definition, the same result).  Of a candidate record only n, x, y, v1, v2 are read.
 * Refused with TSCM_E_INVALID: NULL cands (with n_images > 0) or out, a NULL list of an image with n > 0, a negative
 * n_images or n, an unknown `where`, a coordinate that is not finite or beyond 32767 in magnitude (where the integer
 * squares of the energy's column terms end); more than 65535 candidates are TSCM_E_UNSUPPORTED as above.  n_images = 0
 * and images with n < 9 give empty results.  out[n_images], each freed with the matching free function.  device_index:
 * as `device` elsewhere, read by a device call only (TSCM_E_NO_DEVICE outside the range of tscm_device_count).
 * The stages are the jobs' records per image, in seed order: status (0 blank seed, 1 seed energy > 0, 2 grown, but
 * energy not < -10, 3 board offered to the overlap resolution), rows x cols, accepted growth steps, energy and the
 * row-major cells of the board before the turn (none for status 0, the seed for status 1).  The boards of the batch
 * call are the status-3 records that the ordered overlap resolution keeps, turned so that cols >= rows. */
#define TSCM_BOARDS_HOST   0
#define TSCM_BOARDS_DEVICE 1
#define TSCM_BOARDS_MAX_DEVICE_CANDIDATES 1024
typedef struct tscm_board_seed_stages {
    int n;                  /* seeds = candidates of the image                          */
    int on_device;          /* 1: the image's jobs ran in the kernel                    */
    int *status;            /* [n]                                                      */
    int *rows, *cols;       /* [n] 0 x 0 for status 0, 3 x 3 for status 1               */
    int *steps;             /* [n] rows + cols - 6 for status 2 and 3                   */
    double *energy;         /* [n] 0 for status 0                                       */
    int *offset;            /* [n + 1] start of each record's cells                     */
    int *cells;             /* candidate indices                                        */
} tscm_board_seed_stages;
int tscm_chessboards_from_corners_batch(int n_images, const tscm_corner_candidates *cands, int where, int device_index, tscm_chessboards *out);
int tscm_chessboards_batch_stages(int n_images, const tscm_corner_candidates *cands, int where, int device_index, tscm_board_seed_stages *out);
void tscm_board_seed_stages_free(tscm_board_seed_stages *s);
/* device time of k_board_seeds in the calling thread's last device call, seconds (0 after a host call) */
double tscm_chessboards_batch_seconds(void);

/* ------------------------------------------------------------------ stereo matching on a rectified pair
 * What the rectified pair of tscm_build_maps_ex + tscm_remap is for: matching along rows (PERSPECTIVE or LONGLAT tables of
 * rectify_pair_descs / rectify_pair_maps, where a scene point lies on the same row of both images) and the 3-D points of
 * the disparities.  Census + semi-global matching, integer arithmetic throughout, defined here operation by operation so
 * that a host restatement gives the same bits (tests/stereo_ref.py).  D = num_disparities, d_k = min_disparity + k.
 *   census   9 wide x 7 high window, dy = -3..3 outer, dx = -4..4 inner, centre skipped, coordinates clamped to the image:
 *            code = (code << 1) | (neighbour < centre); 62 bits.
 *   cost     C(y, x, k) = popcount(censusL(y, x) ^ censusR(y, x - d_k)); 64 where x - d_k is outside [0, width).
 *   paths    directions (dx, dy) in the order (1,0) (-1,0) (0,1) (0,-1) (1,1) (-1,-1) (1,-1) (-1,1), the first `paths`.
 *            L_r(p, k) = C(p, k) where p - r is outside the image, otherwise
 *            C(p, k) + min(L_r(p-r, k), L_r(p-r, k-1) + p1, L_r(p-r, k+1) + p1, m + p2) - m,  m = min_k L_r(p-r, k);
 *            terms with k +- 1 outside [0, D) are absent.  S = sum_r L_r (uint16; p2 <= 255 and C <= 64 rule out overflow).
 *   winner   k* = the lowest k at which S is minimal.
 *   uniqueness_ratio > 0: invalid if any k with |k - k*| > 1 has S(k) * (100 - ratio) < S(k*) * 100.
 *   disp12_max_diff >= 0: kR(y, x2) = the lowest k minimising S(y, x2 + d_k, k) over the k whose x2 + d_k is inside the
 *            image; with x2 = x - d_k*: invalid if x2 is outside the image or |kR(y, x2) - k*| > disp12_max_diff.
 *   output   16 d_k*, plus for 0 < k* < D - 1 the parabola term floor(((S(k*-1) - S(k*+1)) * 16 + den) / (2 den)) with
 *            den = max(S(k*-1) + S(k*+1) - 2 S(k*), 1) (floor division, as OpenCV's StereoSGBM); invalid pixels get
 *            16 (min_disparity - 1).
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: NULL images / params /
 * disparity, stride or disp_stride < width, a struct_size other than sizeof(tscm_stereo_params), num_disparities not a
 * multiple of 16 in 16..256, paths other than 4 or 8, p1 or p2 outside 0 <= p1 <= p2 <= 255, uniqueness_ratio outside
 * 0..99, a min_disparity whose 16-fold output leaves 16 bits (below -2047, or min_disparity + D above 2047).
 * width == 0 or height == 0 returns 0 without touching a device.  Elements of `disparity` between width and disp_stride
 * keep the caller's values.  device_index: as `device` elsewhere, TSCM_E_NO_DEVICE outside [0, tscm_device_count()).
 * seconds_kernel (may be NULL): device time of the kernels (HIP events), without the copies. */
typedef struct tscm_stereo_params {
    int struct_size;        /* sizeof(tscm_stereo_params)                     */
    int min_disparity;      /* may be negative                                */
    int num_disparities;    /* D: multiple of 16, 16..256                     */
    int p1, p2;             /* 0 <= p1 <= p2 <= 255                           */
    int paths;              /* 4 or 8                                         */
    int uniqueness_ratio;   /* 0..99, 0 = off                                 */
    int disp12_max_diff;    /* < 0 = no left-right check                      */
} tscm_stereo_params;
void tscm_stereo_default_params(tscm_stereo_params *p);   /* 0, 128, 8, 32, 8, 10, 1 */

int tscm_stereo_match(const unsigned char *left, const unsigned char *right, int width, int height, int stride,
                      const tscm_stereo_params *params, int device_index,
                      short *disparity /* [height][disp_stride], 16 * d, invalid = 16 * (min_disparity - 1) */,
                      int disp_stride, double *seconds_kernel /* may be NULL */);

/* The stages of the same launches, for parity tests (like tscm_corner_planes_batch): any output may be NULL. */
int tscm_stereo_stages(const unsigned char *left, const unsigned char *right, int width, int height, int stride,
                       const tscm_stereo_params *params, int device_index,
                       unsigned long long *census_left, unsigned long long *census_right /* [h*w] */,
                       unsigned char *cost /* [h*w*D] */, unsigned short *aggregated /* [h*w*D] */);

/* Device seconds of the calling thread's last tscm_stereo_match / tscm_stereo_stages by stage: census (both images), cost,
 * path aggregation, kR of the left-right check, winner. */
int tscm_stereo_stage_times(double *seconds /* [5] */);

/* Points of a disparity map in the pair frame of the left camera (x along the baseline, the right camera at +baseline, so
 * disparities are positive).  With x, y the pixel, d = disparity / 16.0 and fx fy cx cy of left_map (fp64):
 *   PERSPECTIVE  Z = fx B / d,  X = (x - cx)/fx Z,  Y = (y - cy)/fy Z
 *   LONGLAT      aL = (x - cx)/fx, aR = aL - d/fx, b = (y - cy)/fy, r = B cos aR / sin(aL - aR)  [law of sines in the
 *                epipolar plane],  P = r (sin aL, cos aL sin b, cos aL cos b)
 * valid = 0 and P = NaN where the disparity is the invalid value 16 (min_disparity - 1) or d <= 0.  Any other projection,
 * a NULL pointer or disp_stride < width: TSCM_E_INVALID before any device is touched. */
int tscm_stereo_points(const short *disparity, int width, int height, int disp_stride, int min_disparity,
                       const tscm_map_desc *left_map, int projection, double baseline, int device_index,
                       double *points /* [h*w*3] */, unsigned char *valid /* [h*w] */);

/* Post-filter of a disparity map: speckle removal (OpenCV's speckleWindowSize / speckleRange, which the matcher above
 * leaves out) and a masked median.  Integers throughout, defined here so that a host restatement gives the same bits
 * (tests/stereo_filter_ref.py).
 *   input       d [height][disp_stride] int16; invalid = 16 (min_disparity - 1); a pixel is valid iff d != invalid.
 *   edges       two 4-neighbours p, q are joined iff both are valid and |d(p) - d(q)| <= 16 speckle_range, the difference
 *               taken in int32.  This is the relation cv::filterSpeckles grows regions by (it compares with the current
 *               pixel, not with the seed), so a ramp whose steps each stay within the range is one component however far
 *               apart its ends are.
 *   components  the connected components of that graph.  label(p) = the smallest linear index y * width + x of p's
 *               component, -1 for an invalid p; size(p) = the component's pixel count, 0 for an invalid p.  Neither
 *               depends on an order of traversal.
 *   speckle     speckle_window_size > 0: every pixel with size(p) <= speckle_window_size becomes invalid (<=, as OpenCV);
 *               0 switches the rule off.
 *   median      median = 3 or 5, on the map after the speckle rule: an invalid pixel stays invalid (no hole filling); for
 *               a valid pixel take the valid pixels of the median x median window that lie inside the image (nothing is
 *               clamped or replicated), n >= 1 of them, sort them ascending: the output is the element at index
 *               (n - 1) >> 1.  median = 0: no median.
 * With speckle_window_size = 0 and median = 0 the output equals the input.  out == disparity with equal strides is allowed
 * (the device works on its own copies); elements of `out` between width and out_stride keep the caller's values.
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: a NULL disparity / params / out,
 * disp_stride or out_stride < width, a struct_size other than sizeof(tscm_stereo_filter_params), speckle_window_size < 0,
 * speckle_range outside 0..255, median other than 0, 3, 5, a min_disparity outside -2047..2031 (what the matcher accepts
 * at its smallest num_disparities), width * height above INT_MAX (labels are int32).  width == 0 or height == 0 returns 0
 * without touching a device.  device_index and seconds_kernel: as for the matcher. */
typedef struct tscm_stereo_filter_params {
    int struct_size;          /* sizeof(tscm_stereo_filter_params)                  */
    int min_disparity;        /* defines the invalid value, as for the matcher      */
    int speckle_window_size;  /* 0 = off; components of at most this many pixels go */
    int speckle_range;        /* whole disparities, 0..255; the edge test uses 16 x */
    int median;               /* 0, 3 or 5                                          */
} tscm_stereo_filter_params;
void tscm_stereo_filter_default_params(tscm_stereo_filter_params *p);   /* 0, 100, 2, 0 */

int tscm_stereo_filter(const short *disparity, int width, int height, int disp_stride,
                       const tscm_stereo_filter_params *params, int device_index,
                       short *out /* [height][out_stride] */, int out_stride, double *seconds_kernel /* may be NULL */);

/* The stages of the same launches, for parity tests: any output may be NULL.  despeckled: the map after the speckle rule
 * and before the median (the input itself with speckle_window_size = 0). */
int tscm_stereo_filter_stages(const short *disparity, int width, int height, int disp_stride,
                              const tscm_stereo_filter_params *params, int device_index,
                              int *label /* [h*w] */, int *size /* [h*w] */, short *despeckled /* [h*w] */);

/* Hole filling of a disparity map or a sweep index map: the interpolation of Hirschmueller's SGM paper, section 2.6.  Every
 * stage above can only invalidate; this one puts values back.  Integers throughout and nothing depends on an order, defined
 * here so that a host restatement gives the same bits (tests/stereo_fill_ref.py).
 *   input       d [height][disp_stride] int16; invalid = 16 (min_disparity - 1); a pixel is valid iff d != invalid.  A sweep
 *               index map (tscm_sweep_depth) is such a map with min_disparity = 0.
 *   directions  (dx, dy) in the matcher's order: (1,0) (-1,0) (0,1) (0,-1) (1,1) (-1,-1) (1,-1) (-1,1); the first `paths`
 *               of them are used, paths = 4 or 8.
 *   walk        for a pixel p = (x, y) and a direction r visit (x + t dx, y + t dy), t = 1, 2, ...  The walk ends without a
 *               result when the row leaves [0, height), when max_distance > 0 and t > max_distance, and with wrap_x = 0 when
 *               the column leaves [0, width).  With wrap_x = 1 the column is taken modulo width, and a horizontal walk ends
 *               after t = width - 1, so it never reaches p itself; diagonals continue over the seam.  The first valid pixel
 *               met gives the candidate v_r and its distance t_r.  The walk reads the input map only, never a filled value.
 *               Candidates are defined for every pixel, valid or not.
 *   fill        a valid pixel keeps its value, mask 0.  For an invalid pixel let n be the number of directions with a
 *               candidate: n < min_directions leaves it invalid, mask 2; otherwise, mask 1, the candidates are sorted
 *               ascending as int32, v[0] <= ... <= v[n - 1], and the output is
 *                 TSCM_FILL_LOWEST         v[0]
 *                 TSCM_FILL_SECOND_LOWEST  v[min(1, n - 1)]     (the background of an occlusion)
 *                 TSCM_FILL_MEDIAN         v[(n - 1) >> 1]      (a mismatch)
 * out == disparity with equal strides is allowed (the device works on its own copies); elements of `out` between width and
 * out_stride keep the caller's values.  mask [h*w] may be NULL.
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: a NULL disparity / params / out,
 * disp_stride or out_stride < width, a struct_size other than sizeof(tscm_stereo_fill_params), rule outside 0..2, paths
 * other than 4 or 8, min_directions outside 1..paths, max_distance outside 0..32767, wrap_x other than 0 or 1, a
 * min_disparity outside -2047..2031 (the filter's range), width or height above 32767 (distances are int16).  width == 0 or
 * height == 0 returns 0 without touching a device.  device_index and seconds_kernel: as for the matcher. */
#define TSCM_FILL_LOWEST 0
#define TSCM_FILL_SECOND_LOWEST 1
#define TSCM_FILL_MEDIAN 2
typedef struct tscm_stereo_fill_params {
    int struct_size;     /* sizeof(tscm_stereo_fill_params)                              */
    int min_disparity;   /* defines the invalid value, as for the matcher; 0 for a sweep */
    int rule;            /* TSCM_FILL_*                                                  */
    int paths;           /* 4 or 8                                                       */
    int max_distance;    /* 0 = unlimited; else the longest walk, 1..32767               */
    int min_directions;  /* 1..paths: fewer candidates leave the pixel invalid           */
    int wrap_x;          /* 1: column 0 follows column width - 1 (a 360 degree map)      */
} tscm_stereo_fill_params;
void tscm_stereo_fill_default_params(tscm_stereo_fill_params *p);   /* 0, MEDIAN, 8, 0, 1, 0 */

int tscm_stereo_fill(const short *disparity, int width, int height, int disp_stride,
                     const tscm_stereo_fill_params *params, int device_index,
                     short *out /* [height][out_stride] */, int out_stride, unsigned char *mask /* [h*w], may be NULL */,
                     double *seconds_kernel /* may be NULL */);

/* The candidates of the same launches, for parity tests: value and distance [paths][h*w], either may be NULL.  Without a
 * candidate value holds the invalid value and distance 0. */
int tscm_stereo_fill_stages(const short *disparity, int width, int height, int disp_stride,
                            const tscm_stereo_fill_params *params, int device_index,
                            short *value /* [paths][h*w] */, short *distance /* [paths][h*w], 0 = none */);

/* Edge-aware refinement of a disparity map or a sweep index map: the joint weighted median (Ma et al., "Constant time
 * weighted median filtering for stereo matching and beyond", ICCV 2013).  Every stage above looks at the map alone; this one
 * looks at the image the map belongs to: each pixel takes the median of its window, the neighbours weighted by how close
 * their grey value is to the centre's, so that a depth edge moves back to the intensity edge and the streaks of a fill are
 * smoothed without a value invented between foreground and background.  Integers throughout and nothing depends on an
 * order, defined here so that a host restatement gives the same bits (tests/stereo_refine_ref.py).
 * One pass on a map d [height][disp_stride] int16 with the guide g [height][guide_stride] uint8 (one channel), the table
 * lut = range_weight (NULL: every entry 255) and inv = 16 (min_disparity - 1):
 *   participants  of p = (x, y): the offsets (dx, dy), |dx|, |dy| <= radius, (0, 0) included, for which the row y + dy lies
 *                 in [0, height) (rows are never clamped or wrapped), the column x + dx lies in [0, width) -- or wrap_x is
 *                 set and it is taken modulo width -- and d(q) != inv at that pixel q.  With wrap_x and a window wider than
 *                 the map a pixel takes part once per offset that names it.
 *   weight        w_q = lut[|g(p) - g(q)|], the difference taken in int.
 *   stage values  W(p) = sum of w_q and count(p) = the number of participants, for every pixel, valid or not;
 *                 W <= 225 * 255.
 *   output        d(p) == inv and fill_invalid == 0: inv.  Otherwise W(p) == 0: d(p).  Otherwise the smallest v among the
 *                 participants' values, compared as int32, with 2 * (sum of w_q over the participants with d(q) <= v) >= W(p):
 *                 the lower weighted median.  Equal values accumulate.
 *   passes        pass i + 1 reads the whole output of pass i (Jacobi), never a value of its own pass; guide and table stay.
 * Consequences: with all weights equal and non-zero and fill_invalid = 0, radius 1 / 2 is the median 3 / 5 of
 * tscm_stereo_filter with the speckle rule off, bit for bit; a constant valid map is a fixed point.
 * tscm_stereo_refine_weights (host code only): lut[k] = floor(255 exp(-k / sigma) + 0.5) in double for sigma > 0, +infinity
 * giving 255 throughout; a sigma that is not > 0 (NaN included) gives 255, 0, 0, ...
 * out == disparity with equal strides is allowed (the device works on its own copies); elements of `out` between width and
 * out_stride keep the caller's values.  Any int16 is accepted as a value, -32768 and 32767 included.
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: a NULL disparity / guide / params /
 * out, disp_stride, guide_stride or out_stride < width, a struct_size other than sizeof(tscm_stereo_refine_params), radius
 * outside 1..7, iterations outside 1..8, fill_invalid or wrap_x other than 0 or 1, a min_disparity outside -2047..2031,
 * width * height above INT_MAX.  width == 0 or height == 0 returns 0 without touching a device.  device_index and
 * seconds_kernel: as for the fill. */
typedef struct tscm_stereo_refine_params {
    int struct_size;     /* sizeof(tscm_stereo_refine_params)                                  */
    int min_disparity;   /* defines the invalid value 16 (min_disparity - 1); 0 for a sweep    */
    int radius;          /* 1..7: the window is (2 radius + 1)^2, at most 225 pixels           */
    int iterations;      /* 1..8 passes, each on the whole output of the one before            */
    int fill_invalid;    /* 0: an invalid pixel stays invalid; 1: it is refined like any other */
    int wrap_x;          /* 1: columns are taken modulo width (a 360 degree map)               */
} tscm_stereo_refine_params;
void tscm_stereo_refine_default_params(tscm_stereo_refine_params *p);   /* 0, 3, 1, 0, 0 */

void tscm_stereo_refine_weights(double sigma, unsigned char *range_weight /* [256] */);

int tscm_stereo_refine(const short *disparity, int width, int height, int disp_stride,
                       const unsigned char *guide /* [height][guide_stride], one channel */, int guide_stride,
                       const unsigned char *range_weight /* [256], NULL = all 255 */,
                       const tscm_stereo_refine_params *params, int device_index,
                       short *out /* [height][out_stride] */, int out_stride, double *seconds_kernel /* may be NULL */);

/* The stage values of the first pass, for parity tests: weight_sum, count and the map after that pass, each [h*w], any of
 * them may be NULL. */
int tscm_stereo_refine_stages(const short *disparity, int width, int height, int disp_stride,
                              const unsigned char *guide, int guide_stride, const unsigned char *range_weight,
                              const tscm_stereo_refine_params *params, int device_index,
                              int *weight_sum /* [h*w] */, unsigned char *count /* [h*w] */, short *first_pass /* [h*w] */);

/* ------------------------------------------------------------------ panorama of a calibrated rig
 * What the tables of panorama_descs (one EQUIRECT or CYLINDRICAL table per camera, all in the rig frame) are for: the
 * stitched image.  A handle keeps everything that does not depend on a frame on the device -- the sample positions, the
 * alphas, the seam labels, the mask pyramids -- so a frame costs its upload, the kernels and the download of the panorama.
 * Every step up to the output bytes is integer arithmetic, defined here operation by operation so that a host restatement
 * gives the same bits (tests/pano_ref.py).  n = n_cameras, C = channels, (i, j) = output row, column.
 *   sample     v_k[c] = the arithmetic of the remap entry point above on image k: sx = round(32 mapx), ix = sat16(sx >> 5),
 *              fx = sx & 31 (y alike), weights 32 (32 - fx)(32 - fy), 32 fx (32 - fy), 32 (32 - fx) fy, 32 fx fy with 32768
 *              replaced by 32767 and the last weight by 1, (acc + 2^14) >> 15, taps outside the image 0.
 *              a_k = the same arithmetic on weight image k (one channel); a NULL weight is a constant 255 image, whose border
 *              taps still ramp a_k to 0, so the (-1, -1) entries of check_w2 give a_k = 0 without a special case.
 *              With a gain g (Q8): v_k[c] = min(255, (v_k[c] g + 128) >> 8).
 *   label      the lowest k whose a_k is maximal, 255 when that maximum is 0.   coverage = the number of k with a_k > 0.
 *   SEAM       out = v_label, 0 without a label.
 *   FEATHER    A = sum_k a_k:  out[c] = A ? (sum_k a_k v_k[c] + (A >> 1)) / A : 0.
 *   MULTIBAND  L = levels; pano_w and pano_h are multiples of 2^L.  Per camera G^0 = v_k (int16), M^0 = 255 where
 *              label == k, else 0.  With taps t = [1, 4, 6, 4, 1], rows clamped (cy) and columns wrapped when wrap_x is set,
 *              else clamped (cx), all shifts arithmetic:
 *                reduce  R(x)(i, j) = (sum_a sum_b t_a t_b x(cy(2i + a - 2), cx(2j + b - 2)) + 128) >> 8
 *                expand  E(x)(i, j) = (sum over a, b in -2..2 with i + a and j + b both even of
 *                                      t_a t_b x(cy((i + a) / 2), cx((j + b) / 2)) + 32) >> 6        (x on the half-size grid)
 *              G^(l+1) = R(G^l), M^(l+1) = R(M^l);  Lap^l = G^l - E(G^(l+1)) for l < L, Lap^L = G^L.
 *              Per level, W = sum_k M_k^l:  B^l[c] = W ? floor((sum_k M_k^l Lap_k^l[c] + (W >> 1)) / W) : 0 -- the division
 *              rounds towards minus infinity.  Collapse R^L = B^L, R^l = B^l + E(R^(l+1)); out = clamp(R^0, 0, 255), and 0
 *              where coverage == 0.  This is OpenCV's multi-band blender, its known weakness included: at the coarse levels
 *              black leaks in within about 2^(L+1) pixels of the edge of a camera's coverage.
 *              With one camera, a NULL weight and every sample inside the image the result is the remapped image, byte for
 *              byte: floor((M x + (M >> 1)) / M) = x.
 *   overlap    lum = v before any gain (C = 1), or its BGR2GRAY value (b 1868 + g 9617 + r 4899 + 2^13) >> 14 (C = 3);
 *              count[a][b] = the number of pixels with a_a > 0 and a_b > 0, sum[a][b] = the sum of lum_a over them; the
 *              diagonal is camera a's own coverage.  Integer sums: the result does not depend on the order.
 * Pyramids of the stage outputs: levels 0..L one after the other, level l a [pano_h >> l][pano_w >> l] plane, S elements in
 * all; mask_pyramid [n][S] (uint8), lap_pyramid [n][C][S] and blend_pyramid [C][S] (int16, B^l before the collapse);
 * sampled [n][pano_h][pano_w][C] (after the gain), alpha [n][pano_h][pano_w], label [pano_h][pano_w].
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: a required pointer that is NULL,
 * n_cameras outside 1..16, channels other than 1 or 3, an unknown mode, levels outside 1..6 in MULTIBAND, pano_w or pano_h
 * below 1 or (MULTIBAND) no multiple of 2^levels, a struct_size other than sizeof(tscm_panorama_params), stride <
 * width * channels, dst_stride < pano_w * channels, a gain outside 1..4095, a source image with a side below 1 or above 32767,
 * a pyramid output of the stages call when the mode is not MULTIBAND.  device_index: as `device` elsewhere, TSCM_E_NO_DEVICE
 * outside [0, tscm_device_count()), after the argument checks.  Bytes of dst between pano_w * channels and dst_stride keep
 * the caller's values.  seconds_kernel (may be NULL): device time of the frame's kernels (HIP events), without the copies.
 * A handle serves one thread at a time. */
enum { TSCM_PANO_SEAM = 0, TSCM_PANO_FEATHER = 1, TSCM_PANO_MULTIBAND = 2 };

typedef struct tscm_panorama_params {
    int struct_size;        /* sizeof(tscm_panorama_params)                                     */
    int mode;               /* TSCM_PANO_*                                                      */
    int levels;             /* MULTIBAND: 1..6, otherwise ignored                               */
    int wrap_x;             /* 1: column -1 is column pano_w - 1 (full 360 degree tables)       */
} tscm_panorama_params;
void tscm_panorama_default_params(tscm_panorama_params *p);   /* MULTIBAND, 4, 1 */

typedef struct tscm_panorama tscm_panorama;   /* opaque: tables, alphas, seam labels, mask pyramids on the device */

int tscm_panorama_create(int n_cameras, int width, int height, int channels /* the source images, all alike */,
                         const unsigned char *const *weights /* [n] of [height][width]; NULL or a NULL entry = all 255 */,
                         const float *mapx, const float *mapy /* [n][pano_h][pano_w] */, int pano_w, int pano_h,
                         const tscm_panorama_params *params, int device_index, tscm_panorama **out);

int tscm_panorama_compose(tscm_panorama *p, const unsigned char *const *images /* [n] of [height][stride] */, int stride,
                          const unsigned short *gain_q8 /* [n], NULL = 256 */,
                          unsigned char *dst /* [pano_h][dst_stride] */, int dst_stride,
                          unsigned char *coverage /* [pano_h][pano_w], may be NULL */, double *seconds_kernel);

/* The stages of the same kernels, for parity tests: any output may be NULL. */
int tscm_panorama_stages(tscm_panorama *p, const unsigned char *const *images, int stride, const unsigned short *gain_q8,
                         unsigned char *sampled, unsigned char *alpha, unsigned char *label,
                         unsigned char *mask_pyramid, short *lap_pyramid, short *blend_pyramid);

int tscm_panorama_overlap(tscm_panorama *p, const unsigned char *const *images, int stride,
                          long long *count /* [n*n] */, long long *sum /* [n*n] */);

void tscm_panorama_destroy(tscm_panorama *p);

/* ------------------------------------------------------------------ sphere-sweep depth of a calibrated rig
 * Depth in the rig frame over the whole panorama, from all cameras at once: for each pixel (i, j) of the rig-frame panorama
 * and each inverse-distance hypothesis z the point dir(i, j) / inv_distance[z] is projected into every camera (the tables of
 * tscm_build_sweep_maps), the cameras that see it are compared by their census codes, and the cost volume is regularised and
 * searched as the stereo matcher's is.  A handle keeps the n x D packed tables on the device: n * D * pano_w * pano_h * 8
 * bytes.  Integer arithmetic up to the index map, defined here operation by operation so that a host restatement gives the
 * same bits (tests/sweep_ref.py).  n = n_cameras, D = num_hypotheses, V(i, j, z) = { k : a_k(i, j, z) > 0 }.
 *   sample     v_k(i, j, z) and a_k(i, j, z): the `sample` rule of the panorama above on table (k, z), one channel, no
 *              gain: 1/32 px positions, 15-bit weights, (acc + 2^14) >> 15, taps outside the image 0; a NULL weight is a
 *              constant 255 image whose border taps ramp a_k to 0.
 *   census     the 9 x 7 code of tscm_stereo_match on the plane v_k(., ., z): rows clamped, columns wrapped when wrap_x is
 *              set and clamped otherwise.  A neighbour without coverage takes part with its sampled value (0 outside the
 *              image); there is no special case.
 *   cost       |V| < 2: C(i, j, z) = 64.  Otherwise, with P = |V| (|V| - 1) / 2 pairs,
 *              C(i, j, z) = (sum over a < b in V of popcount(census_a ^ census_b) + (P >> 1)) / P, at most 62.  So C == 64
 *              says exactly that fewer than two cameras see the point.
 *   paths, S, winner, uniqueness, parabola: the rules of tscm_stereo_match on this C (the diagonal paths restart at the
 *              column ends, also with wrap_x: the aggregation does not run over the 360 degree seam), with
 *              min_disparity = 0 and no left-right check, and one more rule: the pixel is invalid if C(i, j, k*) == 64.
 *   output     index16 = 16 k* + the parabola term (int16); invalid = -16.
 *   points     (fp64) s = index16 / 16, k0 = min(floor(s), D - 2),
 *              inv = inv_distance[k0] + (s - k0) (inv_distance[k0 + 1] - inv_distance[k0]),  P = dir(i, j) / inv in the
 *              output (rig) frame, dir the ray of pano_map's projection kind before R; valid = 0 and P = NaN for an invalid
 *              pixel (index16 < 0) or inv <= 0.
 * Stage outputs: sampled, alpha [n][D][pano_h][pano_w] uint8, census alike uint64, cost [pano_h][pano_w][D] uint8,
 * aggregated alike uint16; any of them may be NULL.
 * Refused with TSCM_E_INVALID before any device is touched, the text naming the argument: a required pointer that is NULL,
 * a struct_size other than sizeof(tscm_sweep_params), num_hypotheses not a multiple of 16 in 16..256, p1 or p2 outside
 * 0 <= p1 <= p2 <= 255, paths other than 4 or 8, uniqueness_ratio outside 0..99, n_cameras outside 2..8, a source image
 * with a side below 1 or above 32767, pano_w or pano_h below 1, stride < width, out_stride < pano_w; for the points a
 * stride < pano_w, D outside 2..2048, an inv_distance that is not finite, an unknown projection kind (PERSPECTIVE is
 * TSCM_E_UNSUPPORTED, as is a panorama of more than 2^31 - 1 pixels).  device_index: as `device` elsewhere,
 * TSCM_E_NO_DEVICE outside [0, tscm_device_count()), after the argument checks.  Elements of index16 between pano_w and
 * out_stride keep the caller's values.  seconds_kernel (may be NULL): device time of the frame's kernels (HIP events),
 * without the copies.  A handle serves one thread at a time. */
typedef struct tscm_sweep_params {
    int struct_size;        /* sizeof(tscm_sweep_params)                                                     */
    int num_hypotheses;     /* D: multiple of 16, 16..256 (what the aggregation serves)                      */
    int p1, p2;             /* 0 <= p1 <= p2 <= 255                                                          */
    int paths;              /* 4 or 8                                                                        */
    int uniqueness_ratio;   /* 0..99, 0 = off                                                                */
    int wrap_x;             /* 1: the census window wraps over the column ends (full 360 degree tables)      */
} tscm_sweep_params;
void tscm_sweep_default_params(tscm_sweep_params *p);   /* 64, 8, 32, 8, 10, 1 */

typedef struct tscm_sweep tscm_sweep;   /* opaque: the packed tables and the frame's volumes on the device */

int tscm_sweep_create(int n_cameras /* 2..8 */, int width, int height /* grey source images, all alike */,
                      const unsigned char *const *weights /* as tscm_panorama_create */,
                      const float *mapx, const float *mapy /* [n][D][pano_h][pano_w] */, int pano_w, int pano_h,
                      const tscm_sweep_params *params, int device_index, tscm_sweep **out);

int tscm_sweep_depth(tscm_sweep *s, const unsigned char *const *images /* [n] of [height][stride] */, int stride,
                     short *index16 /* [pano_h][out_stride] */, int out_stride, double *seconds_kernel);

/* The stages of the same kernels, for parity tests: any output may be NULL. */
int tscm_sweep_stages(tscm_sweep *s, const unsigned char *const *images, int stride,
                      unsigned char *sampled, unsigned char *alpha, unsigned long long *census,
                      unsigned char *cost, unsigned short *aggregated);

/* Device seconds of the calling thread's last tscm_sweep_depth / tscm_sweep_stages by stage: cost volume, path
 * aggregation, winner. */
int tscm_sweep_stage_times(double *seconds /* [3] */);

int tscm_sweep_points(const short *index16, int pano_w, int pano_h, int stride, const tscm_map_desc *pano_map, int projection,
                      const double *inv_distance /* [D] */, int D, int device_index,
                      double *points /* [h*w*3], rig frame */, unsigned char *valid /* [h*w] */);

/* The frame composed at the swept depth.  tscm_panorama_compose samples every camera through its table at infinity, so
 * whatever is nearer than a few tens of metres is doubled where two cameras overlap; the handle already keeps the record of
 * every camera, hypothesis and panorama pixel, the same 8-byte record with its alpha, so the frame can be composed at the
 * hypothesis the index map names.  Integer arithmetic throughout, restated in tests/sweep_compose_ref.py.
 *   hypothesis z(i, j) = index16(i, j) < 0 ? fallback_index : min(D - 1, (index16(i, j) + 8) >> 4): the nearest hypothesis,
 *              no interpolation between two.  Any int16 map is accepted, the raw one of tscm_sweep_depth or one filtered
 *              by tscm_stereo_filter.
 *   sample     v_k(i, j)[c] = the panorama's `sample` rule on the record (k, z(i, j)) at pixel (i, j), on the caller's
 *              images of 1 or 3 channels (they need not be the grey images of the depth pass), then the Q8 gain;
 *              a_k(i, j) = that record's alpha.
 *   blending   label, coverage, SEAM, FEATHER and MULTIBAND (masks, reduce, expand, floor division, collapse, wrap_x) are
 *              the panorama's rules on these v_k and a_k, unchanged.  Labels, coverage and the mask pyramids therefore
 *              depend on the frame.
 * So with a constant map 16 z0 the output equals tscm_panorama_compose on the tables (., z0) byte for byte, and with
 * inv_distance[0] = 0, an all-invalid map and fallback_index = 0 it equals today's panorama at infinity.
 * Stage outputs: hypothesis [pano_h][pano_w] uint8; sampled [n][pano_h][pano_w][C] (after the gain), alpha
 * [n][pano_h][pano_w], label [pano_h][pano_w]; the pyramids as tscm_panorama_stages lays them out; any of them may be NULL.
 * index16 == NULL: the map of this handle's last tscm_sweep_depth, which is still on the device.  The composer's buffers are
 * allocated by the first call and again only when (channels, mode, levels) changes; tscm_sweep_create and tscm_sweep_depth
 * are as before.
 * Refused with TSCM_E_INVALID, the text naming the argument, a NULL handle before any device is touched: what
 * tscm_panorama_compose refuses (a required pointer that is NULL, channels other than 1 or 3, stride < width * channels,
 * dst_stride < pano_w * channels, an unknown mode, levels outside 1..6 and pano_w or pano_h no multiple of 2^levels in
 * MULTIBAND, a gain outside 1..4095, a pyramid output of the stages call when the mode is not MULTIBAND, a wrong
 * struct_size), a fallback_index outside 0..D - 1, index_stride < pano_w, a NULL index16 on a handle that has not run
 * tscm_sweep_depth.  Bytes of dst between pano_w * channels and dst_stride keep the caller's values. */
typedef struct tscm_sweep_compose_params {
    int struct_size;        /* sizeof(tscm_sweep_compose_params)                                */
    int mode;               /* TSCM_PANO_*                                                      */
    int levels;             /* MULTIBAND: 1..6, otherwise ignored                               */
    int wrap_x;             /* 1: the pyramids wrap over the column ends                        */
    int fallback_index;     /* 0..D - 1: the hypothesis of an invalid pixel                     */
} tscm_sweep_compose_params;
void tscm_sweep_compose_default_params(tscm_sweep_compose_params *p);   /* MULTIBAND, 4, 1, 0 */

int tscm_sweep_compose(tscm_sweep *s, const unsigned char *const *images /* [n] of [height][stride] */, int stride, int channels,
                       const short *index16 /* [pano_h][index_stride], or NULL */, int index_stride,
                       const tscm_sweep_compose_params *params, const unsigned short *gain_q8 /* [n], NULL = 256 */,
                       unsigned char *dst /* [pano_h][dst_stride] */, int dst_stride,
                       unsigned char *coverage /* [pano_h][pano_w], may be NULL */, double *seconds_kernel);

/* The stages of the same kernels, for parity tests. */
int tscm_sweep_compose_stages(tscm_sweep *s, const unsigned char *const *images, int stride, int channels,
                              const short *index16, int index_stride, const tscm_sweep_compose_params *params,
                              const unsigned short *gain_q8, unsigned char *hypothesis, unsigned char *sampled,
                              unsigned char *alpha, unsigned char *label, unsigned char *mask_pyramid, short *lap_pyramid,
                              short *blend_pyramid);

/* Per-camera visibility at the swept depth.  tscm_sweep_compose samples every camera whose record has alpha > 0 at the
 * hypothesis of a pixel, whether or not that camera sees the point: a camera off the rig centre that looks at a background
 * point through a nearer object contributes the object's texture.  The handle's records hold the integer camera position
 * (ix, iy) and the alpha a of every (camera, hypothesis, panorama pixel), and the index map lies on the same grid, so
 * visibility is a depth buffer per camera over cells of its image, in ranks of the hypothesis.  Integers throughout, restated
 * in tests/sweep_visibility_ref.py.  rec(k, z, p): the record of camera k, hypothesis z, panorama pixel p; s = cell_shift.
 *   hypothesis   p is tested iff index16(p) >= 0; then z(p) = min(D - 1, (index16(p) + 8) >> 4), the composer's rule, and the
 *                rank q(p) = near_is_high ? z(p) : D - 1 - z(p): a larger rank is nearer.  An untested pixel neither
 *                occludes nor is occluded.
 *   cell         camera k's grid has cw = ((width - 1) >> s) + 1 by ch = ((height - 1) >> s) + 1 cells; the cell of a
 *                record is (clamp(ix, 0, width - 1) >> s, clamp(iy, 0, height - 1) >> s).
 *   depth buffer zbuf[k][cy][cx] = the maximum of q(p) + 1 over the tested p with rec(k, z(p), p).a > 0 whose cell is
 *                (cx, cy), 0 for an empty cell: a maximum, so no order enters.
 *   test         for a tested p and a camera with a_k = rec(k, z(p), p).a > 0: m = the maximum of zbuf[k] over the cells
 *                (cx + dx, cy + dy) inside the grid with |dx|, |dy| <= dilate; visible_k(p) = (m <= q(p) + 1 + tolerance).
 *                a_k == 0 gives visible_k = 0.
 *   state, use   state 0: p is not tested, use_k = 1 for every k; 1: tested and no camera has a_k > 0, use_k = 0; 2: every
 *                camera with a_k > 0 is visible, use_k = (a_k > 0); 3: some of them are occluded and some visible,
 *                use_k = visible_k; 4: all of them are occluded, use_k = (a_k > 0) -- the guard: a pixel never loses its
 *                last source.
 *   composer     tscm_sweep_compose_visible is tscm_sweep_compose with a_k(i, j) replaced by use_k(i, j) ? a_k(i, j) : 0
 *                before label, coverage, SEAM, FEATHER and the MULTIBAND masks (the alpha stage output is the replaced one);
 *                pixels without depth use the record at fallback_index as before, with use_k = 1.
 * So tolerance = 255 gives the states 0, 1, 2 only and the bytes of tscm_sweep_compose, as does a constant valid map, and
 * with dilate = 0 the nearest tested pixel of a cell is visible in that camera.
 * Outputs, any of them NULL: use [n][pano_h][pano_w] uint8 0 / 1, state [pano_h][pano_w] uint8; stages: hypothesis
 * [pano_h][pano_w] uint8 (0 where not tested), depth_buffer [n][ch][cw] uint16, cell [n][pano_h][pano_w] int32 =
 * cy * cw + cx (-1 where a == 0 or p is not tested), visible [n][pano_h][pano_w] uint8.  index16 == NULL: the map of the
 * handle's last tscm_sweep_depth, as for the composer.  The buffers of the pass are allocated by its first call on a handle.
 * Refused with TSCM_E_INVALID, the text naming the argument, a NULL handle before any device is touched: what
 * tscm_sweep_compose refuses (the composing calls), a NULL vparams or a wrong struct_size, cell_shift outside 0..8, tolerance
 * outside 0..255, dilate outside 0..2, near_is_high other than 0 or 1, index_stride < pano_w, a NULL index16 on a handle that
 * has not run tscm_sweep_depth. */
typedef struct tscm_sweep_visibility_params {
    int struct_size;   /* sizeof(tscm_sweep_visibility_params)                                     */
    int cell_shift;    /* 0..8: a depth-buffer cell is 2^cell_shift x 2^cell_shift source pixels   */
    int tolerance;     /* 0..255 hypotheses: an occluder must be nearer by more than this          */
    int dilate;        /* 0..2: the test reads the (2 dilate + 1)^2 cells around the pixel's cell  */
    int near_is_high;  /* 1: index D - 1 is the nearest; 0: index 0 is                             */
} tscm_sweep_visibility_params;
void tscm_sweep_visibility_default_params(tscm_sweep_visibility_params *p);   /* 2, 2, 0, 1 */

int tscm_sweep_visibility(tscm_sweep *s, const short *index16 /* [pano_h][index_stride], or NULL */, int index_stride,
                          const tscm_sweep_visibility_params *vparams, unsigned char *use, unsigned char *state,
                          double *seconds_kernel);

int tscm_sweep_visibility_stages(tscm_sweep *s, const short *index16, int index_stride,
                                 const tscm_sweep_visibility_params *vparams, unsigned char *hypothesis,
                                 unsigned short *depth_buffer, int *cell, unsigned char *visible, unsigned char *use,
                                 unsigned char *state);

int tscm_sweep_compose_visible(tscm_sweep *s, const unsigned char *const *images, int stride, int channels,
                               const short *index16, int index_stride, const tscm_sweep_compose_params *params,
                               const tscm_sweep_visibility_params *vparams, const unsigned short *gain_q8,
                               unsigned char *dst, int dst_stride, unsigned char *coverage, double *seconds_kernel);

/* The stages of tscm_sweep_compose_stages under visibility, and use and state. */
int tscm_sweep_compose_visible_stages(tscm_sweep *s, const unsigned char *const *images, int stride, int channels,
                                      const short *index16, int index_stride, const tscm_sweep_compose_params *params,
                                      const tscm_sweep_visibility_params *vparams, const unsigned short *gain_q8,
                                      unsigned char *hypothesis, unsigned char *sampled, unsigned char *alpha,
                                      unsigned char *label, unsigned char *mask_pyramid, short *lap_pyramid,
                                      short *blend_pyramid, unsigned char *use, unsigned char *state);

void tscm_sweep_destroy(tscm_sweep *s);

#ifdef __cplusplus
}
#endif
#endif /* TSCM_H */
