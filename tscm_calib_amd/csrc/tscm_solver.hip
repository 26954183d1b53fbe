// tscm_solver.hip -- host side of the MI355X-native TSCM LM solver and the C ABI (include/tscm/tscm.h).
//
// Replaces, behind the reference's own call boundary:
//   * ceres::Problem construction (TS.cpp:249-269, multi_calib.cpp:160-207)  -> tscm_solver_create
//   * ceres::Solve, DENSE_SCHUR + LM (TS.cpp:271-278, multi_calib.cpp:209-216) -> tscm_solver_solve
// The host only enqueues kernels and polls a device-resident control block: accept/reject,
// the trust-region radius and the termination tests all run on the GPU (k_control), so one LM
// iteration costs no host<->device round trip.
//
// In this file: the solver object and its settings, the LM driver (run_lm) with the launches of tscm_kernels.h, the one-shot
// and operator-level entry points, the debug read-backs.  Elsewhere: the exchange back-ends and the tscm_comm_* entry points
// in tscm_comm.hip, asked only through tscm_comm.h; the batched mono route in tscm_mono_batch.hip, which uses the services
// this file declares in tscm_host.h.
#include "tscm/tscm.h"
#include "tscm_comm.h"
#include "tscm_host.h"
#include "tscm_kernels.h"
#include "tscm_launch_seq.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

using namespace tscm;

// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
int tscm_set_error(int code, const std::string &msg) { return fail(code, msg); }   // tscm_host.h: HIP_TRY, select_device

double wall() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the Gram kernels k_eval_gram4 / k_eval_gram_f32 share one signature; every family is instantiated per k-step count of a pass
// (tscm_exec_plan.h: g4_plan).  A family is a tier (G4: fp64, F32: the fp32-Jacobian tier on the same pass plan) plus 0 plain,
// 1 with a robust loss (ROBUST: DESIGN 14), 2 with corner weights, with or without a loss (WEIGHTED: DESIGN 27)
typedef void (*EvalKernel)(DevProblem, DevState, int, LossArg);
enum EvalFamily { G4, G4Robust, G4Weighted, F32, F32Robust, F32Weighted, kEvalFamilies };
template <int KS, bool MULTI>
static EvalKernel eval_instance(EvalFamily f)
{
    // several passes: ceil(n / passes) >= 29 corners per pass, i.e. at least 8 k-steps -- nothing below is instantiated
    if constexpr (MULTI && KS < 8) return nullptr;
    else switch (f) {
        case G4: return k_eval_gram4<KS, MULTI, false>;
        case G4Robust: return k_eval_gram4<KS, MULTI, true>;
        case G4Weighted: return k_eval_gram4_weighted<KS, MULTI>;
        case F32: return k_eval_gram_f32<KS, MULTI, false>;
        case F32Robust: return k_eval_gram_f32<KS, MULTI, true>;
        case F32Weighted: return k_eval_gram_f32_weighted<KS, MULTI>;
        default: return nullptr;
    }
}
template <int... I>
static EvalKernel eval_kernel(EvalFamily f, int ks, bool multi, std::integer_sequence<int, I...>)
{
    typedef EvalKernel (*Pick)(EvalFamily);
    static const Pick single[] = { eval_instance<I + 1, false>... }, passes[] = { eval_instance<I + 1, true>... };
    return (multi ? passes : single)[ks - 1](f);
}
static EvalKernel eval_kernel(EvalFamily f, int ks, bool multi) { return eval_kernel(f, ks, multi, std::make_integer_sequence<int, kG4MaxKS>{}); }

struct tscm_solver {
    int device = 0;
    hipStream_t stream = nullptr;
    DevProblem P{};
    DevState S{};
    DeviceMem mem;                      // every device buffer of the solver
    tscm_comm *comm = nullptr;
    Layout L;                           // host copy of the layout (tscm_layout.h: plan_layout)
    int C = 0, B = 0, V = 0, N = 0, n_points = 0, n_pad = 0;     // B, V, N: this rank's boards / views / corners (L.B, L.V, L.N)
    int rank = 0, world = 1;
    int n_views = 0;                    // views of the caller's problem (this rank's with corners: V)
    hipStream_t own_stream = nullptr;   // `stream` is replaced by the group's while a local group solve runs
    bool mono = false;
    // caller-owned parameter arrays (host)
    double *h_cam_rt = nullptr, *h_intr = nullptr, *h_board_rt = nullptr;
    // resident initial parameters for the benchmark
    double *d_init_cam = nullptr, *d_init_intr = nullptr, *d_init_board = nullptr;
    double *d_start_cam = nullptr, *d_start_intr = nullptr, *d_start_board = nullptr;    // start point of the solve in progress (a re-run begins there)
    bool have_init = false;
    Ctrl *h_ctrl = nullptr;             // pinned
    Ctrl *d_h_ctrl = nullptr;           // ... and its address on the device (k_finish_solve writes the control block there itself)
    size_t lds_eval = 0, lds_eval32 = 0, lds_solve = 0, lds_bs = 0;
    ExecDevice dev;                     // residency figures of the launches whose workgroups wait for each other (tscm_exec_plan.h)
    ExecPlan xp;                        // the launch plan of the solve in progress (plan_exec)
    CtrlHead head;                      // ... and the control block it starts from (ctrl_head_from_options)
    int withhold = 0, withhold_next = 0; // this solve / the next one: fault injection, 0 or kWithhold* (tscm_solver_debug_withhold_handoff)
    int n_reruns = 0;                   // solves that were run again on separate launches after a late hand-off
    bool no_rerun = false, no_rerun_next = false;      // fault injection: the late hand-off of this / the next solve stays an error
    tscm_comm *comm_reg = nullptr;      // what tscm_solver_set_comm registered; `comm` is what the current solve uses
    // k_solve_nd: [0] the nested-dissection plan of the camera-pair graph, [1] one dense block (TSCM_EXEC_DENSE_REDUCED_ORDER; also what
    // [0] is when the graph is complete); operand map and tables of each on the device
    NdPlan plan[2];
    const int4 *d_nd_map[2] = { nullptr, nullptr };
    const int *d_nd_tab[2] = { nullptr, nullptr }, *d_nd_bs[2] = { nullptr, nullptr };
    size_t lds_nd[2] = { 0, 0 }, lds_dense4 = 0;
    size_t lds_eval4 = 0;               // dynamic LDS of k_eval_gram4
    EvalKernel eval[kEvalFamilies] = {}; // ... and every family's instantiation for this problem's board (eval_kernel)
    LossArg loss{};                     // tscm_solver_set_loss: kind 0 (TSCM_LOSS_NONE) runs the plain family of the tier
    // corner weights (tscm_solver_set_corner_weights): with weights every evaluation runs the WEIGHTED family,
    // whatever the loss; P.obs_w is d_obs_w then and NULL otherwise
    bool weighted = false;
    double *d_obs_w = nullptr;          // [N] weights in the device's corner order (allocated by the first call with weights)
    std::vector<double> h_obs_u, h_obs_v;   // the observations as created, in that order: a masked corner's device copy is 0, 0 while it is masked
    std::vector<int> p_view_count;      // view_count of the caller's WHOLE problem (the weights' corner order)
    double w_sum = 0.0;                 // sum of the weights and number of corners with a weight > 0, of the WHOLE job
    long n_kept = 0;
    // camera priors (tscm_solver_set_camera_priors): the caller's arrays as given (empty: not given), and what the
    // reductions' PRIOR kernel takes of them under the current free columns -- d_prior holds mean [16 C] | weight [16 C]
    // (effective_priors; allocated by the first call with an effective prior).  n_priors == 0 is the solve without priors
    std::vector<double> pr_cam_mean, pr_cam_w, pr_intr_mean, pr_intr_w;
    std::vector<unsigned char> col_free;    // [16 C] ColumnPlan::col_active as uploaded (apply_columns)
    double *d_prior = nullptr;
    int n_priors = 0;
    PriorArg prior_arg() const { return PriorArg{ d_prior, d_prior + 16 * (size_t)C }; }
    // held intrinsics (tscm_solver_set_fixed_intrinsics): the mask word of every camera (the whole-problem facts the
    // free columns are derived from are L.cam_const, L.cam_active, L.pair_present: plan_columns)
    std::vector<unsigned short> fixed;
    int n_cu = 1;
    int schur_rot = 0;                  // k_schur_gram's rot: the wave its workgroups start their deal of board groups at, 0 (tests: 2, tscm_solver_debug_schur_rot)
    bool ext_planned = false;           // the column plan has the e-row and solution tiles of k_solve_reduced (not its fallback)
    bool force_backsub = false;         // ... but k_solve_reduced back-substitutes all the same (tests, A/B runs: tscm_solver_debug_reduced_backsub)
    double *d_view_sq = nullptr;        // [2 V] k_reproj_error's output for the RMSE of a robust solve (allocated by the first one)
    // dominant-kernel timing
    int timing = 0;                     // 0 = off, n = bracket every n-th launch of the dominant kernel (and every n-th exchange) with HIP events
    unsigned ev_count[3] = { 0, 0, 0 }; // occurrences so far, by kind: 0 dominant kernel, 1 exchange of T, 2 exchange of H_stage
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    std::vector<int> ev_kind;
    size_t ev_used = 0;
    int t_launches[3] = { 0, 0, 0 };
    double t_ms[3] = { 0.0, 0.0, 0.0 };
};

struct SolverDelete { void operator()(tscm_solver *s) const { tscm_solver_destroy(s); } };
using SolverPtr = std::unique_ptr<tscm_solver, SolverDelete>;

// a solver of `p` on `device` that lives as long as `sp`: the create / use / destroy entry points
static int create_scoped(const tscm_problem *p, int device, SolverPtr &sp)
{
    tscm_solver *s = nullptr;
    if (int rc = tscm_solver_create(p, device, &s)) return rc;
    sp.reset(s);
    return 0;
}

// ------------------------------------------------------------------------------------------------
extern "C" int tscm_abi_version(void) { return TSCM_ABI_VERSION; }
extern "C" const char *tscm_last_error(void) { return g_err.c_str(); }

extern "C" int tscm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int tscm_device_synchronize(int device)
{
    if (int rc = select_device(device, "tscm_device_synchronize")) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

extern "C" void tscm_default_options(tscm_options *o, int mono)
{
    o->struct_size = sizeof(tscm_options);
    o->max_num_iterations = mono ? 100 : 50;   // TS.cpp:274 ; Ceres default (multi_calib.cpp:212 is commented out)
    o->function_tolerance = 1e-6;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
    o->initial_trust_region_radius = 1e4;
    o->max_trust_region_radius = 1e16;
    o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->max_num_consecutive_invalid_steps = 5;
    o->jacobi_scaling = 1;
    o->check_every = 4;
    o->jacobian_fp32 = 0;
    o->exec_flags = 0;
}

static int validate(const tscm_problem *p)
{
    std::string err;
    if (int rc = tscm::validate(p, err)) return fail(rc, err);
    return 0;
}

// the refusals of tscm_spec.h with their text in tscm_last_error()
static int make_spec(int kind, double scale, const unsigned short *fixed, int n_cameras, SolveSpec &spec)
{
    std::string err;
    if (int rc = tscm::make_spec(kind, scale, fixed, n_cameras, spec, err)) return fail(rc, err);
    return 0;
}
int check_corner_weights(const int *view_count, int n_views, const double *w, double *sum, long *kept)
{
    std::string err;
    if (int rc = tscm::check_corner_weights(view_count, n_views, w, err, sum, kept)) return fail(rc, err);
    return 0;
}
static int check_camera_priors(const tscm_camera_priors *pr, int n_cameras)
{
    std::string err;
    if (int rc = tscm::check_camera_priors(pr, n_cameras, err)) return fail(rc, err);
    return 0;
}
static bool same_loss(const LossArg &x, const LossArg &y) { return x.kind == y.kind && (x.kind == TSCM_LOSS_NONE || x.a == y.a); }

extern "C" int tscm_solver_set_loss(tscm_solver *s, int kind, double scale)
{
    SolveSpec spec;
    if (int rc = make_spec(kind, scale, nullptr, 0, spec)) return rc;
    if (!s) return fail(TSCM_E_INVALID, "solver is NULL");
    s->loss = spec.loss;
    return 0;
}

extern "C" int tscm_solver_set_corner_weights(tscm_solver *s, const double *weights)
{
    if (!s) return fail(TSCM_E_INVALID, "solver is NULL");
    const size_t N = (size_t)s->N;
    if (!weights) {
        if (!s->weighted) return 0;
        // the observations as created: the solve without weights, bit for bit
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipStreamSynchronize(s->stream));
        if (N) {
            HIP_TRY(hipMemcpy(const_cast<double *>(s->P.obs_u), s->h_obs_u.data(), sizeof(double) * N, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(const_cast<double *>(s->P.obs_v), s->h_obs_v.data(), sizeof(double) * N, hipMemcpyHostToDevice));
        }
        s->weighted = false; s->P.obs_w = nullptr; s->w_sum = 0.0; s->n_kept = 0;
        return 0;
    }
    double sum = 0.0;
    long kept = 0;
    if (int rc = check_corner_weights(s->p_view_count.data(), (int)s->p_view_count.size(), weights, &sum, &kept)) return rc;
    // this rank's part, in the device's corner order; a masked corner's observation is 0, 0 there (scatter_weights)
    std::vector<CornerRun> runs((size_t)s->V);
    for (int i = 0; i < s->V; ++i) runs[i] = CornerRun{ s->L.dev2orig[i], s->L.view_obs[i], s->L.view_count[i] };
    std::vector<double> w(N), u(s->h_obs_u), q(s->h_obs_v);
    scatter_weights(weights, s->p_view_count.data(), (int)s->p_view_count.size(), runs, w.data(), u.data(), q.data());
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (!s->d_obs_w) HIP_TRY(s->mem.alloc(&s->d_obs_w, std::max<size_t>(N, 1)));
    if (N) {
        HIP_TRY(hipMemcpy(s->d_obs_w, w.data(), sizeof(double) * N, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(const_cast<double *>(s->P.obs_u), u.data(), sizeof(double) * N, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(const_cast<double *>(s->P.obs_v), q.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    }
    s->weighted = true; s->P.obs_w = s->d_obs_w; s->w_sum = sum; s->n_kept = kept;
    return 0;
}

// the prior tables of the solver's stored priors under its current free columns (s->col_free), on the device: behind
// tscm_solver_set_camera_priors and every apply_columns
static int refresh_priors(tscm_solver *s)
{
    const tscm_camera_priors pr{ sizeof(tscm_camera_priors), s->pr_cam_mean.empty() ? nullptr : s->pr_cam_mean.data(), s->pr_cam_w.empty() ? nullptr : s->pr_cam_w.data(),
                                 s->pr_intr_mean.empty() ? nullptr : s->pr_intr_mean.data(), s->pr_intr_w.empty() ? nullptr : s->pr_intr_w.data() };
    std::vector<double> mean, weight;
    const int n = effective_priors(&pr, s->C, s->col_free.data(), mean, weight);
    if (n) {
        const size_t n16 = 16 * (size_t)s->C;
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipStreamSynchronize(s->stream));
        if (!s->d_prior) HIP_TRY(s->mem.alloc(&s->d_prior, 2 * n16));
        HIP_TRY(hipMemcpy(s->d_prior, mean.data(), sizeof(double) * n16, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->d_prior + n16, weight.data(), sizeof(double) * n16, hipMemcpyHostToDevice));
    }
    s->n_priors = n;
    return 0;
}

extern "C" int tscm_solver_set_camera_priors(tscm_solver *s, const tscm_camera_priors *priors)
{
    if (!s) return fail(TSCM_E_INVALID, "solver is NULL");
    if (int rc = check_camera_priors(priors, s->C)) return rc;
    if (priors && s->world > 1) return fail(TSCM_E_UNSUPPORTED, "camera priors on a sharded solver (world > 1) are not supported");
    auto keep = [&](std::vector<double> &dst, const double *src, int per) { if (priors && src) dst.assign(src, src + per * (size_t)s->C); else dst.clear(); };
    keep(s->pr_cam_mean, priors ? priors->cam_rt_mean : nullptr, 6); keep(s->pr_cam_w, priors ? priors->cam_rt_weight : nullptr, 6);
    keep(s->pr_intr_mean, priors ? priors->intr_mean : nullptr, 9); keep(s->pr_intr_w, priors ? priors->intr_weight : nullptr, 9);
    return refresh_priors(s);
}

extern "C" void tscm_solver_destroy(tscm_solver *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    s->stream = s->own_stream;
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (auto &e : s->ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (s->h_ctrl) (void)hipHostFree(s->h_ctrl);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;                           // (s->mem frees the device buffers)
}

static std::atomic<bool> g_force_backsub{ false };      // tscm_solver_debug_reduced_backsub(NULL, on)

// Uploads a column plan (tscm_columns.h: plan_columns): col_active, the control step's classes col_ctl, act_map /
// n_act, cam_pre / cam_free (kernel arguments of k_solve_reduced), k_solve_reduced's operand map and both k_solve_nd plans,
// with the LDS bounds and residency that follow from them.  Run by create and by tscm_solver_set_fixed_intrinsics.
static int apply_columns(tscm_solver *s, const ColumnPlan &c)
{
    DevProblem &P = s->P;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(const_cast<unsigned char *>(P.col_active), c.col_active.data(), c.col_active.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(const_cast<unsigned char *>(P.col_ctl), c.col_ctl.data(), c.col_ctl.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(const_cast<int *>(P.act_map), c.act_map.data(), sizeof(int) * c.act_map.size(), hipMemcpyHostToDevice));
    P.n_act = c.n_act;
    std::copy(std::begin(c.cam_pre), std::end(c.cam_pre), P.cam_pre);
    std::copy(std::begin(c.cam_free), std::end(c.cam_free), P.cam_free);
    static_assert(sizeof(Int4) == sizeof(int4), "the operand map is uploaded as it is");
    if (!c.solve_map.empty()) {
        HIP_TRY(hipMemcpy(const_cast<int4 *>(P.solve_map), c.solve_map.data(), sizeof(Int4) * c.solve_map.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(const_cast<int4 *>(P.solve_ext), c.solve_ext.data(), sizeof(Int4) * c.solve_ext.size(), hipMemcpyHostToDevice));
        s->ext_planned = !c.ext_fallback;
        P.solve_ext_on = s->ext_planned && !s->force_backsub;
    }
    if (c.has_nd) {
        for (int v = 0; v < 2; ++v) {
            const NdPlan &pl = c.nd[v];
            s->mem.release(s->d_nd_map[v]); s->mem.release(s->d_nd_tab[v]); s->mem.release(s->d_nd_bs[v]);
            s->d_nd_map[v] = nullptr; s->d_nd_tab[v] = nullptr; s->d_nd_bs[v] = nullptr;
            HIP_TRY(s->mem.upload(&s->d_nd_map[v], reinterpret_cast<const int4 *>(pl.map.data()), pl.map.size() / 4));
            HIP_TRY(s->mem.upload(&s->d_nd_tab[v], pl.tab));
            HIP_TRY(s->mem.upload(&s->d_nd_bs[v], pl.bs_tab));
            s->lds_nd[v] = sizeof(double) * pl.lds_doubles;
            s->plan[v] = pl;
        }
        {
            // ONE dynamic-LDS bound for the four instantiations (either plan may be launched, with or without riders), set
            // before the occupancy queries that depend on it
            const size_t lds_max = std::max(std::max(s->lds_nd[0], s->lds_nd[1]), s->lds_bs);
            if (lds_max > 64 * 1024)
                for (const void *k : { reinterpret_cast<const void *>(k_solve_nd<1, true>), reinterpret_cast<const void *>(k_solve_nd<2, true>),
                                       reinterpret_cast<const void *>(k_solve_nd<1, false>), reinterpret_cast<const void *>(k_solve_nd<2, false>) })
                    HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        }
        for (int v = 0; v < 2; ++v) {
            // workgroups of the fused launch that are resident at once: the back-substitution workgroups that ride in it WAIT
            // for the solver workgroup, so only as many are put there as fit the chip next to it (and the T producers)
            const size_t lds = std::max(s->lds_nd[v], s->lds_bs);
            int per_cu = 0;
            if (s->plan[v].tpt == 1) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(k_solve_nd<1, true>), kNdThreads, lds));
            else HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(k_solve_nd<2, true>), kNdThreads, lds));
            s->dev.nd_resident[v] = per_cu * s->n_cu;
            s->dev.nd_tpt[v] = s->plan[v].tpt;
        }
        s->lds_solve = std::max(s->lds_nd[0], s->lds_nd[1]);
    }
    if (s->C > kMaxCamLds) s->lds_solve = solve_big_lds_bytes((c.n_act + 15) & ~15, s->n_pad);
    // (camera priors: the weight of a column that is not free is taken as 0)
    s->col_free = c.col_active;
    return refresh_priors(s);
}

extern "C" int tscm_solver_set_fixed_intrinsics(tscm_solver *s, const unsigned short *fixed)
{
    if (!s) return fail(TSCM_E_INVALID, "solver is NULL");
    SolveSpec spec;
    if (int rc = make_spec(TSCM_LOSS_NONE, 0.0, fixed, s->C, spec)) return rc;
    std::vector<unsigned short> f(s->C, 0);
    if (fixed) f.assign(fixed, fixed + s->C);
    if (f == s->fixed) return 0;
    // planned first: a refusal leaves the solver as it was
    ColumnPlan c;
    std::string err;
    if (int rc = plan_columns(s->L, s->C, f.data(), c, err)) return fail(rc, err);
    if (int rc = apply_columns(s, c)) return rc;
    s->fixed = f;
    return 0;
}

// Every rank is handed the WHOLE problem description (the view tables are small) and keeps the observations, records
// and pose blocks of the boards it owns; plan_layout (tscm_layout.h) derives this rank's layout, and what the ranks must
// agree on identically on every rank.  Refusals in order: the arguments and validate(), the device, the board size the
// Gram kernel's LDS takes, the layout's (plan_layout), then the LDS board-point tile of k_eval_gram.
extern "C" int tscm_solver_create_sharded(const tscm_problem *p, int device, int rank, int world, tscm_solver **out)
{
    if (!out) return fail(TSCM_E_INVALID, "out is NULL");
    *out = nullptr;
    if (int rc = validate(p)) return rc;
    if (world < 1 || rank < 0 || rank >= world) return fail(TSCM_E_INVALID, "rank / world out of range");
    if (int rc = select_device(device, "the TSCM solver")) return rc;

    SolverPtr sp(new tscm_solver);
    tscm_solver *s = sp.get();
    s->device = device;
    s->rank = rank; s->world = world;
    s->C = p->n_cameras; s->n_points = p->n_points; s->mono = p->mono != 0; s->n_views = p->n_views;
    s->n_pad = 16 * s->C;
    s->h_cam_rt = p->cam_rt; s->h_intr = p->intr; s->h_board_rt = p->board_rt;
    HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    s->own_stream = s->stream;
    const int C = s->C;

    // ---- device setup: LDS and occupancy of the Gram and Schur kernels ---------------------------
    // Jacobian tile geometry of k_eval_gram: HV rows (multiple of 8 covering min(64, n) corners -- the MFMA loops consume the
    // k-steps of 4 rows in PAIRS, so the tile holds an even number of them; u-rows and v-rows take turns), pitch HV + 2
    // (= 2 * odd: the 16 columns x 2 rows of a 32-lane ds_read_b64 group then hit 32 distinct bank pairs)
    const int half_rows = 8 * ((std::min(64, p->n_points) + 7) / 8);
    const int rp = half_rows + 2;      // = 2 * odd (half_rows is a multiple of 8)
    const size_t lds_eval_bytes = sizeof(double) * (std::max<size_t>((size_t)16 * rp, 512) + kCst + 2 * (size_t)p->n_points);
    // k_eval_gram runs 4 single-chunk waves per workgroup (they share only the final camera-tile sum)
    if (4 * lds_eval_bytes > 64 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_eval_gram<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * lds_eval_bytes)));
    // the default Gram kernel: k_eval_gram4 instantiated for this board's pass plan (KS k-steps per pass, ceil(n / 56) passes per view)
    const G4Plan g4 = g4_plan(p->n_points);
    for (int f = 0; f < kEvalFamilies; ++f) s->eval[f] = eval_kernel((EvalFamily)f, g4.ks, g4.passes > 1);
    const size_t lds_eval4 = 4 * sizeof(double) * (size_t)eval_gram4_lds_doubles(p->n_points, g4.ks);
    if (lds_eval4 > 160 * 1024) return fail(TSCM_E_UNSUPPORTED, "board with too many corners for the Gram kernel's LDS (more than about 2,000)");
    if (lds_eval4 > 64 * 1024)
        for (int f = G4; f < F32; ++f) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(s->eval[f]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_eval4));
    // the Gram kernels' view chunks are sized for one round of resident waves: LayoutDevice
    int wgs_per_cu = 0;         // resident workgroups per CU (register- and LDS-limited)
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs_per_cu, reinterpret_cast<const void *>(s->eval[G4]), 256, lds_eval4));
    const int waves_per_cu = 4 * std::max(1, std::min(4, wgs_per_cu));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const void *schur[4][2] = { {}, { reinterpret_cast<const void *>(k_schur_gram<1>), reinterpret_cast<const void *>(k_schur_gram<1, true>) },
                                { reinterpret_cast<const void *>(k_schur_gram<2>), reinterpret_cast<const void *>(k_schur_gram<2, true>) },
                                { reinterpret_cast<const void *>(k_schur_gram<3>), reinterpret_cast<const void *>(k_schur_gram<3, true>) } };
    for (int nv = 1; nv <= 3; ++nv) {
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&s->dev.schur_resident[nv], schur[nv][0], 256, 0));
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&s->dev.schur_resident_ride[nv], schur[nv][1], 256, 0));
        s->dev.schur_resident[nv] *= prop.multiProcessorCount; s->dev.schur_resident_ride[nv] *= prop.multiProcessorCount;
    }
    s->n_cu = std::max(1, prop.multiProcessorCount);

    // ---- layout ----------------------------------------------------------------------------------
    const Layout &L = s->L;
    {
        LayoutDevice dev;
        dev.n_cu = prop.multiProcessorCount; dev.waves_per_cu = waves_per_cu;
        std::string err;
        if (int rc = plan_layout(p, rank, world, dev, s->L, err)) return fail(rc, err);
    }
    s->B = L.B; s->V = L.V; s->N = L.N;
    const int B = L.B, V = L.V, N = L.N;
    s->lds_bs = sizeof(double) * (size_t)(L.bs_threads == 256 ? BsGeom<256>::kLds : BsGeom<128>::kLds);
    for (const void *k : { reinterpret_cast<const void *>(k_backsub_prep<128>), reinterpret_cast<const void *>(k_backsub_prep<256>) })
        HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->lds_bs));

    // ---- upload: the observations gathered into device order, the layout's tables -------------------
    std::vector<double> u((size_t)N), w((size_t)N);
    for (int i = 0; i < V; ++i) {
        const int v = L.dev2orig[i];
        std::memcpy(u.data() + L.view_obs[i], p->obs_u + p->view_offset[v], sizeof(double) * L.view_count[i]);
        std::memcpy(w.data() + L.view_obs[i], p->obs_v + p->view_offset[v], sizeof(double) * L.view_count[i]);
    }
    const std::vector<double> bxy(p->board_xy, p->board_xy + 2 * (size_t)p->n_points);
    auto int4s = [](const std::vector<Int4> &h) {
        std::vector<int4> d(h.size());
        for (size_t i = 0; i < h.size(); ++i) d[i] = make_int4(h[i].x, h[i].y, h[i].z, h[i].w);
        return d;
    };
    std::vector<int4> chunk_desc = int4s(L.chunk_desc);
    const std::vector<int4> bc_desc = int4s(L.bc_desc);
    for (int4 &d : chunk_desc) if (L.cam_const[d.x]) d.x |= kChunkConstPose;     // (k_eval_gram4's constant-pose path)
    const std::vector<short> bid_lut(L.bid_of.begin(), L.bid_of.end());
    DevProblem &P = s->P;
    DevState &S = s->S;
    P.C = C; P.B = B; P.n_points = p->n_points; P.V = V; P.N = N; P.n_pad = s->n_pad;
    P.rank = rank; P.world = world;
    P.rp = rp; P.half = half_rows; P.lds_wave = (int)(lds_eval_bytes / sizeof(double)); P.g4_per = g4.per;
    P.n_chunks = (int)L.chunk_vb.size(); P.n_pchunks = (int)L.pc_begin.size(); P.n_bids = L.n_bids;
    P.n_bchunks = (int)L.bc_desc.size(); P.n_tiles = L.n_tiles; P.n_slow = (int)L.slow_boards.size();
    std::copy(std::begin(L.cam_wg), std::end(L.cam_wg), P.cam_wg);
    std::copy(std::begin(L.bid_part_small), std::end(L.bid_part_small), P.bid_part_small);
    P.pair_mask = L.pair_mask;
    hipError_t he = hipSuccess;     // the first failure of a run of uploads / allocations (the rest are skipped)
    auto up = [&](auto **dst, const auto &h) { if (he == hipSuccess) he = s->mem.upload(dst, h); };
    auto al = [&](auto **dst, size_t n) { if (he == hipSuccess) he = s->mem.alloc(dst, n); };
    up(&P.board_xy, bxy);
    up(&P.view_cam, L.view_cam); up(&P.view_board, L.view_board); up(&P.view_obs, L.view_obs); up(&P.view_count, L.view_count);
    up(&P.obs_u, u); up(&P.obs_v, w);
    s->h_obs_u.swap(u); s->h_obs_v.swap(w);
    s->p_view_count.assign(p->view_count, p->view_count + p->n_views);
    up(&P.chunk_vb, L.chunk_vb); up(&P.chunk_ve, L.chunk_ve); up(&P.chunk_cam, L.chunk_cam); up(&P.chunk_desc, chunk_desc);
    up(&P.cam_chunk_ptr, L.cam_chunk_ptr);
    up(&P.bv_ptr, L.bv_ptr); up(&P.view_slot, L.view_slot); up(&P.slot_cam, L.slot_cam); up(&P.slot_view, L.slot_view); up(&P.slot_board, L.slot_board);
    up(&P.slow_boards, L.slow_boards);
    up(&P.pair_i, L.pair_i); up(&P.pair_j, L.pair_j); up(&P.pc_begin, L.pc_begin); up(&P.pc_end, L.pc_end); up(&P.pc_tile, L.pc_tile);
    up(&P.bid_part_ptr, L.bid_part_ptr); up(&P.pair_board, L.pair_board); up(&P.bc_tile, L.bc_tile); up(&P.bc_desc, bc_desc);
    up(&P.bid_lut, bid_lut); up(&P.board_const, L.board_const);
    // written by apply_columns
    s->fixed.assign(C, 0);
    al(&P.col_active, s->n_pad); al(&P.col_ctl, (size_t)16 * kMaxCam); al(&P.act_map, s->n_pad);

    for (int k = 0; k < 2; ++k) {
        al(&S.cam_rt[k], 6 * (size_t)C); al(&S.intr[k], 9 * (size_t)C); al(&S.board_rt[k], 6 * (size_t)B);
        al(&S.rec[k], (size_t)kRec * V); al(&S.H[k], 256 * (size_t)C);
    }
    al(&s->d_init_cam, 6 * (size_t)C); al(&s->d_init_intr, 9 * (size_t)C); al(&s->d_init_board, 6 * (size_t)B);
    al(&s->d_start_cam, 6 * (size_t)C); al(&s->d_start_intr, 9 * (size_t)C); al(&s->d_start_board, 6 * (size_t)B);
    al(&S.board_pc, (size_t)kBoardConst * B); al(&S.cam_pc, (size_t)kCamConst * C); al(&S.vconst, (size_t)kVStride * V);
    al(&S.cconst[0], (size_t)kCStride * C); al(&S.cconst[1], (size_t)kCStride * C);
    al(&S.campart, 512 * (size_t)(P.n_chunks / 4)); al(&S.campart2, 512 * (size_t)C);
    al(&S.H_stage, 256 * (size_t)C + kScal + world);
    al(&S.s_b, 6 * (size_t)B); al(&S.s_c, s->n_pad); al(&S.fac, (size_t)kFac * B);
    al(&S.pairpart, 256 * (size_t)P.n_tiles); al(&S.T, 256 * (size_t)L.n_bids);
    al(&S.t_count, 1); al(&S.y_flag, 1); al(&S.fac_fail, 1);
    al(&S.yhat, s->n_pad);
    S.n_st_blocks = (B + 255) / 256;
    al(&S.bs_part, 2 * (size_t)((B + 15) / 16));     // (upper bound: groups of 16 boards)
    al(&S.st_part, kStStride * (size_t)S.n_st_blocks);
    S.n_bs_blocks = L.n_bs_blocks;
    al(&S.ctrl, 1); al(&S.ctrl_snap, 1); al(&S.ctl_pub, 1);
    al(&S.stats_count, 64); al(&S.stats_flag, 64);      // (256 bytes each: lines of their own)
    HIP_TRY(he);
    for (int *flag : { S.t_count, S.y_flag, S.fac_fail }) HIP_TRY(hipMemset(flag, 0, sizeof(int)));
    // (the W columns of w_c of a constant camera's views are never written by k_eval_gram4's constant-pose path: zero, not
    // uninitialised, in front of the back-substitution's zero step)
    for (int k = 0; k < 2; ++k) if (V) HIP_TRY(hipMemset(S.rec[k], 0, sizeof(double) * (size_t)kRec * V));
    HIP_TRY(hipMemset(S.stats_count, 0, 256)); HIP_TRY(hipMemset(S.stats_flag, 0, 256));
    HIP_TRY(hipMemset(S.ctl_pub, 0, sizeof(CtlPub)));
    HIP_TRY(hipMemset(S.T, 0, sizeof(double) * 256 * (size_t)L.n_bids));
    HIP_TRY(hipMemset(S.H_stage, 0, sizeof(double) * (256 * (size_t)C + kScal + world)));
    HIP_TRY(hipMemset(S.campart2, 0, sizeof(double) * 512 * (size_t)C));
    HIP_TRY(hipMemset(S.ctrl, 0, sizeof(Ctrl)));
    HIP_TRY(hipMemset(S.ctrl_snap, 0, sizeof(CtrlHead)));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s->h_ctrl), sizeof(Ctrl)));
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&s->d_h_ctrl), s->h_ctrl, 0));

    // ---- the evaluation and solve variants -------------------------------------------------------
    s->lds_eval = 4 * lds_eval_bytes;
    s->lds_eval32 = sizeof(double) * (size_t)eval_f32_lds_doubles(p->n_points, g4.ks);
    s->lds_eval4 = lds_eval4;
    if (s->lds_eval32 > 64 * 1024)
        for (int f = F32; f < kEvalFamilies; ++f) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(s->eval[f]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->lds_eval32));
    // reduced solve: up to 8 cameras k_solve_nd on the plan of the camera-pair graph (tscm_nd_plan.h), larger rigs in global memory.
    // The columns of the creation plan (no held intrinsics) are every camera-side column that can be free: held intrinsics
    // only ever take columns away, so the sizes below hold for every mask
    ColumnPlan cols;
    {
        std::string err;
        if (int rc = plan_columns(L, C, nullptr, cols, err)) return fail(rc, err);
    }
    if (C <= kDense4Cams) {
        // where every thread of k_solve_reduced finds its operands (written by apply_columns)
        int4 *map = nullptr;
        HIP_TRY(s->mem.alloc(&map, (size_t)(kSolveMapSlots / 4) * kSolveMapThreads));
        P.solve_map = map;
        int4 *ext = nullptr;
        HIP_TRY(s->mem.alloc(&ext, (size_t)kSolveMapThreads));
        P.solve_ext = ext;
        s->force_backsub = g_force_backsub.load();
        const size_t NN = 64, TT = 4, NPD = 64;
        s->lds_dense4 = sizeof(double) * (NN * (NN + 2) + 2 * (NN / TT) * (TT * TT + 2) + 2 * NN + 3 * NPD);
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(k_solve_reduced<4, 16, 64, true>), 256, std::max(s->lds_dense4, s->lds_bs)));
        s->dev.dense4_resident = per_cu * prop.multiProcessorCount;
    }
    if (C > kMaxCamLds) {
        // rigs of 9..32 cameras: the compact system (+ rhs row) lives in global memory
        const int NN = (cols.n_act + 15) & ~15;
        const size_t lds_max = solve_big_lds_bytes(NN, s->n_pad);
        HIP_TRY(s->mem.alloc(&S.Abig, (size_t)256 * (NN / 16 + 1) * (NN / 16 + 2) / 2));      // packed lower triangle of 16x16 blocks, incl. the rhs block row
        if (lds_max > 64 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_solve_reduced_big), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    }
    if (int rc = apply_columns(s, cols)) return rc;
    if (s->lds_eval > 160 * 1024) return fail(TSCM_E_UNSUPPORTED, "board has too many corners for the LDS board-point tile");
    HIP_TRY(hipDeviceSynchronize());
    *out = sp.release();
    return 0;
}

extern "C" int tscm_solver_create(const tscm_problem *p, int device, tscm_solver **out)
{
    return tscm_solver_create_sharded(p, device, 0, 1, out);
}

// Fault injection for the tests of the device-side hand-off: in the NEXT solve of this solver one producer of the fused
// hand-off never reports in, and the solve must end with TSCM_E_HIP within the hand-off's time bound.  Not an option of
// a solve (tscm_options carries nothing that can make a production solve fail).
extern "C" int tscm_solver_debug_withhold_handoff(tscm_solver *s, int on)
{
    if (!s) return fail(TSCM_E_INVALID, "solver is NULL");
    s->withhold_next = on == 3 ? kWithholdStats : on ? kWithholdProducer : 0;      // (3: a reduction block riding in the Schur-complement launch, not a producer of the tiles)
    s->no_rerun_next = on == 2;          // 2: ... and the solve is NOT run again on separate launches (the error path itself)
    return 0;
}

// For the tests of k_schur_gram's deal: which wave of a workgroup contracts which boards must not change a bit.
extern "C" int tscm_solver_debug_schur_rot(tscm_solver *s, int rot)
{
    if (!s) return fail(TSCM_E_INVALID, "solver is NULL");
    if (rot != 0 && rot != 2) return fail(TSCM_E_INVALID, "rot must be 0 or 2");
    s->schur_rot = rot;
    return 0;
}

// For tests and A/B runs of k_solve_reduced (rigs of up to four cameras): on = 1 keeps the back-substitution behind the
// factorisation where the plan lets the solution fall out of the factor; 0 is the default.  s NULL: the default of the solvers
// created from now on, in this process (the one-shot entry points create their own).
extern "C" int tscm_solver_debug_reduced_backsub(tscm_solver *s, int on)
{
    if (on != 0 && on != 1) return fail(TSCM_E_INVALID, "on must be 0 or 1");
    if (!s) { g_force_backsub.store(on != 0); return 0; }
    s->force_backsub = on != 0;
    s->P.solve_ext_on = s->ext_planned && !s->force_backsub;
    return 0;
}

extern "C" int tscm_solver_reruns(const tscm_solver *s)
{
    if (!s) return fail(TSCM_E_INVALID, "solver is NULL");
    return s->n_reruns;
}

extern "C" int tscm_solver_set_comm(tscm_solver *s, tscm_comm *comm)
{
    if (!s) return fail(TSCM_E_INVALID, "solver is NULL");
    if (comm && comm_device(comm) != s->device) return fail(TSCM_E_INVALID, "communicator and solver live on different devices");
    if (comm && (comm_world(comm) != s->world || comm_rank(comm) != s->rank))
        return fail(TSCM_E_INVALID, "communicator rank / world differ from the solver's shard (tscm_solver_create_sharded)");
    // a single-rank RCCL communicator is a no-op unless a solve asks for its code path (separate k_control,
    // stream-ordered all-reduces) with TSCM_EXEC_KEEP_SINGLE_RANK_COMM: uses_comm()
    s->comm_reg = comm;
    s->comm = uses_comm(comm_kind(comm), 0) ? comm : nullptr;
    return 0;
}

extern "C" int tscm_solver_upload_params(tscm_solver *s, const double *cam_rt, const double *intr, const double *board_rt)
{
    if (!s || !intr || (!board_rt && s->L.B_total)) return fail(TSCM_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(s->device));
    std::vector<double> zero(6 * (size_t)s->C, 0.0);
    const double *c = (s->mono || !cam_rt) ? zero.data() : cam_rt;
    HIP_TRY(hipMemcpyAsync(s->d_init_cam, c, sizeof(double) * 6 * s->C, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->d_init_intr, intr, sizeof(double) * 9 * s->C, hipMemcpyHostToDevice, s->stream));
    // board_rt is the caller's full-length array; this rank keeps the poses of the boards it owns, in device board order
    std::vector<double> brd(6 * (size_t)s->B);
    for (int i = 0; i < s->B; ++i) std::memcpy(brd.data() + 6 * (size_t)i, board_rt + 6 * ((size_t)s->L.b0 + s->L.board_perm[i]), 6 * sizeof(double));
    if (s->B) HIP_TRY(hipMemcpyAsync(s->d_init_board, brd.data(), sizeof(double) * 6 * s->B, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->have_init = true;
    return 0;
}

// one launch of the dominant kernel, optionally bracketed by HIP events on the solver's stream
// HIP-event brackets on the solver's stream: every `timing`-th occurrence of a kind (0 = the dominant kernel, 1 = the
// exchange of T, 2 = the exchange of H_stage) is timed; an event pair holds the stream for a few microseconds, so the
// sampling keeps the measurement out of the result
static int timed_pair(tscm_solver *s, int kind, hipEvent_t *e0, hipEvent_t *e1)
{
    *e0 = *e1 = nullptr;
    if (!(s->timing > 0 && (s->ev_count[kind]++ % (unsigned)s->timing) == 0)) return 0;
    if (s->ev_used == s->ev.size()) {
        hipEvent_t a, b;
        HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
        s->ev.emplace_back(a, b);
        s->ev_kind.push_back(0);
    }
    s->ev_kind[s->ev_used] = kind;
    *e0 = s->ev[s->ev_used].first;
    *e1 = s->ev[s->ev_used].second;
    ++s->ev_used;
    return 0;
}

static int timed_begin(tscm_solver *s, int kind, hipStream_t stream, hipEvent_t *e1)
{
    hipEvent_t e0 = nullptr;
    if (int rc = timed_pair(s, kind, &e0, e1)) return rc;
    if (e0) HIP_TRY(hipEventRecord(e0, stream));
    return 0;
}

// one launch of the dominant kernel.  A timed launch carries its event pair IN the dispatch (hipExtLaunchKernelGGL:
// the events take the start and end time stamps of this kernel's packet on the solver's stream) -- two hipEventRecord
// around it are two more packets with a drain each, 8.5 us per timed launch at config 4 and 3 % of the driver's
// 20-step run
template <typename K, typename... A>
static void launch_eval_kernel(K kernel, dim3 grid, size_t lds, tscm_solver *s, hipEvent_t e0, hipEvent_t e1, int cand, A... extra)
{
    if (e0) hipExtLaunchKernelGGL(kernel, grid, dim3(256), (std::uint32_t)lds, s->stream, e0, e1, 0, s->P, s->S, cand, extra...);
    else hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s->stream, s->P, s->S, cand, extra...);
}

static int launch_eval(tscm_solver *s, int cand)
{
    const DevProblem &P = s->P;
    if (P.n_chunks == 0) return 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (int rc = timed_pair(s, 0, &e0, &e1)) return rc;
    const dim3 grid(P.n_chunks / 4);
    // (a loss: the ROBUST instantiation; the 16x16 kernel has none -- refused before anything is launched)
    // (corner weights: the WEIGHTED instantiation, with or without a loss; refused with the 16x16 kernel like a loss)
    const int variant = s->weighted ? 2 : s->xp.robust ? 1 : 0;       // (EvalFamily: tier + variant)
    if (s->xp.gram == Gram::F32) launch_eval_kernel(s->eval[F32 + variant], grid, s->lds_eval32, s, e0, e1, cand, s->loss);
    else if (s->xp.gram == Gram::G4)
        launch_eval_kernel(s->eval[G4 + variant], grid, s->lds_eval4, s, e0, e1, cand | (s->xp.skip_const_pose ? kEvalSkipConst : 0), s->loss);
    else if (s->xp.gram == Gram::G16Pitch58) launch_eval_kernel(k_eval_gram<58>, grid, s->lds_eval, s, e0, e1, cand);
    else launch_eval_kernel(k_eval_gram<0>, grid, s->lds_eval, s, e0, e1, cand);
    return 0;
}

static int collect_timing(tscm_solver *s)
{
    for (size_t i = 0; i < s->ev_used; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev[i].first, s->ev[i].second));
        const int k = s->ev_kind[i];
        s->t_ms[k] += ms; s->t_launches[k] += 1;
    }
    s->ev_used = 0;
    return 0;
}

extern "C" int tscm_solver_kernel_time(tscm_solver *s, int enable, int *launches, double *total_ms)
{
    if (!s) return fail(TSCM_E_INVALID, "solver is NULL");
    if (launches) *launches = s->t_launches[0];
    if (total_ms) *total_ms = s->t_ms[0];
    s->t_launches[0] = 0; s->t_ms[0] = 0.0;
    s->timing = enable < 0 ? 0 : enable;
    s->ev_count[0] = s->ev_count[1] = s->ev_count[2] = 0;
    return 0;
}

extern "C" int tscm_solver_exchange_time(tscm_solver *s, int *n_T, double *ms_T, int *n_H, double *ms_H)
{
    if (!s) return fail(TSCM_E_INVALID, "solver is NULL");
    if (n_T) *n_T = s->t_launches[1];
    if (ms_T) *ms_T = s->t_ms[1];
    if (n_H) *n_H = s->t_launches[2];
    if (ms_H) *ms_H = s->t_ms[2];
    s->t_launches[1] = s->t_launches[2] = 0; s->t_ms[1] = s->t_ms[2] = 0.0;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The LM loop over a set of shards.  `members` is ONE solver (single GPU, or one RCCL rank: the peers run the same
// loop in their own processes) or all ranks of a LOCAL group (one process, one device, one stream, lock step).
// Per iteration the ranks exchange exactly two buffers, each with a sum all-reduce:
//   T        n_bids * 256 doubles   the Schur complement tiles, after k_T_reduce
//   H_stage  256 C + kScal + world  camera tiles, cost, model-cost / norm partials, failure flag, per-rank max slots
// (tscm_comm.hip: comm_allreduce, comm_group_sum)
// ------------------------------------------------------------------------------------------------
// the members of a run and, per member, the launch sequence of the phase in progress (tscm_launch_seq.h)
struct LmSeq {
    SeqState st;
    LaunchList todo;
    int at = 0;                         // next entry of todo to enqueue
};
struct LmRun {
    std::vector<tscm_solver *> m;
    std::vector<LmSeq> seq;             // [m.size()], sized once per solve
};

static int exchange(LmRun &run, bool t_buffer)
{
    tscm_solver *s0 = run.m[0];
    if (!s0->comm) return 0;
    const size_t n = t_buffer ? 256 * (size_t)s0->P.n_bids : 256 * (size_t)s0->P.C + kScal + s0->P.world;
    if (n == 0) return 0;
    hipEvent_t e1 = nullptr;
    if (comm_is_local_group(s0->comm)) {
        const hipStream_t gs = comm_group_stream(s0->comm);     // (the members' buffers: comm_group_bind in run_lm_inner)
        if (int rc = timed_begin(s0, t_buffer ? 1 : 2, gs, &e1)) return rc;
        comm_group_sum(s0->comm, t_buffer, n);
        if (e1) HIP_TRY(hipEventRecord(e1, gs));
        return 0;
    }
    double *buf = t_buffer ? s0->S.T : s0->S.H_stage;
    if (int rc = timed_begin(s0, t_buffer ? 1 : 2, s0->stream, &e1)) return rc;
    if (int rc = comm_allreduce(s0->comm, buf, n, s0->stream)) return rc;
    if (e1) HIP_TRY(hipEventRecord(e1, s0->stream));
    return 0;
}

// The only place the LM loop's kernels are launched: one entry of a launch sequence -> its kernel, workgroup size, LDS and
// arguments (the exchange markers are walk()'s)
static int enqueue(tscm_solver *s, const Launch &l)
{
    const DevProblem &P = s->P;
    const DevState &S = s->S;
    hipStream_t st = s->stream;
    const dim3 grid(l.grid);
    auto schur = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, P, S, l.chunk0, l.ctl, l.first_round, l.ce, l.target, l.n_chunks, s->schur_rot); };
    auto nd = [&](auto kernel) {
        const int v = l.nd;
        hipLaunchKernelGGL(kernel, grid, dim3(kNdThreads), std::max(s->lds_nd[v], l.n_bs ? s->lds_bs : (size_t)0), st, P, S, s->d_nd_map[v], s->d_nd_tab[v], s->d_nd_bs[v],
                           s->plan[v].dims(), l.epoch, l.withhold, l.n_prod, l.n_bs, l.f32);
    };
    const size_t lds_dense4 = std::max(s->lds_dense4, l.n_bs ? s->lds_bs : (size_t)0);
    // k_solve_reduced takes the step out of the factor only in the fp64 tier (the fp32-Jacobian tier's systems are the worst
    // conditioned ones: tscm_solve_dense4.h); the tier is the solve's, whatever rides in this launch
    auto dense4 = [&](auto kernel) {
        DevProblem Pd = P;
        if (s->xp.f32()) Pd.solve_ext_on = 0;
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds_dense4, st, Pd, S, l.epoch, l.withhold, l.n_prod, l.n_bs, l.f32);
    };
    switch (l.k) {
    case Kern::BeginViewPrep: {
        const bool init = l.start == Start::Init, bak = l.start == Start::Backup;
        hipLaunchKernelGGL(k_begin_view_prep, grid, dim3(kVPrepThreads), 0, st, P, S, s->head,
                           init ? s->d_init_cam : bak ? s->d_start_cam : nullptr, init ? s->d_init_intr : bak ? s->d_start_intr : nullptr,
                           init ? s->d_init_board : bak ? s->d_start_board : nullptr,
                           bak ? nullptr : s->d_start_cam, bak ? nullptr : s->d_start_intr, bak ? nullptr : s->d_start_board, l.f32);
        break;
    }
    case Kern::Eval: return launch_eval(s, l.cand);
    case Kern::ReduceControl: hipLaunchKernelGGL(k_reduce_control, grid, dim3(256), 0, st, P, S, l.cand, l.init, l.have_backsub); break;
    // (camera priors, ExecPlan::priors: the PRIOR kernel adds them behind the camera-tile sums; such a plan has no k_reduce_control)
    case Kern::ReduceStats:
        if (s->xp.priors) hipLaunchKernelGGL(k_reduce_stats_prior, grid, dim3(256), 0, st, P, S, l.cand, l.init, s->prior_arg());
        else hipLaunchKernelGGL(k_reduce_stats, grid, dim3(256), 0, st, P, S, l.cand, l.init);
        break;
    case Kern::FinalizeEval: hipLaunchKernelGGL(k_finalize_eval, grid, dim3(256), 0, st, P, S, l.have_backsub); break;
    case Kern::Control: hipLaunchKernelGGL(k_control, grid, dim3(256), 0, st, P, S, l.init); break;
    case Kern::SchurFactor: hipLaunchKernelGGL(k_schur_factor, grid, dim3(256), 0, st, P, S); break;
    case Kern::Schur1: schur(k_schur_gram<1>); break;
    case Kern::Schur2: schur(k_schur_gram<2>); break;
    case Kern::Schur3: schur(k_schur_gram<3>); break;
    case Kern::SchurRide1: schur(k_schur_gram<1, true>); break;
    case Kern::SchurRide2: schur(k_schur_gram<2, true>); break;
    case Kern::SchurRide3: schur(k_schur_gram<3, true>); break;
    case Kern::PairGram: hipLaunchKernelGGL(k_pair_gram, grid, dim3(256), 0, st, P, S); break;
    case Kern::TReduce: hipLaunchKernelGGL(k_T_reduce, grid, dim3(kTEntries * kTSlices), 0, st, P, S); break;
    case Kern::SolveDense4: dense4(k_solve_reduced<4, 16, 64>); break;
    case Kern::SolveDense4Ride: dense4(k_solve_reduced<4, 16, 64, true>); break;
    case Kern::SolveNd1: nd(k_solve_nd<1, false>); break;
    case Kern::SolveNd2: nd(k_solve_nd<2, false>); break;
    case Kern::SolveNd1Ride: nd(k_solve_nd<1, true>); break;
    case Kern::SolveNd2Ride: nd(k_solve_nd<2, true>); break;
    // 9 to 32 cameras -- or no free camera-side column (every intrinsic held where the pose is, e.g. a mono problem refining board
    // poses only): nothing to factor.  k_solve_reduced_big on the empty system runs no panel and writes the zero camera step, the
    // unchanged candidate camera parameters and the linear-solve flag; the back-substitution moves the boards
    case Kern::SolveBig: hipLaunchKernelGGL(k_solve_reduced_big, grid, dim3(kBigNT), s->lds_solve, st, P, S); break;
    case Kern::SolveEmpty: hipLaunchKernelGGL(k_solve_reduced_big, grid, dim3(kBigNT), solve_big_lds_bytes(0, s->n_pad), st, P, S); break;
    case Kern::Backsub128: hipLaunchKernelGGL(k_backsub_prep<128>, grid, dim3(128), s->lds_bs, st, P, S, l.f32); break;
    case Kern::Backsub256: hipLaunchKernelGGL(k_backsub_prep<256>, grid, dim3(256), s->lds_bs, st, P, S, l.f32); break;
    case Kern::FinishSolve: hipLaunchKernelGGL(k_finish_solve, grid, dim3(256), 0, st, P, S, l.init, l.have_backsub, s->C, s->B, s->d_h_ctrl); break;
    case Kern::EndSolve: hipLaunchKernelGGL(k_end_solve, grid, dim3(256), 0, st, S, s->C, s->B); break;
    case Kern::CopyCtrl: {
        static_assert(sizeof(Ctrl) == sizeof(CtrlHead) + sizeof(IterLog) * kMaxLog, "the log follows the head without padding");
        const size_t bytes = sizeof(CtrlHead) + sizeof(IterLog) * (size_t)std::min(s->head.opt.max_num_iterations + 1, kMaxLog);
        HIP_TRY(hipMemcpyAsync(s->h_ctrl, S.ctrl, bytes, hipMemcpyDeviceToHost, st));
        break;
    }
    case Kern::ExchangeT: case Kern::ExchangeH: break;
    }
    return 0;
}

// Enqueues the members' sequences of one phase (run.seq[r].todo) in rounds, member after member: a round of a member ends in
// front of an evaluation (all members' Schur sides, solves, evaluations follow each other in turn on a LOCAL group's shared
// stream) or at an exchange marker, where exchange() runs once for the run -- every member's sequence has the same markers
static int walk(LmRun &run)
{
    for (LmSeq &q : run.seq) q.at = 0;
    for (bool left = true; left;) {
        left = false;
        const Launch *mark = nullptr;
        for (size_t r = 0; r < run.m.size(); ++r) {
            LmSeq &q = run.seq[r];
            for (const int from = q.at; q.at < q.todo.n; ++q.at) {
                const Launch &l = q.todo.at[q.at];
                if (is_exchange(l.k) || (l.k == Kern::Eval && q.at > from)) break;
                if (int rc = enqueue(run.m[r], l)) return rc;
            }
            if (q.at < q.todo.n && is_exchange(q.todo.at[q.at].k)) mark = &q.todo.at[q.at++];
            left = left || q.at < q.todo.n;
        }
        if (mark) if (int rc = exchange(run, mark->k == Kern::ExchangeT)) return rc;
    }
    return 0;
}

static const char *reason_message(int r)
{
    switch (r) {
    case kMaxIter: return "Maximum number of iterations reached.";
    case kGradTol: return "Gradient tolerance reached.";
    case kMinRadius: return "Minimum trust region radius reached.";
    case kParamTol: return "Parameter tolerance reached.";
    case kFuncTol: return "Function tolerance reached.";
    case kInvalidSteps: return "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps.";
    default: return "";
    }
}

// restores the per-solve state of the members on every exit path (also the error returns inside the loop)
struct LmRunGuard {
    LmRun &run;
    ~LmRunGuard()
    {
        for (tscm_solver *s : run.m) {
            s->xp = ExecPlan{};              // (per solve: planned again from the options of the next one)
            s->ev_used = 0;
            s->stream = s->own_stream;
        }
    }
};

// a terminated control block and its iteration log as a summary (times excepted); rmse: that of a plain loss, sqrt(2 cost / N)
void fill_summary(const CtrlHead &h, const IterLog *log, long N, tscm_summary *sum)
{
    sum->termination_type = h.term_type;
    sum->num_iterations = std::min(h.n_log, TSCM_MAX_ITERATIONS + 1);
    sum->num_successful_steps = h.num_successful;
    sum->num_unsuccessful_steps = h.num_unsuccessful;
    sum->initial_cost = h.initial_cost;
    sum->final_cost = h.x_cost;
    sum->n_residual_blocks = (int)N;
    sum->lm_iterations = h.lm_iterations;
    for (int i = 0; i < sum->num_iterations; ++i) {
        const IterLog &l = log[i];
        tscm_iteration &o = sum->iterations[i];
        o.iteration = l.iteration; o.step_is_valid = l.step_is_valid; o.step_is_successful = l.step_is_successful;
        o.cost = l.cost; o.cost_change = l.cost_change; o.gradient_max_norm = l.gradient_max_norm; o.gradient_norm = l.gradient_norm;
        o.step_norm = l.step_norm; o.relative_decrease = l.relative_decrease; o.trust_region_radius = l.radius;
    }
    std::snprintf(sum->message, sizeof(sum->message), "%s", reason_message(h.term_reason));
    sum->rmse = N ? std::sqrt(2.0 * h.x_cost / (double)N) : 0.0;
}

static int run_lm_inner(LmRun &run, const tscm_options *opt_in, tscm_summary *sums, int reset, bool rerun, bool *late_handoff);

// the caller's struct may be SHORTER than this library's (built against an older header of ABI >= 6): read what it has, the
// rest keeps its default.  The shortest struct the library knows ends behind exec_flags (ABI 6); a size of 0, a smaller or a
// larger one is refused -- a struct of ABI <= 5 has max_num_iterations where struct_size is and never passes
int read_options(const tscm_options *opt_in, int mono, tscm_options &opt)
{
    tscm_default_options(&opt, mono);
    if (opt_in) {
        constexpr size_t kMinOptions = offsetof(tscm_options, exec_flags) + sizeof(int);
        if (opt_in->struct_size < kMinOptions || opt_in->struct_size > sizeof(tscm_options))
            return fail(TSCM_E_INVALID, "tscm_options.struct_size is not a size this library knows (initialise the struct with tscm_default_options; ABI 6)");
        std::memcpy(&opt, opt_in, opt_in->struct_size);
        opt.struct_size = sizeof(tscm_options);
    }
    return 0;
}
static int check_options(const tscm_options &opt, int loss_kind, bool weighted = false)
{
    std::string err;
    if (const int rc = check_exec_options(opt, loss_kind, err)) return fail(rc, err);
    if (weighted && (opt.exec_flags & TSCM_EXEC_GRAM_16X16)) return fail(TSCM_E_UNSUPPORTED, "TSCM_EXEC_GRAM_16X16 has no corner-weight kernel");
    return 0;
}

// A rank of a multi-rank communicator that leaves the loop on an error other than TSCM_E_INVALID (a refusal: nothing was
// exchanged) makes its communicator unusable (tscm_comm.hip: comm_fail, and what that means for the peers).
static int run_lm(LmRun &run, const tscm_options *opt_in, tscm_summary *sums, int reset)
{
    bool late = false;
    int rc = run_lm_inner(run, opt_in, sums, reset, /*rerun=*/false, &late);
    if (late && !run.m[0]->comm && run.m.size() == 1 && !run.m[0]->no_rerun) {
        // A device-side hand-off of a fused launch came late (0.5 s: a debugger, a co-tenant, a context switch -- or a real
        // fault).  The solve was stopped on the device and nothing of it has left it; it is run again from its start point
        // (k_begin_view_prep kept a copy) on the launches that hand nothing over inside a launch -- same mathematics, same
        // bits as the fused ones (tests/test_gpu_parity.py).  Only if that fails too is it an error.  With a communicator the
        // ranks would have to agree on the re-run: there the late hand-off stays TSCM_E_HIP.
        tscm_options o2;
        (void)read_options(opt_in, run.m[0]->mono, o2);      // (read without a refusal by the first attempt)
        o2.exec_flags |= TSCM_EXEC_SEPARATE_T_REDUCE | TSCM_EXEC_SEPARATE_BACKSUB | TSCM_EXEC_SEPARATE_CONTROL;
        const std::string first = g_err;
        bool late2 = false;
        rc = run_lm_inner(run, &o2, sums, reset, /*rerun=*/true, &late2);
        if (rc == 0) g_err = "note: " + first + "; the solve was run again on separate launches and completed";
        ++run.m[0]->n_reruns;
    }
    if (rc != 0 && rc != TSCM_E_INVALID) comm_fail(run.m[0]->comm);
    return rc;
}

// sum of the squared pixel errors of this solver's corners at the accepted point (buffer 0): k_reproj_error, summed over the
// views in device order -- what tscm_reprojection_error does on an unsharded solver of the same problem
static int accepted_sq(tscm_solver *s, double &sq)
{
    sq = 0.0;
    if (!s->V) return 0;
    if (!s->d_view_sq) HIP_TRY(s->mem.alloc(&s->d_view_sq, 2 * (size_t)s->V));
    // (corner weights: sum omega s, the weighted variant of the launch)
    if (s->weighted) hipLaunchKernelGGL(k_reproj_error<true>, dim3(s->V), dim3(64), 0, s->stream, s->P, s->S.cam_rt[0], s->S.intr[0], s->S.board_rt[0], s->d_view_sq, s->d_view_sq + s->V);
    else hipLaunchKernelGGL(k_reproj_error<false>, dim3(s->V), dim3(64), 0, s->stream, s->P, s->S.cam_rt[0], s->S.intr[0], s->S.board_rt[0], s->d_view_sq, s->d_view_sq + s->V);
    std::vector<double> q(s->V);
    HIP_TRY(hipMemcpyAsync(q.data(), s->d_view_sq + s->V, sizeof(double) * s->V, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipGetLastError());
    for (int v = 0; v < s->V; ++v) sq += q[v];
    return 0;
}
// summary.rmse of a robust solve: one k_reproj_error launch per solver; the shards' sums are added (a local group) or
// all-reduced (a communicator across processes), over N of the whole job
static int robust_rmse(LmRun &run, tscm_summary *sums)
{
    double sq = 0.0;
    for (tscm_solver *s : run.m) {
        double q = 0.0;
        if (int rc = accepted_sq(s, q)) return rc;
        sq += q;
    }
    tscm_solver *s0 = run.m[0];
    if (run.m.size() == 1 && s0->comm && s0->world > 1) {
        DeviceMem mem;
        double *d = nullptr;
        HIP_TRY(mem.alloc(&d, 1));
        HIP_TRY(hipMemcpyAsync(d, &sq, sizeof(double), hipMemcpyHostToDevice, s0->stream));
        if (int rc = comm_allreduce(s0->comm, d, 1, s0->stream)) return rc;
        HIP_TRY(hipMemcpyAsync(&sq, d, sizeof(double), hipMemcpyDeviceToHost, s0->stream));
        HIP_TRY(hipStreamSynchronize(s0->stream));
        if (int rc = comm_check(s0->comm)) return rc;
    }
    for (size_t r = 0; r < run.m.size(); ++r) {
        // (corner weights: sum omega s over sum omega)
        const double den = run.m[r]->weighted ? run.m[r]->w_sum : (double)run.m[r]->L.N_total;
        sums[r].rmse = den > 0.0 ? std::sqrt(sq / den) : 0.0;
    }
    return 0;
}

static int run_lm_inner(LmRun &run, const tscm_options *opt_in, tscm_summary *sums, int reset, bool rerun, bool *late_handoff)
{
    tscm_solver *s0 = run.m[0];
    for (tscm_solver *s : run.m) if (!s->have_init) return fail(TSCM_E_INVALID, "tscm_solver_upload_params has not been called");
    tscm_options opt;
    if (int rc = read_options(opt_in, s0->mono, opt)) return rc;
    if (int rc = check_options(opt, s0->loss.kind, s0->weighted)) return rc;
    for (tscm_solver *s : run.m) if (!same_loss(s->loss, s0->loss)) return fail(TSCM_E_INVALID, "the solvers of a group carry different losses (tscm_solver_set_loss)");
    for (tscm_solver *s : run.m) if (s->weighted != s0->weighted) return fail(TSCM_E_INVALID, "the solvers of a group must all have corner weights or all have none (tscm_solver_set_corner_weights)");
    for (tscm_solver *s : run.m) if (s->fixed != s0->fixed) return fail(TSCM_E_INVALID, "the solvers of a group hold different intrinsics (tscm_solver_set_fixed_intrinsics)");
    HIP_TRY(hipSetDevice(s0->device));
    LmRunGuard guard{ run };
    for (tscm_solver *s : run.m) {
        s->xp = plan_exec(s->L, s->C, s->P.n_act, comm_kind(s->comm_reg), opt.exec_flags, opt.jacobian_fp32, s->loss.kind, s->P.rp, s->dev, false, s->n_priors > 0);
        s->comm = s->xp.comm ? s->comm_reg : nullptr;
        s->head = ctrl_head_from_options(opt);
        s->head.inert_cols = has_inert_columns(s->fixed.data(), s->L.cam_active.data(), s->C);
        s->withhold = s->withhold_next; s->withhold_next = 0;
        if (!rerun) { s->no_rerun = s->no_rerun_next; s->no_rerun_next = false; }
    }
    if (int rc = comm_usable(s0->comm)) return rc;
    if (comm_is_local_group(s0->comm)) {
        // a local group runs on ONE stream: lock step by stream order, no events
        const int world = comm_world(s0->comm);
        if ((int)run.m.size() != world) return fail(TSCM_E_INVALID, "a local group solves with all of its members (tscm_solver_solve_group)");
        std::vector<double *> ptrs(2 * (size_t)world);      // [0, world) the members' T, [world, 2 world) their H_stage
        for (int r = 0; r < world; ++r) { ptrs[r] = run.m[r]->S.T; ptrs[world + r] = run.m[r]->S.H_stage; }
        if (int rc = comm_group_bind(s0->comm, ptrs)) return rc;
        for (tscm_solver *s : run.m) { HIP_TRY(hipStreamSynchronize(s->own_stream)); s->stream = comm_group_stream(s0->comm); }
    }
    for (size_t r = 0; r < run.m.size(); ++r) std::memset(&sums[r], 0, sizeof(tscm_summary));

    // plan -> walk, per phase: the start (k_begin_view_prep and the initial evaluation), the iterations with a poll of the
    // control block every check_every, the end (one synchronisation for the whole solve)
    const double t0 = wall();
    run.seq.assign(run.m.size(), LmSeq{});
    // (start point: the registered arrays with `reset`, buffer 0 otherwise, the backup of the first attempt on a re-run)
    const Start start = rerun ? Start::Backup : reset ? Start::Init : Start::Current;
    for (size_t r = 0; r < run.m.size(); ++r) { tscm_solver *s = run.m[r]; seq_begin(s->L, s->C, s->xp, start, run.seq[r].st, run.seq[r].todo); }
    int rc;
    if ((rc = walk(run))) return rc;
    const int check_every = std::max(1, opt.check_every);
    bool done = false;
    for (int it = 1; it <= opt.max_num_iterations && !done; ++it) {
        for (size_t r = 0; r < run.m.size(); ++r) { tscm_solver *s = run.m[r]; seq_iteration(s->L, s->C, s->xp, s->dev, s->withhold, run.seq[r].st, run.seq[r].todo); }
        if ((rc = walk(run))) return rc;
        if (it % check_every == 0 && it < opt.max_num_iterations) {
            // every rank takes the same decisions from the same all-reduced bits: polling one member is enough
            HIP_TRY(hipMemcpyAsync(s0->h_ctrl, s0->S.ctrl, 64, hipMemcpyDeviceToHost, s0->stream));
            if ((rc = comm_wait(s0->comm, s0->stream))) return rc;
            done = s0->h_ctrl->done != 0;
        }
    }
    for (size_t r = 0; r < run.m.size(); ++r) seq_finish(run.m[r]->L, run.m[r]->C, run.seq[r].st, run.seq[r].todo);
    if ((rc = walk(run))) return rc;
    if ((rc = comm_wait(s0->comm, s0->stream))) return rc;
    for (tscm_solver *s : run.m) if (s->stream != s0->stream) HIP_TRY(hipStreamSynchronize(s->stream));
    if ((rc = comm_check(s0->comm))) return rc;
    const double t1 = wall();
    HIP_TRY(hipGetLastError());
    for (size_t r = 0; r < run.m.size(); ++r) {
        tscm_solver *s = run.m[r];
        Ctrl *h = s->h_ctrl;
        tscm_summary *sum = &sums[r];
        if ((rc = collect_timing(s))) return rc;
        if (h->fault) { *late_handoff = true; return fail(TSCM_E_HIP, "a device-side hand-off (Schur-complement tiles -> reduced solve) did not arrive within its time bound: the solve was stopped"); }
        if (!h->done) return fail(TSCM_E_HIP, "device LM loop did not terminate");
        fill_summary(*h, h->log, (long)s->L.N_total, sum);                // cost and N of the WHOLE job
        if (s->weighted) {
            // corner weights: the blocks are the corners with a weight > 0, and rmse = sqrt(sum omega s / sum omega) -- without a loss
            // the cost is sum omega s / 2
            sum->n_residual_blocks = (int)s->n_kept;
            sum->rmse = s->w_sum > 0.0 ? std::sqrt(2.0 * h->x_cost / s->w_sum) : 0.0;
        }
        sum->seconds_solve = 1e-8 * (double)(h->t_end - h->t_begin);      // on the device: first to last kernel of the solve
        sum->seconds_total = t1 - t0;                                     // wall time of the call
    }
    // with a loss the cost is sum rho / 2, not the squared pixel error: the RMSE is measured at the accepted point instead; with
    // camera priors the cost holds the prior term as well
    if (s0->loss.kind != TSCM_LOSS_NONE || s0->n_priors > 0) return robust_rmse(run, sums);
    return 0;
}

extern "C" int tscm_solver_solve_resident(tscm_solver *s, const tscm_options *opt_in, tscm_summary *sum, int reset)
{
    if (!s || !sum) return fail(TSCM_E_INVALID, "NULL argument");
    if (comm_is_local_group(s->comm_reg) && s->world > 1) return fail(TSCM_E_INVALID, "member of a local group: use tscm_solver_solve_group");
    if (s->world > 1 && !s->comm_reg) return fail(TSCM_E_INVALID, "sharded solver without a communicator (tscm_solver_set_comm)");
    LmRun run;
    run.m.push_back(s);
    return run_lm(run, opt_in, sum, reset);
}

extern "C" int tscm_solver_solve_group(tscm_solver **solvers, int n, const tscm_options *opt, tscm_summary *summaries, int reset)
{
    if (!solvers || !summaries || n < 1) return fail(TSCM_E_INVALID, "NULL argument");
    LmRun run;
    for (int r = 0; r < n; ++r) {
        tscm_solver *s = solvers[r];
        if (!s || s->world != n || s->rank != r) return fail(TSCM_E_INVALID, "solvers[r] must be shard r of n (tscm_solver_create_sharded)");
        if (n > 1 && !comm_same_group(s->comm_reg, solvers[0]->comm_reg))
            return fail(TSCM_E_INVALID, "the solvers of a group need the communicators of ONE tscm_comm_create_local call");
        run.m.push_back(s);
    }
    return run_lm(run, opt, summaries, reset);
}

// parameter buffer `buf` (0: the accepted point, 1: the candidate) in the caller's layout
static int download_buffer(tscm_solver *s, int buf, double *cam_rt, double *intr, double *board_rt)
{
    HIP_TRY(hipSetDevice(s->device));
    if (cam_rt && !s->mono) HIP_TRY(hipMemcpy(cam_rt, s->S.cam_rt[buf], sizeof(double) * 6 * s->C, hipMemcpyDeviceToHost));
    if (intr) HIP_TRY(hipMemcpy(intr, s->S.intr[buf], sizeof(double) * 9 * s->C, hipMemcpyDeviceToHost));
    // only the owned boards: the other entries of the caller's array are left untouched (see tscm_solver_gather_boards)
    if (board_rt && s->B) {
        std::vector<double> brd(6 * (size_t)s->B);
        HIP_TRY(hipMemcpy(brd.data(), s->S.board_rt[buf], sizeof(double) * 6 * s->B, hipMemcpyDeviceToHost));
        for (int i = 0; i < s->B; ++i) std::memcpy(board_rt + 6 * ((size_t)s->L.b0 + s->L.board_perm[i]), brd.data() + 6 * (size_t)i, 6 * sizeof(double));
    }
    return 0;
}

extern "C" int tscm_solver_download_params(tscm_solver *s, double *cam_rt, double *intr, double *board_rt)
{
    if (!s) return fail(TSCM_E_INVALID, "solver is NULL");
    return download_buffer(s, 0, cam_rt, intr, board_rt);
}

// After a sharded solve every rank holds the poses of its own boards.  This makes the caller's full-length array
// complete on every rank (what MultiCalib::calibrate() leaves behind: all chessboards_[i].rt_ updated): the owned
// slice in a zeroed full-length device buffer, one sum all-reduce (x + 0 is exact), one download.
extern "C" int tscm_solver_gather_boards(tscm_solver *s, double *board_rt)
{
    if (!s || (!board_rt && s->L.B_total)) return fail(TSCM_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(s->device));
    if (!s->comm_reg || s->world == 1 || comm_is_local_group(s->comm_reg)) return tscm_solver_download_params(s, nullptr, nullptr, board_rt);   // local groups share the caller's array
    if (s->L.B_total == 0) return 0;
    const size_t n = 6 * (size_t)s->L.B_total;
    std::vector<double> mine(n, 0.0);
    if (int rc = tscm_solver_download_params(s, nullptr, nullptr, mine.data())) return rc;     // owned boards at their own positions
    DeviceMem mem;
    double *full = nullptr;
    HIP_TRY(mem.upload(&full, mine));
    if (int rc = comm_allreduce(s->comm_reg, full, n, s->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(board_rt, full, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return comm_check(s->comm_reg);
}

extern "C" int tscm_solver_solve(tscm_solver *s, const tscm_options *opt, tscm_summary *sum)
{
    if (!s || !sum) return fail(TSCM_E_INVALID, "NULL argument");
    const double t0 = wall();
    int rc;
    if ((rc = tscm_solver_upload_params(s, s->h_cam_rt, s->h_intr, s->h_board_rt))) return rc;
    if ((rc = tscm_solver_solve_resident(s, opt, sum, 1))) return rc;
    if ((rc = tscm_solver_download_params(s, s->h_cam_rt, s->h_intr, nullptr))) return rc;
    if ((rc = tscm_solver_gather_boards(s, s->h_board_rt))) return rc;
    sum->seconds_total = wall() - t0;
    return 0;
}

// The refusals of a one-shot entry point ahead of its problem, in the one order tscm.h documents ("Refusal order"): the loss,
// NULL arguments (null: one of the entry point's is; null_text: its text for that), the mask, the options struct.  The option
// values follow once the entry point has put its own in (check_options), the problem and the weights in create_configured.
// in: the caller's arguments (spec_args); spec: checked, what configures the solver.
static int preamble(const tscm_problem *p, bool null, const char *null_text, const tscm_options *opt_in, const SolveSpec &in, SolveSpec &spec,
                    tscm_options &opt)
{
    if (int rc = make_spec(in.loss.kind, in.loss.a, nullptr, 0, spec)) return rc;
    if (null) return fail(TSCM_E_INVALID, null_text);
    if (int rc = make_spec(in.loss.kind, in.loss.a, in.fixed, p->n_cameras, spec)) return rc;
    spec.weights = in.weights; spec.priors = in.priors;
    return read_options(opt_in, p->mono, opt);
}

// a solver of `p` on `device` with a checked spec's loss, mask, weights and priors, alive as long as `sp`.  The problem's, the
// weights' and the priors' refusals come before the device is touched
static int create_configured(const tscm_problem *p, int device, const SolveSpec &spec, SolverPtr &sp)
{
    if (int rc = validate(p)) return rc;
    if (spec.weights) if (int rc = check_corner_weights(p->view_count, p->n_views, spec.weights)) return rc;
    if (int rc = check_camera_priors(spec.priors, p->n_cameras)) return rc;
    if (int rc = create_scoped(p, device, sp)) return rc;
    sp->loss = spec.loss;
    if (spec.fixed) if (int rc = tscm_solver_set_fixed_intrinsics(sp.get(), spec.fixed)) return rc;
    if (spec.weights) if (int rc = tscm_solver_set_corner_weights(sp.get(), spec.weights)) return rc;
    if (spec.priors) if (int rc = tscm_solver_set_camera_priors(sp.get(), spec.priors)) return rc;
    return 0;
}

// one solve on the calling thread's device, with a checked spec (tscm_host.h)
int solve_configured(const tscm_problem *p, const tscm_options *opt, const SolveSpec &spec, tscm_summary *sum)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    SolverPtr sp;
    if (int rc = create_configured(p, dev, spec, sp)) return rc;
    return tscm_solver_solve(sp.get(), opt, sum);
}

static int solve_once(const tscm_problem *p, const tscm_options *opt_in, const SolveSpec &in, tscm_summary *sum)
{
    SolveSpec spec;
    tscm_options opt;
    if (int rc = preamble(p, !p || !sum, "NULL argument", opt_in, in, spec, opt)) return rc;
    if (int rc = check_options(opt, spec.loss.kind, spec.weights != nullptr)) return rc;
    return solve_configured(p, opt_in, spec, sum);
}

extern "C" int tscm_solve_weighted(const tscm_problem *p, const tscm_options *opt, const double *weights, const unsigned short *fixed, int kind, double scale,
                                   tscm_summary *sum)
{
    return solve_once(p, opt, spec_args(kind, scale, fixed, weights), sum);
}

extern "C" int tscm_solve_prior(const tscm_problem *p, const tscm_options *opt, const double *weights, const unsigned short *fixed, int kind, double scale,
                                const tscm_camera_priors *priors, tscm_summary *sum)
{
    return solve_once(p, opt, spec_args(kind, scale, fixed, weights, priors), sum);
}

extern "C" int tscm_solve_multi(const tscm_problem *p, const tscm_options *opt, tscm_summary *sum)
{
    if (!p) return validate(p);         // (these two name the problem)
    if (p->mono) return fail(TSCM_E_INVALID, "tscm_solve_multi called with a mono problem");
    return solve_once(p, opt, spec_args(TSCM_LOSS_NONE, 0.0, nullptr, nullptr), sum);
}

extern "C" int tscm_solve_mono(const tscm_problem *p, const tscm_options *opt, tscm_summary *sum)
{
    if (!p) return validate(p);
    if (!p->mono) return fail(TSCM_E_INVALID, "tscm_solve_mono called with a multi-camera problem");
    return solve_once(p, opt, spec_args(TSCM_LOSS_NONE, 0.0, nullptr, nullptr), sum);
}

extern "C" int tscm_solve_robust(const tscm_problem *p, const tscm_options *opt, int kind, double scale, tscm_summary *sum)
{
    return solve_once(p, opt, spec_args(kind, scale, nullptr, nullptr), sum);
}

extern "C" int tscm_solve_fixed(const tscm_problem *p, const tscm_options *opt, const unsigned short *fixed, int kind, double scale, tscm_summary *sum)
{
    return solve_once(p, opt, spec_args(kind, scale, fixed, nullptr), sum);
}

// The candidate of a solve's first trust-region step: the solve itself, stopped after one iteration (termination
// tolerances zeroed, so nothing ends it before the step is taken).  The first iteration writes its candidate into buffer 1
// (ctrl->cur = 0 at the start); k_end_solve / k_finish_solve copy it into buffer 0 only if the step was accepted and never
// write buffer 1, so buffer 1 holds the candidate whether the step was accepted or not
static int eval_step(const tscm_problem *p, int device, const tscm_options *opt_in, const SolveSpec &in, double *cam_rt, double *intr,
                     double *board_rt, int *valid, tscm_summary *summary)
{
    SolveSpec spec;
    tscm_options opt;
    int rc = preamble(p, !p || !intr || !valid || (!cam_rt && !p->mono) || (!board_rt && p->n_boards), "NULL argument", opt_in, in, spec, opt);
    if (rc) return rc;
    opt.max_num_iterations = 1;
    opt.function_tolerance = opt.gradient_tolerance = opt.parameter_tolerance = 0.0;
    if ((rc = check_options(opt, spec.loss.kind, spec.weights != nullptr))) return rc;
    SolverPtr sp;
    if ((rc = create_configured(p, device, spec, sp))) return rc;
    tscm_solver *s = sp.get();
    if ((rc = tscm_solver_upload_params(s, p->cam_rt, p->intr, p->board_rt))) return rc;
    tscm_summary sum;
    if ((rc = tscm_solver_solve_resident(s, &opt, &sum, 1))) return rc;
    // what the device does not hold (a mono problem's camera pose, boards without views) is the input
    if (cam_rt) { if (p->cam_rt) std::memcpy(cam_rt, p->cam_rt, sizeof(double) * 6 * p->n_cameras); else std::memset(cam_rt, 0, sizeof(double) * 6 * p->n_cameras); }
    if (p->n_boards) std::memcpy(board_rt, p->board_rt, sizeof(double) * 6 * p->n_boards);
    if ((rc = download_buffer(s, 1, cam_rt, intr, board_rt))) return rc;
    *valid = sum.num_iterations > 1 && sum.iterations[1].step_is_valid ? 1 : 0;
    if (summary) *summary = sum;
    return 0;
}

extern "C" int tscm_eval_step_ex(const tscm_problem *p, int device, const tscm_options *opt, double *cam_rt, double *intr,
                                 double *board_rt, int *valid, tscm_summary *summary)
{
    return eval_step(p, device, opt, spec_args(TSCM_LOSS_NONE, 0.0, nullptr, nullptr), cam_rt, intr, board_rt, valid, summary);
}

extern "C" int tscm_eval_step_robust(const tscm_problem *p, int device, const tscm_options *opt, int kind, double scale, double *cam_rt,
                                     double *intr, double *board_rt, int *valid, tscm_summary *summary)
{
    return eval_step(p, device, opt, spec_args(kind, scale, nullptr, nullptr), cam_rt, intr, board_rt, valid, summary);
}

extern "C" int tscm_eval_step_fixed(const tscm_problem *p, int device, const tscm_options *opt, const unsigned short *fixed, int kind, double scale,
                                    double *cam_rt, double *intr, double *board_rt, int *valid, tscm_summary *summary)
{
    return eval_step(p, device, opt, spec_args(kind, scale, fixed, nullptr), cam_rt, intr, board_rt, valid, summary);
}

extern "C" int tscm_eval_step_weighted(const tscm_problem *p, int device, const tscm_options *opt, const double *weights, const unsigned short *fixed,
                                       int kind, double scale, double *cam_rt, double *intr, double *board_rt, int *valid, tscm_summary *summary)
{
    return eval_step(p, device, opt, spec_args(kind, scale, fixed, weights), cam_rt, intr, board_rt, valid, summary);
}

extern "C" int tscm_eval_step_prior(const tscm_problem *p, int device, const tscm_options *opt, const double *weights, const unsigned short *fixed,
                                    int kind, double scale, const tscm_camera_priors *priors, double *cam_rt, double *intr, double *board_rt, int *valid,
                                    tscm_summary *summary)
{
    return eval_step(p, device, opt, spec_args(kind, scale, fixed, weights, priors), cam_rt, intr, board_rt, valid, summary);
}

// ------------------------------------------------------------------------------------------------
// operator level
// ------------------------------------------------------------------------------------------------
// upload the problem's current parameters into buffer 0 and compute the pose constants
// with_floats: the fp32-Jacobian kernel also reads the float half of the per-view records
static int prepare_eval(tscm_solver *s, int with_floats = 0)
{
    int rc;
    if ((rc = tscm_solver_upload_params(s, s->h_cam_rt, s->h_intr, s->h_board_rt))) return rc;
    DevState &S = s->S;
    HIP_TRY(hipMemset(S.ctrl, 0, sizeof(Ctrl)));
    HIP_TRY(hipMemcpy(S.cam_rt[0], s->d_init_cam, sizeof(double) * 6 * s->C, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(S.intr[0], s->d_init_intr, sizeof(double) * 9 * s->C, hipMemcpyDeviceToDevice));
    if (s->B) HIP_TRY(hipMemcpy(S.board_rt[0], s->d_init_board, sizeof(double) * 6 * s->B, hipMemcpyDeviceToDevice));
    hipLaunchKernelGGL(k_pose_prep, dim3((s->P.B + s->P.C + 255) / 256), dim3(256), 0, s->stream, s->P, S, 0);
    hipLaunchKernelGGL(k_view_prep, dim3((s->P.V + s->P.C + kVPrepThreads - 1) / kVPrepThreads), dim3(kVPrepThreads), 0, s->stream, s->P, S, 0, with_floats);
    HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int tscm_eval_functor(const tscm_problem *p, int device, double *residuals, double *J_cam,
                                 double *J_board, double *J_intr, double *cost)
{
    SolverPtr sp;
    int rc = create_scoped(p, device, sp);
    if (rc) return rc;
    tscm_solver *s = sp.get();
    if ((rc = prepare_eval(s))) return rc;
    const size_t N = (size_t)s->N;
    std::vector<int> corner_view(N);
    for (int v = 0; v < s->V; ++v) for (int j = 0; j < s->L.view_count[v]; ++j) corner_view[s->L.view_obs[v] + j] = v;
    const int *d_cv = nullptr;
    double *d_res = nullptr, *d_Jc = nullptr, *d_Jb = nullptr, *d_Ji = nullptr;
    HIP_TRY(s->mem.upload(&d_cv, corner_view));
    HIP_TRY(s->mem.alloc(&d_res, 2 * N));
    if (J_cam) HIP_TRY(s->mem.alloc(&d_Jc, 12 * N));
    if (J_board) HIP_TRY(s->mem.alloc(&d_Jb, 12 * N));
    if (J_intr) HIP_TRY(s->mem.alloc(&d_Ji, 18 * N));
    if (N) hipLaunchKernelGGL(k_eval_functor, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, s->P, s->S, d_cv, d_res, d_Jc, d_Jb, d_Ji);
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipGetLastError());
    // device corner order -> problem corner order (views in problem order, empty views skipped)
    std::vector<double> h_res(2 * N), h_Jc(d_Jc ? 12 * N : 0), h_Jb(d_Jb ? 12 * N : 0), h_Ji(d_Ji ? 18 * N : 0);
    if (N) HIP_TRY(hipMemcpy(h_res.data(), d_res, sizeof(double) * 2 * N, hipMemcpyDeviceToHost));
    if (d_Jc && N) HIP_TRY(hipMemcpy(h_Jc.data(), d_Jc, sizeof(double) * 12 * N, hipMemcpyDeviceToHost));
    if (d_Jb && N) HIP_TRY(hipMemcpy(h_Jb.data(), d_Jb, sizeof(double) * 12 * N, hipMemcpyDeviceToHost));
    if (d_Ji && N) HIP_TRY(hipMemcpy(h_Ji.data(), d_Ji, sizeof(double) * 18 * N, hipMemcpyDeviceToHost));
    std::vector<long> orig_row(p->n_views, 0);
    { long k = 0; for (int v = 0; v < p->n_views; ++v) { orig_row[v] = k; k += p->view_count[v]; } }
    double c = 0.0;
    for (int dv = 0; dv < s->V; ++dv) {
        const long dst = orig_row[s->L.dev2orig[dv]], src = s->L.view_obs[dv];
        const int cnt = s->L.view_count[dv];
        if (residuals) std::memcpy(residuals + 2 * dst, h_res.data() + 2 * src, sizeof(double) * 2 * cnt);
        if (J_cam) std::memcpy(J_cam + 12 * dst, h_Jc.data() + 12 * src, sizeof(double) * 12 * cnt);
        if (J_board) std::memcpy(J_board + 12 * dst, h_Jb.data() + 12 * src, sizeof(double) * 12 * cnt);
        if (J_intr) std::memcpy(J_intr + 18 * dst, h_Ji.data() + 18 * src, sizeof(double) * 18 * cnt);
    }
    for (size_t k = 0; k < N; ++k) c += 0.5 * (h_res[2 * k] * h_res[2 * k] + h_res[2 * k + 1] * h_res[2 * k + 1]);     // device corner order
    if (cost) *cost = c;
    return 0;
}

extern "C" int tscm_eval_normal_equations(const tscm_problem *p, int device, double *board_gram, double *board_grad,
                                          double *view_cross, double *cam_gram, double *cam_grad, double *cost)
{
    return tscm_eval_normal_equations_ex(p, device, nullptr, board_gram, board_grad, view_cross, cam_gram, cam_grad, cost);
}

// the Gram kernel is the one a solve with these options runs: jacobian_fp32 -> k_eval_gram_f32, TSCM_EXEC_GRAM_16X16 ->
// k_eval_gram, k_eval_gram4 otherwise (the other flags do not touch the evaluation).  Every kernel writes the same fp64
// record layout, so the extraction below is shared
// as_solved: the launch a solve makes (ExecPlan::skip_const_pose); otherwise every column (inspection)
static int solver_normal_equations(tscm_solver *s, const tscm_options &opt, bool as_solved, double *board_gram, double *board_grad,
                                   double *view_cross, double *cam_gram, double *cam_grad, double *cost)
{
    int rc;
    s->xp = plan_exec(s->L, s->C, s->P.n_act, kCommNone, opt.exec_flags, opt.jacobian_fp32, s->loss.kind, s->P.rp, s->dev, !as_solved, s->n_priors > 0);     // (its Gram kernel)
    if ((rc = prepare_eval(s, s->xp.f32() ? 1 : 0))) return rc;
    const DevProblem &P = s->P;
    DevState &S = s->S;
    if ((rc = launch_eval(s, 0))) return rc;
    // camera blocks only (camera priors: added there, at the problem's parameters in buffer 0)
    if (s->xp.priors) hipLaunchKernelGGL(k_reduce_stats_prior, dim3(P.C * kCamSl), dim3(256), 0, s->stream, P, S, 0, 0, s->prior_arg());
    else hipLaunchKernelGGL(k_reduce_stats, dim3(P.C * kCamSl), dim3(256), 0, s->stream, P, S, 0, 0);
    hipLaunchKernelGGL(k_finalize_eval, dim3(P.C), dim3(256), 0, s->stream, P, S, 0);            // camera blocks only
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipGetLastError());
    std::vector<double> rec((size_t)kRec * s->V), H(256 * (size_t)s->C), cc((size_t)kCStride * s->C);
    if (s->V) HIP_TRY(hipMemcpy(rec.data(), S.rec[0], sizeof(double) * rec.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(H.data(), S.H_stage, sizeof(double) * H.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cc.data(), S.cconst[0], sizeof(double) * cc.size(), hipMemcpyDeviceToHost));
    if (board_gram) std::memset(board_gram, 0, sizeof(double) * 36 * (size_t)s->B);
    if (board_grad) std::memset(board_grad, 0, sizeof(double) * 6 * (size_t)s->B);
    if (view_cross) std::memset(view_cross, 0, sizeof(double) * 90 * (size_t)s->n_views);
    for (int dv = 0; dv < s->V; ++dv) {
        // the view's record: W = E^T [F | r] (14 columns x 6 rows, column-major), E = E^T E_wb (3 columns x 6 rows); the
        // t_b x t_b block of E^T E follows from the t_c columns of W and the camera rotation (tb_tb), the block above
        // the diagonal by symmetry -- what the device-side consumers do
        const double *rw = rec.data() + (size_t)kRecW * s->L.view_slot[dv];
        const double *re = rec.data() + (size_t)kRecW * s->V + (size_t)kRecE * s->L.view_slot[dv];
        const double *Rc = cc.data() + (size_t)kCStride * s->L.view_cam[dv];
        const int b = s->L.b0 + s->L.board_perm[s->L.view_board[dv]], ov = s->L.dev2orig[dv];
        for (int i = 0; i < 6; ++i) {
            if (board_gram)
                for (int j = 0; j < 6; ++j) {
                    const int hi = std::max(i, j), lo = std::min(i, j);
                    board_gram[36 * (size_t)b + 6 * i + j] += lo < 3 ? re[6 * lo + hi] : tb_tb(rw, Rc, hi - 3, lo - 3);
                }
            if (board_grad) board_grad[6 * (size_t)b + i] += rw[6 * kFR + i];
            if (view_cross) {
                for (int j = 0; j < 13; ++j) view_cross[90 * (size_t)ov + 15 * i + j] = rw[6 * j + i];
            }
        }
    }
    double c = 0.0;
    for (int m = 0; m < s->C; ++m) {
        const double *h = H.data() + 256 * (size_t)m;
        if (cam_gram) { std::memset(cam_gram + 225 * (size_t)m, 0, sizeof(double) * 225); for (int i = 0; i < 13; ++i) for (int j = 0; j < 13; ++j) cam_gram[225 * (size_t)m + 15 * i + j] = h[16 * i + j]; }
        if (cam_grad) { std::memset(cam_grad + 15 * (size_t)m, 0, sizeof(double) * 15); for (int i = 0; i < 13; ++i) cam_grad[15 * (size_t)m + i] = h[16 * i + kFR]; }
        c += 0.5 * h[16 * kFR + kFR];
    }
    if (cost) *cost = c;
    return 0;
}

// the one-shot normal equations of every entry point that has them (tscm_host.h: tscm_covariance's blocks too).  A mask plays
// no part in an evaluation: in.fixed is not looked at
int tscm_eval_normal_equations_spec(const tscm_problem *p, int device, const tscm_options *opt_in, const SolveSpec &in, double *board_gram,
                                    double *board_grad, double *view_cross, double *cam_gram, double *cam_grad, double *cost)
{
    SolveSpec spec;
    tscm_options opt;
    int rc = preamble(p, !p, "problem is NULL", opt_in, spec_args(in.loss.kind, in.loss.a, nullptr, in.weights, in.priors), spec, opt);
    if (rc) return rc;
    opt.max_num_iterations = 0;         // (no iteration runs: the caller's count is not used)
    if ((rc = check_options(opt, spec.loss.kind, spec.weights != nullptr))) return rc;
    SolverPtr sp;
    if ((rc = create_configured(p, device, spec, sp))) return rc;
    return solver_normal_equations(sp.get(), opt, false, board_gram, board_grad, view_cross, cam_gram, cam_grad, cost);
}

extern "C" int tscm_solver_eval_normal_equations(tscm_solver *s, const tscm_options *opt_in, int as_solved, double *board_gram,
                                                 double *board_grad, double *view_cross, double *cam_gram, double *cam_grad, double *cost)
{
    if (!s) return fail(TSCM_E_INVALID, "solver is NULL");
    if (s->world != 1) return fail(TSCM_E_UNSUPPORTED, "tscm_solver_eval_normal_equations: a sharded solver holds a part of the problem");
    tscm_options opt;
    int rc = read_options(opt_in, s->mono ? 1 : 0, opt);
    if (rc) return rc;
    opt.max_num_iterations = 0;
    if ((rc = check_options(opt, s->loss.kind, s->weighted))) return rc;
    HIP_TRY(hipSetDevice(s->device));
    rc = solver_normal_equations(s, opt, as_solved != 0, board_gram, board_grad, view_cross, cam_gram, cam_grad, cost);
    s->xp = ExecPlan{};                 // (per solve: planned again from the options of the next one)
    return rc;
}

extern "C" int tscm_eval_normal_equations_ex(const tscm_problem *p, int device, const tscm_options *opt, double *board_gram,
                                             double *board_grad, double *view_cross, double *cam_gram, double *cam_grad, double *cost)
{
    return tscm_eval_normal_equations_spec(p, device, opt, spec_args(TSCM_LOSS_NONE, 0.0, nullptr, nullptr), board_gram, board_grad, view_cross, cam_gram, cam_grad, cost);
}

extern "C" int tscm_eval_normal_equations_robust(const tscm_problem *p, int device, const tscm_options *opt, int kind, double scale,
                                                 double *board_gram, double *board_grad, double *view_cross, double *cam_gram,
                                                 double *cam_grad, double *cost)
{
    return tscm_eval_normal_equations_spec(p, device, opt, spec_args(kind, scale, nullptr, nullptr), board_gram, board_grad, view_cross, cam_gram, cam_grad, cost);
}

extern "C" int tscm_eval_normal_equations_weighted(const tscm_problem *p, int device, const tscm_options *opt, const double *weights, int kind,
                                                   double scale, double *board_gram, double *board_grad, double *view_cross, double *cam_gram,
                                                   double *cam_grad, double *cost)
{
    return tscm_eval_normal_equations_spec(p, device, opt, spec_args(kind, scale, nullptr, weights), board_gram, board_grad, view_cross, cam_gram, cam_grad, cost);
}

extern "C" int tscm_eval_normal_equations_prior(const tscm_problem *p, int device, const tscm_options *opt, const double *weights, int kind, double scale,
                                                const tscm_camera_priors *priors, double *board_gram, double *board_grad, double *view_cross,
                                                double *cam_gram, double *cam_grad, double *cost)
{
    return tscm_eval_normal_equations_spec(p, device, opt, spec_args(kind, scale, nullptr, weights, priors), board_gram, board_grad, view_cross, cam_gram, cam_grad, cost);
}

// k_project (3 -> 2) and k_unproject (2 -> 3): n rows of `in` through one camera's intrinsics
static int map_rows(void (*kernel)(const double *, const double *, int, double *), const char *who, const double *intr9, const double *in, int w_in,
                    int n, int device, double *out, int w_out)
{
    if (!intr9 || (n > 0 && (!in || !out)) || n < 0) return fail(TSCM_E_INVALID, "NULL argument");
    if (int rc = select_device(device, who)) return rc;
    if (n == 0) return 0;
    DeviceMem mem;
    const double *d_i = nullptr, *d_p = nullptr;
    double *d_o = nullptr;
    HIP_TRY(mem.upload(&d_i, intr9, 9));
    HIP_TRY(mem.upload(&d_p, in, w_in * (size_t)n));
    HIP_TRY(mem.alloc(&d_o, w_out * (size_t)n));
    hipLaunchKernelGGL(kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d_i, d_p, n, d_o);
    HIP_TRY(hipMemcpy(out, d_o, w_out * (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tscm_project_points(const double *intr9, const double *points, int n, int device, double *pixels)
{
    return map_rows(k_project, "tscm_project_points", intr9, points, 3, n, device, pixels, 2);
}

extern "C" int tscm_unproject_pixels(const double *intr9, const double *pixels, int n, int device, double *rays)
{
    return map_rows(k_unproject, "tscm_unproject_pixels", intr9, pixels, 2, n, device, rays, 3);
}

extern "C" int tscm_reprojection_error(const tscm_problem *p, int device, double *per_camera_mean, double *global_mean, double *rmse)
{
    SolverPtr sp;
    int rc = create_scoped(p, device, sp);
    if (rc) return rc;
    tscm_solver *s = sp.get();
    if ((rc = tscm_solver_upload_params(s, s->h_cam_rt, s->h_intr, s->h_board_rt))) return rc;
    double *d_e = nullptr, *d_q = nullptr;
    HIP_TRY(s->mem.alloc(&d_e, (size_t)s->V));
    HIP_TRY(s->mem.alloc(&d_q, (size_t)s->V));
    if (s->V) hipLaunchKernelGGL(k_reproj_error<false>, dim3(s->V), dim3(64), 0, s->stream, s->P, s->d_init_cam, s->d_init_intr, s->d_init_board, d_e, d_q);
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipGetLastError());
    std::vector<double> e(s->V), q(s->V);
    if (s->V) { HIP_TRY(hipMemcpy(e.data(), d_e, sizeof(double) * s->V, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(q.data(), d_q, sizeof(double) * s->V, hipMemcpyDeviceToHost)); }
    std::vector<double> err(s->C, 0.0);
    std::vector<long> cnt(s->C, 0);
    double sq = 0.0;
    for (int v = 0; v < s->V; ++v) { err[s->L.view_cam[v]] += e[v]; cnt[s->L.view_cam[v]] += s->L.view_count[v]; sq += q[v]; }
    double tot = 0.0; long n = 0;
    for (int m = 0; m < s->C; ++m) { tot += err[m]; n += cnt[m]; if (per_camera_mean) per_camera_mean[m] = cnt[m] ? err[m] / (double)cnt[m] : 0.0; }
    if (global_mean) *global_mean = n ? tot / (double)n : 0.0;
    if (rmse) *rmse = n ? std::sqrt(sq / (double)n) : 0.0;
    return 0;
}

extern "C" int tscm_shard_frames(const tscm_problem *p, int world, int *owner)
{
    if (!p || !owner || world < 1) return fail(TSCM_E_INVALID, "bad arguments");
    if (int rc = validate(p)) return rc;
    std::vector<int> o;
    shard_owner(p, world, o);
    std::copy(o.begin(), o.end(), owner);
    return 0;
}

#ifdef TSCM_WAVE_TIMELINE
// profiling builds only: the per-wave timeline of the last recorded k_eval_gram launch (tools/wave_timeline.py)
extern "C" int tscm_debug_wave_timeline(long long *out, int max_waves)
{
    const int n = std::min(max_waves, tscm::kTimelineWaves);
    if (hipDeviceSynchronize() != hipSuccess) return TSCM_E_HIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(tscm::g_timeline), sizeof(long long) * 4 * (size_t)n) != hipSuccess) return TSCM_E_HIP;
    return n;
}
extern "C" int tscm_debug_kernel_timeline(long long *out, int max_groups)
{
    if (max_groups < tscm::kKtlGroups) return TSCM_E_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return TSCM_E_HIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(tscm::g_ktl), sizeof(long long) * 2 * tscm::kKtlKernels * tscm::kKtlGroups) != hipSuccess) return TSCM_E_HIP;
    return tscm::kKtlKernels;
}
extern "C" int tscm_debug_control_stamps(long long *out)
{
    if (hipDeviceSynchronize() != hipSuccess) return TSCM_E_HIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(tscm::g_ktlx), sizeof(long long) * 32) != hipSuccess) return TSCM_E_HIP;
    return 32;
}
extern "C" int tscm_debug_phase_stamps(long long *out, int max_groups)
{
    if (max_groups < tscm::kKtlGroups) return TSCM_E_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return TSCM_E_HIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(tscm::g_phs), sizeof(long long) * 3 * tscm::kPhStamps * tscm::kKtlGroups) != hipSuccess) return TSCM_E_HIP;
    return tscm::kPhStamps;
}
extern "C" int tscm_debug_wave_views(long long *out, int max_waves)
{
    const int n = std::min(max_waves, tscm::kTimelineWaves);
    if (hipDeviceSynchronize() != hipSuccess) return TSCM_E_HIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(tscm::g_tlv), sizeof(long long) * (4 + tscm::kTlViews) * (size_t)n) != hipSuccess) return TSCM_E_HIP;
    return 4 + tscm::kTlViews;
}
extern "C" int tscm_debug_wave_phases(long long *out, int max_waves)
{
    const int n = std::min(max_waves, tscm::kTimelineWaves);
    if (hipDeviceSynchronize() != hipSuccess) return TSCM_E_HIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(tscm::g_phase), sizeof(long long) * 5 * (size_t)n) != hipSuccess) return TSCM_E_HIP;
    return n;
}
#endif
