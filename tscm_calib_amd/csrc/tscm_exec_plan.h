// tscm_exec_plan.h -- host side of a solve's launch sequence: which kernels one LM iteration enqueues and where the
// hand-offs between them ride, decided once per solve from the layout, the options and the residency figures measured at
// creation.  Plain C++17 like tscm_layout.h; tscm_launch_seq.h turns the plan into the launches, and
// tests/native/exec_plan_check.cpp checks it against the launch table of DESIGN 4 on the CPU.
#ifndef TSCM_EXEC_PLAN_H
#define TSCM_EXEC_PLAN_H

#include "tscm_layout.h"

#include <algorithm>
#include <string>

// g4_plan is shared with device code (as lm_step, tscm_ctrl.h): unmarked under a plain C++ compiler
#ifdef __HIPCC__
#define TSCM_PLAN_FN __host__ __device__ inline
#else
#define TSCM_PLAN_FN inline
#endif

namespace tscm {

constexpr int kCamSl = 16;         // the per-camera tile reduction runs in slices of 32 of the 512 raw entries: C * kCamSl workgroups
constexpr int kTSlices = 16;       // slices of the T reduction (k_T_reduce and its fused form)
constexpr int kTEntries = 64;      // entries of a tile per workgroup of k_T_reduce: n_bids * 256 / kTEntries workgroups
constexpr int kFusedEntries = 256 / kTSlices;        // fused T reduction: 16 entries x 16 slices = the solver's 256 threads
constexpr int kVPrepThreads = 128; // workgroup of k_view_prep / k_begin_view_prep: a thread per view or camera
constexpr int kDense4Cams = 4;     // rigs of up to 4 cameras: k_solve_reduced factors the reduced system as one dense block

// Bits of k_schur_gram's `ctl` argument, and of the host's eval_pending: an evaluation waits for its control step, which
// the next Schur kernel takes in its head
constexpr int kCtlOneGpu = 1;      // ... from the reductions' finished sums (one GPU)
constexpr int kCtlComm = 2;        // ... from the all-reduced H_stage (communicator)
constexpr int kCtlInit = 4;        // ... of the solve's initial evaluation (IterationZero)
constexpr int kCtlRide = 8;        // its reductions ride in that launch (k_schur_gram<NV, true>; host only: the kernel gets ctl & 7)
constexpr int kCtlWithhold = 16;   // fault injection: a riding reduction block never reports in

// the communicator tscm_solver_set_comm registered: none, one of a single rank, one of several ranks or a local group
enum CommKind { kCommNone, kCommOneRank, kCommShared };
inline bool uses_comm(int kind, int exec_flags) { return kind == kCommShared || (kind == kCommOneRank && (exec_flags & TSCM_EXEC_KEEP_SINGLE_RANK_COMM)); }

enum class Gram { G4, F32, G16, G16Pitch58 };        // k_eval_gram4, k_eval_gram_f32, k_eval_gram<0>, k_eval_gram<58>
// where an evaluation's reductions and control step go
enum class EvalTail {
    ReduceControl,      // k_reduce_control: reductions, statistics and the step in one launch
    StatsThenHead,      // k_reduce_stats; the step in the next Schur kernel's head
    Ride,               // a candidate's reductions ride in k_schur_gram<NV, true> (the initial evaluation: StatsThenHead)
    Exchange,           // k_reduce_stats + k_finalize_eval, all-reduce of H_stage, then k_control or (ctl_in_schur, a
                        // candidate) the step in the next Schur kernel's head
};
enum class Solver { Empty, Dense4, Nd, Big };        // n_act == 0, k_solve_reduced<4, 16, 64>, k_solve_nd<tpt>, k_solve_reduced_big

// workgroups resident at once (occupancy x CUs), measured at creation: a launch whose workgroups wait for each other is
// only made if all of them are
struct ExecDevice {
    int schur_resident[4] = {}, schur_resident_ride[4] = {};     // k_schur_gram<NV>, k_schur_gram<NV, true>
    int dense4_resident = 0;                                      // k_solve_reduced<4, 16, 64, true>
    int nd_resident[2] = {}, nd_tpt[2] = { 1, 1 };                // k_solve_nd<tpt, true> on plan v, and its tpt
};

struct ExecPlan {
    bool comm = false;                  // the communicator path: two all-reduces per iteration
    Gram gram = Gram::G4;
    bool robust = false;                // the ROBUST instantiation of the Gram kernel (a loss)
    // k_eval_gram4 leaves out the rotation columns w_c of a camera whose pose block is constant (L.cam_const: no pose column
    // in the reduced system, plan_columns): what a solve does.  The inspection entries (tscm_eval_normal_equations*) return
    // every column and plan with inspect = true; the 16x16 and fp32 kernels always form all columns
    bool skip_const_pose = false;
    EvalTail tail = EvalTail::ReduceControl;
    bool ctl_in_schur = false;          // the control step of an evaluation is taken in the head of the next k_schur_gram
    bool stats_ride = false;            // a candidate's reductions ride in it (tail == Ride)
    bool priors = false;                // the reductions add camera priors: k_reduce_stats_prior
    bool t_in_solve = false;            // k_T_reduce rides in the reduced solve's launch as n_prod producer workgroups
    Solver solver = Solver::Empty;
    int nd = 0, tpt = 1;                // Solver::Nd: plan nd (0 the camera-pair graph, 1 one dense block) and its tpt
    int n_prod = 0, n_bs = 0;           // producers and back-substitution workgroups in the solve's launch (n_bs: all or none)
    int bs_threads = 0;                 // the back-substitution's launch of its own: 128 or 256 threads, 0 none
    bool f32() const { return gram == Gram::F32; }
};

// the workgroups of the evaluation's reductions (k_reduce_stats, k_reduce_control): camera slices and board statistics
inline int reduction_blocks(const Layout &L, int C) { return C * kCamSl + (L.B + 255) / 256; }

// jacobian_fp32 -> k_eval_gram_f32, TSCM_EXEC_GRAM_16X16 -> k_eval_gram (the pitch-58 instantiation for 53..56 corners
// per pass), k_eval_gram4 otherwise
inline Gram plan_gram(int exec_flags, int jacobian_fp32, int rp)
{
    if (jacobian_fp32) return Gram::F32;
    if (!(exec_flags & TSCM_EXEC_GRAM_16X16)) return Gram::G4;
    return rp == 58 ? Gram::G16Pitch58 : Gram::G16;
}

// Pass plan of the Gram kernels k_eval_gram4 / k_eval_gram_f32 (round 6: every board size): a pass holds 4 KS <= 56 rows
constexpr int kG4MaxKS = 14;                    // k-steps of a pass: at most 56 rows
// pass plan of a board of n corners: ceil(n / 56) passes of `per` corners each (a multiple of four; the last pass takes what is left)
struct G4Plan { int passes, per, ks; };
TSCM_PLAN_FN G4Plan g4_plan(int n_points)
{
    G4Plan g;
    g.passes = (n_points + 4 * kG4MaxKS - 1) / (4 * kG4MaxKS);
    if (g.passes < 1) g.passes = 1;
    g.ks = ((n_points + g.passes - 1) / g.passes + 3) / 4;
    if (g.ks < 1) g.ks = 1;
    g.per = 4 * g.ks;
    return g;
}

inline ExecPlan plan_exec(const Layout &L, int C, int n_act, int comm_kind, int exec_flags, int jacobian_fp32, int loss_kind, int rp,
                          const ExecDevice &dev, bool inspect = false, bool priors = false)
{
    ExecPlan p;
    p.comm = uses_comm(comm_kind, exec_flags);
    p.gram = plan_gram(exec_flags, jacobian_fp32, rp);
    p.robust = loss_kind != TSCM_LOSS_NONE;
    p.priors = priors;
    p.skip_const_pose = !inspect && p.gram == Gram::G4;
    // one GPU with <= 8 cameras (finish_evaluation's LDS fits k_schur_gram's) or a communicator; exactly one Schur kernel
    // per iteration.  (A grid of several rounds -- config 5 on one GPU: 1256 workgroups, 2.5 rounds -- pays the step in its
    // first round only: the later rounds read the outcome workgroup 0 publishes)
    const int n_variants = (L.nv_chunks[1] ? 1 : 0) + (L.nv_chunks[2] ? 1 : 0) + (L.nv_chunks[3] ? 1 : 0);
    const bool small = C <= kMaxCamLds;
    p.ctl_in_schur = (p.comm || small) && L.slow_boards.empty() && L.pc_begin.empty() && n_variants == 1 &&
                     !(exec_flags & TSCM_EXEC_SEPARATE_CONTROL);
    // the reductions ride: one GPU (the step from the finished sums themselves, not behind an all-reduce), and a grid of
    // ONE round -- every workgroup that takes a reduction block in front of its chunk is resident (they wait for each
    // other); at config 5 (1256 chunks, 2.5 rounds) the ride costs 2.5 us where it saves 4 at config 4
    const int nv = L.nv_chunks[1] ? 1 : L.nv_chunks[2] ? 2 : 3;
    // (camera priors, DESIGN 28: the prior enters in the reductions' launches of their own -- k_schur_gram has no prior
    // instantiation -- so a solve with priors plans as under TSCM_EXEC_SEPARATE_STATS)
    p.stats_ride = p.ctl_in_schur && !p.comm && small && !(exec_flags & TSCM_EXEC_SEPARATE_STATS) && !priors &&
                   std::max(reduction_blocks(L, C), L.nv_chunks[nv]) + 1 <= dev.schur_resident_ride[nv];
    // (rigs of more than 8 cameras: k_control as a launch of its own)
    p.tail = p.comm || !small ? EvalTail::Exchange : !p.ctl_in_schur ? EvalTail::ReduceControl : p.stats_ride ? EvalTail::Ride : EvalTail::StatsThenHead;
    // (camera priors: k_reduce_control has no prior instantiation either -- where it would run, the reductions, k_finalize_eval
    // and k_control do, as for a rig of more than 8 cameras)
    if (priors && p.tail == EvalTail::ReduceControl) p.tail = EvalTail::Exchange;
    // one GPU, up to 8 cameras: the T reduction rides in the reduced solve's launch; with a communicator the all-reduce of T
    // sits between the two
    p.t_in_solve = !(exec_flags & TSCM_EXEC_SEPARATE_T_REDUCE) && small && !p.comm && L.n_bids > 0 && L.n_bids <= kSmallBids && n_act > 0;
    p.n_prod = p.t_in_solve ? L.n_bids * (256 / kFusedEntries) : 0;
    // the reduced solver: k_solve_nd also for a rig of up to 4 cameras with TSCM_EXEC_GRAPH_ or _DENSE_REDUCED_ORDER
    p.nd = (exec_flags & TSCM_EXEC_DENSE_REDUCED_ORDER) ? 1 : 0;
    const bool graph_order = (exec_flags & TSCM_EXEC_GRAPH_REDUCED_ORDER) || p.nd;
    p.solver = n_act == 0 ? Solver::Empty : C <= kDense4Cams && !graph_order ? Solver::Dense4 : small ? Solver::Nd : Solver::Big;
    if (p.solver != Solver::Nd) p.nd = 0;
    p.tpt = p.solver == Solver::Nd ? dev.nd_tpt[p.nd] : 1;
    // the back-substitution workgroups wait for the camera step with their operands loaded in the solve's launch -- if ALL
    // of them are resident next to the solver workgroup and the producers (a waiting workgroup that keeps the solver off
    // the chip would wait for ever); otherwise it is a launch of its own.  Splitting it between the two was measured and
    // lost: at config 5 (5,000 groups, 255 of them riding) 364.3 against 356.7 us per iteration
    if (p.solver == Solver::Dense4 || p.solver == Solver::Nd) {
        const int resident = p.solver == Solver::Dense4 ? dev.dense4_resident : dev.nd_resident[p.nd];
        if (!(exec_flags & TSCM_EXEC_SEPARATE_BACKSUB) && L.bs_threads == 256 && L.n_bs_blocks <= resident - 1 - p.n_prod) p.n_bs = L.n_bs_blocks;
    }
    p.bs_threads = !p.n_bs && L.n_bs_blocks ? L.bs_threads : 0;
    return p;
}

// the refusals of a solve's options (struct_size is read_options' own): 0 or a TSCM_E_* code and its message in err
inline int check_exec_options(const tscm_options &o, int loss_kind, std::string &err)
{
    if (o.max_num_iterations < 0 || o.max_num_iterations > TSCM_MAX_ITERATIONS) return layout_fail(err, TSCM_E_INVALID, "max_num_iterations must be in [0, 255]");
    if (o.exec_flags & ~TSCM_EXEC_ALL) return layout_fail(err, TSCM_E_INVALID, "unknown bits in tscm_options.exec_flags (an options struct of an older ABI?)");
    if (loss_kind != TSCM_LOSS_NONE && (o.exec_flags & TSCM_EXEC_GRAM_16X16)) return layout_fail(err, TSCM_E_UNSUPPORTED, "TSCM_EXEC_GRAM_16X16 has no robust-loss kernel");
    return 0;
}

}  // namespace tscm

#endif
