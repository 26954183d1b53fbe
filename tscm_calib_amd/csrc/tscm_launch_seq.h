// tscm_launch_seq.h -- host side of the LM loop's launches: which kernels a solve enqueues, in which order, with which grids
// and arguments, and the hand-off counts its waiting workgroups compare against -- worked out from the ExecPlan
// (tscm_exec_plan.h) for one phase of a solve at a time.  Plain C++17 like tscm_exec_plan.h; tscm_solver.hip's enqueue()
// maps each Launch to its kernel, and tests/native/launch_seq_check.cpp replays whole solves against a model of the device
// counters on the CPU.
#ifndef TSCM_LAUNCH_SEQ_H
#define TSCM_LAUNCH_SEQ_H

#include "tscm_ctrl.h"
#include "tscm_exec_plan.h"

#include <algorithm>
#include <cassert>
#include <cstring>

namespace tscm {

enum class Kern {
    BeginViewPrep,                          // k_begin_view_prep: control block, hand-off counters at zero, start point, its constants
    Eval,                                   // the Gram kernel of ExecPlan::gram (launch_eval)
    ReduceControl,                          // k_reduce_control: reductions, statistics and the control step
    ReduceStats,                            // k_reduce_stats
    FinalizeEval,                           // k_finalize_eval
    Control,                                // k_control
    SchurFactor,                            // k_schur_factor (boards seen by more than three cameras)
    Schur1, Schur2, Schur3,                 // k_schur_gram<NV>
    SchurRide1, SchurRide2, SchurRide3,     // k_schur_gram<NV, true>: an evaluation's reductions ride in front of the chunks
    PairGram,                               // k_pair_gram
    TReduce,                                // k_T_reduce
    SolveDense4, SolveDense4Ride,           // k_solve_reduced<4, 16, 64[, true]>
    SolveNd1, SolveNd2, SolveNd1Ride, SolveNd2Ride,     // k_solve_nd<tpt[, true]>
    SolveBig,                               // k_solve_reduced_big
    SolveEmpty,                             // ... on the empty system: no free camera-side column
    Backsub128, Backsub256,                 // k_backsub_prep<128 / 256>: the back-substitution as a launch of its own
    FinishSolve,                            // k_finish_solve: the last control step, the accepted point, the control block to the host
    EndSolve,                               // k_end_solve
    CopyCtrl,                               // the control block and the iteration log to the host (a copy, not a kernel)
    ExchangeT, ExchangeH,                   // markers: the all-reduce of T / of H_stage, once for all members of a run (exchange())
};

inline bool is_exchange(Kern k) { return k == Kern::ExchangeT || k == Kern::ExchangeH; }
inline bool is_schur(Kern k) { return k >= Kern::Schur1 && k <= Kern::SchurRide3; }
inline bool is_schur_ride(Kern k) { return k >= Kern::SchurRide1 && k <= Kern::SchurRide3; }
inline int schur_nv(Kern k) { return is_schur_ride(k) ? (int)k - (int)Kern::SchurRide1 + 1 : (int)k - (int)Kern::Schur1 + 1; }
inline bool is_solve(Kern k) { return k >= Kern::SolveDense4 && k <= Kern::SolveEmpty; }
inline bool is_solve_ride(Kern k) { return k == Kern::SolveDense4Ride || k == Kern::SolveNd1Ride || k == Kern::SolveNd2Ride; }

// where k_begin_view_prep finds the start point: buffer 0 as it is, the registered arrays (`reset`), or -- a re-run -- the
// backup the first attempt left behind; every start but a re-run's keeps such a backup
enum class Start { Current, Init, Backup };

// the solver's fault injection (tscm_solver_debug_withhold_handoff): the hand-off a solve withholds
constexpr int kWithholdProducer = 1;    // a T producer of the riding solve launches (debug values 1 and 2)
constexpr int kWithholdStats = 2;       // a reduction block riding in k_schur_gram<NV, true> (debug value 3)

struct Launch {
    Kern k = Kern::Eval;
    int grid = 0;                       // workgroups
    int cand = 0, init = 0, have_backsub = 0;   // an evaluation's kernels: which point, the solve's first evaluation, after a back-substitution
    int ctl = 0;                        // k_schur_gram: the waiting evaluation's kCtl* bits as the kernel takes them (0: none)
    int ce = 0;                         // ... its control epoch: the control steps of Schur heads in this solve, this one included
    int target = 0;                     // ... the riding reductions' arrival count to wait for (over the solve)
    int chunk0 = 0, n_chunks = 0;       // ... its view-class chunks
    int first_round = 0;                // ... resident workgroups: the ones that take the control step themselves
    int epoch = 0;                      // a riding solve launch: the riding solve launches of this solve, this one included
    int withhold = 0;                   // ... fault injection: one T producer never reports in
    int n_prod = 0, n_bs = 0;           // ... T producers and back-substitution workgroups in it
    int nd = 0;                         // k_solve_nd: the plan (ExecPlan::nd)
    int f32 = 0;                        // with_floats: the fp32-Jacobian tier's constants as well
    Start start = Start::Current;       // k_begin_view_prep
};

// one phase of a solve; no heap: the longest phase is an iteration of a communicator plan with boards seen by more than three
// cameras (14 entries)
constexpr int kMaxLaunches = 16;
struct LaunchList {
    Launch at[kMaxLaunches];
    int n = 0;
    Launch &add(Kern k, int grid)
    {
        assert(n < kMaxLaunches);
        Launch &l = at[n++];
        l = Launch{};
        l.k = k; l.grid = grid;
        return l;
    }
};

// what the host counts over a solve (reset by seq_begin); the device's counters are zeroed by k_begin_view_prep and count the same
struct SeqState {
    int eval_pending = 0;               // an evaluation waits for its control step in the next k_schur_gram: its kCtl* bits
    int ctl_epoch = 0;                  // control steps taken in k_schur_gram's head so far (S.ctl_pub->epoch)
    int stats_epoch = 0;                // launches of k_schur_gram<NV, true> so far (S.stats_count counts their reduction workgroups)
    int t_epoch = 0;                    // riding solve launches so far (S.t_count, S.y_flag)
};

// the control block a solve starts from (k_begin_view_prep's argument)
inline CtrlHead ctrl_head_from_options(const tscm_options &o)
{
    CtrlHead h;
    std::memset(&h, 0, sizeof(h));
    h.radius = o.initial_trust_region_radius;
    h.decrease_factor = 2.0;
    h.opt.max_num_iterations = o.max_num_iterations;
    h.opt.function_tolerance = o.function_tolerance;
    h.opt.gradient_tolerance = o.gradient_tolerance;
    h.opt.parameter_tolerance = o.parameter_tolerance;
    h.opt.initial_radius = o.initial_trust_region_radius;
    h.opt.max_radius = o.max_trust_region_radius;
    h.opt.min_radius = o.min_trust_region_radius;
    h.opt.min_relative_decrease = o.min_relative_decrease;
    h.opt.min_lm_diagonal = o.min_lm_diagonal;
    h.opt.max_lm_diagonal = o.max_lm_diagonal;
    h.opt.max_invalid = o.max_num_consecutive_invalid_steps;
    h.opt.jacobi_scaling = o.jacobi_scaling;
    return h;
}

// An evaluation of the candidate, or of the start point (init): the Gram kernel, then ExecPlan::tail -- its reductions and
// control step, or the kCtl* bits with which it waits in st.eval_pending for the next Schur kernel's head
inline void seq_eval(const Layout &L, int C, const ExecPlan &x, bool init, SeqState &st, LaunchList &out)
{
    const int nr = reduction_blocks(L, C), cand = init ? 0 : 1;
    out.add(Kern::Eval, (int)L.chunk_vb.size() / 4).cand = cand;
    // a candidate's reductions ride in the next k_schur_gram<NV, true>
    if (x.tail == EvalTail::Ride && !init) { st.eval_pending = kCtlOneGpu | kCtlRide; return; }
    if (x.tail == EvalTail::ReduceControl) {
        Launch &r = out.add(Kern::ReduceControl, nr);
        r.cand = cand; r.init = init; r.have_backsub = cand;
        return;
    }
    Launch &r = out.add(Kern::ReduceStats, nr);
    r.cand = cand; r.init = init;
    // ... or the reductions alone: the next k_schur_gram takes the control step in its head (k_control_tail behind the last
    // evaluation of the solve).  Round 5: the solve's INITIAL evaluation as well (IterationZero in the head of the first Schur
    // kernel) -- k_reduce_control's last workgroup cost every solve 18.4 us where k_reduce_stats takes 5.5 and the head 4.4
    if (x.tail != EvalTail::Exchange) { st.eval_pending = kCtlOneGpu | (init ? kCtlInit : 0); return; }
    out.add(Kern::FinalizeEval, C + 1).have_backsub = cand;
    if (x.comm) out.add(Kern::ExchangeH, 0);
    // behind the all-reduce: k_control -- or, for a candidate's evaluation, the head of the next k_schur_gram
    if (x.ctl_in_schur && !init) st.eval_pending = kCtlComm;
    else out.add(Kern::Control, 1).init = init;
}

// the start of a solve: k_begin_view_prep (the control block, the hand-off counters and the start point with its constants in
// one launch) and the initial evaluation
inline void seq_begin(const Layout &L, int C, const ExecPlan &x, Start start, SeqState &st, LaunchList &out)
{
    st = SeqState{};
    out.n = 0;
    Launch &b = out.add(Kern::BeginViewPrep, (L.V + C + kVPrepThreads - 1) / kVPrepThreads);
    b.start = start; b.f32 = x.f32();
    seq_eval(L, C, x, /*init=*/true, st, out);
}

// One LM iteration: the Schur side (the waiting evaluation's reductions and control step in its head), the exchange of T, the
// reduced solve (T producers and back-substitution riding where the plan puts them), the back-substitution, the candidate's
// evaluation.  withhold: 0 or kWithhold*
inline void seq_iteration(const Layout &L, int C, const ExecPlan &x, const ExecDevice &dev, int withhold, SeqState &st, LaunchList &out)
{
    out.n = 0;
    const int ctl = st.eval_pending;        // (ctl_in_schur: exactly one of the three Schur variants is launched)
    st.eval_pending = 0;
    if (!L.slow_boards.empty()) out.add(Kern::SchurFactor, ((int)L.slow_boards.size() + 255) / 256);
    const bool ride = ctl & kCtlRide;
    const int nr = reduction_blocks(L, C);
    const int ce = ctl ? ++st.ctl_epoch : 0;
    const int target = ride ? nr * ++st.stats_epoch : 0;
    for (int nv = 1; nv <= 3; ++nv) {
        const int n = L.nv_chunks[nv];
        if (!n) continue;
        Launch &l = ride ? out.add(Kern((int)Kern::SchurRide1 + nv - 1), std::max(nr, n) + 1) : out.add(Kern((int)Kern::Schur1 + nv - 1), n + (ctl ? 1 : 0));
        l.ctl = ride ? (ctl & ~kCtlRide) | (withhold == kWithholdStats ? kCtlWithhold : 0) : ctl;
        l.ce = ce; l.target = target;
        l.chunk0 = L.nv_chunk0[nv]; l.n_chunks = n;
        l.first_round = ride ? dev.schur_resident_ride[nv] : dev.schur_resident[nv];
    }
    if (!L.pc_begin.empty()) out.add(Kern::PairGram, (int)L.pc_begin.size());
    if (L.n_bids && !x.t_in_solve) out.add(Kern::TReduce, L.n_bids * (256 / kTEntries));
    if (x.comm) out.add(Kern::ExchangeT, 0);
    // T producers, reduced solve and the waiting back-substitution workgroups in ONE launch where the plan puts them there
    const bool rides = x.n_prod || x.n_bs;
    Kern k = Kern::SolveBig;
    switch (x.solver) {
    case Solver::Dense4: k = rides ? Kern::SolveDense4Ride : Kern::SolveDense4; break;
    case Solver::Nd: k = x.tpt == 2 ? (rides ? Kern::SolveNd2Ride : Kern::SolveNd2) : (rides ? Kern::SolveNd1Ride : Kern::SolveNd1); break;
    case Solver::Big: k = Kern::SolveBig; break;
    case Solver::Empty: k = Kern::SolveEmpty; break;
    }
    Launch &s = out.add(k, rides ? 1 + x.n_prod + x.n_bs : 1);
    s.nd = x.nd;
    if (rides) {
        s.epoch = ++st.t_epoch;
        s.withhold = withhold == kWithholdProducer ? 1 : 0;
        s.n_prod = x.n_prod; s.n_bs = x.n_bs; s.f32 = x.f32();
    }
    if (x.bs_threads) out.add(x.bs_threads == 128 ? Kern::Backsub128 : Kern::Backsub256, L.n_bs_blocks).f32 = x.f32();
    seq_eval(L, C, x, /*init=*/false, st, out);
}

// The end of a solve, behind the last iteration -- ONE synchronisation for the whole solve: the last evaluation's control step
// if the steps were taken in k_schur_gram's head, the accepted point into buffer 0, the control block and the iteration log
// to the host.  One GPU: k_finish_solve; communicator (or a rig of more than 8 cameras): k_control, k_end_solve and a copy
inline void seq_finish(const Layout &L, int C, SeqState &st, LaunchList &out)
{
    out.n = 0;
    const int ctl = st.eval_pending, nb = std::min(256, (6 * std::max(L.B, C) + 255) / 256 + 1);
    st.eval_pending = 0;
    if (ctl & kCtlOneGpu) {
        // (the reductions of the solve's last evaluation found no Schur kernel to ride in)
        if (ctl & kCtlRide) out.add(Kern::ReduceStats, reduction_blocks(L, C)).cand = 1;
        const int was_init = (ctl & kCtlInit) ? 1 : 0;
        Launch &f = out.add(Kern::FinishSolve, nb + 1);
        f.init = was_init; f.have_backsub = !was_init;
        return;
    }
    if (ctl == kCtlComm) out.add(Kern::Control, 1);
    out.add(Kern::EndSolve, nb);
    out.add(Kern::CopyCtrl, 0);
}

}  // namespace tscm

#endif
