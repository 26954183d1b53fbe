// CPU check of the LM loop's launch sequence (tscm_calib_amd/csrc/tscm_launch_seq.h): whole solves of 0, 1, 2 and K
// iterations on random problems (planned with plan_layout) under random and boundary residency figures, replayed against a
// model of the device's hand-off counters -- the riding reductions' targets, the control epochs of the Schur heads, the
// riding solve launches' epochs, one control step per evaluation, no reductions dropped at the end, residency of every
// waiting launch, the re-run without waiting launches, the fault injection, the exchange markers.  Host logic only (no GPU).
//   usage: launch_seq_check rows                         one JSON line: per fixed configuration, the kernels of each phase
//          launch_seq_check random <seed> <problems>     one JSON line: counts of what the solves exercised
//          launch_seq_check head                         one JSON line: ctrl_head_from_options against every option field
//          launch_seq_check route < problem              one JSON line: layout, columns, plan and kernels of the problem on stdin
#include "exec_problems.h"
#include "../../tscm_calib_amd/csrc/tscm_columns.h"
#include "../../tscm_calib_amd/csrc/tscm_launch_seq.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace tscm;

static std::string g_fail;
#define CHECK(cond) do { if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; } while (0)

static const char *kern_name(Kern k)
{
    static const char *names[] = { "begin_view_prep", "eval", "reduce_control", "reduce_stats", "finalize_eval", "control", "schur_factor",
                                   "schur1", "schur2", "schur3", "schur_ride1", "schur_ride2", "schur_ride3", "pair_gram", "T_reduce",
                                   "solve_dense4", "solve_dense4_ride", "solve_nd1", "solve_nd2", "solve_nd1_ride", "solve_nd2_ride",
                                   "solve_big", "solve_empty", "backsub128", "backsub256", "finish_solve", "end_solve", "copy_ctrl",
                                   "exchange_T", "exchange_H" };
    static_assert(sizeof(names) / sizeof(names[0]) == (size_t)Kern::ExchangeH + 1, "a name per Kern");
    return names[(int)k];
}

// the inputs of one solve's sequence
struct Case {
    const Layout *L = nullptr;
    int C = 0;
    ExecPlan x;
    ExecDevice d;
};

// a whole solve of n_iter iterations, as the driver plans it: begin, iterations, finish (one list per phase)
static std::vector<LaunchList> plan_solve(const Case &c, int n_iter, int withhold, Start start, SeqState &st, int *max_len)
{
    std::vector<LaunchList> phases(n_iter + 2);
    seq_begin(*c.L, c.C, c.x, start, st, phases[0]);
    for (int it = 1; it <= n_iter; ++it) seq_iteration(*c.L, c.C, c.x, c.d, withhold, st, phases[it]);
    seq_finish(*c.L, c.C, st, phases[n_iter + 1]);
    for (const LaunchList &q : phases) *max_len = std::max(*max_len, q.n);
    return phases;
}

static bool waits(const Launch &l) { return is_schur_ride(l.k) || is_solve_ride(l.k) || (is_schur(l.k) && l.ctl != 0); }
static bool schur_side(Kern k) { return k == Kern::SchurFactor || is_schur(k) || k == Kern::PairGram || k == Kern::TReduce; }

static long g_count[16];
enum { C_SOLVES, C_ITERS, C_SCHUR_RIDE, C_SOLVE_RIDE, C_HEAD_STEPS, C_FINISH_RIDE, C_COMM, C_BIG, C_WITHHOLD1, C_WITHHOLD2, C_RERUN, C_MAX_LEN };

// Replays one solve against the device's counters (zeroed by k_begin_view_prep) and the state of its evaluations
static void replay(const Case &c, const std::vector<LaunchList> &phases, Start start, int n_iter)
{
    const Layout &L = *c.L;
    const ExecPlan &x = c.x;
    const int nr = reduction_blocks(L, c.C);
    int stats_count = 0, ctl_epoch = 0, t_count = 0, y_epoch = 0;       // S.stats_count, S.ctl_pub->epoch, S.t_count, S.y_flag >> 1
    int open = 0;                      // evaluations waiting for their control step
    bool unreduced = false;            // ... whose reductions have not run
    int cur_init = -1, n_eval = 0;     // the open (or last) evaluation is the initial one
    bool finished = false;
    Kern prev = Kern::ExchangeH;       // the entry before, across phases (a marker at the start: no launch yet)
    bool have_prev = false;
    for (size_t ph = 0; ph < phases.size(); ++ph) {
        const LaunchList &q = phases[ph];
        const bool begin = ph == 0, finish = ph + 1 == phases.size();
        int n_solve = 0, n_eval_ph = 0, n_xt = 0, n_xh = 0;
        for (int i = 0; i < q.n; ++i) {
            const Launch &l = q.at[i];
            CHECK(!finished);
            CHECK((l.k == Kern::BeginViewPrep) == (begin && i == 0));
            if (waits(l)) CHECK(!is_schur(l.k) || x.ctl_in_schur);
            switch (l.k) {
            case Kern::BeginViewPrep:
                CHECK(!have_prev && l.start == start && l.f32 == (int)x.f32() && l.grid * kVPrepThreads >= L.V + c.C);
                break;
            case Kern::Eval:
                CHECK(open == 0);                        // the evaluation before got its control step
                open = 1; unreduced = true; cur_init = n_eval == 0; ++n_eval; ++n_eval_ph;
                CHECK(l.cand == (cur_init ? 0 : 1) && l.grid == (int)L.chunk_vb.size() / 4);
                break;
            case Kern::ReduceStats: case Kern::ReduceControl:
                CHECK(open == 1 && unreduced && l.grid == nr && l.cand == (cur_init ? 0 : 1) && l.init == cur_init);
                unreduced = false;
                if (l.k == Kern::ReduceControl) { CHECK(l.have_backsub == l.cand && x.tail == EvalTail::ReduceControl); open = 0; }
                break;
            case Kern::FinalizeEval:
                CHECK(open == 1 && !unreduced && l.have_backsub == (cur_init ? 0 : 1) && l.grid == c.C + 1);
                break;
            case Kern::Control:
                CHECK(open == 1 && !unreduced && l.init == cur_init && l.grid == 1);
                CHECK(!x.comm || prev == Kern::ExchangeH);
                open = 0;
                break;
            case Kern::Schur1: case Kern::Schur2: case Kern::Schur3:
            case Kern::SchurRide1: case Kern::SchurRide2: case Kern::SchurRide3: {
                const int nv = schur_nv(l.k);
                CHECK(l.n_chunks == L.nv_chunks[nv] && l.n_chunks > 0 && l.chunk0 == L.nv_chunk0[nv]);
                CHECK(l.first_round == (is_schur_ride(l.k) ? c.d.schur_resident_ride[nv] : c.d.schur_resident[nv]));
                if (is_schur_ride(l.k)) {
                    // the evaluation's reductions ride: every one of them has a workgroup, and all of the grid is resident
                    CHECK(open == 1 && unreduced && !cur_init && x.tail == EvalTail::Ride);
                    stats_count += nr;
                    CHECK(l.target == stats_count);
                    CHECK(l.grid >= nr + 1 && l.grid >= l.n_chunks + 1 && l.grid <= c.d.schur_resident_ride[nv]);
                    unreduced = false;
                    ++g_count[C_SCHUR_RIDE];
                } else {
                    CHECK(l.target == 0 && (l.ctl & kCtlWithhold) == 0 && l.grid == l.n_chunks + (l.ctl ? 1 : 0));
                }
                if (l.ctl & (kCtlOneGpu | kCtlComm)) {
                    // the control step of the waiting evaluation, in this launch's head
                    CHECK(open == 1 && !unreduced && x.ctl_in_schur);
                    CHECK((l.ctl & (kCtlOneGpu | kCtlComm)) == (x.comm ? kCtlComm : kCtlOneGpu) && ((l.ctl & kCtlInit) != 0) == (cur_init == 1));
                    CHECK((l.ctl & kCtlRide) == 0);
                    ++ctl_epoch;
                    CHECK(l.ce == ctl_epoch);
                    open = 0;
                    ++g_count[C_HEAD_STEPS];
                } else CHECK(l.ctl == 0 && l.ce == 0);
                break;
            }
            case Kern::SolveDense4: case Kern::SolveDense4Ride: case Kern::SolveNd1: case Kern::SolveNd2: case Kern::SolveNd1Ride:
            case Kern::SolveNd2Ride: case Kern::SolveBig: case Kern::SolveEmpty:
                ++n_solve;
                CHECK(!x.comm || prev == Kern::ExchangeT);
                if (is_solve_ride(l.k)) {
                    // the producers count in over the solve; the back-substitution waits for the solver's flag of this epoch
                    t_count += l.n_prod;
                    ++y_epoch;
                    CHECK(l.epoch == y_epoch && l.epoch * l.n_prod == t_count);
                    CHECK(l.n_prod == x.n_prod && l.n_bs == x.n_bs && l.grid == 1 + l.n_prod + l.n_bs && l.f32 == (int)x.f32());
                    if (l.n_bs) CHECK(l.grid <= (l.k == Kern::SolveDense4Ride ? c.d.dense4_resident : c.d.nd_resident[l.nd]));
                    ++g_count[C_SOLVE_RIDE];
                } else CHECK(l.grid == 1 && l.epoch == 0 && l.withhold == 0 && l.n_prod == 0 && l.n_bs == 0 && l.f32 == 0);
                CHECK(l.nd == x.nd);
                break;
            case Kern::Backsub128: case Kern::Backsub256:
                CHECK(is_solve(prev) && l.grid == L.n_bs_blocks && (l.k == Kern::Backsub128 ? 128 : 256) == x.bs_threads && l.f32 == (int)x.f32());
                break;
            case Kern::SchurFactor:
                CHECK(l.grid * 256 >= (int)L.slow_boards.size());
                break;
            case Kern::PairGram:
                CHECK(l.grid == (int)L.pc_begin.size());
                break;
            case Kern::TReduce:
                CHECK(!x.t_in_solve && l.grid * kTEntries == 256 * L.n_bids);
                break;
            case Kern::FinishSolve:
                // the last evaluation's control step; its reductions ran (riding ones found no Schur kernel: k_reduce_stats)
                CHECK(finish && open == 1 && !unreduced && l.init == cur_init && l.have_backsub == !cur_init);
                CHECK(x.tail == EvalTail::Ride || x.tail == EvalTail::StatsThenHead);
                if (prev == Kern::ReduceStats && x.tail == EvalTail::Ride) ++g_count[C_FINISH_RIDE];
                open = 0;
                finished = i + 1 == q.n;
                CHECK(finished);
                break;
            case Kern::EndSolve:
                CHECK(finish && open == 0 && i + 2 == q.n && q.at[i + 1].k == Kern::CopyCtrl);
                CHECK(x.tail == EvalTail::Exchange || x.tail == EvalTail::ReduceControl);
                break;
            case Kern::CopyCtrl:
                CHECK(finish && prev == Kern::EndSolve);
                finished = true;
                break;
            case Kern::ExchangeT:
                CHECK(x.comm && !begin && !finish && (!L.n_bids || prev == Kern::TReduce));
                ++n_xt;
                break;
            case Kern::ExchangeH:
                CHECK(x.comm && prev == Kern::FinalizeEval);
                ++n_xh;
                break;
            }
            if (schur_side(l.k)) CHECK(open == 0);       // every evaluation has had its control step when the Schur side starts
            prev = l.k;
            have_prev = true;
        }
        // one solve and one evaluation per iteration; a communicator's two all-reduces per iteration, one behind the
        // initial evaluation
        if (!begin && !finish) CHECK(n_solve == 1 && n_eval_ph == 1);
        if (begin) CHECK(n_eval_ph == 1 && n_solve == 0);
        CHECK(n_xt == (x.comm && !begin && !finish ? 1 : 0) && n_xh == (x.comm && !finish ? 1 : 0));
    }
    CHECK(finished && open == 0 && n_eval == n_iter + 1);
    CHECK(stats_count == nr * (x.tail == EvalTail::Ride ? std::max(n_iter - 1, 0) : 0));
    // (a communicator's initial evaluation takes its step in k_control)
    CHECK(ctl_epoch == (!x.ctl_in_schur ? 0 : x.comm ? std::max(n_iter - 1, 0) : n_iter));
}

// The solves of one plan: 0, 1, 2 and K iterations, each with every fault injection word, two in a row on the same state
static void check_case(const Case &c, int flags, std::mt19937_64 &rng)
{
    const int K = std::uniform_int_distribution<int>(3, 20)(rng);
    const int rerun = TSCM_EXEC_SEPARATE_T_REDUCE | TSCM_EXEC_SEPARATE_BACKSUB | TSCM_EXEC_SEPARATE_CONTROL;
    int max_len = 0;
    for (int n_iter : { 0, 1, 2, K }) {
        SeqState st;
        std::vector<LaunchList> base;
        for (int w : { 0, kWithholdProducer, kWithholdStats }) {
            for (Start start : { Start::Init, Start::Current, Start::Backup }) {
                // (the state of the solve before: seq_begin starts from zero, as the device does)
                const std::vector<LaunchList> ph = plan_solve(c, n_iter, w, start, st, &max_len);
                replay(c, ph, start, n_iter);
                ++g_count[C_SOLVES];
                g_count[C_ITERS] += n_iter;
                if (start == Start::Init && w == 0) base = ph;
                if ((flags & rerun) == rerun) {
                    for (const LaunchList &q : ph) for (int i = 0; i < q.n; ++i) CHECK(!waits(q.at[i]));
                    ++g_count[C_RERUN];
                }
                if (start != Start::Init) continue;
                // the fault injection marks exactly the launches it names, and changes nothing else
                CHECK(ph.size() == base.size());
                for (size_t p = 0; p < ph.size() && p < base.size(); ++p) {
                    CHECK(ph[p].n == base[p].n);
                    for (int i = 0; i < ph[p].n && i < base[p].n; ++i) {
                        const Launch &a = ph[p].at[i], &b = base[p].at[i];
                        const bool fault_t = a.withhold != 0, fault_s = (a.ctl & kCtlWithhold) != 0;
                        CHECK(fault_t == (w == kWithholdProducer && is_solve_ride(a.k)));
                        CHECK(fault_s == (w == kWithholdStats && is_schur_ride(a.k)));
                        if (fault_t) ++g_count[C_WITHHOLD1];
                        if (fault_s) ++g_count[C_WITHHOLD2];
                        Launch a2 = a;
                        a2.withhold = 0; a2.ctl &= ~kCtlWithhold;
                        CHECK(std::memcmp(&a2, &b, sizeof(Launch)) == 0);
                    }
                }
            }
        }
    }
    g_count[C_MAX_LEN] = std::max<long>(g_count[C_MAX_LEN], max_len);
    CHECK(max_len <= kMaxLaunches);
    if (c.x.comm) ++g_count[C_COMM];
    if (c.x.solver == Solver::Big) ++g_count[C_BIG];
}

static int random_run(unsigned long long seed, int problems)
{
    std::mt19937_64 rng(seed);
    auto uni = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
    const int rerun = TSCM_EXEC_SEPARATE_T_REDUCE | TSCM_EXEC_SEPARATE_BACKSUB | TSCM_EXEC_SEPARATE_CONTROL;
    for (int it = 0; it < problems && g_fail.empty(); ++it) {
        Prob q = random_problem(rng);
        const Layout L = q.plan(uni(0, 1) ? 256 : uni(1, 64));
        const int C = q.C, n_act = uni(0, 9) == 0 ? 0 : uni(1, 13 * C);
        const int rp = uni(0, 1) ? 58 : 2 + 8 * uni(1, 8), fp32 = uni(0, 3) == 0, loss = uni(0, 3) == 0 ? uni(1, 3) : 0;
        for (int trial = 0; trial < 6 && g_fail.empty(); ++trial) {
            // residency: ample, random, or at the exact limit of a riding launch / one below it
            Case c;
            c.L = &L; c.C = C;
            c.d = ample();
            c.d.nd_tpt[0] = uni(1, 2); c.d.nd_tpt[1] = uni(1, 2);
            const int kind = uni(0, 2), flags = uni(0, 2) == 0 ? rerun : uni(0, 1) ? 0 : uni(0, TSCM_EXEC_ALL);
            if (trial % 3 == 1) random_residency(rng, c.d);
            else if (trial % 3 == 2) limit_residency(L, C, plan_exec(L, C, n_act, kind, flags, fp32, loss, rp, c.d), uni(0, 1), c.d);
            c.x = plan_exec(L, C, n_act, kind, flags, fp32, loss, rp, c.d);
            check_case(c, flags, rng);
        }
        if (!g_fail.empty()) { std::printf("{\"ok\": false, \"problem\": %d, \"C\": %d, \"B\": %d, \"failed\": \"%s\"}\n", it, q.C, q.B, g_fail.c_str()); return 1; }
    }
    std::printf("{\"ok\": true, \"solves\": %ld, \"iterations\": %ld, \"schur_ride\": %ld, \"solve_ride\": %ld, \"head_steps\": %ld, \"finish_ride\": %ld, "
                "\"comm\": %ld, \"big\": %ld, \"withhold_producer\": %ld, \"withhold_stats\": %ld, \"rerun\": %ld, \"max_len\": %ld, \"capacity\": %d}\n",
                g_count[C_SOLVES], g_count[C_ITERS], g_count[C_SCHUR_RIDE], g_count[C_SOLVE_RIDE], g_count[C_HEAD_STEPS], g_count[C_FINISH_RIDE],
                g_count[C_COMM], g_count[C_BIG], g_count[C_WITHHOLD1], g_count[C_WITHHOLD2], g_count[C_RERUN], g_count[C_MAX_LEN], kMaxLaunches);
    return 0;
}

// ---- fixed configurations: the kernels of each phase of a two-iteration solve -----------------------------------------
static void print_list(const LaunchList &q)
{
    std::printf("[");
    for (int i = 0; i < q.n; ++i) std::printf("\"%s\"%s", kern_name(q.at[i].k), i + 1 < q.n ? ", " : "");
    std::printf("]");
}

static void row(const char *name, const Layout &L, int C, const ExecPlan &x, bool last = false)
{
    Case c;
    c.L = &L; c.C = C; c.x = x; c.d = ample();
    SeqState st;
    int max_len = 0;
    const std::vector<LaunchList> ph = plan_solve(c, 2, 0, Start::Init, st, &max_len);
    replay(c, ph, Start::Init, 2);
    std::printf("\"%s\": {\"begin\": ", name); print_list(ph[0]);
    std::printf(", \"first\": "); print_list(ph[1]);
    std::printf(", \"iteration\": "); print_list(ph[2]);
    std::printf(", \"finish\": "); print_list(ph[3]);
    std::printf("}%s", last ? "" : ", ");
}

static int rows()
{
    const int none = kCommNone, rerun = TSCM_EXEC_SEPARATE_T_REDUCE | TSCM_EXEC_SEPARATE_BACKSUB | TSCM_EXEC_SEPARATE_CONTROL;
    std::printf("{");
    const Layout L4 = ring(4, 5000).plan(), L8 = ring(8, 5000).plan(), L12 = ring(12, 3000).plan(), L4w = ring(4, 2000, 2).plan();
    ExecDevice d8 = ample();
    d8.schur_resident_ride[2] = std::max(reduction_blocks(L8, 8), L8.nv_chunks[2]);       // config 5's Schur grid: more than one round
    d8.nd_resident[0] = 1;                                                                   // the back-substitution does not fit next to the solver
    row("config4", L4, 4, plan_exec(L4, 4, 48, none, 0, 0, 0, 58, ample()));
    row("config4_separate_stats", L4, 4, plan_exec(L4, 4, 48, none, TSCM_EXEC_SEPARATE_STATS, 0, 0, 58, ample()));
    row("config4_rerun", L4, 4, plan_exec(L4, 4, 48, none, rerun, 0, 0, 58, ample()));
    row("config4_comm", L4, 4, plan_exec(L4, 4, 48, kCommShared, 0, 0, 0, 58, ample()));
    row("ring8", L8, 8, plan_exec(L8, 8, 100, none, 0, 0, 0, 58, d8));
    row("rig12", L12, 12, plan_exec(L12, 12, 150, none, 0, 0, 0, 58, ample()));
    row("seen_by_four_comm", L4w, 4, plan_exec(L4w, 4, 48, kCommShared, 0, 0, 0, 58, ample()), true);
    std::printf(", \"ok\": %s, \"failed\": \"%s\"}\n", g_fail.empty() ? "true" : "false", g_fail.c_str());
    return 0;
}

// ---- ctrl_head_from_options: every option field, nothing else -----------------------------------------------------------
static int head()
{
    tscm_options o{};
    o.struct_size = sizeof(o);
    o.max_num_iterations = 17; o.function_tolerance = 1.5; o.gradient_tolerance = 2.5; o.parameter_tolerance = 3.5;
    o.initial_trust_region_radius = 4.5; o.max_trust_region_radius = 5.5; o.min_trust_region_radius = 6.5; o.min_relative_decrease = 7.5;
    o.min_lm_diagonal = 8.5; o.max_lm_diagonal = 9.5; o.max_num_consecutive_invalid_steps = 11; o.jacobi_scaling = 13;
    o.check_every = 19; o.jacobian_fp32 = 1; o.exec_flags = TSCM_EXEC_ALL;
    const CtrlHead h = ctrl_head_from_options(o);
    const Options &p = h.opt;
    CHECK(p.max_num_iterations == 17 && p.function_tolerance == 1.5 && p.gradient_tolerance == 2.5 && p.parameter_tolerance == 3.5);
    CHECK(p.initial_radius == 4.5 && p.max_radius == 5.5 && p.min_radius == 6.5 && p.min_relative_decrease == 7.5);
    CHECK(p.min_lm_diagonal == 8.5 && p.max_lm_diagonal == 9.5 && p.max_invalid == 11 && p.jacobi_scaling == 13);
    CHECK(h.radius == 4.5 && h.decrease_factor == 2.0);
    // everything else of the head starts at zero (padding included: the head is a kernel argument)
    CtrlHead z = h;
    std::memset(&z.opt, 0, sizeof(z.opt));
    z.radius = 0.0; z.decrease_factor = 0.0;
    const unsigned char *b = reinterpret_cast<const unsigned char *>(&z);
    for (size_t i = 0; i < sizeof(z); ++i) CHECK(b[i] == 0);
    std::printf("{\"ok\": %s, \"failed\": \"%s\"}\n", g_fail.empty() ? "true" : "false", g_fail.c_str());
    return 0;
}

// ---- one problem from stdin: what creation and a solve of two iterations decide on the host ------------------------------
// Whitespace-separated integers:
//   C B n_points mono   V   V x (camera board count)   C x cam_pose_constant   has B x board_pose_constant   has C x fixed mask
//   exec_flags jacobian_fp32 loss_kind comm_kind   n_cu waves_per_cu
//   workgroups per CU: k_schur_gram<1..3>, k_schur_gram<1..3, true>, k_solve_reduced<4, 16, 64, true>, k_solve_nd<tpt, true> on a plan
//   of up to `split` bytes of LDS and on a larger one, then `split`
static int next_int()
{
    int v = 0;
    if (std::scanf("%d", &v) != 1) { std::fprintf(stderr, "route: input ends early\n"); std::exit(2); }
    return v;
}

static int route()
{
    Prob q;
    q.C = next_int(); q.B = next_int(); q.n_points = next_int(); q.mono = next_int();
    for (int v = next_int(); v > 0; --v) { const int c = next_int(), b = next_int(); q.add(c, b, next_int()); }
    for (int m = 0; m < q.C; ++m) q.cam_const.push_back((unsigned char)next_int());
    if (next_int()) for (int b = 0; b < q.B; ++b) q.board_const.push_back((unsigned char)next_int());
    std::vector<unsigned short> fixed;
    if (next_int()) for (int m = 0; m < q.C; ++m) fixed.push_back((unsigned short)next_int());
    tscm_options o{};
    o.struct_size = sizeof(o);
    o.exec_flags = next_int(); o.jacobian_fp32 = next_int();
    const int loss = next_int(), comm = next_int(), n_cu = next_int(), waves_per_cu = next_int();
    std::string err;
    if (check_exec_options(o, loss, err)) { std::fprintf(stderr, "route: %s\n", err.c_str()); return 2; }
    // tscm_solver_create_sharded: the layout, the residency of the launches that wait, the columns (apply_columns: both
    // k_solve_nd plans' tpt and residency); tscm_solver_set_fixed_intrinsics: the columns under the mask
    const Layout L = q.plan(n_cu, waves_per_cu);
    ExecDevice d;
    for (int nv = 1; nv <= 3; ++nv) d.schur_resident[nv] = next_int() * n_cu;
    for (int nv = 1; nv <= 3; ++nv) d.schur_resident_ride[nv] = next_int() * n_cu;
    const int dense4_per_cu = next_int(), nd_per_cu[2] = { next_int(), next_int() }, nd_lds_split = next_int();
    if (q.C <= kDense4Cams) d.dense4_resident = dense4_per_cu * n_cu;
    ColumnPlan cols;
    if (int rc = plan_columns(L, q.C, fixed.empty() ? nullptr : fixed.data(), cols, err)) { std::fprintf(stderr, "route: %d %s\n", rc, err.c_str()); return 2; }
    if (cols.has_nd)
        for (int v = 0; v < 2; ++v) {
            d.nd_resident[v] = nd_per_cu[sizeof(double) * cols.nd[v].lds_doubles > (size_t)nd_lds_split ? 1 : 0] * n_cu;
            d.nd_tpt[v] = cols.nd[v].tpt;
        }
    // run_lm_inner: the plan (rp: the Jacobian tile's pitch of tscm_solver_create_sharded), then begin, two iterations, finish
    Case c;
    c.L = &L; c.C = q.C; c.d = d;
    const int rp = 8 * ((std::min(64, q.n_points) + 7) / 8) + 2;
    c.x = plan_exec(L, q.C, cols.n_act, comm, o.exec_flags, o.jacobian_fp32, loss, rp, d);
    const ExecPlan &x = c.x;
    // the back-substitution is a launch of its own only because the solve's launch would not be resident with it
    ExecDevice roomy = d;
    roomy.dense4_resident = roomy.nd_resident[0] = roomy.nd_resident[1] = 1 << 24;
    const bool bs_ride_refused = !x.n_bs && plan_exec(L, q.C, cols.n_act, comm, o.exec_flags, o.jacobian_fp32, loss, rp, roomy).n_bs;
    SeqState st;
    int max_len = 0;
    const std::vector<LaunchList> ph = plan_solve(c, 2, 0, Start::Init, st, &max_len);
    replay(c, ph, Start::Init, 2);
    static const char *solver[] = { "empty", "dense4", "nd", "big" }, *tail[] = { "reduce_control", "stats_head", "ride", "exchange" };
    std::printf("{\"bs_threads\": %d, \"n_bs_blocks\": %d, \"nv_chunks\": [0, %d, %d, %d], \"n_bids\": %d, \"slow_boards\": %d, \"fallback_pairs\": %d, "
                "\"n_act\": %d, \"dense4_cams\": %d, \"bs_ride_refused\": %d, ", L.bs_threads, L.n_bs_blocks, L.nv_chunks[1], L.nv_chunks[2], L.nv_chunks[3], L.n_bids, (int)L.slow_boards.size(),
                (int)L.pair_i.size(), cols.n_act, kDense4Cams, (int)bs_ride_refused);
    std::printf("\"last_dev_view\": %d, \"eval_chunks\": %d, ", L.dev2orig.empty() ? -1 : L.dev2orig.back(), (int)L.chunk_vb.size());      // (the last view of the last evaluation chunk)
    std::printf("\"plan\": {\"comm\": %d, \"gram\": %d, \"robust\": %d, \"tail\": \"%s\", \"ctl_in_schur\": %d, \"stats_ride\": %d, \"t_in_solve\": %d, "
                "\"solver\": \"%s\", \"nd\": %d, \"tpt\": %d, \"n_prod\": %d, \"n_bs\": %d, \"bs_threads\": %d}, ", x.comm, (int)x.gram, x.robust,
                tail[(int)x.tail], x.ctl_in_schur, x.stats_ride, x.t_in_solve, solver[(int)x.solver], x.nd, x.tpt, x.n_prod, x.n_bs, x.bs_threads);
    if (x.solver == Solver::Nd) std::printf("\"nd_tpt\": %d, \"nd_dense\": %d, ", cols.nd[x.nd].tpt, (int)cols.nd[x.nd].dense);
    std::printf("\"begin\": "); print_list(ph[0]);
    std::printf(", \"first\": "); print_list(ph[1]);
    std::printf(", \"iteration\": "); print_list(ph[2]);
    std::printf(", \"finish\": "); print_list(ph[3]);
    std::printf(", \"ok\": %s, \"failed\": \"%s\"}\n", g_fail.empty() ? "true" : "false", g_fail.c_str());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "rows")) return rows();
    if (argc >= 4 && !std::strcmp(argv[1], "random")) return random_run(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc >= 2 && !std::strcmp(argv[1], "head")) return head();
    if (argc >= 2 && !std::strcmp(argv[1], "route")) return route();
    std::fprintf(stderr, "usage: launch_seq_check rows | random <seed> <problems> | head | route < problem\n");
    return 2;
}
