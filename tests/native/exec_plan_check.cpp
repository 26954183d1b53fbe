// CPU check of a solve's launch plan (tscm_calib_amd/csrc/tscm_exec_plan.h): the rows of DESIGN 4's launch table as
// decisions, and on random problems (planned with plan_layout) under random and boundary residency figures: a re-run never
// waits inside a launch, every launch whose workgroups wait for each other fits on the chip, and each exec flag changes only
// what tscm.h says it does.  Host logic only (no GPU).
//   usage: exec_plan_check rows                         one JSON line: per row, the facts the Python test asserts
//          exec_plan_check random <seed> <problems>     one JSON line: counts of what the problems exercised
//          exec_plan_check refusals                     one JSON line: code and message of every refusal case
//          exec_plan_check g4 <n>...                    one JSON line: kG4MaxKS and g4_plan's passes, per, ks of every board size n
#include "exec_problems.h"
#include "../../tscm_calib_amd/csrc/tscm_launch_seq.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

using namespace tscm;

// kernel launches of one iteration whose evaluation is a candidate's (the exchange markers not counted): seq_iteration's list
static int launches(const ExecPlan &x, const Layout &L, int C)
{
    SeqState st;
    LaunchList q;
    seq_begin(L, C, x, Start::Current, st, q);
    seq_iteration(L, C, x, ample(), 0, st, q);
    int n = 0;
    for (int i = 0; i < q.n; ++i) n += is_exchange(q.at[i].k) ? 0 : 1;
    return n;
}

static std::string g_fail;
#define CHECK(cond) do { if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; } while (0)

static const char *solver_name(Solver s) { return s == Solver::Empty ? "empty" : s == Solver::Dense4 ? "dense4" : s == Solver::Nd ? "nd" : "big"; }
static const char *tail_name(EvalTail t) { return t == EvalTail::Ride ? "ride" : t == EvalTail::StatsThenHead ? "stats_head" : t == EvalTail::ReduceControl ? "reduce_control" : "exchange"; }

static void row(const char *name, const ExecPlan &x, const Layout &L, int C, bool last = false)
{
    std::printf("\"%s\": {\"launches\": %d, \"tail\": \"%s\", \"ctl_in_schur\": %d, \"stats_ride\": %d, \"t_in_solve\": %d, \"solver\": \"%s\", "
                "\"nd\": %d, \"tpt\": %d, \"n_prod\": %d, \"n_bs\": %d, \"n_bs_blocks\": %d, \"bs_threads\": %d, \"comm\": %d, \"gram\": %d}%s",
                name, launches(x, L, C), tail_name(x.tail), x.ctl_in_schur, x.stats_ride, x.t_in_solve, solver_name(x.solver), x.nd, x.tpt,
                x.n_prod, x.n_bs, L.n_bs_blocks, x.bs_threads, x.comm, (int)x.gram, last ? "" : ", ");
}

static int rows()
{
    const int none = kCommNone;
    std::printf("{");
    {   // config 4: 4 cameras, every board seen by two of them, ample residency
        const Layout L = ring(4, 5000).plan();
        const ExecDevice d = ample();
        row("config4", plan_exec(L, 4, 48, none, 0, 0, 0, 58, d), L, 4);
        row("config4_separate_stats", plan_exec(L, 4, 48, none, TSCM_EXEC_SEPARATE_STATS, 0, 0, 58, d), L, 4);
        row("config4_comm", plan_exec(L, 4, 48, kCommShared, 0, 0, 0, 58, d), L, 4);
        row("config4_one_rank_comm", plan_exec(L, 4, 48, kCommOneRank, 0, 0, 0, 58, d), L, 4);
        row("config4_keep_one_rank_comm", plan_exec(L, 4, 48, kCommOneRank, TSCM_EXEC_KEEP_SINGLE_RANK_COMM, 0, 0, 58, d), L, 4);
        row("config4_graph_order", plan_exec(L, 4, 48, none, TSCM_EXEC_GRAPH_REDUCED_ORDER, 0, 0, 58, d), L, 4);
        row("config4_dense_order", plan_exec(L, 4, 48, none, TSCM_EXEC_DENSE_REDUCED_ORDER, 0, 0, 58, d), L, 4);
    }
    {   // 8-camera ring whose Schur grid is more than one resident round: the back-substitution rides iff all of it fits
        const Layout L = ring(8, 5000).plan();
        ExecDevice d = ample();
        d.schur_resident_ride[2] = std::max(reduction_blocks(L, 8), L.nv_chunks[2]);       // one short of the riding grid
        ExecPlan x = plan_exec(L, 8, 100, none, 0, 0, 0, 58, d);
        d.nd_resident[0] = 1 + x.n_prod + L.n_bs_blocks;
        row("ring8_bs_fits", plan_exec(L, 8, 100, none, 0, 0, 0, 58, d), L, 8);
        d.nd_resident[0] -= 1;
        row("ring8_bs_one_short", plan_exec(L, 8, 100, none, 0, 0, 0, 58, d), L, 8);
        row("ring8_comm", plan_exec(L, 8, 100, kCommShared, 0, 0, 0, 58, ample()), L, 8);
    }
    {   // 12-camera rig: k_solve_reduced_big, the T reduction and the back-substitution on launches of their own
        const Layout L = ring(12, 3000).plan();
        row("rig12", plan_exec(L, 12, 150, none, 0, 0, 0, 58, ample()), L, 12);
        row("rig12_comm", plan_exec(L, 12, 150, kCommShared, 0, 0, 0, 58, ample()), L, 12);
    }
    {   // boards seen by four cameras: k_schur_factor + k_pair_gram, the control step out of the Schur head
        const Layout L = ring(4, 2000, 2).plan();
        std::printf("\"slow_boards\": %d, ", (int)L.slow_boards.size());
        row("seen_by_four", plan_exec(L, 4, 48, none, 0, 0, 0, 58, ample()), L, 4);
        row("seen_by_four_comm", plan_exec(L, 4, 48, kCommShared, 0, 0, 0, 58, ample()), L, 4);
    }
    {   // no free camera-side column
        const Layout L = ring(4, 500).plan();
        row("empty", plan_exec(L, 4, 0, none, 0, 0, 0, 58, ample()), L, 4, true);
    }
    std::printf("}\n");
    return 0;
}

// ---- random problems -------------------------------------------------------------------------------
// the fields of a plan, one bit each, for "a flag changes only what it names"
enum { F_COMM = 1, F_GRAM = 2, F_ROBUST = 4, F_TAIL = 8, F_CTL = 16, F_RIDE = 32, F_TSOLVE = 64, F_SOLVER = 128, F_ND = 256, F_TPT = 512,
       F_PROD = 1024, F_BS = 2048, F_BSTH = 4096 };
static int changed(const ExecPlan &a, const ExecPlan &b)
{
    return (a.comm != b.comm ? F_COMM : 0) | (a.gram != b.gram ? F_GRAM : 0) | (a.robust != b.robust ? F_ROBUST : 0) | (a.tail != b.tail ? F_TAIL : 0) |
           (a.ctl_in_schur != b.ctl_in_schur ? F_CTL : 0) | (a.stats_ride != b.stats_ride ? F_RIDE : 0) | (a.t_in_solve != b.t_in_solve ? F_TSOLVE : 0) |
           (a.solver != b.solver ? F_SOLVER : 0) | (a.nd != b.nd ? F_ND : 0) | (a.tpt != b.tpt ? F_TPT : 0) | (a.n_prod != b.n_prod ? F_PROD : 0) |
           (a.n_bs != b.n_bs ? F_BS : 0) | (a.bs_threads != b.bs_threads ? F_BSTH : 0);
}

static long g_count[32];
enum { C_PLANS, C_RIDE, C_BS_RIDE, C_BS_LIMIT, C_STATS_LIMIT, C_T_SOLVE, C_BIG, C_EMPTY, C_SLOW, C_FLAG0 };

// what every plan satisfies
static void check_plan(const ExecPlan &x, const Layout &L, int C, int n_act, int kind, int flags, const ExecDevice &d)
{
    const bool small = C <= kMaxCamLds;
    CHECK(x.comm == (kind == kCommShared || (kind == kCommOneRank && (flags & TSCM_EXEC_KEEP_SINGLE_RANK_COMM))));
    CHECK(x.stats_ride == (x.tail == EvalTail::Ride));
    CHECK(x.tail == EvalTail::Exchange ? (x.comm || !small) : !x.comm && small);
    CHECK(!x.ctl_in_schur || (nv_classes(L) == 1 && L.slow_boards.empty() && L.pc_begin.empty() && !(flags & TSCM_EXEC_SEPARATE_CONTROL)));
    CHECK(x.ctl_in_schur || x.tail == EvalTail::Exchange || x.tail == EvalTail::ReduceControl);
    CHECK(x.t_in_solve == (x.n_prod > 0));
    CHECK(!x.t_in_solve || (!x.comm && small && n_act > 0 && L.n_bids > 0 && L.n_bids <= kSmallBids && x.n_prod == 16 * L.n_bids));
    CHECK(x.solver == (n_act == 0 ? Solver::Empty : !small ? Solver::Big : C <= 4 && !(flags & (TSCM_EXEC_GRAPH_REDUCED_ORDER | TSCM_EXEC_DENSE_REDUCED_ORDER)) ? Solver::Dense4 : Solver::Nd));
    CHECK(x.solver != Solver::Nd ? x.nd == 0 && x.tpt == 1 : x.nd == ((flags & TSCM_EXEC_DENSE_REDUCED_ORDER) ? 1 : 0) && x.tpt == d.nd_tpt[x.nd]);
    // every waiting launch fits on the chip: the back-substitution rides only whole, next to the solver and the producers
    // (the producers themselves never wait: a launch of producers alone needs no residency)
    if (x.n_bs) {
        const int resident = x.solver == Solver::Dense4 ? d.dense4_resident : d.nd_resident[x.nd];
        CHECK(x.solver == Solver::Dense4 || x.solver == Solver::Nd);
        CHECK(x.n_bs == L.n_bs_blocks && L.bs_threads == 256 && 1 + x.n_prod + x.n_bs <= resident);
        CHECK(!(flags & TSCM_EXEC_SEPARATE_BACKSUB));
    }
    if (x.stats_ride) {
        const int nv = used_nv(L);
        CHECK(std::max(reduction_blocks(L, C), L.nv_chunks[nv]) + 1 <= d.schur_resident_ride[nv]);
        CHECK(!x.comm && small && !(flags & (TSCM_EXEC_SEPARATE_STATS | TSCM_EXEC_SEPARATE_CONTROL)));
    }
    CHECK(x.bs_threads == (x.n_bs == 0 && L.n_bs_blocks ? L.bs_threads : 0));
    CHECK(x.n_bs == 0 || x.n_bs == L.n_bs_blocks);
    // a re-run never waits inside a launch
    const int rerun = TSCM_EXEC_SEPARATE_T_REDUCE | TSCM_EXEC_SEPARATE_BACKSUB | TSCM_EXEC_SEPARATE_CONTROL;
    if ((flags & rerun) == rerun) CHECK(!x.stats_ride && !x.ctl_in_schur && x.n_prod == 0 && x.n_bs == 0);
}

// a single flag against the default plan: what it may change (tscm.h), and whether it changed that
static void check_flag(const ExecPlan &base, const ExecPlan &x, int bit, int kind, bool fp32, const Layout &L)
{
    const int down = F_PROD | F_BS | F_BSTH;              // a launch shape that frees or takes slots moves the back-substitution's fit
    int allowed = 0;
    switch (bit) {
    case TSCM_EXEC_SEPARATE_T_REDUCE: allowed = F_TSOLVE | down; break;
    case TSCM_EXEC_KEEP_SINGLE_RANK_COMM: allowed = kind == kCommOneRank ? F_COMM | F_TAIL | F_CTL | F_RIDE | F_TSOLVE | down : 0; break;
    case TSCM_EXEC_GRAM_16X16: allowed = fp32 ? 0 : F_GRAM; break;
    case TSCM_EXEC_SEPARATE_BACKSUB: allowed = F_BS | F_BSTH; break;
    case TSCM_EXEC_SEPARATE_CONTROL: allowed = F_TAIL | F_CTL | F_RIDE; break;
    case TSCM_EXEC_DENSE_REDUCED_ORDER: allowed = F_SOLVER | F_ND | F_TPT | F_BS | F_BSTH; break;
    case TSCM_EXEC_GRAPH_REDUCED_ORDER: allowed = F_SOLVER | F_TPT | F_BS | F_BSTH; break;
    case TSCM_EXEC_SEPARATE_STATS: allowed = F_TAIL | F_RIDE; break;
    }
    const int c = changed(base, x);
    CHECK((c & ~allowed) == 0);
    if (bit == TSCM_EXEC_SEPARATE_T_REDUCE && (c & F_BS)) CHECK(base.n_bs == 0 && x.n_bs == L.n_bs_blocks);      // freed slots only ever let it ride
    if (bit == TSCM_EXEC_KEEP_SINGLE_RANK_COMM) CHECK(x.comm == (kind != kCommNone));
    if (bit == TSCM_EXEC_SEPARATE_BACKSUB) CHECK(x.n_bs == 0);
    if (bit == TSCM_EXEC_SEPARATE_CONTROL) CHECK(!x.ctl_in_schur && !x.stats_ride);
    if (bit == TSCM_EXEC_SEPARATE_STATS) CHECK(!x.stats_ride && x.ctl_in_schur == base.ctl_in_schur);
    if (bit == TSCM_EXEC_GRAM_16X16 && !fp32) CHECK(x.gram == Gram::G16 || x.gram == Gram::G16Pitch58);
    for (int k = 0; k < 8; ++k) if (bit == 1 << k && c) ++g_count[C_FLAG0 + k];
}

static int random_run(unsigned long long seed, int problems)
{
    std::mt19937_64 rng(seed);
    auto uni = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
    for (int it = 0; it < problems && g_fail.empty(); ++it) {
        Prob q = random_problem(rng);
        const Layout L = q.plan(uni(0, 1) ? 256 : uni(1, 64));
        const int C = q.C, n_act = uni(0, 9) == 0 ? 0 : uni(1, 13 * C);
        const int rp = uni(0, 1) ? 58 : 2 + 8 * uni(1, 8), fp32 = uni(0, 3) == 0, loss = uni(0, 3) == 0 ? uni(1, 3) : 0;
        if (!L.slow_boards.empty()) ++g_count[C_SLOW];
        for (int trial = 0; trial < 12 && g_fail.empty(); ++trial) {
            // residency: ample, random, or at the exact limit of a riding launch / one below it
            ExecDevice d = ample();
            d.nd_tpt[0] = uni(1, 2); d.nd_tpt[1] = uni(1, 2);
            const int kind = uni(0, 2), flags = uni(0, 1) ? 0 : uni(0, TSCM_EXEC_ALL);
            if (trial % 3 == 1) random_residency(rng, d);
            else if (trial % 3 == 2) {
                const int below = uni(0, 1);
                const ExecPlan x0 = plan_exec(L, C, n_act, kind, flags, fp32, loss, rp, d);
                limit_residency(L, C, x0, below, d);
                const ExecPlan x = plan_exec(L, C, n_act, kind, flags, fp32, loss, rp, d);
                const bool could_bs = (x.solver == Solver::Dense4 || x.solver == Solver::Nd) && L.bs_threads == 256 && L.n_bs_blocks > 0 && !(flags & TSCM_EXEC_SEPARATE_BACKSUB);
                if (could_bs) { CHECK((x.n_bs > 0) == !below); ++g_count[C_BS_LIMIT]; }
                if (x0.ctl_in_schur && !x0.comm && C <= kMaxCamLds && !(flags & TSCM_EXEC_SEPARATE_STATS)) { CHECK(x.stats_ride == !below); ++g_count[C_STATS_LIMIT]; }
            }
            const ExecPlan x = plan_exec(L, C, n_act, kind, flags, fp32, loss, rp, d);
            check_plan(x, L, C, n_act, kind, flags, d);
            ++g_count[C_PLANS];
            if (x.stats_ride) ++g_count[C_RIDE];
            if (x.n_bs) ++g_count[C_BS_RIDE];
            if (x.t_in_solve) ++g_count[C_T_SOLVE];
            if (x.solver == Solver::Big) ++g_count[C_BIG];
            if (x.solver == Solver::Empty) ++g_count[C_EMPTY];
            const ExecPlan base = plan_exec(L, C, n_act, kind, 0, fp32, loss, rp, d);
            for (int k = 0; k < 8; ++k) check_flag(base, plan_exec(L, C, n_act, kind, 1 << k, fp32, loss, rp, d), 1 << k, kind, fp32, L);
            const int rerun = TSCM_EXEC_SEPARATE_T_REDUCE | TSCM_EXEC_SEPARATE_BACKSUB | TSCM_EXEC_SEPARATE_CONTROL;
            check_plan(plan_exec(L, C, n_act, kind, flags | rerun, fp32, loss, rp, d), L, C, n_act, kind, flags | rerun, d);
        }
        if (!g_fail.empty()) { std::printf("{\"ok\": false, \"problem\": %d, \"C\": %d, \"B\": %d, \"failed\": \"%s\"}\n", it, q.C, q.B, g_fail.c_str()); return 1; }
    }
    std::printf("{\"ok\": true, \"plans\": %ld, \"stats_ride\": %ld, \"bs_ride\": %ld, \"bs_limit\": %ld, \"stats_limit\": %ld, \"t_in_solve\": %ld, "
                "\"big\": %ld, \"empty\": %ld, \"slow\": %ld, \"flag_changes\": [%ld, %ld, %ld, %ld, %ld, %ld, %ld, %ld]}\n",
                g_count[C_PLANS], g_count[C_RIDE], g_count[C_BS_RIDE], g_count[C_BS_LIMIT], g_count[C_STATS_LIMIT], g_count[C_T_SOLVE],
                g_count[C_BIG], g_count[C_EMPTY], g_count[C_SLOW], g_count[C_FLAG0], g_count[C_FLAG0 + 1], g_count[C_FLAG0 + 2],
                g_count[C_FLAG0 + 3], g_count[C_FLAG0 + 4], g_count[C_FLAG0 + 5], g_count[C_FLAG0 + 6], g_count[C_FLAG0 + 7]);
    return 0;
}

// ---- refusals --------------------------------------------------------------------------------------
static void refusal(const char *name, int max_iter, int flags, int loss, bool last = false)
{
    tscm_options o{};
    o.struct_size = sizeof(tscm_options);
    o.max_num_iterations = max_iter;
    o.exec_flags = flags;
    std::string err;
    const int rc = check_exec_options(o, loss, err);
    std::printf("\"%s\": [%d, \"%s\"]%s", name, rc, rc ? err.c_str() : "", last ? "" : ", ");
}

static int refusals()
{
    std::printf("{");
    refusal("valid", 50, 0, TSCM_LOSS_NONE);
    refusal("iterations_0", 0, 0, TSCM_LOSS_NONE);
    refusal("iterations_255", 255, 0, TSCM_LOSS_NONE);
    refusal("iterations_256", 256, 0, TSCM_LOSS_NONE);
    refusal("iterations_negative", -1, 0, TSCM_LOSS_NONE);
    refusal("all_flags", 50, TSCM_EXEC_ALL, TSCM_LOSS_NONE);
    refusal("flag_256", 50, 256, TSCM_LOSS_NONE);
    refusal("flag_sign_bit", 50, (int)0x80000000u, TSCM_LOSS_NONE);
    refusal("gram16_huber", 50, TSCM_EXEC_GRAM_16X16, TSCM_LOSS_HUBER);
    refusal("gram16_soft_l1", 50, TSCM_EXEC_GRAM_16X16, TSCM_LOSS_SOFT_L1);
    refusal("gram16_cauchy", 50, TSCM_EXEC_GRAM_16X16, TSCM_LOSS_CAUCHY);
    refusal("huber_other_flags", 50, TSCM_EXEC_ALL & ~TSCM_EXEC_GRAM_16X16, TSCM_LOSS_HUBER);
    refusal("unknown_bits_before_gram16_loss", 50, 256 | TSCM_EXEC_GRAM_16X16, TSCM_LOSS_HUBER);
    refusal("iterations_before_unknown_bits", 300, 256, TSCM_LOSS_NONE, true);
    std::printf("}\n");
    return 0;
}

// ---- the Gram kernels' pass plan ----------------------------------------------------------------------
static int g4(int n, char **sizes)
{
    std::printf("{\"max_ks\": %d, \"plans\": {", kG4MaxKS);
    for (int i = 0; i < n; ++i) {
        const G4Plan g = g4_plan(std::atoi(sizes[i]));
        std::printf("\"%d\": [%d, %d, %d]%s", std::atoi(sizes[i]), g.passes, g.per, g.ks, i + 1 < n ? ", " : "");
    }
    std::printf("}}\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "rows")) return rows();
    if (argc >= 4 && !std::strcmp(argv[1], "random")) return random_run(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc >= 2 && !std::strcmp(argv[1], "refusals")) return refusals();
    if (argc >= 2 && !std::strcmp(argv[1], "g4")) return g4(argc - 2, argv + 2);
    std::fprintf(stderr, "usage: exec_plan_check rows | random <seed> <problems> | refusals | g4 <n>...\n");
    return 2;
}
