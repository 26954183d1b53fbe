// CPU check of the camera priors' host plan (tscm_calib_amd/csrc/tscm_spec.h: check_camera_priors, effective_priors;
// tscm_exec_plan.h: plan_exec's `priors` input).
//   prior_check refusals        -> {"name": [code, "text"], ...}
//   prior_check table           -> effective_priors on the fixed example of tests/test_prior_reference.py: {"n": n, "mean": [...], "weight": [...]}
//   prior_check effective SEED N -> random problems, masks and priors against the rule written out by hand on the layout's facts:
//                                  {"ok": bool, "cases": n, "held": n, "const_pose": n, "mono": n, "inactive": n, "bc": n, "kept": n, "why": "..."}
//   prior_check plan SEED N     -> rings of 1..32 cameras and random problems, both tiers, every exec_flags combination, ample and
//                                  random residency: a plan with priors is the plan under TSCM_EXEC_SEPARATE_STATS, never rides, and
//                                  its launch sequence runs exactly one k_reduce_stats behind every evaluation and no k_reduce_control:
//                                  {"ok": bool, "plans": n, "would_ride": n, "tails": [stats_head, exchange <= 8 cameras, exchange > 8], "why": "..."}
// Built by tests/test_prior_reference.py, plain and under AddressSanitizer + UBSan.  Host logic only (no GPU).
#include "exec_problems.h"
#include "../../tscm_calib_amd/csrc/tscm_columns.h"
#include "../../tscm_calib_amd/csrc/tscm_launch_seq.h"
#include "../../tscm_calib_amd/csrc/tscm_spec.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

using namespace tscm;

static std::string g_fail;
#define CHECK(cond) do { if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; } while (0)

static tscm_camera_priors priors_of(const double *cm, const double *cw, const double *im, const double *iw)
{
    return tscm_camera_priors{ sizeof(tscm_camera_priors), cm, cw, im, iw };
}

static int refusals_mode()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::printf("{");
    bool first = true;
    auto put = [&](const char *name, const tscm_camera_priors *pr, int C) {
        std::string err;
        const int rc = check_camera_priors(pr, C, err);
        std::printf("%s\"%s\": [%d, \"%s\"]", first ? "" : ", ", name, rc, rc ? err.c_str() : "");
        first = false;
    };
    // two cameras
    std::vector<double> cm(12, 0.5), cw(12, 0.0), im(18, 1.0), iw(18, 2.0);
    tscm_camera_priors pr = priors_of(cm.data(), cw.data(), im.data(), iw.data());
    put("null", nullptr, 2);
    put("ok", &pr, 2);
    tscm_camera_priors none = priors_of(nullptr, nullptr, nullptr, nullptr);
    put("ok_no_arrays", &none, 2);
    tscm_camera_priors q = pr; q.struct_size = sizeof(tscm_camera_priors) - 8;
    put("struct_size", &q, 2);
    q = pr; q.struct_size = 0;
    put("struct_size_zero", &q, 2);
    q = pr; q.cam_rt_weight = nullptr;
    put("cam_mean_alone", &q, 2);
    q = pr; q.cam_rt_mean = nullptr;
    put("cam_weight_alone", &q, 2);
    q = pr; q.intr_weight = nullptr;
    put("intr_mean_alone", &q, 2);
    q = pr; q.intr_mean = nullptr;
    put("intr_weight_alone", &q, 2);
    auto with = [&](const char *name, std::vector<double> &v, int i, double x) { const double keep = v[i]; v[i] = x; put(name, &pr, 2); v[i] = keep; };
    with("w_negative", iw, 13, -1.0);           // camera 1, intrinsic 4
    with("w_nan", cw, 7, nan);                  // camera 1, pose coordinate 1
    with("w_inf", iw, 2, inf);
    with("mean_nan_live", im, 9, nan);          // its weight is 2
    with("mean_inf_live", im, 17, -inf);
    with("mean_nan_dead", cm, 3, nan);          // its weight is 0: not looked at
    with("w_beyond_n", iw, 17, -1.0);
    {   // only n_cameras cameras are read
        const double keep = iw[17]; iw[17] = -1.0; put("one_camera", &pr, 1); iw[17] = keep;
    }
    std::printf("}\n");
    return 0;
}

// the example of tests/test_prior_reference.py: 3 cameras; camera 0's pose constant, camera 1 holds cx and lambda, camera 2
// has no view; weights k + 1 on every coordinate (pose and intrinsics), means 100 m + k
static int table_mode()
{
    Prob q;
    q.C = 3; q.B = 2;
    q.add(0, 0, 54); q.add(1, 0, 54); q.add(1, 1, 40); q.add(0, 1, 54);
    q.cam_const = { 1, 0, 0 };
    const Layout L = q.plan();
    const unsigned short fixed[3] = { 0, TSCM_FIX_CX | TSCM_FIX_LAMBDA, 0 };
    ColumnPlan c;
    std::string err;
    if (plan_columns(L, 3, fixed, c, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 2; }
    std::vector<double> cm(18), cw(18), im(27), iw(27);
    for (int m = 0; m < 3; ++m) {
        for (int k = 0; k < 6; ++k) { cm[6 * m + k] = 100 * m + k; cw[6 * m + k] = k + 1; }
        for (int k = 0; k < 9; ++k) { im[9 * m + k] = 100 * m + 6 + k; iw[9 * m + k] = 6 + k + 1; }
    }
    const tscm_camera_priors pr = priors_of(cm.data(), cw.data(), im.data(), iw.data());
    std::vector<double> mean, weight;
    const int n = effective_priors(&pr, 3, c.col_active.data(), mean, weight);
    std::printf("{\"n\": %d, \"mean\": [", n);
    for (size_t i = 0; i < mean.size(); ++i) std::printf("%s%.17g", i ? ", " : "", mean[i]);
    std::printf("], \"weight\": [");
    for (size_t i = 0; i < weight.size(); ++i) std::printf("%s%.17g", i ? ", " : "", weight[i]);
    std::printf("]}\n");
    return 0;
}

static int effective_mode(unsigned long long seed, int n_cases)
{
    std::mt19937_64 rng(seed);
    auto uni = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
    long cases = 0, held = 0, cpose = 0, mono = 0, inactive = 0, bc = 0, kept = 0;
    for (int it = 0; it < n_cases; ++it) {
        Prob q = random_problem(rng);
        if (uni(0, 3) == 0) { q.cam_const.assign(q.C, 0); for (auto &x : q.cam_const) x = uni(0, 1); }
        if (q.C == 1 && uni(0, 1)) q.mono = 1;
        const Layout L = q.plan();
        std::vector<unsigned short> fixed(q.C, 0);
        const bool masks = uni(0, 1);
        for (auto &f : fixed) f = masks ? (unsigned short)(uni(0, 3) == 0 ? TSCM_FIX_INTRINSICS : uni(0, TSCM_FIX_ALL)) : 0;
        ColumnPlan c;
        std::string err;
        if (plan_columns(L, q.C, masks ? fixed.data() : nullptr, c, err)) continue;       // (a system no solver takes: creation refuses it)
        const bool has_cam = uni(0, 3) != 0, has_intr = uni(0, 3) != 0;
        std::vector<double> cm(6 * q.C), cw(6 * q.C), im(9 * q.C), iw(9 * q.C);
        auto val = [&] { return uni(0, 2) == 0 ? 0.0 : 0.25 * uni(1, 40); };
        for (auto &x : cm) x = 0.125 * uni(-80, 80);
        for (auto &x : im) x = 0.125 * uni(-80, 80);
        for (auto &x : cw) x = val();
        for (auto &x : iw) x = val();
        // a mean that is not finite under a weight of 0 is never read
        if (has_intr && iw[0] == 0.0) im[0] = std::numeric_limits<double>::quiet_NaN();
        const tscm_camera_priors pr = priors_of(has_cam ? cm.data() : nullptr, has_cam ? cw.data() : nullptr, has_intr ? im.data() : nullptr, has_intr ? iw.data() : nullptr);
        CHECK(check_camera_priors(&pr, q.C, err) == 0);
        std::vector<double> mean, weight;
        const int n = effective_priors(&pr, q.C, c.col_active.data(), mean, weight);
        CHECK((int)mean.size() == 16 * q.C && (int)weight.size() == 16 * q.C);
        int want_n = 0;
        for (int m = 0; m < q.C; ++m)
            for (int a = 0; a < 16; ++a) {
                // the rule of tscm.h, on the layout's facts
                const bool active = L.cam_active[m] != 0, pose_held = q.mono || (!q.cam_const.empty() && q.cam_const[m]);
                const bool is_held = masks && a >= 6 && a < 13 && ((fixed[m] >> (a - 6)) & 1);
                const bool is_free = a < 13 && active && !(a < 6 && pose_held) && !is_held;
                const bool given = a < 6 ? has_cam : a < 15 ? has_intr : false;
                const double w = !given ? 0.0 : a < 6 ? cw[6 * m + a] : iw[9 * m + a - 6], mu = !given ? 0.0 : a < 6 ? cm[6 * m + a] : im[9 * m + a - 6];
                const bool live = is_free && w > 0.0;
                CHECK(weight[16 * m + a] == (live ? w : 0.0));
                CHECK(mean[16 * m + a] == (live ? mu : 0.0));
                want_n += live;
                if (w > 0.0) { held += is_held; cpose += a < 6 && pose_held && active && !q.mono; mono += a < 6 && q.mono; inactive += !active; bc += a == 13 || a == 14; kept += live; }
            }
        CHECK(n == want_n);
        // no priors at all
        CHECK(effective_priors(nullptr, q.C, c.col_active.data(), mean, weight) == 0);
        for (double x : weight) CHECK(x == 0.0);
        ++cases;
    }
    std::printf("{\"ok\": %s, \"cases\": %ld, \"held\": %ld, \"const_pose\": %ld, \"mono\": %ld, \"inactive\": %ld, \"bc\": %ld, \"kept\": %ld, \"why\": \"%s\"}\n",
                g_fail.empty() ? "true" : "false", cases, held, cpose, mono, inactive, bc, kept, g_fail.c_str());
    return 0;
}

static long g_plans = 0, g_would_ride = 0, g_tails[3] = { 0, 0, 0 };

// a solve of three iterations under plan x: every evaluation is followed, before the next evaluation and before the end of the
// solve, by exactly one launch that runs cam_reduce_block in a kernel of its own, and no Schur kernel carries reductions
static void check_sequence(const Layout &L, int C, const ExecPlan &x, const ExecDevice &d)
{
    SeqState st;
    LaunchList q;
    int open = 0, evals = 0, reductions = 0;
    auto scan = [&] {
        for (int i = 0; i < q.n; ++i) {
            const Kern k = q.at[i].k;
            CHECK(!is_schur_ride(k));
            if (k == Kern::Eval) { CHECK(open == 0); open = 1; ++evals; }
            CHECK(k != Kern::ReduceControl);
            if (k == Kern::ReduceStats) { CHECK(open == 1); open = 0; ++reductions; CHECK(q.at[i].grid == reduction_blocks(L, C)); }
            if (is_schur(k) || k == Kern::FinishSolve || k == Kern::Control || k == Kern::FinalizeEval) CHECK(open == 0);
        }
    };
    seq_begin(L, C, x, Start::Init, st, q); scan();
    for (int it = 0; it < 3; ++it) { seq_iteration(L, C, x, d, 0, st, q); scan(); }
    seq_finish(L, C, st, q); scan();
    CHECK(open == 0 && evals == 4 && reductions == 4);
}

static bool C_small(int C) { return C <= kMaxCamLds; }

static void check_plans(Prob &q, const ExecDevice &d)
{
    const Layout L = q.plan();
    if (L.chunk_vb.empty()) return;
    for (int fp32 = 0; fp32 < 2; ++fp32)
        for (int flags = 0; flags <= TSCM_EXEC_ALL; ++flags) {
            if (flags & TSCM_EXEC_KEEP_SINGLE_RANK_COMM) continue;     // (no communicator: a sharded solver has no priors)
            for (int n_act : { 13 * q.C, 0 }) {
                const ExecPlan plain = plan_exec(L, q.C, n_act, kCommNone, flags, fp32, 0, 58, d);
                const ExecPlan sep = plan_exec(L, q.C, n_act, kCommNone, flags | TSCM_EXEC_SEPARATE_STATS, fp32, 0, 58, d);
                ExecPlan x = plan_exec(L, q.C, n_act, kCommNone, flags, fp32, 0, 58, d, false, true);
                CHECK(x.priors && !plain.priors && !sep.priors);
                CHECK(!x.stats_ride && x.tail != EvalTail::Ride);
                g_would_ride += plain.stats_ride;
                g_tails[x.tail == EvalTail::StatsThenHead ? 0 : C_small(q.C) ? 1 : 2] += 1;
                CHECK(x.tail == EvalTail::StatsThenHead || x.tail == EvalTail::Exchange);
                // ... and where k_reduce_control would run (which has no prior kernel): the reductions, k_finalize_eval, k_control
                ExecPlan same = x;
                same.priors = false;
                if (sep.tail == EvalTail::ReduceControl) { CHECK(x.tail == EvalTail::Exchange && !x.comm); same.tail = EvalTail::ReduceControl; }
                CHECK(std::memcmp(&same, &sep, sizeof(ExecPlan)) == 0);
                check_sequence(L, q.C, x, d);
                ++g_plans;
            }
        }
}

static int plan_mode(unsigned long long seed, int n_random)
{
    std::mt19937_64 rng(seed);
    for (int C = 1; C <= 32; ++C) {
        Prob q = ring(C, C == 1 ? 40 : 30 * C);
        check_plans(q, ample());
        ExecDevice d = ample();
        random_residency(rng, d);
        check_plans(q, d);
    }
    {   // boards seen by four cameras: the control step out of the Schur head (k_reduce_control)
        Prob q = ring(4, 400, 2);
        check_plans(q, ample());
    }
    for (int i = 0; i < n_random; ++i) {
        Prob q = random_problem(rng);
        ExecDevice d = ample();
        if (i & 1) random_residency(rng, d);
        check_plans(q, d);
    }
    std::printf("{\"ok\": %s, \"plans\": %ld, \"would_ride\": %ld, \"tails\": [%ld, %ld, %ld], \"why\": \"%s\"}\n", g_fail.empty() ? "true" : "false", g_plans,
                g_would_ride, g_tails[0], g_tails[1], g_tails[2], g_fail.c_str());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "refusals")) return refusals_mode();
    if (argc >= 2 && !std::strcmp(argv[1], "table")) return table_mode();
    if (argc >= 4 && !std::strcmp(argv[1], "effective")) return effective_mode(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc >= 4 && !std::strcmp(argv[1], "plan")) return plan_mode(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    std::fprintf(stderr, "usage: prior_check refusals | table | effective SEED N | plan SEED N\n");
    return 2;
}
