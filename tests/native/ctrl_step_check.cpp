// CPU check of the trust-region step (tscm_calib_amd/csrc/tscm_ctrl.h: lm_step), the one copy every LM route of the library
// runs.  Scripted scalar sequences drive it from the control block a solve starts with (ctrl_head_from_options); what the
// head and the log entry must hold afterwards is written here from Ceres' rules as oracle/tscm_oracle.c states them
// (orc_solve, "HandleInvalidStep" to "StepRejected"), as literals and closed forms.  Prints one JSON line; exit code 1 on a
// failure.
#include "../../tscm_calib_amd/csrc/tscm_ctrl.h"
#include "../../tscm_calib_amd/csrc/tscm_launch_seq.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace tscm;

namespace {

std::vector<std::string> failures, scenarios;
int checks = 0;

#define CHECK(cond) do { ++checks; if (!(cond)) failures.push_back(scenarios.back() + ":" + std::to_string(__LINE__) + ": " #cond); } while (0)

constexpr double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();

tscm_options defaults()
{
    tscm_options o{};
    o.struct_size = sizeof(o);
    o.max_num_iterations = 50; o.function_tolerance = 1e-6; o.gradient_tolerance = 1e-10; o.parameter_tolerance = 1e-8;
    o.initial_trust_region_radius = 1e4; o.max_trust_region_radius = 1e16; o.min_trust_region_radius = 1e-32;
    o.min_relative_decrease = 1e-3; o.min_lm_diagonal = 1e-6; o.max_lm_diagonal = 1e32;
    o.max_num_consecutive_invalid_steps = 5; o.jacobi_scaling = 1;
    return o;
}

struct Run {
    CtrlHead c;
    IterLog it;
    bool logged = false;
    explicit Run(const tscm_options &o = defaults()) : c(ctrl_head_from_options(o)) { start(); }
    // iteration 0 at cost 100, |g|_inf 5, |g| 7, |x| 10
    void start() { const StepInput in = { 100.0, 5.0, 7.0, 10.0, 0.0, 0.0 }; logged = lm_step(c, 1, c.cur, in, it); }
    // a candidate in the other buffer: cost, model cost change, with fresh norms that an acceptance must take over
    void step(double cost, double model, double step_norm = 1.0)
    {
        const StepInput in = { cost, 4.0, 6.0, 11.0, model, step_norm };
        it = IterLog{};
        logged = lm_step(c, 0, c.cur ^ 1, in, it);
    }
};

bool entry(const IterLog &it, int iteration, int valid, int ok, double cost, double change, double gmax, double gnorm, double step, double q, double radius)
{
    return it.iteration == iteration && it.step_is_valid == valid && it.step_is_successful == ok && it.pad == 0 && it.cost == cost && it.cost_change == change &&
           it.gradient_max_norm == gmax && it.gradient_norm == gnorm && it.step_norm == step && it.relative_decrease == q && it.radius == radius;
}

bool evaluator(const CtrlHead &c, double mn, double cur, double ref, double cand, double acc_ref, double acc_cand)
{
    return c.se_min == mn && c.se_cur == cur && c.se_ref == ref && c.se_cand == cand && c.se_acc_ref == acc_ref && c.se_acc_cand == acc_cand;
}

bool counts(const CtrlHead &c, int iteration, int n_log, int ok, int bad, int invalid)
{
    return c.iteration == iteration && c.lm_iterations == iteration && c.n_log == n_log && c.num_successful == ok && c.num_unsuccessful == bad &&
           c.num_invalid == invalid && c.lin_fail == 0;
}

bool ended(const CtrlHead &c, int type, int reason) { return c.done == 1 && c.term_type == type && c.term_reason == reason; }

void iteration_zero()
{
    scenarios.push_back("iteration_zero");
    Run r;
    CHECK(r.logged && entry(r.it, 0, 1, 1, 100.0, 0.0, 5.0, 7.0, 0.0, 0.0, 1e4));
    CHECK(r.c.x_cost == 100.0 && r.c.initial_cost == 100.0 && r.c.x_norm == 10.0 && r.c.gmax == 5.0 && r.c.gnorm == 7.0);
    CHECK(evaluator(r.c, 100.0, 100.0, 100.0, 100.0, 0.0, 0.0));
    CHECK(counts(r.c, 0, 1, 1, 0, 0) && r.c.done == 0 && r.c.cur == 0 && r.c.radius == 1e4 && r.c.decrease_factor == 2.0);
}

void accepted_steps()
{
    scenarios.push_back("accepted_steps");
    Run r;
    r.step(60.0, 40.0, 0.5);                        // quality (100 - 60) / 40 = 1: the radius grows by 1 / (1/3)
    CHECK(r.logged && entry(r.it, 1, 1, 1, 60.0, 40.0, 4.0, 6.0, 0.5, 1.0, 1e4 / (1.0 / 3.0)));
    CHECK(std::fabs(r.c.radius - 3e4) <= 1e-11 && r.c.cur == 1 && r.c.x_cost == 60.0 && r.c.x_norm == 11.0 && r.c.gmax == 4.0 && r.c.gnorm == 6.0);
    CHECK(evaluator(r.c, 60.0, 60.0, 60.0, 60.0, 0.0, 0.0) && counts(r.c, 1, 2, 2, 0, 0) && r.c.done == 0 && r.c.initial_cost == 100.0);
    r.step(70.0, 10.0);                             // rejected: decrease_factor 4
    CHECK(r.c.decrease_factor == 4.0 && r.c.cur == 1);
    const double r0 = r.c.radius;
    r.step(57.0, 12.0);                             // quality 3 / 12 = 0.25: w = -0.5, radius / (1 - w^3) = radius / 1.125
    CHECK(r.logged && entry(r.it, 3, 1, 1, 57.0, 3.0, 4.0, 6.0, 1.0, 0.25, r0 / 1.125));
    CHECK(r.c.radius == r0 / 1.125 && r.c.decrease_factor == 2.0 && r.c.cur == 0 && r.c.x_cost == 57.0);
    CHECK(evaluator(r.c, 57.0, 57.0, 57.0, 57.0, 0.0, 0.0) && counts(r.c, 3, 4, 3, 1, 0));
    tscm_options o = defaults();
    o.max_trust_region_radius = 2e4;
    Run capped(o);
    capped.step(60.0, 30.0);                        // quality 4 / 3: three times the radius is past max_radius
    CHECK(capped.it.relative_decrease == 40.0 / 30.0 && capped.c.radius == 2e4 && capped.it.radius == 2e4);
}

void rejected_steps()
{
    scenarios.push_back("rejected_steps");
    Run r;
    r.step(110.0, 10.0);
    CHECK(r.logged && entry(r.it, 1, 1, 0, 110.0, -10.0, 5.0, 7.0, 1.0, -1.0, 5e3));
    CHECK(r.c.radius == 5e3 && r.c.decrease_factor == 4.0 && r.c.cur == 0 && r.c.x_cost == 100.0 && r.c.x_norm == 10.0 && r.c.gmax == 5.0);
    r.step(120.0, 10.0);
    CHECK(r.logged && entry(r.it, 2, 1, 0, 120.0, -20.0, 5.0, 7.0, 1.0, -2.0, 1250.0));
    CHECK(r.c.radius == 1250.0 && r.c.decrease_factor == 8.0 && counts(r.c, 2, 3, 1, 2, 0));
    CHECK(evaluator(r.c, 100.0, 100.0, 100.0, 100.0, 0.0, 0.0));
    r.step(90.0, 20.0);                             // quality 0.5: radius unchanged (1 - 0^3), decrease_factor back to 2
    CHECK(r.it.step_is_successful == 1 && r.c.radius == 1250.0 && r.c.decrease_factor == 2.0);
    r.step(95.0, 10.0);
    CHECK(r.it.step_is_successful == 0 && r.c.radius == 625.0 && r.c.decrease_factor == 4.0 && counts(r.c, 4, 5, 2, 3, 0));
}

void invalid_steps()
{
    scenarios.push_back("invalid_steps");
    Run r;
    const double models[4] = { 10.0, kNaN, -1.0, 0.0 };     // the first with a failed factorisation
    double radius = 1e4;
    for (int i = 0; i < 4; ++i) {
        r.c.lin_fail = i == 0;
        r.step(50.0, models[i]);
        radius /= (double)(2 << i);
        CHECK(r.logged && entry(r.it, i + 1, 0, 0, 100.0, 0.0, 5.0, 7.0, 0.0, 0.0, radius));
        CHECK(r.c.radius == radius && r.c.decrease_factor == (double)(4 << i) && counts(r.c, i + 1, i + 2, 1, i + 1, i + 1) && r.c.done == 0 && r.c.cur == 0);
    }
    const CtrlHead before = r.c;
    r.step(50.0, 10.0, kInf);                               // the fifth in a row: no log entry, no step counted
    CHECK(!r.logged && ended(r.c, 2, kInvalidSteps) && r.c.num_invalid == 5 && r.c.iteration == 5 && r.c.lm_iterations == 5);
    CHECK(r.c.n_log == before.n_log && r.c.num_unsuccessful == before.num_unsuccessful && r.c.radius == before.radius && r.c.x_cost == 100.0);
    Run s;
    s.step(50.0, -1.0);
    s.step(50.0, -1.0);
    s.step(110.0, 10.0);                                    // a valid step ends the streak
    CHECK(s.it.step_is_valid == 1 && counts(s.c, 3, 4, 1, 3, 0) && s.c.radius == 1e4 / 2.0 / 4.0 / 8.0);
}

void non_finite_cost()
{
    scenarios.push_back("non_finite_cost");
    for (double cost : { kInf, kNaN }) {
        Run r;
        r.step(cost, 10.0);
        CHECK(r.logged && entry(r.it, 1, 1, 0, DBL_MAX, 100.0 - DBL_MAX, 5.0, 7.0, 1.0, -DBL_MAX, 5e3));
        CHECK(r.c.x_cost == 100.0 && r.c.cur == 0 && r.c.done == 0 && counts(r.c, 1, 2, 1, 1, 0));
    }
}

// From iteration 0 every accepted step lowers the cost, so the reference cost never leaves the current one and both
// quotients are equal.  The state in which they differ (Ceres' evaluator after tolerated non-monotonic steps) is set here.
void history_branch()
{
    scenarios.push_back("history_branch");
    Run r;
    r.c.x_cost = 60.0; r.c.se_min = 55.0; r.c.se_cur = 60.0; r.c.se_ref = 80.0; r.c.se_cand = 80.0; r.c.se_acc_ref = 10.0; r.c.se_acc_cand = 10.0;
    r.step(62.0, 5.0);                              // rel = (60 - 62) / 5 < 0 refuses, hist = (80 - 62) / (10 + 5) = 1.2 accepts
    CHECK(r.logged && entry(r.it, 1, 1, 1, 62.0, -2.0, 4.0, 6.0, 1.0, 18.0 / 15.0, 1e4 / (1.0 / 3.0)));
    CHECK(r.c.cur == 1 && r.c.x_cost == 62.0 && evaluator(r.c, 55.0, 62.0, 80.0, 80.0, 15.0, 15.0));
    r.c.se_cur = 60.0; r.c.se_ref = 60.0; r.c.se_acc_ref = 0.0; r.c.x_cost = 60.0;
    r.step(62.0, 5.0);                              // without the history the same candidate is refused
    CHECK(r.it.step_is_successful == 0 && r.it.relative_decrease == -0.4 && r.c.cur == 1);
    r.c.se_min = 50.0; r.c.se_cur = 60.0; r.c.se_ref = 60.0; r.c.se_cand = 55.0; r.c.se_acc_ref = 0.0; r.c.se_acc_cand = 7.0;
    r.step(58.0, 4.0);                              // accepted above the candidate cost: it becomes the candidate and the reference
    CHECK(r.it.step_is_successful == 1 && evaluator(r.c, 50.0, 58.0, 58.0, 58.0, 0.0, 0.0));
}

void exits()
{
    scenarios.push_back("exits");
    {
        Run r;
        const CtrlHead before = r.c;
        r.step(90.0, 20.0, 1e-9);                   // 1e-9 <= 1e-8 (10 + 1e-8)
        CHECK(!r.logged && ended(r.c, 0, kParamTol) && r.c.n_log == 1 && r.c.num_successful == 1 && r.c.num_unsuccessful == 0 && r.c.iteration == 1);
        CHECK(r.c.cur == 0 && r.c.x_cost == 100.0 && r.c.radius == before.radius && r.c.decrease_factor == 2.0);
    }
    {
        Run r;
        r.step(100.0 - 5e-5, 20.0);                 // |change| 5e-5 <= 1e-6 * 100
        CHECK(!r.logged && ended(r.c, 0, kFuncTol) && r.c.n_log == 1 && r.c.num_successful == 1 && r.c.num_unsuccessful == 0 && r.c.iteration == 1);
        CHECK(r.c.cur == 0 && r.c.x_cost == 100.0 && r.c.radius == 1e4);
    }
    {
        tscm_options o = defaults();
        o.max_num_iterations = 2;
        Run r(o);
        r.step(90.0, 20.0);
        CHECK(r.logged && r.c.done == 0);
        r.step(95.0, 20.0);                         // a rejected step is logged and counted, then the limit
        CHECK(r.logged && ended(r.c, 1, kMaxIter) && counts(r.c, 2, 3, 2, 1, 0) && r.it.iteration == 2);
    }
    {
        Run r;
        r.c.opt.gradient_tolerance = 4.5;           // between the norm of the start point (5) and of the candidates (4)
        r.step(110.0, 10.0);                        // rejected: the norm in the entry is the start point's
        CHECK(r.logged && r.c.done == 0);
        r.c.opt.gradient_tolerance = 5.5;
        r.step(110.0, 10.0);                        // rejected below the tolerance: not an exit
        CHECK(r.logged && r.c.done == 0 && r.it.gradient_max_norm == 5.0);
        r.c.opt.gradient_tolerance = 4.5;
        r.step(90.0, 20.0);
        CHECK(r.logged && ended(r.c, 0, kGradTol) && r.it.gradient_max_norm == 4.0 && r.c.cur == 1 && counts(r.c, 3, 4, 2, 2, 0));
        tscm_options o = defaults();
        o.gradient_tolerance = 5.0;
        Run z(o);                                   // the start point already meets it
        CHECK(z.logged && ended(z.c, 0, kGradTol) && counts(z.c, 0, 1, 1, 0, 0));
    }
    {
        tscm_options o = defaults();
        o.min_trust_region_radius = 3e3;
        Run r(o);
        r.step(110.0, 10.0);
        CHECK(r.logged && r.c.done == 0 && r.c.radius == 5e3);
        r.step(110.0, 10.0);
        CHECK(r.logged && ended(r.c, 0, kMinRadius) && r.c.radius == 1250.0 && r.it.radius == 1250.0 && counts(r.c, 2, 3, 1, 2, 0));
    }
    {
        // free columns without a Jacobian (b, c): their pivot clamp(0) / radius is 0 with min_lm_diagonal = 0, and the step invalid
        const unsigned short held[2] = { 128 | 256, 128 | 256 }, one[2] = { 128 | 256, 128 };
        const unsigned char idle1[2] = { 1, 0 };
        CHECK(has_inert_columns(nullptr, nullptr, 2) && !has_inert_columns(held, nullptr, 2) && has_inert_columns(one, nullptr, 2) && !has_inert_columns(one, idle1, 2));
        // all of fx .. alpha held: the block is constant and b, c leave the program with it
        const unsigned short block[2] = { 127, 127 | 128 }, part[2] = { 127, 126 };
        CHECK(!has_inert_columns(block, nullptr, 2) && has_inert_columns(part, nullptr, 2) && !has_inert_columns(part, idle1, 2));
        tscm_options o = defaults();
        o.min_lm_diagonal = 0.0;
        Run r(o);
        r.step(90.0, 20.0);                         // the program has no such column: a good step
        CHECK(r.logged && r.it.step_is_valid == 1 && r.it.step_is_successful == 1);
        r.c.inert_cols = 1;
        r.step(80.0, 20.0);
        CHECK(r.logged && r.it.step_is_valid == 0 && r.c.num_invalid == 1 && r.c.x_cost == 90.0);
        r.c.opt.min_lm_diagonal = 1e-6;
        r.step(80.0, 20.0);
        CHECK(r.logged && r.it.step_is_valid == 1 && r.it.step_is_successful == 1 && r.c.num_invalid == 0);
    }
}

}  // namespace

int main()
{
    iteration_zero();
    accepted_steps();
    rejected_steps();
    invalid_steps();
    non_finite_cost();
    history_branch();
    exits();
    std::printf("{\"ok\": %d, \"checks\": %d, \"scenarios\": [", failures.empty() ? 1 : 0, checks);
    for (size_t i = 0; i < scenarios.size(); ++i) std::printf("%s\"%s\"", i ? ", " : "", scenarios[i].c_str());
    std::printf("], \"failures\": [");
    for (size_t i = 0; i < failures.size(); ++i) std::printf("%s\"%s\"", i ? ", " : "", failures[i].c_str());
    std::printf("]}\n");
    return failures.empty() ? 0 : 1;
}
