// CPU check of tscm_calib_amd/csrc/tscm_spec.h: make_spec and check_corner_weights answer every single fault with their code
// and text, and scatter_weights agrees with a brute-force loop on random ragged problems -- a solver's layout that keeps a
// permuted subset of the views, and a batch's slot order over problems with and without weights.
//   spec_check refusals       -> {"name": [code, "text"], ...}
//   spec_check loss           -> {"ok": bool, "why": "..."}
//   spec_check scatter SEED N -> {"ok": bool, "cases": N, "empty_views": n, "subsets": n, "masked_nan": n, "unweighted": n, "why": "..."}
// Built by tests/test_spec_native.py, plain and under AddressSanitizer + UBSan.
#include "../../tscm_calib_amd/csrc/tscm_spec.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

using namespace tscm;

static bool g_fail = false;
static std::string g_why;
static void check(bool ok, const std::string &why) { if (!ok && !g_fail) { g_fail = true; g_why = why; } }

static int refusals_mode()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::printf("{");
    bool first = true;
    auto put = [&](const char *name, int rc, const std::string &err) {
        std::printf("%s\"%s\": [%d, \"%s\"]", first ? "" : ", ", name, rc, rc ? err.c_str() : "");
        first = false;
    };
    auto spec = [&](const char *name, int kind, double scale, const unsigned short *fixed, int n) {
        SolveSpec s = spec_args(TSCM_LOSS_NONE, 0.0, nullptr, nullptr);
        const SolveSpec before = s;
        std::string err;
        const int rc = make_spec(kind, scale, fixed, n, s, err);
        if (rc) check(std::memcmp(&s, &before, sizeof(s)) == 0, std::string(name) + ": a refusal wrote the spec");
        else check(s.fixed == fixed && s.weights == nullptr && s.loss.kind == kind, std::string(name) + ": spec fields");
        put(name, rc, err);
    };
    const unsigned short good[3] = { 0, TSCM_FIX_ALL, TSCM_MODEL_UCM }, bad[3] = { 0, TSCM_FIX_CX, 1u << 9 };
    spec("ok_none", TSCM_LOSS_NONE, 0.0, nullptr, 3);
    spec("ok_none_any_scale", TSCM_LOSS_NONE, nan, good, 3);       // the scale of no loss is not looked at
    spec("ok_cauchy", TSCM_LOSS_CAUCHY, 2.0, good, 3);
    spec("kind_low", -1, 1.0, nullptr, 3);
    spec("kind_high", TSCM_LOSS_CAUCHY + 1, 1.0, nullptr, 3);
    spec("scale_zero", TSCM_LOSS_HUBER, 0.0, nullptr, 3);
    spec("scale_negative", TSCM_LOSS_SOFT_L1, -1.0, nullptr, 3);
    spec("scale_nan", TSCM_LOSS_CAUCHY, nan, nullptr, 3);
    spec("scale_inf", TSCM_LOSS_HUBER, inf, nullptr, 3);
    spec("mask_bits", TSCM_LOSS_NONE, 0.0, bad, 3);
    spec("mask_bits_beyond_n", TSCM_LOSS_NONE, 0.0, bad, 2);        // (only n_cameras words are read)
    // a ragged problem: views of 3, 0, 2, 4 corners
    const int count[4] = { 3, 0, 2, 4 };
    auto weights = [&](const char *name, std::vector<double> w, double want_sum, long want_kept) {
        std::string err;
        double sum = -1.0;
        long kept = -1;
        const int rc = check_corner_weights(count, 4, w.data(), err, &sum, &kept);
        if (rc) check(sum == -1.0 && kept == -1, std::string(name) + ": a refusal wrote sum / kept");
        else check(sum == want_sum && kept == want_kept, std::string(name) + ": sum / kept");
        put(name, rc, err);
    };
    weights("w_ok", { 1, 0, 2, 0.5, 0, 1, 1, 1, 0.25 }, 6.75, 7);
    weights("w_negative", { 1, 0, 2, 0.5, 0, 1, -1, 1, 1 }, 0, 0);             // corner 6 = view 3, corner 1
    weights("w_nan", { 1, 0, 2, 0.5, nan, 1, 1, 1, 1 }, 0, 0);                  // corner 4 = view 2, corner 1
    weights("w_inf", { 1, 0, inf, 0.5, 1, 1, 1, 1, 1 }, 0, 0);                  // corner 2 = view 0, corner 2
    weights("w_view_all_zero", { 1, 0, 2, 0, 0, 1, 1, 1, 1 }, 0, 0);            // view 2
    std::printf(", \"ok\": %s, \"why\": \"%s\"}\n", g_fail ? "false" : "true", g_why.c_str());
    return 0;
}

static int loss_mode()
{
    for (int kind = TSCM_LOSS_HUBER; kind <= TSCM_LOSS_CAUCHY; ++kind)
        for (double a : { 0.125, 1.0, 1.5, 3.0, 1e-3, 7e5 }) {
            SolveSpec s = spec_args(TSCM_LOSS_NONE, -1.0, nullptr, nullptr);
            std::string err;
            check(make_spec(kind, a, nullptr, 0, s, err) == 0, "a loss refused");
            check(s.loss.kind == kind && s.loss.a == a && s.loss.b == a * a && s.loss.c == 1.0 / (a * a), "loss constants: b = a^2, c = 1 / b");
        }
    SolveSpec s = spec_args(TSCM_LOSS_HUBER, -1.0, nullptr, nullptr);
    std::string err;
    check(make_spec(TSCM_LOSS_NONE, 5.0, nullptr, 0, s, err) == 0 && s.loss.kind == 0 && s.loss.a == 0.0 && s.loss.b == 0.0 && s.loss.c == 0.0, "no loss carries zeros");
    std::printf("{\"ok\": %s, \"why\": \"%s\"}\n", g_fail ? "false" : "true", g_why.c_str());
    return 0;
}

// one random ragged problem: view counts (some 0), observations, weights (some 0, on NaN observations too)
struct Prob {
    std::vector<int> count;
    std::vector<long> first;            // view -> first corner in corner order
    std::vector<double> u, v, w;        // corner order
    bool weighted = true;
};
static Prob make(std::mt19937 &rng, long &empty_views, long &masked_nan)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Prob p;
    const int V = 1 + (int)(rng() % 9);
    long n = 0;
    for (int i = 0; i < V; ++i) {
        const int c = rng() % 4 == 0 ? 0 : 1 + (int)(rng() % 7);
        if (!c) ++empty_views;
        p.count.push_back(c); p.first.push_back(n); n += c;
    }
    for (long k = 0; k < n; ++k) {
        const bool masked = rng() % 4 == 0, hole = masked && rng() % 2 == 0;
        p.w.push_back(masked ? 0.0 : 0.25 * (1 + rng() % 8));
        p.u.push_back(hole ? nan : 1.0 + (double)(rng() % 1000)); p.v.push_back(hole ? nan : 1.0 + (double)(rng() % 1000));
        if (hole) ++masked_nan;
    }
    return p;
}

// the brute force: every device corner looks its own source corner up
static void compare(const std::vector<const Prob *> &src, const std::vector<std::vector<CornerRun>> &runs, long N, const char *what)
{
    // the observations as created: gathered into device order; -7 where no run writes (must stay)
    std::vector<double> u0(N, -7.0), v0(N, -7.0);
    for (size_t q = 0; q < src.size(); ++q)
        for (const CornerRun &r : runs[q])
            for (int j = 0; j < r.count; ++j) { u0[r.first + j] = src[q]->u[src[q]->first[r.view] + j]; v0[r.first + j] = src[q]->v[src[q]->first[r.view] + j]; }
    std::vector<double> w(N, -7.0), u(u0), v(v0);
    for (size_t q = 0; q < src.size(); ++q)
        scatter_weights(src[q]->weighted ? src[q]->w.data() : nullptr, src[q]->count.data(), (int)src[q]->count.size(), runs[q], w.data(), u.data(), v.data());
    std::vector<double> we(N, -7.0), ue(u0), ve(v0);
    for (long k = 0; k < N; ++k)
        for (size_t q = 0; q < src.size(); ++q)
            for (const CornerRun &r : runs[q]) {
                if (k < r.first || k >= r.first + r.count) continue;
                const double x = src[q]->weighted ? src[q]->w[src[q]->first[r.view] + (k - r.first)] : 1.0;
                we[k] = x;
                if (!(x > 0.0)) { ue[k] = 0.0; ve[k] = 0.0; }
            }
    // byte for byte: a kept corner keeps its observation, a masked one is exactly +0, +0 -- no NaN survives under weight 0
    auto same = [&](const std::vector<double> &a, const std::vector<double> &b) { return N == 0 || std::memcmp(a.data(), b.data(), sizeof(double) * N) == 0; };
    check(same(w, we), std::string(what) + ": weights");
    check(same(u, ue) && same(v, ve), std::string(what) + ": observations");
    for (long k = 0; k < N; ++k) if (we[k] == 0.0) check(u[k] == 0.0 && v[k] == 0.0 && !std::signbit(u[k]) && !std::signbit(v[k]), std::string(what) + ": a masked corner is not 0, 0");
}

static int scatter_mode(unsigned seed, int cases)
{
    std::mt19937 rng(seed);
    long empty_views = 0, subsets = 0, masked_nan = 0, unweighted = 0;
    for (int c = 0; c < cases; ++c) {
        {   // a solver's layout: a shuffled subset of the views with corners (a shard), device corners in that order, with a gap
            const Prob p = make(rng, empty_views, masked_nan);
            std::vector<int> keep;
            for (int i = 0; i < (int)p.count.size(); ++i) if (p.count[i] > 0 && rng() % 3 != 0) keep.push_back(i);
            std::shuffle(keep.begin(), keep.end(), rng);
            if (keep.size() < p.count.size()) ++subsets;
            std::vector<CornerRun> runs;
            long at = 0;
            for (int i : keep) { runs.push_back(CornerRun{ i, at, p.count[i] }); at += p.count[i] + (rng() % 4 == 0 ? 1 : 0); }
            compare({ &p }, { runs }, at, "layout");
        }
        {   // a batch: several problems' views as slots of one concatenated corner order; some problems carry no weights
            const int K = 1 + (int)(rng() % 5);
            std::vector<Prob> ps;
            for (int k = 0; k < K; ++k) { ps.push_back(make(rng, empty_views, masked_nan)); ps.back().weighted = rng() % 3 != 0; if (!ps.back().weighted) ++unweighted; }
            std::vector<const Prob *> src;
            std::vector<std::vector<CornerRun>> runs(K);
            long at = 0;
            for (int k = 0; k < K; ++k) {
                src.push_back(&ps[k]);
                std::vector<int> order;
                for (int i = 0; i < (int)ps[k].count.size(); ++i) if (ps[k].count[i] > 0) order.push_back(i);
                std::shuffle(order.begin(), order.end(), rng);          // (board order, not view order)
                for (int i : order) { runs[k].push_back(CornerRun{ i, at, ps[k].count[i] }); at += ps[k].count[i]; }
            }
            compare(src, runs, at, "batch");
        }
    }
    std::printf("{\"ok\": %s, \"cases\": %d, \"empty_views\": %ld, \"subsets\": %ld, \"masked_nan\": %ld, \"unweighted\": %ld, \"why\": \"%s\"}\n",
                g_fail ? "false" : "true", cases, empty_views, subsets, masked_nan, unweighted, g_why.c_str());
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "refusals") return refusals_mode();
    if (mode == "loss") return loss_mode();
    if (mode == "scatter" && argc == 4) return scatter_mode((unsigned)std::atoi(argv[2]), std::atoi(argv[3]));
    std::fprintf(stderr, "usage: spec_check refusals | loss | scatter SEED CASES\n");
    return 2;
}
