// CPU check of the reduced system's column plan (tscm_calib_amd/csrc/tscm_columns.h): random problems -- 1 to 32 cameras
// and mono, cameras without views, cameras whose pose is held -- are planned with plan_layout and then with plan_columns
// under held-intrinsics masks (none, all held, DS, UCM, cx_cy, a different mask per camera).  Every table is re-derived here
// from the problem and DESIGN 15's rules, not from the planner's code: the column classes, the compact numbering and its
// kernel-argument form, the contiguous tables and k_solve_nd plans without a mask, monotonicity in the mask, and
// k_solve_reduced's operand map read on operands tagged with their (row, column).  Host logic only (no GPU).
//   usage: columns_check random <seed> <problems>     one JSON line: counts of what the problems exercised
#include "../../tscm_calib_amd/csrc/tscm_layout.h"
#include "../../tscm_calib_amd/csrc/tscm_columns.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace tscm;

// a problem's view tables and held poses (the parameter arrays only need to be non-NULL: the plan does not read them)
struct Prob {
    int C = 1, B = 0, n_points = 1, mono = 0;
    std::vector<int> cam, board, offset, count;
    std::vector<unsigned char> cconst;
    double dummy[2] = { 0.0, 0.0 };
    tscm_problem p{};
    const tscm_problem *get()
    {
        p = tscm_problem{};
        p.n_cameras = C; p.n_boards = B; p.n_points = n_points; p.n_views = (int)cam.size(); p.mono = mono;
        p.board_xy = dummy; p.intr = dummy; p.board_rt = dummy; p.cam_rt = dummy; p.obs_u = dummy; p.obs_v = dummy;
        p.view_camera = cam.data(); p.view_board = board.data(); p.view_offset = offset.data(); p.view_count = count.data();
        p.cam_pose_constant = cconst.empty() ? nullptr : cconst.data();
        return &p;
    }
    void add(int c, int b, int n) { offset.push_back(offset.empty() ? 0 : offset.back() + count.back()); cam.push_back(c); board.push_back(b); count.push_back(n); }
};

static std::string g_fail;
#define CHECK(cond) do { if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; } while (0)

static Prob random_problem(std::mt19937_64 &rng)
{
    auto uni = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
    Prob q;
    q.mono = uni(0, 5) == 0;
    q.C = q.mono ? 1 : uni(0, 2) == 0 ? uni(1, 32) : uni(1, 8);
    q.n_points = uni(4, 60);
    q.B = uni(0, 40);
    // cameras without views: never picked for a board (and now and then a view without corners)
    std::vector<int> alive;
    for (int m = 0; m < q.C; ++m) if (uni(0, 4) > 0) alive.push_back(m);
    for (int b = 0; b < q.B && !alive.empty(); ++b) {
        std::shuffle(alive.begin(), alive.end(), rng);
        const int k = std::min<int>((int)alive.size(), uni(0, 9) == 0 ? uni(4, 8) : uni(0, 3));
        for (int i = 0; i < k; ++i) q.add(alive[i], b, uni(0, 19) == 0 ? 0 : uni(1, q.n_points));
    }
    if (uni(0, 1)) { q.cconst.resize(q.C); for (auto &x : q.cconst) x = uni(0, 2) == 0; }
    return q;
}

// the mask words of one kind: 0 none (NULL), 1 all held, 2 DS, 3 UCM, 4 cx_cy, 5 a different mask per camera
constexpr int kMaskKinds = 6;
static std::vector<unsigned short> masks(int kind, int C, std::mt19937_64 &rng)
{
    auto uni = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
    std::vector<unsigned short> f(C, 0);
    for (int m = 0; m < C; ++m)
        f[m] = kind == 1 ? (uni(0, 1) ? TSCM_FIX_INTRINSICS : TSCM_FIX_ALL) : kind == 2 ? TSCM_MODEL_DS : kind == 3 ? TSCM_MODEL_UCM
             : kind == 4 ? (TSCM_FIX_CX | TSCM_FIX_CY) : kind == 5 ? (unsigned short)uni(0, TSCM_FIX_ALL) : 0;
    return f;
}

static bool same_plan(const NdPlan &a, const NdPlan &b)
{
    bool tiles = a.tiles.size() == b.tiles.size();
    for (size_t i = 0; tiles && i < a.tiles.size(); ++i)
        tiles = a.tiles[i].ri == b.tiles[i].ri && a.tiles[i].cj == b.tiles[i].cj && a.tiles[i].kind == b.tiles[i].kind && a.tiles[i].lt == b.tiles[i].lt;
    return tiles && a.NP == b.NP && a.n_phases == b.n_phases && a.max_slots == b.max_slots && a.n_lt == b.n_lt && a.tpt == b.tpt &&
           a.dense == b.dense && a.levels == b.levels && a.pcol == b.pcol && a.lmask == b.lmask && a.rowstart == b.rowstart &&
           a.phase_of == b.phase_of && a.slot_of == b.slot_of && a.phase_panels == b.phase_panels && a.tab == b.tab &&
           a.bs_rounds == b.bs_rounds && a.bs_tab == b.bs_tab && a.map == b.map && a.lds_doubles == b.lds_doubles;
}

static long g_count[16];
enum { C_PLANS, C_MONO, C_BIG, C_DENSE4, C_ND, C_EMPTY, C_HOLES, C_NO_VIEWS, C_POSE_HELD, C_RHS_TILES, C_REFUSED };

// facts of the problem itself (not of the layout): camera m has a view with corners / its pose is held
struct Facts { std::vector<bool> views, held; };
static Facts facts(const tscm_problem *p)
{
    Facts f{ std::vector<bool>(p->n_cameras, false), std::vector<bool>(p->n_cameras, false) };
    for (int v = 0; v < p->n_views; ++v) if (p->view_count[v] > 0) f.views[p->view_camera[v]] = true;
    for (int m = 0; m < p->n_cameras; ++m) f.held[m] = p->mono || (p->cam_pose_constant && p->cam_pose_constant[m]);
    return f;
}

// k_solve_reduced's operand map (rigs of <= kDense4Cams cameras), read on H and T tagged with the (row, column) of each entry
static void check_solve_map(const ColumnPlan &c, const Layout &L, int C)
{
    constexpr int NT = kSolveMapThreads, G = 16;
    CHECK((int)c.solve_map.size() == kSolveMapSlots / 4 * NT);
    if (!g_fail.empty()) return;
    auto tag = [](int i, int j) { return (double)(1 + 1024 * i + j); };
    // H: the camera tiles, T: one tile per camera pair with a block (mi <= mj), both tagged by padded (row, column)
    std::vector<double> H((size_t)256 * C), T((size_t)256 * std::max(1, L.n_bids), -1.0);
    for (int m = 0; m < C; ++m) for (int a = 0; a < 16; ++a) for (int b = 0; b < 16; ++b) H[256 * m + 16 * a + b] = tag(16 * m + a, 16 * m + b);
    for (int mi = 0; mi < C; ++mi)
        for (int mj = mi; mj < C; ++mj) {
            const int bid = L.bid_of[mi * C + mj];
            if (bid >= 0) for (int a = 0; a < 16; ++a) for (int b = 0; b < 16; ++b) T[256 * bid + 16 * a + b] = tag(16 * mi + a, 16 * mj + b);
        }
    auto pair_tile = [&](int i, int j) { return L.bid_of[std::min(i >> 4, j >> 4) * C + std::max(i >> 4, j >> 4)]; };
    auto t_tag = [&](int i, int j) { return (i >> 4) <= (j >> 4) ? tag(i, j) : tag(j, i); };     // the lower blocks are the transposed upper ones
    auto read = [&](const std::vector<double> &X, int off) { return off >= 0 && off < (int)X.size() ? X[off] : -2.0; };
    const int NP = (c.n_act + 3) / 4;
    auto col = [&](int ci) { return ci < c.n_act ? c.act_map[ci] : -1; };
    // the right-hand side tiles, derived as stated: the threads without a matrix tile, counted down from the end of the wave of
    // tile (NP - 1, NP - 1) (never the look-ahead thread NT - 1), take tiles (NP, NP - 1), (NP, NP - 2), ..., (NP, 0)
    std::vector<int> rhs_of(NT, -1);
    if (NP > 0) {
        int p = NP - 1;
        for (int u = std::min(NT - 2, ((NP - 1) * G + NP - 1) | 63); u >= 0 && p >= 0; --u)
            if (!(u % G <= u / G && u / G < NP)) rhs_of[u] = p--;
        CHECK(p < 0);
    }
    std::vector<int> owners((size_t)(NP + 1) * (NP + 1), 0);
    for (int tid = 0; tid < NT; ++tid) {
        int off[kSolveMapSlots];
        for (int q = 0; q < kSolveMapSlots / 4; ++q) {
            const Int4 v = c.solve_map[(size_t)q * NT + tid];
            off[4 * q] = v.x; off[4 * q + 1] = v.y; off[4 * q + 2] = v.z; off[4 * q + 3] = v.w;
        }
        const int ri = off[kMapTile], cj = off[kMapTile + 1], kind = off[kMapTile + 2];
        CHECK(off[kMapTile + 3] == -1);
        const bool matrix = tid % G <= tid / G && tid / G < NP;
        CHECK(kind == (matrix ? 1 : rhs_of[tid] >= 0 ? 2 : 0));
        if (tid == NT - 1) CHECK(kind == 0);
        if (kind == 1) {
            // lower tile (ti, tj) of the matrix on thread ti * G + tj
            CHECK(ri == tid / G && cj == tid % G && cj <= ri && ri < NP);
            owners[(size_t)ri * (NP + 1) + cj]++;
            for (int r = 0; r < 4; ++r) {
                const int i = col(4 * ri + r);
                CHECK(off[kMapSci + r] == i && off[kMapScj + r] == col(4 * cj + r));
                for (int q = 0; q < 4; ++q) {
                    const int j = col(4 * cj + q), oh = off[kMapH + 4 * r + q], ot = off[kMapT + 4 * r + q];
                    const bool h_there = i >= 0 && j >= 0 && (i >> 4) == (j >> 4), t_there = i >= 0 && j >= 0 && pair_tile(i, j) >= 0;
                    CHECK(h_there ? read(H, oh) == tag(i, j) : oh == -1);
                    CHECK(t_there ? read(T, ot) == t_tag(i, j) : ot == -1);
                }
            }
        } else if (kind == 2) {
            // right-hand side tile (NP, p): row 0 is column kFR of the panel's columns, scaling 1
            CHECK(ri == NP && cj == rhs_of[tid] && cj >= 0 && cj < NP);
            if (ri == NP && cj >= 0 && cj < NP) owners[(size_t)NP * (NP + 1) + cj]++;
            CHECK(off[kMapSci] == kMapOne && off[kMapSci + 1] == -1 && off[kMapSci + 2] == -1 && off[kMapSci + 3] == -1);
            for (int q = 0; q < 4; ++q) {
                const int j = col(4 * cj + q), g = 16 * (j >> 4) + kColGrad;
                CHECK(off[kMapScj + q] == j);
                CHECK(j >= 0 ? read(H, off[kMapH + q]) == tag(j, g) : off[kMapH + q] == -1);
                CHECK(j >= 0 && pair_tile(j, j) >= 0 ? read(T, off[kMapT + q]) == tag(j, g) : off[kMapT + q] == -1);
            }
            for (int e = 4; e < 16; ++e) CHECK(off[kMapH + e] == -1 && off[kMapT + e] == -1);
            g_count[C_RHS_TILES]++;
        } else {
            // a thread without a tile: its grid position, nothing else
            CHECK(ri == tid / G && cj == tid % G);
            for (int e = 0; e < kMapTile; ++e) CHECK(off[e] == -1);
        }
    }
    // every lower tile of the NP panels and every right-hand side tile: exactly one owner
    for (int ri = 0; ri <= NP; ++ri) for (int cj = 0; cj <= std::min(ri, NP - 1); ++cj) CHECK(owners[(size_t)ri * (NP + 1) + cj] == 1);
}

// one plan against the rules; none: the plan of the same problem without a mask (null on the unmasked plan itself)
static void check_columns(const tscm_problem *p, const Layout &L, const unsigned short *fixed, const ColumnPlan &c, const ColumnPlan *none)
{
    const int C = p->n_cameras, n_pad = 16 * C;
    const Facts fa = facts(p);
    CHECK((int)c.col_active.size() == n_pad && (int)c.col_ctl.size() == 16 * kMaxCam && (int)c.act_map.size() == n_pad);
    if (!g_fail.empty()) return;
    // the classes: a column of a camera with views is free unless it is padding (a >= 13), a held pose (a < 6) or a held
    // intrinsic; it counts in |x| if its block is part of the program: the pose unless held, the nine intrinsics unless all
    // seven of the model are held (the block is then constant)
    int n_act = 0;
    for (int i = 0; i < 16 * kMaxCam; ++i) {
        if (i >= n_pad) { CHECK(c.col_ctl[i] == 0); continue; }
        const int m = i / 16, a = i % 16;
        const unsigned f = fixed ? fixed[m] : 0u;
        const bool pose = a < 6, intr = a >= 6 && a < 15;
        const bool held_intr = intr && a < 13 && (f >> (a - 6)) & 1u, all_seven = (f & 127u) == 127u;
        const bool free_col = fa.views[m] && a < 13 && !(pose && fa.held[m]) && !held_intr;
        const bool in_x = fa.views[m] && ((pose && !fa.held[m]) || (intr && !all_seven));
        CHECK(c.col_active[i] == (free_col ? 1 : 0));
        CHECK(c.col_ctl[i] == (in_x ? 1 : 0) + (free_col ? 2 : 0));
        if (fa.held[m] && pose) CHECK(!c.col_active[i]);
        if (all_seven && intr) CHECK(!c.col_active[i] && !(c.col_ctl[i] & 1));
        n_act += free_col;
    }
    // the compact numbering: strictly increasing, exactly the free columns, then -1
    CHECK(c.n_act == n_act);
    for (int ci = 0; ci < n_pad; ++ci) {
        if (ci < n_act) { const int i = c.act_map[ci]; CHECK(i >= 0 && i < n_pad && c.col_active[i] && (ci == 0 || c.act_map[ci - 1] < i)); }
        else CHECK(c.act_map[ci] == -1);
    }
    if (!g_fail.empty()) return;
    // ... as kernel arguments: camera q's free columns are compact [cam_pre[q], cam_pre[q + 1]), 16 q + the set bits of cam_free[q]
    for (int q = 0; q < 9; ++q) if (C > kMaxCamLds || q >= C) CHECK(c.cam_pre[q] == n_act);
    for (int q = 0; q < 8; ++q) if (C > kMaxCamLds || q >= C) CHECK(c.cam_free[q] == 0);
    if (C <= kMaxCamLds) {
        for (int q = 0; q < C; ++q) {
            unsigned word = 0;
            for (int a = 0; a < 16; ++a) if (c.col_active[16 * q + a]) word |= 1u << a;
            CHECK(c.cam_free[q] == word);
            if (word & (word + (word & -word))) g_count[C_HOLES]++;                  // not one run of set bits
        }
        for (int ci = 0; ci < n_act; ++ci) {
            int q = 0;
            while (q + 1 < kMaxCamLds && ci >= c.cam_pre[q + 1]) ++q;              // the last camera that starts at or before ci
            int k = ci - c.cam_pre[q], bit = -1;
            for (int b = 0; b < 16 && bit < 0; ++b) if ((c.cam_free[q] >> b) & 1u) { if (k == 0) bit = b; else --k; }
            CHECK(bit >= 0 && 16 * q + bit == c.act_map[ci]);
        }
    }
    // the reduced solvers' tables
    CHECK(c.has_nd == (C <= kMaxCamLds && n_act > 0));
    CHECK(c.solve_map.empty() == (C > kDense4Cams));
    if (C <= kDense4Cams) check_solve_map(c, L, C);
    if (c.has_nd)
        for (const NdPlan &pl : c.nd) {
            std::vector<int> pc;
            for (int x : pl.pcol) if (x >= 0) pc.push_back(x);
            std::sort(pc.begin(), pc.end());
            CHECK(pc == std::vector<int>(c.act_map.begin(), c.act_map.begin() + n_act));
        }
    if (!none) {
        // no mask: the contiguous blocks (13 columns, the last 7 of a held pose, none without views) and their plans
        int ncols[kMaxCam], col0[kMaxCam], n_max = 0, k = 0;
        for (int m = 0; m < C; ++m) {
            ncols[m] = !fa.views[m] ? 0 : fa.held[m] ? 7 : 13;
            col0[m] = 16 * m + (fa.held[m] ? 6 : 0);
            n_max += ncols[m];
            for (int j = 0; j < ncols[m]; ++j) CHECK(k < n_act && c.act_map[k++] == col0[m] + j);
        }
        CHECK(n_act == n_max);
        if (C <= kMaxCamLds && n_act > 0) {
            NdPlan ref[2];
            CHECK(nd_build_plans(C, ncols, col0, L.pair_present.data(), L.bid_of.data(), ref));
            CHECK(same_plan(c.nd[0], ref[0]) && same_plan(c.nd[1], ref[1]));
        }
    } else {
        // monotone in the mask: held intrinsics only ever take columns away (what sizes Abig at creation)
        CHECK(n_act <= none->n_act);
        for (int i = 0; i < n_pad; ++i) CHECK(!c.col_active[i] || none->col_active[i]);
    }
}

static int random_run(unsigned long long seed, int n)
{
    std::mt19937_64 rng(seed);
    for (int it = 0; it < n && g_fail.empty(); ++it) {
        Prob q = random_problem(rng);
        const tscm_problem *p = q.get();
        Layout L;
        std::string err;
        LayoutDevice dev;
        if (int rc = plan_layout(p, 0, 1, dev, L, err)) { std::fprintf(stderr, "plan_layout: %d %s\n", rc, err.c_str()); return 2; }
        const int C = q.C;
        const Facts fa = facts(p);
        g_count[C_MONO] += q.mono; g_count[C_BIG] += C > kMaxCamLds;
        for (int m = 0; m < C; ++m) { g_count[C_NO_VIEWS] += !fa.views[m]; g_count[C_POSE_HELD] += fa.held[m] && fa.views[m]; }
        ColumnPlan none;
        const int rc0 = plan_columns(L, C, nullptr, none, err);
        CHECK(rc0 == 0);
        if (rc0) break;
        check_columns(p, L, nullptr, none, nullptr);
        g_count[C_DENSE4] += C <= kDense4Cams; g_count[C_ND] += none.has_nd;
        for (int kind = 0; kind < kMaskKinds && g_fail.empty(); ++kind) {
            const std::vector<unsigned short> f = masks(kind, C, rng);
            ColumnPlan c;
            // never refused where the unmasked plan is not; the refusals keep their code and message
            const int rc = plan_columns(L, C, f.data(), c, err);
            if (rc) {
                g_count[C_REFUSED]++;
                CHECK(rc == TSCM_E_UNSUPPORTED && (err == "internal error: the reduced system does not fit the register/LDS solver" ||
                                                  err == "internal error: elimination plan does not cover the free columns"));
                CHECK(rc == 0);
                break;
            }
            check_columns(p, L, f.data(), c, &none);
            g_count[C_PLANS]++; g_count[C_EMPTY] += c.n_act == 0;
            // an all-zero mask is no mask
            if (kind == 0) CHECK(c.col_ctl == none.col_ctl && c.act_map == none.act_map && c.n_act == none.n_act);
        }
        if (!g_fail.empty()) std::fprintf(stderr, "problem %d: C %d, mono %d, boards %d, views %zu\n", it, C, q.mono, q.B, q.cam.size());
    }
    std::printf("{\"ok\": %s, \"fail\": \"%s\", \"plans\": %ld, \"mono\": %ld, \"big_rigs\": %ld, \"dense4\": %ld, \"nd\": %ld, \"empty\": %ld, "
                "\"holes\": %ld, \"no_views\": %ld, \"pose_held\": %ld, \"rhs_tiles\": %ld, \"refused\": %ld}\n",
                g_fail.empty() ? "true" : "false", g_fail.c_str(), g_count[C_PLANS], g_count[C_MONO], g_count[C_BIG], g_count[C_DENSE4],
                g_count[C_ND], g_count[C_EMPTY], g_count[C_HOLES], g_count[C_NO_VIEWS], g_count[C_POSE_HELD], g_count[C_RHS_TILES],
                g_count[C_REFUSED]);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !std::strcmp(argv[1], "random")) return random_run(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    std::fprintf(stderr, "usage: columns_check random <seed> <problems>\n");
    return 2;
}
