// CPU check of the e-row and solution tiles of k_solve_reduced (tscm_calib_amd/csrc/tscm_columns.h: plan_solve_ext), with
// which the camera step falls out of the reduced system's factorisation instead of a back-substitution behind it.
//   usage: solve_ext_check plan <seed> <rounds>    rigs of 1..4 cameras (every subset of held poses, now and then a camera
//                                                  without views) under the six kinds of held-intrinsics masks of
//                                                  columns_check: every tile (e_i, j), i <= j < NP, and every solution tile
//                                                  has exactly one owner; owners have no entry in solve_map and do not sit
//                                                  in the look-ahead thread's wave; the recorded wave sums equal a recount;
//                                                  "fallback" exactly when the tiles do not fit
//          solve_ext_check emulate                 the blocked step in plain C++ over the planned tiles -- the kernel's tile
//                                                  roles, panel order and operation order -- on Jacobi-scaled SPD systems of
//                                                  n_act = 7, 20, 41, 46 (partial last panels among them).  Reference: a long
//                                                  double Cholesky solve of the same system.  Yardstick: the forward error of
//                                                  the emulated back-substitution path on the same matrix; the new path may
//                                                  exceed it by a factor of 2 and no more.
// Measured ratios new / old (largest over 8 matrices each; cond 1e4, 1e8, 1e11):
//   n_act  7: 1.003 1.000 1.000   n_act 20: 1.006 1.000 1.000   n_act 41: 1.002 1.000 1.000   n_act 46: 1.004 1.000 1.000
//   (forward errors of both paths at n_act 46: 9.6e-14, 3.9e-10, 2.7e-7 -- the shared factor and w dominate)
// Each prints one JSON line.  Host logic only (no GPU).
#include "../../tscm_calib_amd/csrc/tscm_layout.h"
#include "../../tscm_calib_amd/csrc/tscm_columns.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace tscm;

static std::string g_fail;
#define CHECK(cond) do { if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; } while (0)

constexpr int TS = 4, G = 16, NT = kSolveMapThreads, NW = NT / 64;

struct Tile { int kind, ri, cj, from; };
// what the kernel makes of the two tables: the tile of every thread
static std::vector<Tile> thread_tiles(const ColumnPlan &c, bool ext_on)
{
    std::vector<Tile> t(NT);
    for (int tid = 0; tid < NT; ++tid) {
        const Int4 m = c.solve_map[(size_t)(kMapTile / 4) * NT + tid], e = ext_on ? c.solve_ext[tid] : Int4{ 0, 0, 0, 0 };
        t[tid] = e.x ? Tile{ e.x, e.y, e.z, e.w } : Tile{ m.z, m.x, m.y, 0 };
    }
    return t;
}
static int recount_wave_sum(const std::vector<Tile> &t, int NP)
{
    int sum = 0;
    for (int tk = 0; tk < NP; ++tk)
        for (int w = 0; w < NW; ++w) {
            bool any = false;
            for (int l = 0; l < 64; ++l) { const Tile &x = t[64 * w + l]; any = any || solve_tile_live(x.kind, x.ri, x.cj, x.from, tk); }
            sum += any;
        }
    return sum;
}

// ---------------------------------------------------------------------------------------------------------------- plan
struct Prob {
    int C = 1, mono = 0;
    std::vector<int> cam, board, offset, count;
    std::vector<unsigned char> cconst;
    double dummy[2] = { 0.0, 0.0 };
    tscm_problem p{};
    const tscm_problem *get(int B)
    {
        p = tscm_problem{};
        p.n_cameras = C; p.n_boards = B; p.n_points = 12; p.n_views = (int)cam.size(); p.mono = mono;
        p.board_xy = dummy; p.intr = dummy; p.board_rt = dummy; p.cam_rt = dummy; p.obs_u = dummy; p.obs_v = dummy;
        p.view_camera = cam.data(); p.view_board = board.data(); p.view_offset = offset.data(); p.view_count = count.data();
        p.cam_pose_constant = cconst.data();
        return &p;
    }
    void add(int c, int b, int n) { offset.push_back(offset.empty() ? 0 : offset.back() + count.back()); cam.push_back(c); board.push_back(b); count.push_back(n); }
};

static long g_plans, g_ext, g_fallback, g_tiles, g_sum_old_max, g_sum_new_max, g_np_max;

static void check_ext(const ColumnPlan &c)
{
    const int NP = (c.n_act + TS - 1) / TS;
    CHECK((int)c.solve_ext.size() == NT && (int)c.solve_map.size() == kSolveMapSlots / 4 * NT);
    if (!g_fail.empty()) return;
    // do the tiles fit?  All tiles of the scheme below the look-ahead thread's wave, the new ones on threads without an entry
    const int n_new = NP * (NP + 1) / 2 + NP;
    int room = 0;
    for (int tid = 0; tid < NT - 64; ++tid) room += c.solve_map[(size_t)(kMapTile / 4) * NT + tid].z == 0;
    const bool fits = 2 * n_new <= NT - 64 && n_new <= room;
    CHECK(c.ext_fallback == !fits);
    const std::vector<Tile> old_t = thread_tiles(c, false), new_t = thread_tiles(c, true);
    CHECK(c.wave_sum_old == recount_wave_sum(old_t, NP));
    CHECK(c.wave_sum_new == recount_wave_sum(new_t, NP));
    g_plans++; g_np_max = std::max<long>(g_np_max, NP);
    g_sum_old_max = std::max<long>(g_sum_old_max, c.wave_sum_old); g_sum_new_max = std::max<long>(g_sum_new_max, c.wave_sum_new);
    if (c.ext_fallback) {
        for (int tid = 0; tid < NT; ++tid) { const Int4 e = c.solve_ext[tid]; CHECK(e.x == kExtNone && e.y == 0 && e.z == 0 && e.w == 0); }
        CHECK(c.wave_sum_new == c.wave_sum_old);
        g_fallback++;
        return;
    }
    g_ext += NP > 0;
    std::vector<int> owners((size_t)NP * (NP + 1), 0);          // [i][j], j == NP: the solution tile
    for (int tid = 0; tid < NT; ++tid) {
        const Int4 e = c.solve_ext[tid];
        if (e.x == kExtNone) { CHECK(e.y == 0 && e.z == 0 && e.w == 0); continue; }
        CHECK(e.x == kExtRow || e.x == kExtSol);
        CHECK(c.solve_map[(size_t)(kMapTile / 4) * NT + tid].z == 0);           // no entry in solve_map
        CHECK(tid / 64 < NW - 1 && tid / 64 != (NT - 1) / 64);                  // not in the look-ahead thread's wave
        const int i = e.w, j = e.z;
        CHECK(i >= 0 && i < NP && e.y == NP + 1 + i);
        CHECK(e.x == kExtRow ? (j >= i && j < NP) : j == NP);
        if (!g_fail.empty()) return;
        owners[(size_t)i * (NP + 1) + j]++;
        g_tiles++;
    }
    for (int i = 0; i < NP; ++i) for (int j = 0; j <= NP; ++j) CHECK(owners[(size_t)i * (NP + 1) + j] == (j >= i ? 1 : 0));
}

// the mask words of one kind, as columns_check: 0 none, 1 all held, 2 DS, 3 UCM, 4 cx_cy, 5 a different mask per camera
static std::vector<unsigned short> masks(int kind, int C, std::mt19937_64 &rng)
{
    auto uni = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
    std::vector<unsigned short> f(C, 0);
    for (int m = 0; m < C; ++m)
        f[m] = kind == 1 ? (uni(0, 1) ? TSCM_FIX_INTRINSICS : TSCM_FIX_ALL) : kind == 2 ? TSCM_MODEL_DS : kind == 3 ? TSCM_MODEL_UCM
             : kind == 4 ? (TSCM_FIX_CX | TSCM_FIX_CY) : kind == 5 ? (unsigned short)uni(0, TSCM_FIX_ALL) : 0;
    return f;
}

static int plan_run(unsigned long long seed, int rounds)
{
    std::mt19937_64 rng(seed);
    long counts_np[G + 1] = {};
    for (int round = 0; round < rounds && g_fail.empty(); ++round)
        for (int C = 1; C <= kDense4Cams && g_fail.empty(); ++C)
            for (int held = 0; held < (1 << C) && g_fail.empty(); ++held) {
                Prob q;
                q.C = C;
                q.cconst.assign(C, 0);
                for (int m = 0; m < C; ++m) q.cconst[m] = (held >> m) & 1;
                // a ring of camera pairs, one board each; in later rounds now and then a camera without views
                const int idle = round > 0 && C > 1 && rng() % 4 == 0 ? (int)(rng() % C) : -1;
                int B = 0;
                for (int m = 0; m < C; ++m) {
                    const int m2 = (m + 1) % C;
                    if (m != idle) q.add(m, B, 12);
                    if (m2 != m && m2 != idle) q.add(m2, B, 12);
                    ++B;
                }
                const tscm_problem *p = q.get(B);
                Layout L;
                std::string err;
                LayoutDevice dev;
                if (int rc = plan_layout(p, 0, 1, dev, L, err)) { std::fprintf(stderr, "plan_layout: %d %s\n", rc, err.c_str()); return 2; }
                for (int kind = 0; kind < 6 && g_fail.empty(); ++kind) {
                    const std::vector<unsigned short> f = masks(kind, C, rng);
                    ColumnPlan c;
                    const int rc = plan_columns(L, C, kind ? f.data() : nullptr, c, err);
                    CHECK(rc == 0);
                    if (rc) break;
                    check_ext(c);
                    counts_np[(c.n_act + TS - 1) / TS]++;
                    if (!g_fail.empty()) std::fprintf(stderr, "C %d held %d mask kind %d n_act %d\n", C, held, kind, c.n_act);
                }
            }
    int np_seen = 0;
    for (int k = 0; k <= G; ++k) np_seen += counts_np[k] > 0;
    std::printf("{\"ok\": %s, \"fail\": \"%s\", \"plans\": %ld, \"ext\": %ld, \"fallback\": %ld, \"tiles\": %ld, \"np_max\": %ld, \"np_seen\": %d, "
                "\"wave_sum_old_max\": %ld, \"wave_sum_new_max\": %ld}\n", g_fail.empty() ? "true" : "false", g_fail.c_str(), g_plans, g_ext, g_fallback,
                g_tiles, g_np_max, np_seen, g_sum_old_max, g_sum_new_max);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------- emulate
typedef double T4[TS][TS];
struct Factor { T4 l; double il[TS]; };

// k_solve_reduced<4, 16> on the compact system A y = b (n x n), thread by thread; y_new: the solution tiles, y_old: the
// back-substitution behind the same factor
static bool emulate(const ColumnPlan &c, int n, const std::vector<double> &A, const std::vector<double> &b, std::vector<double> &y_new, std::vector<double> &y_old)
{
    const int NP = (n + TS - 1) / TS, N = G * TS, rows = 2 * NP + 1;
    const std::vector<Tile> tl = thread_tiles(c, true);
    std::vector<double> a((size_t)NT * 16, 0.0), Xb((size_t)2 * rows * 16, 0.0), Ld((size_t)NP * 16, 0.0), idg((size_t)N, 0.0), sdt(2 * 16, 0.0), wp((size_t)N, 0.0);
    bool fail = false;
    auto at = [&](int tid) { return reinterpret_cast<double (*)[TS]>(&a[(size_t)tid * 16]); };
    auto xb = [&](int buf, int row) { return &Xb[((size_t)buf * rows + row) * 16]; };
    auto elem = [&](int i, int j) { return i < n && j < n ? A[(size_t)i * n + j] : i == j ? 1.0 : 0.0; };
    for (int tid = 0; tid < NT; ++tid) {
        const Tile &t = tl[tid];
        for (int r = 0; r < TS; ++r)
            for (int q = 0; q < TS; ++q) {
                double v = 0.0;
                if (t.kind == 1) v = elem(TS * t.ri + r, TS * t.cj + q);
                else if (t.kind == 2) v = r == 0 && TS * t.cj + q < n ? b[TS * t.cj + q] : 0.0;
                else if (t.kind == kExtRow) v = t.cj == t.from && r == q ? 1.0 : 0.0;
                at(tid)[r][q] = v;
            }
    }
    auto publish = [&](double *dst, const double (*t)[TS]) { for (int r = 0; r < TS; ++r) for (int q = 0; q < TS; ++q) dst[r * TS + q] = t[r][q]; };
    auto load = [&](const double *src, T4 &t) { for (int r = 0; r < TS; ++r) for (int q = 0; q < TS; ++q) t[r][q] = src[r * TS + q]; };
    auto factor_diag = [&](T4 &t, int tk) {
        double il[TS];
        for (int q = 0; q < TS; ++q) {
            double d = t[q][q];
            for (int k = 0; k < q; ++k) d -= t[q][k] * t[q][k];
            if (!(d > 0.0)) { fail = true; d = 1.0; }
            const double isd = 1.0 / std::sqrt(d);
            t[q][q] = d * isd; il[q] = isd;
            for (int r = q + 1; r < TS; ++r) {
                double v = t[r][q];
                for (int k = 0; k < q; ++k) v -= t[r][k] * t[q][k];
                t[r][q] = v * isd;
            }
        }
        for (int r = 0; r < TS; ++r) {
            idg[tk * TS + r] = il[r];
            for (int q = 0; q < TS; ++q) Ld[(size_t)tk * 16 + r * TS + q] = q <= r ? t[r][q] : 0.0;
        }
    };
    auto load_factor = [&](Factor &f, int tk) { for (int r = 0; r < TS; ++r) { f.il[r] = idg[tk * TS + r]; for (int q = 0; q < TS; ++q) f.l[r][q] = Ld[(size_t)tk * 16 + r * TS + q]; } };
    auto panel_solve = [&](const T4 &At, const Factor &f, T4 &x) {
        for (int r = 0; r < TS; ++r)
            for (int q = 0; q < TS; ++q) {
                double v = At[r][q];
                for (int k = 0; k < q; ++k) v -= x[r][k] * f.l[q][k];
                x[r][q] = v * f.il[q];
            }
    };
    const bool pubk[5] = { false, true, true, true, false };
    for (int tid = 0; tid < NT; ++tid) {
        const Tile &t = tl[tid];
        if (t.cj == 0 && t.ri > 0 && pubk[t.kind]) publish(xb(0, t.ri), at(tid));
        if (t.ri == 1 && t.cj == 1 && t.kind == 1) publish(&sdt[0], at(tid));
    }
    if (NP > 0) { T4 t; load(&a[0], t); factor_diag(t, 0); publish(&a[0], t); }
    for (int tk = 0; tk < NP; ++tk) {
        if (tk + 1 < NP) {                                  // the look-ahead thread
            Factor f; T4 araw, dt, x, t = {};
            load_factor(f, tk); load(xb(tk & 1, tk + 1), araw); load(&sdt[(size_t)(tk & 1) * 16], dt);
            panel_solve(araw, f, x);
            for (int r = 0; r < TS; ++r)
                for (int q = 0; q <= r; ++q) { double v = dt[r][q]; for (int k = 0; k < TS; ++k) v -= x[r][k] * x[q][k]; t[r][q] = v; }
            factor_diag(t, tk + 1);
        }
        for (int tid = 0; tid < NT; ++tid) {
            const Tile &t = tl[tid];
            if (solve_tile_live(t.kind, t.ri, t.cj, t.from, tk)) {
                Factor f; T4 ai, aj, xi, xj;
                load_factor(f, tk); load(xb(tk & 1, t.ri), ai); load(xb(tk & 1, t.cj), aj);
                panel_solve(ai, f, xi);
                if (t.cj == tk) {
                    publish(&a[(size_t)tid * 16], xi);
                    if (t.kind == 2) for (int q = 0; q < TS; ++q) wp[tk * TS + q] = xi[0][q];
                } else {
                    panel_solve(aj, f, xj);
                    for (int r = 0; r < TS; ++r)
                        for (int q = 0; q < TS; ++q) { double v = at(tid)[r][q]; for (int k = 0; k < TS; ++k) v -= xi[r][k] * xj[q][k]; at(tid)[r][q] = v; }
                }
            }
            const bool col = t.cj == tk + 1 && t.ri > tk + 1 && pubk[t.kind], dg = t.ri == tk + 2 && t.cj == tk + 2 && t.kind == 1;
            if (col || dg) publish(col ? xb((tk + 1) & 1, t.ri) : &sdt[(size_t)((tk + 1) & 1) * 16], at(tid));
        }
    }
    // the solution tiles
    y_new.assign((size_t)n, 0.0);
    for (int tid = 0; tid < NT; ++tid)
        if (tl[tid].kind == kExtSol) for (int r = 0; r < TS; ++r) if (TS * tl[tid].from + r < n) y_new[TS * tl[tid].from + r] = -at(tid)[r][0];
    // the back-substitution path: L to "LDS", then TS unknowns per step as the kernel's one wave does
    std::vector<double> Lm((size_t)N * N, 0.0), w(wp);
    for (int tk = 0; tk < NP; ++tk) for (int r = 0; r < TS; ++r) for (int q = 0; q < TS; ++q) Lm[(size_t)(tk * TS + r) * N + tk * TS + q] = Ld[(size_t)tk * 16 + r * TS + q];
    for (int tid = 0; tid < NT; ++tid) {
        const Tile &t = tl[tid];
        if (t.kind == 1 && t.cj < t.ri) for (int r = 0; r < TS; ++r) for (int q = 0; q < TS; ++q) Lm[(size_t)(t.ri * TS + r) * N + t.cj * TS + q] = at(tid)[r][q];
    }
    for (int tk = NP - 1; tk >= 0; --tk) {
        const int k0 = tk * TS;
        double y[TS];
        for (int q = 0; q < TS; ++q) y[q] = w[k0 + q];
        for (int q = TS - 1; q >= 0; --q) {
            double v = y[q];
            for (int k = q + 1; k < TS; ++k) v -= Lm[(size_t)(k0 + k) * N + k0 + q] * y[k];
            y[q] = v * idg[k0 + q];
        }
        for (int i = 0; i < k0; ++i) { double v = w[i]; for (int q = 0; q < TS; ++q) v -= Lm[(size_t)(k0 + q) * N + i] * y[q]; w[i] = v; }
        for (int q = 0; q < TS; ++q) w[k0 + q] = y[q];
    }
    y_old.assign(w.begin(), w.begin() + n);
    return !fail;
}

// Jacobi-scaled SPD matrix with eigenvalues spread over `cond` before the scaling
static void make_system(int n, double cond, std::mt19937_64 &rng, std::vector<double> &A, std::vector<double> &b)
{
    typedef long double ld;
    std::normal_distribution<double> nd;
    std::vector<ld> Q((size_t)n * n);
    for (auto &x : Q) x = nd(rng);
    for (int i = 0; i < n; ++i) {                             // modified Gram-Schmidt on the rows
        for (int k = 0; k < i; ++k) { ld d = 0; for (int j = 0; j < n; ++j) d += Q[(size_t)i * n + j] * Q[(size_t)k * n + j]; for (int j = 0; j < n; ++j) Q[(size_t)i * n + j] -= d * Q[(size_t)k * n + j]; }
        ld s = 0; for (int j = 0; j < n; ++j) s += Q[(size_t)i * n + j] * Q[(size_t)i * n + j];
        s = 1 / std::sqrt(s); for (int j = 0; j < n; ++j) Q[(size_t)i * n + j] *= s;
    }
    std::vector<ld> M((size_t)n * n, 0);
    for (int k = 0; k < n; ++k) {
        const ld lam = std::pow((ld)cond, -(ld)k / std::max(1, n - 1));
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) M[(size_t)i * n + j] += lam * Q[(size_t)k * n + i] * Q[(size_t)k * n + j];
    }
    A.assign((size_t)n * n, 0.0); b.assign((size_t)n, 0.0);
    for (int i = 0; i < n; ++i) for (int j = 0; j <= i; ++j) A[(size_t)i * n + j] = A[(size_t)j * n + i] = (double)(M[(size_t)i * n + j] / std::sqrt(M[(size_t)i * n + i] * M[(size_t)j * n + j]));
    for (int i = 0; i < n; ++i) { A[(size_t)i * n + i] = 1.0; b[i] = nd(rng); }
}

static bool solve_long_double(int n, const std::vector<double> &A, const std::vector<double> &b, std::vector<long double> &x)
{
    typedef long double ld;
    std::vector<ld> Lc((size_t)n * n, 0);
    for (int j = 0; j < n; ++j) {
        ld d = A[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= Lc[(size_t)j * n + k] * Lc[(size_t)j * n + k];
        if (!(d > 0)) return false;
        d = std::sqrt(d); Lc[(size_t)j * n + j] = d;
        for (int i = j + 1; i < n; ++i) { ld v = A[(size_t)i * n + j]; for (int k = 0; k < j; ++k) v -= Lc[(size_t)i * n + k] * Lc[(size_t)j * n + k]; Lc[(size_t)i * n + j] = v / d; }
    }
    x.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) { ld v = b[i]; for (int k = 0; k < i; ++k) v -= Lc[(size_t)i * n + k] * x[k]; x[i] = v / Lc[(size_t)i * n + i]; }
    for (int i = n - 1; i >= 0; --i) { ld v = x[i]; for (int k = i + 1; k < n; ++k) v -= Lc[(size_t)k * n + i] * x[k]; x[i] = v / Lc[(size_t)i * n + i]; }
    return true;
}

static int emulate_run()
{
    const int sizes[4] = { 7, 20, 41, 46 };
    const double conds[3] = { 1e4, 1e8, 1e11 };
    std::mt19937_64 rng(20241);
    std::string out = "{";
    double worst = 0.0;
    for (int n : sizes) {
        ColumnPlan c;
        Layout L;
        c.n_act = n;
        c.act_map.assign(64, -1);
        for (int i = 0; i < n; ++i) c.act_map[i] = i;
        c.solve_map = plan_solve_map(L, c);
        plan_solve_ext(c);
        CHECK(!c.ext_fallback);
        for (double cond : conds) {
            double ratio = 0.0, e_old_max = 0.0, e_new_max = 0.0;
            for (int rep = 0; rep < 8 && g_fail.empty(); ++rep) {
                std::vector<double> A, b, y_new, y_old;
                std::vector<long double> x;
                make_system(n, cond, rng, A, b);
                CHECK(solve_long_double(n, A, b, x));
                CHECK(emulate(c, n, A, b, y_new, y_old));
                long double xm = 0, en = 0, eo = 0;
                for (int i = 0; i < n; ++i) { xm = std::max(xm, std::fabs(x[i])); en = std::max(en, std::fabs(y_new[i] - x[i])); eo = std::max(eo, std::fabs(y_old[i] - x[i])); }
                CHECK(xm > 0 && eo > 0);
                // the yardstick is sane itself: the substitution path solves the system to cond * eps, with room for the growth of this small n
                CHECK((double)(eo / xm) <= 100.0 * cond * 1.1e-16);
                CHECK(en <= 2 * eo);
                ratio = std::max(ratio, (double)(en / eo));
                e_old_max = std::max(e_old_max, (double)(eo / xm)); e_new_max = std::max(e_new_max, (double)(en / xm));
            }
            char buf[200];
            std::snprintf(buf, sizeof buf, "\"n%d_cond%.0e\": [%.3g, %.3g, %.3f], ", n, cond, e_old_max, e_new_max, ratio);
            out += buf;
            worst = std::max(worst, ratio);
        }
    }
    std::printf("%s\"worst_ratio\": %.3f, \"ok\": %s, \"fail\": \"%s\"}\n", out.c_str(), worst, g_fail.empty() ? "true" : "false", g_fail.c_str());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !std::strcmp(argv[1], "plan")) return plan_run(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc >= 2 && !std::strcmp(argv[1], "emulate")) return emulate_run();
    std::fprintf(stderr, "usage: solve_ext_check plan <seed> <rounds> | emulate\n");
    return 2;
}
