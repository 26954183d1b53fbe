// tscm_columns.h -- host side of the reduced camera system's columns: which camera-side columns are free under
// the held-intrinsics masks, their compact numbering, and the tables of the reduced solvers built on it -- k_solve_reduced's
// operand map (rigs of up to kDense4Cams cameras) and both k_solve_nd plans (up to kMaxCamLds).  Plain C++17 like
// tscm_layout.h; tscm_solver.hip uploads what plan_columns returns at creation and on tscm_solver_set_fixed_intrinsics,
// and tests/native/columns_check.cpp checks it on the CPU.
#ifndef TSCM_COLUMNS_H
#define TSCM_COLUMNS_H

#include "tscm_layout.h"
#include "tscm_nd_plan.h"
#include "tscm_exec_plan.h"

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace tscm {

constexpr int kColFree = 13;       // kFA (tscm_math.h): the camera-side parameter columns of a camera's 16
constexpr int kColGrad = 13;       // kFR (tscm_math.h): the gradient column of a camera tile

// Tile of thread tid in k_solve_reduced's G x G grid (NP panels of free columns).  Lower tile (ti, tj) of the matrix on
// thread ti * G + tj.  The right-hand side tiles (NP, p), p < NP, go to threads that own no matrix tile, counted
// downwards from the end of the last wave that holds matrix tiles: tile p is needed up to panel step p, so the
// longest-lived ones share a wave with the longest-lived matrix rows and the early waves retire early.  The
// look-ahead thread (the last thread of the workgroup) is never used.
struct SolveTile { bool mine, rhsrow; int ri, cj; };
template <int TS, int G>
inline SolveTile solve_tile(int tid, int NP)
{
    constexpr int NT = (G * G + 63) / 64 * 64;
    auto owns = [&](int t) { const int ti = t / G, tj = t % G; return tj <= ti && ti < NP; };
    SolveTile t;
    t.mine = owns(tid); t.rhsrow = false;
    t.ri = tid / G; t.cj = tid % G;
    if (t.mine || tid == NT - 1) return t;
    const int last = std::min(NT - 2, ((NP - 1) * G + NP - 1) | 63);   // end of the wave of tile (NP-1, NP-1)
    if (tid > last) return t;
    int rank = 0;                                                       // free threads in (tid, last]
    for (int u = tid + 1; u <= last; ++u) rank += owns(u) ? 0 : 1;
    if (rank < NP) { t.rhsrow = true; t.ri = NP; t.cj = NP - 1 - rank; }
    return t;
}
// slots of the per-thread operand map (ints): offsets into H[cur] and T per tile element (-1: the element is 0),
// s_c indices of the tile's rows and columns (-1: padding / rhs row, where 1 is used through kMapOne)
constexpr int kMapH = 0, kMapT = 16, kMapSci = 32, kMapScj = 36, kMapTile = 40, kSolveMapSlots = 44;   // kMapTile: row, column, 1 = matrix tile / 2 = rhs tile
constexpr int kMapOne = 1 << 30;       // "scaling 1": the row of a right-hand side tile
constexpr int kSolveMapThreads = 256;  // k_solve_reduced<4, 16>: G = 16, one map entry per thread and slot quadruple

// The solution rides through the factorisation (plan_solve_ext): NP more tile rows e_0 .. e_NP-1 = NP + 1 + i start as the
// identity, tile (e_i, j) for i <= j < NP, and row e_i has one more tile in the right-hand side's column NP, which starts at
// 0 and ends as -y_i.  Those tiles go to threads without an entry in solve_map; per thread { kind, ri, cj, i }.
constexpr int kExtNone = 0, kExtRow = 3, kExtSol = 4;   // (1 and 2 are solve_map's matrix and right-hand side tiles)
constexpr int kSolveExtPanels = 12;     // NP of that path at most: the kernel has LDS for 12 e-rows of a panel column
// whether the tile of a thread takes part in the trailing update of panel tk: the plan, the CPU checks and k_solve_reduced
// itself all ask this one function.  kind: solve_map's (1 matrix, 2 right-hand side) or solve_ext's, 0 no tile.  from: the
// first panel of an e-row's tiles (0 for the others).  An e-row tile of column tk would only become a block of L^-T that
// nobody reads: it was published raw at the end of panel tk - 1 and rests from then on
TSCM_LAYOUT_FN bool solve_tile_live(int kind, int ri, int cj, int from, int tk)
{
    if (kind == kExtNone || !(ri > tk && cj >= tk && tk >= from)) return false;
    if (ri == cj && ri == tk + 1) return false;                 // the look-ahead thread has that one
    return !(kind == kExtRow && cj == tk);
}

struct ColumnPlan {
    std::vector<unsigned char> col_active;      // [n_pad] 1 = free camera-side column
    std::vector<unsigned char> col_ctl;         // [16 * kMaxCam] the control step's classes: bit 0 counts in |x|, bit 1 free; 0 past n_pad
    std::vector<int> act_map;                   // [n_pad] compact index -> padded column, -1 past n_act
    int n_act = 0;
    int cam_pre[9] = {};                        // the compact numbering as kernel arguments (rigs of <= kMaxCamLds cameras):
    unsigned short cam_free[8] = {};            // camera q's free columns are compact [cam_pre[q], cam_pre[q + 1]) = 16 q + the set bits of cam_free[q]
    std::vector<Int4> solve_map;                // [kSolveMapSlots / 4][kSolveMapThreads] k_solve_reduced's operand map; C <= kDense4Cams only
    std::vector<Int4> solve_ext;                // [kSolveMapThreads] { kind, ri, cj, i } of the e-row and solution tiles (plan_solve_ext); all kExtNone on the fallback
    bool ext_fallback = false;                  // the tiles do not fit below the look-ahead thread's wave: k_solve_reduced back-substitutes
    int wave_sum_old = 0, wave_sum_new = 0;     // sum over the panels of the waves with a tile in the trailing update: solve_map alone / with solve_ext
    bool has_nd = false;                        // C <= kMaxCamLds and n_act > 0: nd holds k_solve_nd's plans
    NdPlan nd[2];                               // [0] along the camera-pair graph, [1] the whole system as one dense block
};

// the operand map of k_solve_reduced<4, 16>: where every thread finds its tile's entries of H and T and the scaling of its
// rows and columns (a function of the camera/pair structure and the compact numbering only)
inline std::vector<Int4> plan_solve_map(const Layout &L, const ColumnPlan &c)
{
    constexpr int TS = 4, G = 16, NT = kSolveMapThreads;
    static_assert(NT == (G * G + 63) / 64 * 64, "one map entry per thread of k_solve_reduced<4, 16>");
    const int NP = (c.n_act + TS - 1) / TS;
    auto cmap = [&](int ci) { return ci < c.n_act ? c.act_map[ci] : -1; };
    auto t_offset = [&](int i, int j) {                         // as load_T_small
        int lo = i >> 4, hi = j >> 4, a = i & 15, b = j & 15;
        if (lo > hi) { std::swap(lo, hi); std::swap(a, b); }
        const int bit = lo * 8 + hi;
        const unsigned long long m = L.pair_mask;
        return ((m >> bit) & 1ull) ? 256 * __builtin_popcountll(m & ((1ull << bit) - 1ull)) + a * 16 + b : -1;
    };
    std::vector<Int4> map((size_t)(kSolveMapSlots / 4) * NT);
    for (int tid = 0; tid < NT; ++tid) {
        const SolveTile tl = solve_tile<TS, G>(tid, NP);
        int off[kSolveMapSlots];
        std::fill(off, off + kSolveMapSlots, -1);
        off[kMapTile] = tl.ri; off[kMapTile + 1] = tl.cj; off[kMapTile + 2] = tl.mine ? 1 : tl.rhsrow ? 2 : 0;
        if (tl.mine || tl.rhsrow) {
            int mi[TS], mj[TS];
            for (int r = 0; r < TS; ++r) { mi[r] = tl.mine ? cmap(tl.ri * TS + r) : -1; mj[r] = cmap(tl.cj * TS + r); }
            for (int r = 0; r < TS; ++r) { off[kMapSci + r] = mi[r]; off[kMapScj + r] = mj[r]; }
            if (tl.mine) {
                for (int r = 0; r < TS; ++r)
                    for (int q = 0; q < TS; ++q) {
                        const int i = mi[r], j = mj[q];
                        if (i < 0 || j < 0) continue;
                        if ((i >> 4) == (j >> 4)) off[kMapH + r * TS + q] = 256 * (i >> 4) + (i & 15) * 16 + (j & 15);
                        off[kMapT + r * TS + q] = t_offset(i, j);
                    }
            } else {
                // right-hand side tile: row 0 = g - t_r of the panel's columns (the fused column kFR of H and T)
                for (int q = 0; q < TS; ++q) {
                    const int j = mj[q];
                    if (j < 0) continue;
                    const int m = j >> 4, b = j & 15;
                    off[kMapH + q] = 256 * m + b * 16 + kColGrad;
                    off[kMapT + q] = t_offset(j, m * 16 + kColGrad);
                }
                off[kMapSci] = kMapOne;
            }
        }
        for (int q = 0; q < kSolveMapSlots / 4; ++q) map[(size_t)q * NT + tid] = Int4{ off[4 * q], off[4 * q + 1], off[4 * q + 2], off[4 * q + 3] };
    }
    return map;
}

// Owners of the e-row and solution tiles of k_solve_reduced<4, 16> (needs c.solve_map).  Rules: an owner has no entry in
// solve_map and does not sit in the wave of the look-ahead thread NT - 1 (a lane there would put the trailing update in
// series with the diagonal factorisation, the panel's critical path).  The scheme is planned only if ALL its tiles --
// matrix, right-hand side, e-rows, solution -- fit into the waves below that one (NT - 64 threads: NP <= 12); otherwise
// ext_fallback, an empty table, and the kernel back-substitutes as before.  Among the placements the sum over the panels
// of the waves that take part in the trailing update is kept small greedily: tiles in the order of their last panel
// (longest-lived first), each into the wave where it adds the fewest live panels, on a tie the wave that works longest
// anyway.  wave_sum_old / wave_sum_new record that sum without and with the new tiles.
inline void plan_solve_ext(ColumnPlan &c)
{
    constexpr int TS = 4, NT = kSolveMapThreads, NW = NT / 64;
    const int NP = (c.n_act + TS - 1) / TS;
    c.solve_ext.assign((size_t)NT, Int4{ kExtNone, 0, 0, 0 });
    c.ext_fallback = false; c.wave_sum_old = c.wave_sum_new = 0;
    std::vector<std::vector<char>> live(NW, std::vector<char>((size_t)std::max(NP, 1), 0));
    std::vector<std::vector<int>> free_tid(NW);
    for (int tid = 0; tid < NT; ++tid) {
        const Int4 v = c.solve_map[(size_t)(kMapTile / 4) * NT + tid];        // { ri, cj, kind, -1 }
        if (v.z == 0) { if (tid / 64 < NW - 1) free_tid[tid / 64].push_back(tid); continue; }
        for (int tk = 0; tk < NP; ++tk) if (solve_tile_live(v.z, v.x, v.y, 0, tk)) live[tid / 64][tk] = 1;
    }
    auto wave_sum = [&] { int s = 0; for (const auto &w : live) for (char x : w) s += x; return s; };
    c.wave_sum_old = c.wave_sum_new = wave_sum();
    if (NP * (NP + 1) + 2 * NP > NT - 64 || NP > kSolveExtPanels) { c.ext_fallback = true; return; }
    struct Tile { int kind, ri, cj, i, first, last; };      // takes part in the update of panels first .. last (none: last < first)
    std::vector<Tile> tiles;
    for (int i = 0; i < NP; ++i) {
        for (int j = i; j < NP; ++j) tiles.push_back(Tile{ kExtRow, NP + 1 + i, j, i, i, j - 1 });
        tiles.push_back(Tile{ kExtSol, NP + 1 + i, NP, i, i, NP - 1 });
    }
    std::stable_sort(tiles.begin(), tiles.end(), [](const Tile &a, const Tile &b) { return a.last != b.last ? a.last > b.last : a.first < b.first; });
    size_t room = 0;
    for (const auto &f : free_tid) room += f.size();
    if (room < tiles.size()) { c.ext_fallback = true; return; }
    std::vector<size_t> used(NW, 0);
    for (const Tile &t : tiles) {
        int best = -1, best_add = 0, best_base = 0;
        for (int w = 0; w < NW - 1; ++w) {
            if (used[w] == free_tid[w].size()) continue;
            int add = 0, base = 0;
            for (int tk = 0; tk < NP; ++tk) { add += tk >= t.first && tk <= t.last && !live[w][tk]; base += live[w][tk]; }
            if (best < 0 || add < best_add || (add == best_add && base > best_base)) { best = w; best_add = add; best_base = base; }
        }
        c.solve_ext[(size_t)free_tid[best][used[best]++]] = Int4{ t.kind, t.ri, t.cj, t.i };
        for (int tk = t.first; tk <= t.last; ++tk) live[best][tk] = 1;
    }
    c.wave_sum_new = wave_sum();
}

// The free camera-side columns of the reduced system and every table derived from them.  A padded column
// 16 m + a is free if camera m has views, a < kFA, the pose is not held (a < 6) and intrinsic a - 6 is not held (bit a - 6 of
// fixed[m]; fixed NULL: none is).  Held intrinsics leave the tangent space: no column, no Jacobi scale, no LM diagonal, no
// gradient; their values stay in |x| unless all seven are held, which makes the block constant (Ceres' SubsetManifold /
// SetParameterBlockConstant).  With no held intrinsics the tables are the ones of the contiguous blocks, bit for bit.
// 0, or a TSCM_E_* code and its message in err (out is then untouched)
inline int plan_columns(const Layout &L, int C, const unsigned short *fixed, ColumnPlan &out, std::string &err)
{
    ColumnPlan c;
    const int n_pad = 16 * C;
    c.col_active.assign((size_t)n_pad, 0); c.col_ctl.assign((size_t)16 * kMaxCam, 0);
    std::vector<unsigned short> word(C, 0);
    for (int i = 0; i < n_pad; ++i) {
        const int m = i >> 4, a = i & 15;
        const bool act = L.cam_active[m] != 0, cst = L.cam_const[m] != 0;
        const unsigned f = fixed ? fixed[m] : 0u;
        const bool held = a >= 6 && a < kColFree && ((f >> (a - 6)) & 1u);
        const bool block_const = (f & TSCM_FIX_INTRINSICS) == TSCM_FIX_INTRINSICS;
        c.col_active[i] = (a < kColFree && act && !(a < 6 && cst) && !held) ? 1 : 0;
        const bool in_x = a < 6 ? (act && !cst) : a < 15 ? (act && !block_const) : false;
        c.col_ctl[i] = (unsigned char)((in_x ? 1 : 0) | (c.col_active[i] ? 2 : 0));
        if (c.col_active[i]) word[m] |= (unsigned short)(1u << a);
    }
    // compact numbering of the free camera-side columns: the reduced system is factored without the identity rows of held /
    // padding columns
    c.act_map.assign((size_t)n_pad, -1);
    for (int i = 0; i < n_pad; ++i) if (c.col_active[i]) c.act_map[c.n_act++] = i;
    std::fill(c.cam_pre, c.cam_pre + 9, c.n_act);
    if (C <= kMaxCamLds) {
        int run = 0;
        for (int m = 0; m < C; ++m) { c.cam_pre[m] = run; c.cam_free[m] = word[m]; run += __builtin_popcount(word[m]); }
    }
    if (C <= kDense4Cams) { c.solve_map = plan_solve_map(L, c); plan_solve_ext(c); }
    if (C <= kMaxCamLds && c.n_act > 0) {
        // two plans: [0] along the camera-pair graph, [1] the whole system as one dense block.  A graph whose per-camera panel
        // padding does not fit the tile budget (dense but incomplete pair graphs of 8 free cameras) is solved on the dense plan;
        // only a system that fits neither is refused.  (No free column at all: no plan -- that system is not factored, see
        // enqueue_iteration.)
        int ncols[kMaxCamLds];
        std::vector<int> cols((size_t)16 * C, -1);
        for (int m = 0; m < C; ++m) {
            ncols[m] = 0;
            for (int a = 0; a < 16; ++a) if ((word[m] >> a) & 1u) cols[16 * (size_t)m + ncols[m]++] = 16 * m + a;
        }
        if (!nd_build_plans_cols(C, ncols, cols.data(), L.pair_present.data(), L.bid_of.data(), c.nd))
            return layout_fail(err, TSCM_E_UNSUPPORTED, "internal error: the reduced system does not fit the register/LDS solver");
        // (replica check: each plan's columns are exactly the free columns)
        const std::vector<int> want(c.act_map.begin(), c.act_map.begin() + c.n_act);
        for (const NdPlan &pl : c.nd) {
            std::vector<int> pc;
            for (int col : pl.pcol) if (col >= 0) pc.push_back(col);
            std::sort(pc.begin(), pc.end());
            if (pc != want) return layout_fail(err, TSCM_E_UNSUPPORTED, "internal error: elimination plan does not cover the free columns");
        }
        c.has_nd = true;
    }
    out = std::move(c);
    return 0;
}

}  // namespace tscm

#endif
