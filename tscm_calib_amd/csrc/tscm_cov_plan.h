// tscm_cov_plan.h -- host side of the covariance stage (tscm.h: tscm_covariance): which columns of the normal
// equations are free, their compact numbering with holes, the views of every free board, and the work lists of
// k_cov_schur -- the camera-pair tiles that have a common free board, each tile's (view, view') pairs cut into chunks.
// Plain C++17 like tscm_columns.h; tscm_covariance.hip uploads what plan_covariance returns and tests/native/cov_plan_check.cpp
// checks it on the CPU.
#ifndef TSCM_COV_PLAN_H
#define TSCM_COV_PLAN_H

#include "../../include/tscm/tscm.h"

#include <string>
#include <utility>
#include <vector>

namespace tscm {

constexpr int kCovCam = 15;          // a camera's columns in the host layout: pose 6, fx fy cx cy xi lambda alpha b c
constexpr int kCovCamFree = 13;      // b and c are never free
constexpr int kCovMaxCam = 32;
constexpr int kCovChunk = 64;        // (view, view') pairs of one k_cov_schur workgroup
constexpr int kCovBoardGroup = 64;   // free boards of one k_cov_boards workgroup

// The free columns of a problem under the held-intrinsics masks (fixed: [C] TSCM_FIX_* words or NULL), tscm.h's rules:
// a camera with a view that has corners frees its intrinsics k < 7 unless bit k of its mask is set, and its pose unless
// the problem is mono or cam_pose_constant[m]; a board with such a view is free unless board_pose_constant[i].
// The problem must have passed tscm::validate.
inline void cov_masks(const tscm_problem *p, const unsigned short *fixed, std::vector<unsigned char> &cam_free, std::vector<unsigned char> &board_free)
{
    const int C = p->n_cameras, B = p->n_boards;
    std::vector<unsigned char> cam_seen((size_t)C, 0), board_seen((size_t)B, 0);
    for (int v = 0; v < p->n_views; ++v)
        if (p->view_count[v] > 0) { cam_seen[p->view_camera[v]] = 1; board_seen[p->view_board[v]] = 1; }
    cam_free.assign((size_t)C * kCovCam, 0);
    board_free.assign((size_t)B, 0);
    for (int m = 0; m < C; ++m) {
        if (!cam_seen[m]) continue;
        const bool pose = !p->mono && !(p->cam_pose_constant && p->cam_pose_constant[m]);
        const unsigned f = fixed ? fixed[m] : 0u;
        for (int a = 0; a < kCovCamFree; ++a) cam_free[(size_t)m * kCovCam + a] = a < 6 ? (pose ? 1 : 0) : (((f >> (a - 6)) & 1u) ? 0 : 1);
    }
    for (int i = 0; i < B; ++i) board_free[i] = board_seen[i] && !(p->board_pose_constant && p->board_pose_constant[i]) ? 1 : 0;
}

struct CovPlan {
    int C = 0, B = 0, V = 0;
    int n_cam_free = 0;                  // free camera columns: the order of the reduced system
    int n_free = 0;                      // n_cam_free + 6 * free boards
    std::vector<int> compact_of;         // [C * 15] 15-wide column -> compact index, -1 where not free
    std::vector<int> wide_of;            // [n_cam_free] compact index -> 15-wide column, increasing
    std::vector<int> free_boards;        // the free boards, increasing
    std::vector<int> board_start;        // [free boards + 1] CSR into board_views, in free_boards order
    std::vector<int> board_views;        // the views of each free board, in view order
    std::vector<int> view_slot;          // [board_views.size()] index of the view's board in free_boards
    // k_cov_schur: tile t is the camera pair (tile_a[t] <= tile_b[t]); its pairs (v, v') have v on camera a, v' on camera b
    // and one free board; they are listed by board, then v, then v'.  A diagonal tile lists v = v' and, if a board has two
    // views of one camera, both orders.
    std::vector<int> tile_a, tile_b;
    std::vector<int> tile_of;            // [C * C] tile of the pair (a <= b), -1 without a common free board (and for a > b)
    std::vector<int> tile_start;         // [tiles + 1] CSR into pair_v / pair_w
    std::vector<int> pair_v, pair_w;
    std::vector<int> tile_chunk;         // [tiles + 1] CSR into chunk_*: a tile's chunks in list order
    std::vector<int> chunk_begin, chunk_end;   // [chunks] range of pair_v / pair_w, at most kCovChunk long
};

inline int cov_fail(std::string &err, const std::string &msg) { err = msg; return TSCM_E_INVALID; }

// 0, or TSCM_E_INVALID and the text naming the argument (out is then untouched).  cam_free [C * 15], board_free [B].
inline int plan_covariance(int C, int B, int V, const int *view_camera, const int *view_board, const unsigned char *cam_free,
                           const unsigned char *board_free, CovPlan &out, std::string &err)
{
    if (C < 1 || C > kCovMaxCam) return cov_fail(err, "n_cameras " + std::to_string(C) + " outside 1..32");
    if (B < 0) return cov_fail(err, "n_boards is negative");
    if (V < 0) return cov_fail(err, "n_views is negative");
    if (V > 0 && !view_camera) return cov_fail(err, "view_camera is NULL");
    if (V > 0 && !view_board) return cov_fail(err, "view_board is NULL");
    if (!cam_free) return cov_fail(err, "cam_free is NULL");
    if (B > 0 && !board_free) return cov_fail(err, "board_free is NULL");
    for (int v = 0; v < V; ++v) {
        if (view_camera[v] < 0 || view_camera[v] >= C) return cov_fail(err, "view_camera[" + std::to_string(v) + "] out of range");
        if (view_board[v] < 0 || view_board[v] >= B) return cov_fail(err, "view_board[" + std::to_string(v) + "] out of range");
    }
    for (int m = 0; m < C; ++m)
        for (int a = kCovCamFree; a < kCovCam; ++a)
            if (cam_free[(size_t)m * kCovCam + a]) return cov_fail(err, "cam_free: b and c (columns 13, 14 of a camera) are never free");
    CovPlan c;
    c.C = C; c.B = B; c.V = V;
    c.compact_of.assign((size_t)C * kCovCam, -1);
    for (int i = 0; i < C * kCovCam; ++i)
        if (cam_free[i]) { c.compact_of[i] = c.n_cam_free++; c.wide_of.push_back(i); }
    std::vector<int> slot_of((size_t)B, -1);
    for (int i = 0; i < B; ++i)
        if (board_free[i]) { slot_of[i] = (int)c.free_boards.size(); c.free_boards.push_back(i); }
    const int nfb = (int)c.free_boards.size();
    c.n_free = c.n_cam_free + 6 * nfb;
    // the views of the free boards, by board and in view order (counting sort)
    c.board_start.assign((size_t)nfb + 1, 0);
    for (int v = 0; v < V; ++v) if (slot_of[view_board[v]] >= 0) c.board_start[slot_of[view_board[v]] + 1]++;
    for (int s = 0; s < nfb; ++s) c.board_start[s + 1] += c.board_start[s];
    c.board_views.assign((size_t)c.board_start[nfb], 0);
    c.view_slot.assign((size_t)c.board_start[nfb], 0);
    {
        std::vector<int> at(c.board_start.begin(), c.board_start.end() - 1);
        for (int v = 0; v < V; ++v) {
            const int s = slot_of[view_board[v]];
            if (s >= 0) { c.view_slot[at[s]] = s; c.board_views[at[s]++] = v; }
        }
    }
    // the camera-pair tiles: count, then fill in board order
    std::vector<int> count((size_t)C * C, 0);
    long long n_pairs = 0;
    for (int s = 0; s < nfb; ++s) n_pairs += (long long)(c.board_start[s + 1] - c.board_start[s]) * (c.board_start[s + 1] - c.board_start[s]);
    if (n_pairs > (1ll << 30)) return cov_fail(err, "view_board: more than 2^30 pairs of views share a board");
    for (int s = 0; s < nfb; ++s)
        for (int i = c.board_start[s]; i < c.board_start[s + 1]; ++i)
            for (int j = c.board_start[s]; j < c.board_start[s + 1]; ++j) {
                const int a = view_camera[c.board_views[i]], b = view_camera[c.board_views[j]];
                if (a <= b) count[(size_t)a * C + b]++;
            }
    c.tile_of.assign((size_t)C * C, -1);
    c.tile_start.push_back(0);
    for (int a = 0; a < C; ++a)
        for (int b = a; b < C; ++b)
            if (count[(size_t)a * C + b]) {
                c.tile_of[(size_t)a * C + b] = (int)c.tile_a.size();
                c.tile_a.push_back(a); c.tile_b.push_back(b);
                c.tile_start.push_back(c.tile_start.back() + count[(size_t)a * C + b]);
            }
    const int nt = (int)c.tile_a.size();
    c.pair_v.assign((size_t)c.tile_start[nt], 0);
    c.pair_w.assign((size_t)c.tile_start[nt], 0);
    {
        std::vector<int> at(c.tile_start.begin(), c.tile_start.end() - 1);
        for (int s = 0; s < nfb; ++s)
            for (int i = c.board_start[s]; i < c.board_start[s + 1]; ++i)
                for (int j = c.board_start[s]; j < c.board_start[s + 1]; ++j) {
                    const int v = c.board_views[i], w = c.board_views[j], a = view_camera[v], b = view_camera[w];
                    if (a > b) continue;
                    const int t = c.tile_of[(size_t)a * C + b];
                    c.pair_v[at[t]] = v; c.pair_w[at[t]++] = w;
                }
    }
    c.tile_chunk.push_back(0);
    for (int t = 0; t < nt; ++t) {
        for (int k = c.tile_start[t]; k < c.tile_start[t + 1]; k += kCovChunk) {
            c.chunk_begin.push_back(k);
            c.chunk_end.push_back(k + kCovChunk < c.tile_start[t + 1] ? k + kCovChunk : c.tile_start[t + 1]);
        }
        c.tile_chunk.push_back((int)c.chunk_begin.size());
    }
    out = std::move(c);
    return 0;
}

}  // namespace tscm

#endif
