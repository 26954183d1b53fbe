// Random and fixed problems for the CPU checks of a solve's launch plan and launch sequence (exec_plan_check.cpp,
// launch_seq_check.cpp): view tables planned with plan_layout, and the residency figures the plans are made against --
// ample, random, or at the exact limit of the riding launches and one below it.  Host logic only (no GPU).
#ifndef TSCM_TESTS_EXEC_PROBLEMS_H
#define TSCM_TESTS_EXEC_PROBLEMS_H

#include "../../tscm_calib_amd/csrc/tscm_layout.h"
#include "../../tscm_calib_amd/csrc/tscm_exec_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

namespace tscm {

// a problem's view tables (the parameter arrays only need to be non-NULL: the plan does not read them)
struct Prob {
    int C = 1, B = 0, n_points = 54, mono = 0;
    std::vector<int> cam, board, offset, count;
    std::vector<unsigned char> cam_const, board_const;      // held pose blocks; empty: the problem carries no such array
    double dummy[2] = { 0.0, 0.0 };
    tscm_problem p{};
    void add(int c, int b, int n) { offset.push_back(offset.empty() ? 0 : offset.back() + count.back()); cam.push_back(c); board.push_back(b); count.push_back(n); }
    Layout plan(int n_cu = 256, int waves_per_cu = 16) {
        p = tscm_problem{};
        p.n_cameras = C; p.n_boards = B; p.n_points = n_points; p.n_views = (int)cam.size(); p.mono = mono;
        p.cam_pose_constant = cam_const.empty() ? nullptr : cam_const.data();
        p.board_pose_constant = board_const.empty() ? nullptr : board_const.data();
        p.board_xy = dummy; p.intr = dummy; p.board_rt = dummy; p.cam_rt = dummy; p.obs_u = dummy; p.obs_v = dummy;
        p.view_camera = cam.data(); p.view_board = board.data(); p.view_offset = offset.data(); p.view_count = count.data();
        Layout L;
        std::string err;
        LayoutDevice dev;
        dev.n_cu = n_cu; dev.waves_per_cu = waves_per_cu;
        if (plan_layout(&p, 0, 1, dev, L, err)) { std::fprintf(stderr, "plan_layout: %s\n", err.c_str()); std::exit(2); }
        return L;
    }
};

// a ring of C cameras: board b is seen by cameras b mod C and b + 1 mod C (and by `extra` more cameras every 10th board)
inline Prob ring(int C, int B, int extra = 0)
{
    Prob q;
    q.C = C; q.B = B;
    for (int b = 0; b < B; ++b) {
        const int k = 2 + (b % 10 == 0 ? extra : 0);
        for (int i = 0; i < k && i < C; ++i) q.add((b + i) % C, b, q.n_points);
    }
    return q;
}

inline ExecDevice ample()
{
    ExecDevice d;
    for (int nv = 1; nv <= 3; ++nv) d.schur_resident[nv] = d.schur_resident_ride[nv] = 1 << 20;
    d.dense4_resident = d.nd_resident[0] = d.nd_resident[1] = 1 << 20;
    d.nd_tpt[0] = 2; d.nd_tpt[1] = 1;
    return d;
}

inline int nv_classes(const Layout &L) { return (L.nv_chunks[1] ? 1 : 0) + (L.nv_chunks[2] ? 1 : 0) + (L.nv_chunks[3] ? 1 : 0); }
inline int used_nv(const Layout &L) { return L.nv_chunks[1] ? 1 : L.nv_chunks[2] ? 2 : 3; }

inline Prob random_problem(std::mt19937_64 &rng)
{
    auto uni = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
    Prob q;
    q.C = uni(0, 2) == 0 ? uni(1, 32) : uni(1, 9);
    q.n_points = uni(4, 90);
    q.B = uni(0, 3) == 0 ? uni(0, 12) : uni(100, 2000);
    const int wide = uni(0, 3) == 0;          // boards seen by more than three cameras
    for (int b = 0; b < q.B; ++b) {
        int k = uni(0, 9) < 1 ? 0 : wide && uni(0, 4) == 0 ? uni(4, 8) : uni(1, 3);
        if (!wide) k = std::min(k, uni(0, 1) ? 2 : 3);
        k = std::min(k, q.C);
        const int m0 = uni(0, q.C - 1);
        for (int i = 0; i < k; ++i) q.add((m0 + i) % q.C, b, uni(1, q.n_points));
    }
    return q;
}

// random residency figures of every launch whose workgroups wait for each other
inline void random_residency(std::mt19937_64 &rng, ExecDevice &d)
{
    auto uni = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
    for (int nv = 1; nv <= 3; ++nv) { d.schur_resident[nv] = uni(1, 4000); d.schur_resident_ride[nv] = uni(1, 4000); }
    d.dense4_resident = uni(1, 2000); d.nd_resident[0] = uni(1, 2000); d.nd_resident[1] = uni(1, 2000);
}

// residency at the exact limit of the riding launches of plan x0 (below = 0) or one workgroup short of it (below = 1): the
// solve launch with every back-substitution workgroup, and k_schur_gram<NV, true> with the reductions
inline void limit_residency(const Layout &L, int C, const ExecPlan &x0, int below, ExecDevice &d)
{
    d.dense4_resident = d.nd_resident[0] = d.nd_resident[1] = 1 + x0.n_prod + L.n_bs_blocks - below;
    const int nv = used_nv(L);
    d.schur_resident_ride[nv] = std::max(reduction_blocks(L, C), L.nv_chunks[nv]) + 1 - below;
}

}  // namespace tscm

#endif
