// tscm_residual_plan.h -- host side of the residual report (tscm.h: tscm_residual_report): the corner order of
// the outputs, every camera's views in problem order (the order k_residual_cameras sums them in) and the chunk lists of
// k_residual_field -- a camera's views that have corners, in problem order, cut where a chunk reaches a target corner
// count.  The field is summed in integers, so where the chunks are cut changes no output byte: the target is a
// performance parameter, and tests lower it to run several chunks on a small problem.
// Plain C++17 like tscm_cov_plan.h; tscm_residuals.hip uploads what plan_residuals returns and
// tests/native/residual_plan_check.cpp checks it on the CPU.
#ifndef TSCM_RESIDUAL_PLAN_H
#define TSCM_RESIDUAL_PLAN_H

#include "../../include/tscm/tscm.h"

#include <string>
#include <utility>
#include <vector>

namespace tscm {

constexpr int kResidualChunkTarget = 8192;      // corners of one k_residual_field workgroup, unless one view has more
constexpr int kResidualMaxCam = 32;

struct ResidualPlan {
    int C = 0, V = 0;
    long long N = 0;                     // corners: the sum of view_count
    std::vector<long long> view_first;   // [V + 1] a view's first corner in corner order (the order of the weights)
    std::vector<int> cam_start;          // [C + 1] CSR into cam_views
    std::vector<int> cam_views;          // every view of a camera, in problem order
    std::vector<long long> cam_corners;  // [C] corners of a camera
    std::vector<int> field_views;        // the views with corners, by camera and in problem order
    std::vector<int> chunk_camera;       // [chunks]
    std::vector<int> chunk_begin, chunk_end;   // [chunks] range of field_views: one camera's views, at least one
};

// 0, or TSCM_E_INVALID and the text naming the argument (out is then untouched).  target: the corner count at which a
// chunk is closed (<= 0: kResidualChunkTarget); a view is never split, so a view larger than the target is a chunk alone.
inline int plan_residuals(int C, int V, const int *view_camera, const int *view_count, int target, ResidualPlan &out, std::string &err)
{
    auto fail = [&err](const std::string &msg) { err = msg; return TSCM_E_INVALID; };
    if (C < 1 || C > kResidualMaxCam) return fail("n_cameras " + std::to_string(C) + " outside 1..32");
    if (V < 0) return fail("n_views is negative");
    if (V > 0 && !view_camera) return fail("view_camera is NULL");
    if (V > 0 && !view_count) return fail("view_count is NULL");
    for (int v = 0; v < V; ++v) {
        if (view_camera[v] < 0 || view_camera[v] >= C) return fail("view_camera[" + std::to_string(v) + "] out of range");
        if (view_count[v] < 0) return fail("view_count[" + std::to_string(v) + "] is negative");
    }
    if (target <= 0) target = kResidualChunkTarget;
    ResidualPlan r;
    r.C = C; r.V = V;
    r.view_first.assign((size_t)V + 1, 0);
    for (int v = 0; v < V; ++v) r.view_first[v + 1] = r.view_first[v] + view_count[v];
    r.N = r.view_first[V];
    r.cam_start.assign((size_t)C + 1, 0);
    r.cam_corners.assign((size_t)C, 0);
    for (int v = 0; v < V; ++v) { r.cam_start[view_camera[v] + 1]++; r.cam_corners[view_camera[v]] += view_count[v]; }
    for (int m = 0; m < C; ++m) r.cam_start[m + 1] += r.cam_start[m];
    r.cam_views.assign((size_t)V, 0);
    {
        std::vector<int> at(r.cam_start.begin(), r.cam_start.end() - 1);
        for (int v = 0; v < V; ++v) r.cam_views[at[view_camera[v]]++] = v;
    }
    for (int m = 0; m < C; ++m) {
        long long in_chunk = 0;
        bool open = false;
        for (int k = r.cam_start[m]; k < r.cam_start[m + 1]; ++k) {
            const int v = r.cam_views[k];
            if (view_count[v] == 0) continue;
            if (open && in_chunk + view_count[v] > target) { r.chunk_end.push_back((int)r.field_views.size()); open = false; }
            if (!open) { r.chunk_camera.push_back(m); r.chunk_begin.push_back((int)r.field_views.size()); in_chunk = 0; open = true; }
            r.field_views.push_back(v);
            in_chunk += view_count[v];
        }
        if (open) r.chunk_end.push_back((int)r.field_views.size());
    }
    out = std::move(r);
    return 0;
}

}  // namespace tscm

#endif
