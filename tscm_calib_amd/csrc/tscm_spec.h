// tscm_spec.h -- what a solve is configured with beyond its problem and options: the robust loss, the held
// intrinsics, the corner weights and the camera priors.  One struct, the refusals of its
// parts, the permutation that brings a caller's weights into a device's corner order, and the prior tables a device takes.
// Every entry point that takes a loss, a mask, weights or priors goes through here (tscm_solver.hip, tscm_batch_plan.h,
// tscm_covariance.hip), so the next per-solve feature is a field of SolveSpec.  Plain C++17 like tscm_layout.h;
// tests/native/spec_check.cpp and prior_check.cpp check it on the CPU.
#ifndef TSCM_SPEC_H
#define TSCM_SPEC_H

#include "../../include/tscm/tscm.h"

#include <cmath>
#include <string>
#include <vector>

namespace tscm {

// a loss as the robust Gram kernels take it (kernel argument, tscm_geometry.h: robust_rho): a the scale in pixels, b = a^2,
// c = 1 / b, as Ceres' constructors compute them; kind TSCM_LOSS_NONE carries zeros
struct LossArg { double a, b, c; int kind, pad; };

// An entry point hands its arguments on as spec_args(): kind and scale as the caller gave them, in loss.kind / loss.a.
// make_spec() checks them and completes the loss; only its output configures a solver.
struct SolveSpec {
    LossArg loss;
    const unsigned short *fixed;        // [n_cameras] mask words (TSCM_FIX_*), or NULL: nothing held
    const double *weights;              // [sum of view_count] in the problem's corner order, or NULL: none
    const tscm_camera_priors *priors;   // Gaussian priors on camera-side coordinates, or NULL: none
};
inline SolveSpec spec_args(int kind, double scale, const unsigned short *fixed, const double *weights, const tscm_camera_priors *priors = nullptr)
{
    return SolveSpec{ LossArg{ scale, 0.0, 0.0, kind, 0 }, fixed, weights, priors };
}

// The loss and the masks of a call, checked before any device is touched: 0, or TSCM_E_INVALID and its message in err (spec
// is then untouched).  fixed: [n_cameras] mask words or NULL.  spec.weights and spec.priors come back NULL:
// check_corner_weights and check_camera_priors need the problem.
inline int make_spec(int kind, double scale, const unsigned short *fixed, int n_cameras, SolveSpec &spec, std::string &err)
{
    if (kind < TSCM_LOSS_NONE || kind > TSCM_LOSS_CAUCHY) { err = "unknown loss kind"; return TSCM_E_INVALID; }
    LossArg L{};
    if (kind != TSCM_LOSS_NONE) {
        if (!std::isfinite(scale) || !(scale > 0.0)) { err = "the scale of a loss must be finite and > 0"; return TSCM_E_INVALID; }
        L.kind = kind; L.a = scale; L.b = scale * scale; L.c = 1.0 / L.b;
    }
    if (fixed)
        for (int m = 0; m < n_cameras; ++m)
            if (fixed[m] & ~TSCM_FIX_ALL) { err = "unknown bits in a fixed-intrinsics mask (bits 0-8 only)"; return TSCM_E_INVALID; }
    spec = SolveSpec{ L, fixed, nullptr, nullptr };
    return 0;
}

// corner weights [sum of view_count] in the problem's corner order (views in problem order, corners in order): checked before any
// device is touched.  sum / kept: the sum of the weights and the number of corners with a weight > 0
inline int check_corner_weights(const int *view_count, int n_views, const double *w, std::string &err, double *sum = nullptr, long *kept = nullptr)
{
    double sm = 0.0;
    long k = 0, n = 0;
    for (int v = 0; v < n_views; ++v) {
        bool any = false;
        for (int j = 0; j < view_count[v]; ++j, ++n) {
            const double x = w[n];
            if (!std::isfinite(x) || x < 0.0) {
                err = "corner weight " + std::to_string(n) + " (view " + std::to_string(v) + ", corner " + std::to_string(j) + ") is negative, NaN or infinite";
                return TSCM_E_INVALID;
            }
            if (x > 0.0) { any = true; ++k; sm += x; }
        }
        if (view_count[v] > 0 && !any) {
            err = "every corner weight of view " + std::to_string(v) + " is 0: pass view_count = 0 for a view without corners";
            return TSCM_E_INVALID;
        }
    }
    if (sum) *sum = sm;
    if (kept) *kept = k;
    return 0;
}

// `count` corners of the problem's view `view`, in order, at [first, first + count) of a device's corner order: a view of a
// solver's layout (a shard keeps a subset of the views, in its own order), a slot of a batch
struct CornerRun { int view; long first; int count; };

// The caller's weights (checked; NULL: every weight is 1) from the problem's corner order into the device's: w[k] for every
// corner k of the runs.  u, v: the observations as created, in device order -- a corner whose weight is not > 0 gets 0, 0
// there (a masked corner's observation may hold anything, NaN included; no other entry is written).
inline void scatter_weights(const double *weights, const int *view_count, int n_views, const std::vector<CornerRun> &runs, double *w, double *u, double *v)
{
    std::vector<long> first((size_t)n_views + 1, 0);        // view -> its first corner in the problem's corner order
    for (int i = 0; i < n_views; ++i) first[i + 1] = first[i] + view_count[i];
    for (const CornerRun &r : runs)
        for (int j = 0; j < r.count; ++j) {
            const double x = weights ? weights[first[r.view] + j] : 1.0;
            w[r.first + j] = x;
            if (!(x > 0.0)) { u[r.first + j] = 0.0; v[r.first + j] = 0.0; }
        }
}

// camera priors (tscm.h: tscm_camera_priors) of a problem of n_cameras cameras, checked before any device is touched: 0, or
// TSCM_E_INVALID and its message, naming the argument, in err.  NULL is no priors.
inline int check_camera_priors(const tscm_camera_priors *pr, int n_cameras, std::string &err)
{
    if (!pr) return 0;
    if (pr->struct_size != sizeof(tscm_camera_priors)) { err = "priors: struct_size is not sizeof(tscm_camera_priors)"; return TSCM_E_INVALID; }
    struct Part { const char *name; const double *mean, *weight; int n; };
    const Part parts[2] = { { "cam_rt", pr->cam_rt_mean, pr->cam_rt_weight, 6 }, { "intr", pr->intr_mean, pr->intr_weight, 9 } };
    for (const Part &q : parts) {
        if (!q.mean != !q.weight) {
            err = std::string("priors: ") + q.name + (q.mean ? "_mean is given without its " : "_weight is given without its ") + q.name + (q.mean ? "_weight" : "_mean");
            return TSCM_E_INVALID;
        }
        if (!q.mean) continue;
        for (int i = 0; i < q.n * n_cameras; ++i) {
            const std::string at = "[" + std::to_string(i) + "] (camera " + std::to_string(i / q.n) + ", coordinate " + std::to_string(i % q.n) + ")";
            if (!std::isfinite(q.weight[i]) || q.weight[i] < 0.0) { err = std::string("priors: ") + q.name + "_weight" + at + " is negative, NaN or infinite"; return TSCM_E_INVALID; }
            if (q.weight[i] > 0.0 && !std::isfinite(q.mean[i])) { err = std::string("priors: ") + q.name + "_mean" + at + " is not finite where its weight is > 0"; return TSCM_E_INVALID; }
        }
    }
    return 0;
}

// What a device takes of checked priors: mean and weight per camera-side column, [n_cameras][16] each in the column order of a
// camera tile (0-5 the pose, 6-14 the intrinsics fx fy cx cy xi lambda alpha b c, 15 padding), the weight 0 -- and the mean 0
// with it -- where the column is not free.  col_free: [16 * n_cameras], != 0 where the column is a free column of the solve
// (ColumnPlan::col_active of plan_columns: never b, c or the padding).  Returns the number of effective priors (weight > 0).
inline int effective_priors(const tscm_camera_priors *pr, int n_cameras, const unsigned char *col_free, std::vector<double> &mean, std::vector<double> &weight)
{
    mean.assign((size_t)16 * n_cameras, 0.0);
    weight.assign((size_t)16 * n_cameras, 0.0);
    if (!pr) return 0;
    int n = 0;
    for (int m = 0; m < n_cameras; ++m)
        for (int a = 0; a < 15; ++a) {
            const double *w = a < 6 ? pr->cam_rt_weight : pr->intr_weight, *mu = a < 6 ? pr->cam_rt_mean : pr->intr_mean;
            const size_t k = a < 6 ? 6 * (size_t)m + a : 9 * (size_t)m + (a - 6);
            if (!w || !col_free[16 * m + a] || !(w[k] > 0.0)) continue;
            weight[16 * (size_t)m + a] = w[k];
            mean[16 * (size_t)m + a] = mu[k];
            ++n;
        }
    return n;
}

}  // namespace tscm

#endif
