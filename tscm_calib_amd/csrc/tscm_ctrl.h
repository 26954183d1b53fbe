// tscm_ctrl.h -- the head of the device-resident LM control block: what the host installs at the start of a solve
// (k_begin_view_prep's argument, tscm_launch_seq.h: ctrl_head_from_options) and reads back at its end, and the kernels
// read and write in between, and the trust-region step that advances it (lm_step).  Plain C++17, shared by the host planning
// headers, tscm_kernels.h and tscm_mono_batch.h.
#ifndef TSCM_CTRL_H
#define TSCM_CTRL_H

#include <cstddef>
#include <float.h>
#include <math.h>

#ifdef __HIPCC__
#define TSCM_CTRL_FN __host__ __device__ __forceinline__
#else
#define TSCM_CTRL_FN inline
#endif

namespace tscm {

constexpr int kMaxLog = 256;

struct Options {
    int max_num_iterations;
    double function_tolerance, gradient_tolerance, parameter_tolerance;
    double initial_radius, max_radius, min_radius;
    double min_relative_decrease, min_lm_diagonal, max_lm_diagonal;
    int max_invalid;
    int jacobi_scaling;
};

enum TermReason { kNone = 0, kMaxIter, kGradTol, kMinRadius, kParamTol, kFuncTol, kInvalidSteps };

struct IterLog {
    int iteration, step_is_valid, step_is_successful, pad;
    double cost, cost_change, gradient_max_norm, gradient_norm, step_norm, relative_decrease, radius;
};

struct CtrlHead {
    // ---- header (polled by the host) ----
    int done, term_type, term_reason, iteration;
    int cur, lin_fail, num_successful, num_unsuccessful;
    int num_invalid, n_log, lm_iterations, fin_count;   // fin_count: arrival counter of k_reduce_control
    int fault, inert_cols;              // fault: a device-side hand-off timed out (sticky; the host turns it into TSCM_E_HIP)
                                        // inert_cols: the program has free columns without a Jacobian (has_inert_columns)
    double radius, decrease_factor;
    double x_cost, x_norm, gmax, gnorm;
    double model_cam, stepsq_cam;
    double se_min, se_cur, se_ref, se_cand, se_acc_ref, se_acc_cand;
    double initial_cost;
    Options opt;
    long long t_begin, t_end;           // s_memrealtime (100 MHz) in k_begin_solve / k_end_solve: device time of the solve
};

// the bytes the kernels were built against: the host and the device must agree on every offset (the host polls the first
// 64 bytes of the block, copies the head and the log, and passes the head as a kernel argument)
static_assert(sizeof(Options) == 88 && offsetof(Options, function_tolerance) == 8 && offsetof(Options, max_invalid) == 80, "Options layout");
static_assert(sizeof(IterLog) == 72 && offsetof(IterLog, cost) == 16, "IterLog layout");
static_assert(offsetof(CtrlHead, fault) == 48 && offsetof(CtrlHead, radius) == 56 && offsetof(CtrlHead, initial_cost) == 168 &&
              offsetof(CtrlHead, opt) == 176 && offsetof(CtrlHead, t_begin) == 264 && sizeof(CtrlHead) == 280, "CtrlHead layout");

// the scalars of one evaluated point: the start point (init) or the candidate of an iteration
struct StepInput {
    double cost, gmax, gnorm, xnorm;    // cost, |x - Plus(x, -g)|_inf and its 2-norm, |x|
    double model_cost_change;           // -(J h)^T (r + J h / 2): positive for a descent step (Ceres' sign)
    double step_norm;                   // |h|, square-rooted
};

// The skew intrinsics b and c have no Jacobian column.  Ceres keeps them in its program where they are not held: their damped
// pivots are clamp(0, min_lm_diagonal, max_lm_diagonal) / radius, and a pivot that is not > 0 fails its factorisation, so the
// step is invalid (min_lm_diagonal = 0, or one that underflows over the radius).  The kernels leave the two columns out of their
// systems; the control step takes the decision in their place.  A camera's word f leaves b or c in the program unless it holds
// both (SubsetManifold) or holds all of fx .. alpha (SetParameterBlockConstant: the whole block, b and c with it, leaves the
// program -- block_const of plan_columns and k_mb_control).  fixed: the TSCM_FIX_* word of each of the n cameras (null: none
// held), active: whether the camera has views in the whole job (null: all have).
constexpr unsigned kInertFixBits = 128 | 256;              // TSCM_FIX_B | TSCM_FIX_C
constexpr unsigned kBlockFixBits = 127;                    // TSCM_FIX_INTRINSICS
TSCM_CTRL_FN bool inert_free(unsigned f) { return (f & kInertFixBits) != kInertFixBits && (f & kBlockFixBits) != kBlockFixBits; }
inline int has_inert_columns(const unsigned short *fixed, const unsigned char *active, int n)
{
    for (int m = 0; m < n; ++m)
        if ((!active || active[m]) && (!fixed || inert_free(fixed[m]))) return 1;
    return 0;
}

// One step of the LM control (TrustRegionMinimizer + LevenbergMarquardtStrategy + TrustRegionStepEvaluator) on the head c,
// for every route of the library.  `init` = IterationZero; otherwise the tail of one loop iteration followed by
// FinalizeIterationAndCheckIfMinimizerCanContinue.  tgt: the buffer that holds the evaluated point (c.cur becomes tgt when
// the step is accepted).  c.lin_fail (a factorisation failed: the step is invalid) is set by the caller, read and cleared
// here.  Returns whether `it` is a log entry, then meant for slot c.n_log - 1: the invalid-step limit and the parameter and
// function tolerances terminate without one, as in Ceres.  Touches nothing but its arguments (tests/native/ctrl_step_check.cpp
// runs it on the CPU).
TSCM_CTRL_FN bool lm_step(CtrlHead &c, int init, int tgt, const StepInput &in, IterLog &it)
{
    const Options &o = c.opt;
    it.pad = 0;
    if (init) {
        c.x_cost = in.cost; c.initial_cost = in.cost; c.x_norm = in.xnorm; c.gmax = in.gmax; c.gnorm = in.gnorm;
        c.se_min = c.se_cur = c.se_ref = c.se_cand = in.cost; c.se_acc_ref = 0.0; c.se_acc_cand = 0.0;
        it.iteration = 0; it.step_is_valid = 1; it.step_is_successful = 1;
        it.cost = in.cost; it.cost_change = 0.0; it.gradient_max_norm = in.gmax; it.gradient_norm = in.gnorm;
        it.step_norm = 0.0; it.relative_decrease = 0.0;
        c.iteration = 0;
    } else {
        c.iteration += 1;
        c.lm_iterations += 1;
        it.iteration = c.iteration;
        const double model = in.model_cost_change;
        const double step_norm = in.step_norm;
        const bool inert_fail = c.inert_cols && !(fmin(fmax(0.0, o.min_lm_diagonal), o.max_lm_diagonal) / c.radius > 0.0);
        const bool valid = !c.lin_fail && !inert_fail && isfinite(model) && isfinite(step_norm) && model > 0.0;
        c.lin_fail = 0;
        it.step_is_valid = valid ? 1 : 0;
        it.gradient_max_norm = c.gmax; it.gradient_norm = c.gnorm;
        if (!valid) {
            // HandleInvalidStep
            if (++c.num_invalid >= o.max_invalid) { c.done = 1; c.term_type = 2; c.term_reason = kInvalidSteps; return false; }
            c.radius = c.radius / c.decrease_factor; c.decrease_factor *= 2.0;
            it.cost = c.x_cost; it.cost_change = 0.0; it.step_norm = 0.0; it.relative_decrease = 0.0; it.step_is_successful = 0;
        } else {
            c.num_invalid = 0;
            double cand = in.cost;
            if (!isfinite(cand)) cand = DBL_MAX;
            it.step_norm = step_norm;
            it.cost_change = c.x_cost - cand;
            it.cost = c.x_cost;
            it.relative_decrease = 0.0;
            it.step_is_successful = 0;
            // ParameterToleranceReached / FunctionToleranceReached: return before accepting
            if (step_norm <= o.parameter_tolerance * (c.x_norm + o.parameter_tolerance)) {
                c.done = 1; c.term_type = 0; c.term_reason = kParamTol; return false;
            }
            if (fabs(it.cost_change) <= o.function_tolerance * c.x_cost) {
                c.done = 1; c.term_type = 0; c.term_reason = kFuncTol; return false;
            }
            double q;
            if (cand >= DBL_MAX) q = -DBL_MAX;
            else {
                const double rel = (c.se_cur - cand) / model;
                const double hist = (c.se_ref - cand) / (c.se_acc_ref + model);
                q = rel > hist ? rel : hist;
            }
            it.relative_decrease = q;
            if (q > o.min_relative_decrease) {
                // HandleSuccessfulStep
                c.cur = tgt;
                c.x_cost = cand; c.x_norm = in.xnorm; c.gmax = in.gmax; c.gnorm = in.gnorm;
                it.cost = cand; it.gradient_max_norm = in.gmax; it.gradient_norm = in.gnorm;
                it.step_is_successful = 1;
                { const double w = 2.0 * q - 1.0; c.radius = c.radius / fmax(1.0 / 3.0, 1.0 - w * w * w); }
                c.radius = fmin(o.max_radius, c.radius);
                c.decrease_factor = 2.0;
                c.se_cur = cand; c.se_acc_cand += model; c.se_acc_ref += model;
                if (c.se_cur < c.se_min) { c.se_min = c.se_cur; c.se_cand = c.se_cur; c.se_acc_cand = 0.0; }
                else if (c.se_cur > c.se_cand) { c.se_cand = c.se_cur; c.se_acc_cand = 0.0; }
                c.se_ref = c.se_cand; c.se_acc_ref = c.se_acc_cand;
            } else {
                it.cost = cand;
                c.radius = c.radius / c.decrease_factor; c.decrease_factor *= 2.0;
            }
        }
    }
    // FinalizeIterationAndCheckIfMinimizerCanContinue
    if (it.step_is_successful) ++c.num_successful; else ++c.num_unsuccessful;
    it.radius = c.radius;
    ++c.n_log;
    if (it.iteration >= o.max_num_iterations) { c.done = 1; c.term_type = 1; c.term_reason = kMaxIter; }
    else if (it.step_is_successful && it.gradient_max_norm <= o.gradient_tolerance) { c.done = 1; c.term_type = 0; c.term_reason = kGradTol; }
    else if (c.radius <= o.min_radius) { c.done = 1; c.term_type = 0; c.term_reason = kMinRadius; }
    return true;
}

}  // namespace tscm

#endif
