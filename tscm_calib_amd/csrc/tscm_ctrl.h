// tscm_ctrl.h -- the head of the device-resident LM control block: what the host installs at the start of a solve
// (k_begin_view_prep's argument, tscm_launch_seq.h: ctrl_head_from_options) and reads back at its end, and the kernels
// read and write in between.  Plain C++17, shared by the host planning headers and tscm_kernels.h.
#ifndef TSCM_CTRL_H
#define TSCM_CTRL_H

#include <cstddef>

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

struct IterLog {
    int iteration, step_is_valid, step_is_successful, pad;
    double cost, cost_change, gradient_max_norm, gradient_norm, step_norm, relative_decrease, radius;
};

struct CtrlHead {
    // ---- header (polled by the host) ----
    int done, term_type, term_reason, iteration;
    int cur, lin_fail, num_successful, num_unsuccessful;
    int num_invalid, n_log, lm_iterations, fin_count;   // fin_count: arrival counter of k_reduce_control
    int fault, pad0;                    // fault: a device-side hand-off timed out (sticky; the host turns it into TSCM_E_HIP)
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

}  // namespace tscm

#endif
