// tscm_mono_batch.hip -- the batched mono refinement: the host driver of tscm_solve_mono_batch and
// tscm_solve_mono_batch_weighted with the k_mb_* kernels of tscm_mono_batch.h.  A problem of the batch without a corner goes
// through the single-problem solver (tscm_host.h: solve_configured).
#include "tscm/tscm.h"
#include "tscm_host.h"
// what the k_mb_* kernels use of tscm_kernels.h, in its order: the plain headers, then of the stage headers the two without
// kernels of their own (tools/same_kernels.py: the batch kernels' machine code is the same behind either)
#include "tscm_math.h"
#include "tscm_fastmath.h"
#include "tscm_nd_plan.h"
#include "tscm_layout.h"
#include "tscm_exec_plan.h"
#include "tscm_columns.h"
#include "tscm_ctrl.h"
#include "tscm_spec.h"
namespace tscm {
#include "tscm_dev.h"
#include "tscm_geometry.h"
}  // namespace tscm
#include "tscm_launch_seq.h"
#include "tscm_mono_batch.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace tscm;

struct MbStream {
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~MbStream() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); if (s) (void)hipStreamDestroy(s); }
};

// plain pixel RMSE of one problem at its parameters (a robust solve's summary.rmse, as tscm_reprojection_error computes it);
// w: the problem's corner weights or NULL -- sqrt(sum omega s / sum omega), a corner with omega = 0 is not read
static double mb_pixel_rmse(const tscm_problem &p, const double *w = nullptr)
{
    ViewConst vc;
    mono_view_const(p.intr, vc);
    double sq = 0.0, wsum = 0.0;
    long n = 0;
    for (int v = 0; v < p.n_views; ++v) {
        if (p.view_count[v] <= 0) continue;
        const double *rt = p.board_rt + 6 * (size_t)p.view_board[v];
        double bc[kBoardConst];
        board_constants(rt, bc);
        for (int q = 0; q < 3; ++q) { vc.r1[q] = bc[q]; vc.r2[q] = bc[3 + q]; vc.tb[q] = rt[3 + q]; }
        for (int kk = 0; kk < 3; ++kk) for (int q = 0; q < 6; ++q) vc.db[kk][q] = bc[6 + 6 * kk + q];
        for (int j = 0; j < p.view_count[v]; ++j) {
            double r[2], JE[2][kE], JF[2][kFA];
            const int o = p.view_offset[v] + j;
            if (w && !(w[n + j] > 0.0)) continue;
            corner_residual_jacobian(vc, p.board_xy[2 * j], p.board_xy[2 * j + 1], p.obs_u[o], p.obs_v[o], r, JE, JF);
            if (w) { sq += w[n + j] * (r[0] * r[0] + r[1] * r[1]); wsum += w[n + j]; }
            else sq += r[0] * r[0] + r[1] * r[1];
        }
        n += p.view_count[v];
    }
    if (w) return wsum > 0.0 ? std::sqrt(sq / wsum) : 0.0;
    return n ? std::sqrt(sq / (double)n) : 0.0;
}

// weights: [n_problems] pointers to the problems' corner weights (entries may be NULL), or NULL for none
static int solve_mono_batch(const tscm_problem *problems, int n_problems, int device, const tscm_options *opt_in, const unsigned short *fixed,
                            const double *const *weights, int loss_kind, double loss_scale, tscm_summary *summaries)
{
    const double t_call = wall();
    if (!summaries) return tscm_set_error(TSCM_E_INVALID, "summaries is NULL");
    tscm_options opt;
    if (int rc = read_options(opt_in, 1, opt)) return rc;
    BatchPlan bp;
    {
        std::string err;
        if (int rc = plan_batch(problems, n_problems, opt, fixed, loss_kind, loss_scale, bp, err)) return tscm_set_error(rc, err);
    }
    const LossArg loss = bp.loss;
    // corner weights: checked per problem before any device is touched; w_sum / n_kept of each for its summary
    bool any_w = false;
    std::vector<double> w_sum(n_problems, 0.0);
    std::vector<long> n_kept(n_problems, 0);
    for (int i = 0; weights && i < n_problems; ++i) {
        if (!weights[i]) continue;
        if (int rc = check_corner_weights(problems[i].view_count, problems[i].n_views, weights[i], &w_sum[i], &n_kept[i]))
            return tscm_set_error(rc, "problem " + std::to_string(i) + ": " + tscm_last_error());
        any_w = true;
    }
    if (int rc = select_device(device, "tscm_solve_mono_batch")) return rc;
    for (int i = 0; i < n_problems; ++i) std::memset(&summaries[i], 0, sizeof(tscm_summary));

    const int K = bp.K, nc = (int)bp.chunk.size(), ns = (int)bp.slot_prob.size(), B = bp.B;
    double seconds_solve = 0.0;
    if (K > 0) {
        // ---- upload: concatenated observations (slot order), boards, intrinsics; both parameter buffers hold the start point
        std::vector<double> ou((size_t)bp.N), ov((size_t)bp.N), intr((size_t)9 * K), board((size_t)6 * B, 0.0);
        for (int s = 0; s < ns; ++s) {
            const tscm_problem &p = problems[bp.dev_prob[bp.slot_prob[s]]];
            const int v = bp.slot_view[s];
            for (int j = 0; j < bp.slot_count[s]; ++j) { ou[bp.slot_obs[s] + j] = p.obs_u[p.view_offset[v] + j]; ov[bp.slot_obs[s] + j] = p.obs_v[p.view_offset[v] + j]; }
        }
        // the weights in slot order (a problem without weights: 1); a masked corner's observation is uploaded as 0, 0
        std::vector<double> ow(any_w ? (size_t)bp.N : 0);
        for (int k = 0; any_w && k < K; ++k) {
            const tscm_problem &p = problems[bp.dev_prob[k]];
            std::vector<CornerRun> runs;
            for (int s = bp.slot_ptr[k]; s < bp.slot_ptr[k + 1]; ++s) runs.push_back(CornerRun{ bp.slot_view[s], bp.slot_obs[s], bp.slot_count[s] });
            scatter_weights(weights[bp.dev_prob[k]], p.view_count, p.n_views, runs, ow.data(), ou.data(), ov.data());
        }
        for (int k = 0; k < K; ++k) {
            const tscm_problem &p = problems[bp.dev_prob[k]];
            std::memcpy(&intr[9 * (size_t)k], p.intr, 9 * sizeof(double));
            if (p.n_boards) std::memcpy(&board[6 * (size_t)bp.board_ptr[k]], p.board_rt, 6 * sizeof(double) * p.n_boards);
        }
        std::vector<int4> chunk(nc);
        for (int c = 0; c < nc; ++c) chunk[c] = make_int4(bp.chunk[c].x, bp.chunk[c].y, bp.chunk[c].z, 0);

        DeviceMem A;
        MbDev D{};
        D.K = K; D.n_points = bp.n_points; D.n_chunks = nc; D.n_slots = ns; D.loss = loss;
        char *d_ctrl = nullptr;
        const size_t ctrl_bytes = sizeof(CtrlHead) * (size_t)K + sizeof(IterLog) * (size_t)kMaxLog * K;
        HIP_TRY(A.upload(&D.board_xy, problems[0].board_xy, 2 * (size_t)bp.n_points));
        HIP_TRY(A.upload(&D.obs_u, ou)); HIP_TRY(A.upload(&D.obs_v, ov));
        if (any_w) HIP_TRY(A.upload(&D.obs_w, ow));
        HIP_TRY(A.upload(&D.chunk, chunk));
        HIP_TRY(A.upload(&D.chunk_ptr, bp.chunk_ptr)); HIP_TRY(A.upload(&D.board_ptr, bp.board_ptr));      // [K + 1]
        HIP_TRY(A.upload(&D.slot_board, bp.slot_board)); HIP_TRY(A.upload(&D.slot_obs, bp.slot_obs));      // [ns]
        HIP_TRY(A.upload(&D.slot_count, bp.slot_count)); HIP_TRY(A.upload(&D.slot_active, bp.slot_active));
        HIP_TRY(A.upload(&D.mask, bp.mask));                                                                // [K]
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(A.upload(&D.intr[b], intr)); HIP_TRY(A.upload(&D.board[b], board));
            HIP_TRY(A.alloc(&D.rec[b], (size_t)kMbRec * ns)); HIP_TRY(A.alloc(&D.part[b], (size_t)kMbPart * nc)); HIP_TRY(A.alloc(&D.tot[b], (size_t)kMbTot * K));
        }
        HIP_TRY(A.alloc(&D.schur, (size_t)kMbSp * nc)); HIP_TRY(A.alloc(&D.solvep, 4 * (size_t)nc)); HIP_TRY(A.alloc(&D.cam_mp, 4 * (size_t)K));
        HIP_TRY(A.alloc(&D.s_b, 6 * (size_t)ns)); HIP_TRY(A.alloc(&D.s_f, 7 * (size_t)K));
        HIP_TRY(A.alloc(&d_ctrl, ctrl_bytes)); HIP_TRY(A.alloc(&D.n_done, 1)); HIP_TRY(A.alloc(&D.out, 9 * (size_t)K + 6 * (size_t)B));
        D.head = reinterpret_cast<CtrlHead *>(d_ctrl);
        D.log = reinterpret_cast<IterLog *>(d_ctrl + sizeof(CtrlHead) * (size_t)K);

        // ---- the loop: four launches per iteration for the whole batch; the host polls the count of terminated problems
        MbStream ms;
        HIP_TRY(hipStreamCreateWithFlags(&ms.s, hipStreamNonBlocking));
        HIP_TRY(hipEventCreate(&ms.e0)); HIP_TRY(hipEventCreate(&ms.e1));
        const hipStream_t st = ms.s;
        const CtrlHead head = ctrl_head_from_options(opt);
        const size_t lds_eval = sizeof(double) * (2 * kMbJw + 1) * (size_t)bp.n_points;
        HIP_TRY(hipEventRecord(ms.e0, st));
        hipLaunchKernelGGL(k_mb_begin, dim3((K + 255) / 256), dim3(256), 0, st, D, head);
        hipLaunchKernelGGL(k_mb_eval, dim3(nc), dim3(kMbThreads), lds_eval, st, D, 1);
        hipLaunchKernelGGL(k_mb_control, dim3(K), dim3(64), 0, st, D, 1);
        HIP_TRY(hipGetLastError());
        const int check_every = std::max(1, opt.check_every);
        for (int it = 1; it <= opt.max_num_iterations; ++it) {
            hipLaunchKernelGGL(k_mb_schur, dim3(nc), dim3(kMbThreads), 0, st, D);
            hipLaunchKernelGGL(k_mb_solve, dim3(nc), dim3(kMbThreads), 0, st, D);
            hipLaunchKernelGGL(k_mb_eval, dim3(nc), dim3(kMbThreads), lds_eval, st, D, 0);
            hipLaunchKernelGGL(k_mb_control, dim3(K), dim3(64), 0, st, D, 0);
            HIP_TRY(hipGetLastError());
            if (it % check_every == 0 && it < opt.max_num_iterations) {
                int done = 0;
                HIP_TRY(hipMemcpyAsync(&done, D.n_done, sizeof(int), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                if (done >= K) break;
            }
        }
        hipLaunchKernelGGL(k_mb_finish, dim3(K), dim3(256), 0, st, D);
        HIP_TRY(hipEventRecord(ms.e1, st));
        std::vector<double> out(9 * (size_t)K + 6 * (size_t)B);
        std::vector<char> ctrl(ctrl_bytes);
        HIP_TRY(hipMemcpyAsync(out.data(), D.out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(ctrl.data(), d_ctrl, ctrl_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipGetLastError());
        float ms_solve = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms_solve, ms.e0, ms.e1));
        seconds_solve = 1e-3 * (double)ms_solve;

        // ---- results: parameters in place, one summary per problem
        const CtrlHead *heads = reinterpret_cast<const CtrlHead *>(ctrl.data());
        const IterLog *logs = reinterpret_cast<const IterLog *>(ctrl.data() + sizeof(CtrlHead) * (size_t)K);
        for (int k = 0; k < K; ++k) if (!heads[k].done) return tscm_set_error(TSCM_E_HIP, "device LM loop of a batch problem did not terminate");
        for (int k = 0; k < K; ++k) {
            const int i = bp.dev_prob[k];
            const tscm_problem &p = problems[i];
            const CtrlHead &h = heads[k];
            tscm_summary *sum = &summaries[i];
            std::memcpy(p.intr, &out[9 * (size_t)k], 9 * sizeof(double));
            if (p.n_boards) std::memcpy(p.board_rt, &out[9 * (size_t)K + 6 * (size_t)bp.board_ptr[k]], 6 * sizeof(double) * p.n_boards);
            const long N_k = bp.obs_ptr[k + 1] - bp.obs_ptr[k];
            fill_summary(h, logs + (size_t)kMaxLog * k, N_k, sum);
            const double *w = weights ? weights[i] : nullptr;
            if (w) {
                sum->n_residual_blocks = (int)n_kept[i];
                sum->rmse = w_sum[i] > 0.0 ? std::sqrt(2.0 * h.x_cost / w_sum[i]) : 0.0;
            }
            if (loss.kind != TSCM_LOSS_NONE) sum->rmse = mb_pixel_rmse(p, w);
        }
    }
    // problems without a single corner: what the single-problem entry point returns for them
    for (int i = 0; i < n_problems; ++i) {
        if (bp.dev_of[i] >= 0) continue;
        if (int rc = solve_configured(&problems[i], opt_in, SolveSpec{ loss, fixed ? fixed + i : nullptr, nullptr, nullptr }, &summaries[i])) return rc;
    }
    // the batch's times in every summary
    const double t_end = wall();
    for (int i = 0; i < n_problems; ++i) { summaries[i].seconds_total = t_end - t_call; summaries[i].seconds_solve = seconds_solve; }
    return 0;
}

extern "C" int tscm_solve_mono_batch(const tscm_problem *problems, int n_problems, int device, const tscm_options *opt_in,
                                     const unsigned short *fixed, int loss_kind, double loss_scale, tscm_summary *summaries)
{
    return solve_mono_batch(problems, n_problems, device, opt_in, fixed, nullptr, loss_kind, loss_scale, summaries);
}

extern "C" int tscm_solve_mono_batch_weighted(const tscm_problem *problems, int n_problems, int device, const tscm_options *opt_in,
                                              const unsigned short *fixed, const double *const *weights, int loss_kind, double loss_scale,
                                              tscm_summary *summaries)
{
    return solve_mono_batch(problems, n_problems, device, opt_in, fixed, weights, loss_kind, loss_scale, summaries);
}
