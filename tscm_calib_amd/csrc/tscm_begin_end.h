// tscm_begin_end.h -- around the LM iterations: the stand-alone control launch (communicator path) and the first and last
// launch of a solve.
#pragma once
// (included from tscm_kernels.h inside namespace tscm)

__global__ __launch_bounds__(256) void k_control(DevProblem P, DevState S, int init)
{
    __shared__ double sm[256];
    ControlPre pre;
    control_prefetch(P, S, init, pre, S.ctrl);
    control_step(P, S, init, pre, sm, S.H_stage, S.H_stage + 256 * P.C, nullptr);
}

// ---------------------------------------------------------------------------------------------
// first and last launch of a solve.  What the host did with five stream operations in front of a solve (control block
// H2D, counter memset, three D2D copies of the start point, a stream synchronisation) and four synchronous copies
// behind it cost 0.25 ms per solve -- as much as two LM iterations of config 4.
// ---------------------------------------------------------------------------------------------
// the control block as the host set it up (kernel argument), the arrival counter of the fused T reduction at zero and,
// with `reset`, the registered start point in buffer 0
// The first launch of a solve also computes the constants of the initial evaluation (round 5: k_begin_solve + k_view_prep were
// 4.8 + 8.0 us in front of every solve): the grid is k_view_prep's, every thread also moves its share of the start point into buffer 0, and the
// constants are computed from where the start point IS (the registered arrays with `reset`, buffer 0 otherwise) -- nothing in
// this launch reads what another of its workgroups writes.  The control block it installs has cur = 0, done = 0.
__global__ __launch_bounds__(kVPrepThreads) void k_begin_view_prep(DevProblem P, DevState S, CtrlHead head, const double *src_cam, const double *src_intr,
                                                                   const double *src_board, double *bak_cam, double *bak_intr, double *bak_board, int with_floats)
{
    // src_*: where the start point is if not in buffer 0 already (the registered arrays with `reset`; the backup on a re-run);
    // bak_*: where a copy of the start point goes (what a re-run of this solve starts from: a late hand-off, tscm_solver.hip)
    const int i0 = blockIdx.x * kVPrepThreads + threadIdx.x, n = gridDim.x * kVPrepThreads;
    if (i0 == 0) { head.t_begin = wall_clock64(); static_cast<CtrlHead &>(*S.ctrl) = head; }
    if (i0 == 0) { *S.t_count = 0; *S.y_flag = 0; *S.fac_fail = 0; S.ctl_pub->epoch = 0; *S.stats_count = 0; *S.stats_flag = 0; }      // every solve starts with the hand-off counters of the fused launches at zero
    const double *cam = src_cam ? src_cam : S.cam_rt[0], *intr = src_intr ? src_intr : S.intr[0], *board = src_board ? src_board : S.board_rt[0];
    for (int i = i0; i < 6 * P.C; i += n) { const double v = cam[i]; if (src_cam) S.cam_rt[0][i] = v; if (bak_cam) bak_cam[i] = v; }
    for (int i = i0; i < 9 * P.C; i += n) { const double v = intr[i]; if (src_intr) S.intr[0][i] = v; if (bak_intr) bak_intr[i] = v; }
    for (int i = i0; i < 6 * P.B; i += n) { const double v = board[i]; if (src_board) S.board_rt[0][i] = v; if (bak_board) bak_board[i] = v; }
    view_prep_body(P, S, 0, with_floats, cam, intr, board);
}

// the accepted point lives in buffer `cur`: it becomes buffer 0 (what the caller downloads and the next resident solve
// starts from)
__global__ __launch_bounds__(256) void k_end_solve(DevState S, int C, int B)
{
    const int i0 = blockIdx.x * 256 + threadIdx.x, n = gridDim.x * 256;
    if (i0 == 0) S.ctrl->t_end = wall_clock64();
    if (S.ctrl->cur == 0) return;
    for (int i = i0; i < 6 * C; i += n) S.cam_rt[0][i] = S.cam_rt[1][i];
    for (int i = i0; i < 9 * C; i += n) S.intr[0][i] = S.intr[1][i];
    for (int i = i0; i < 6 * B; i += n) S.board_rt[0][i] = S.board_rt[1][i];
}

// Last launch of a one-GPU solve whose last evaluation still waits for its control step (the steps in between were taken in
// k_schur_gram's head): k_control_tail, k_end_solve and the copy of the control block to the host in ONE launch (round 5; they
// were three, 10.4 + 5.0 + 4.1 us by rocprofv3 behind every solve).  Block 0 takes and commits the step, stamps the end of the
// solve and writes the control block's head and the iteration log straight into the host's pinned copy; every other block
// derives the step's OUTCOME itself (control_outcome on the snapshot, exactly like a workgroup of k_schur_gram: same inputs,
// same bits, no hand-off) and moves its slice of the accepted point into buffer 0.
__global__ __launch_bounds__(256) void k_finish_solve(DevProblem P, DevState S, int init, int have_backsub, int C, int B, Ctrl *host_ctrl)
{
    constexpr int kHl = 256 * kMaxCamLds + kScal + 8, kGall = 512 * kMaxCamLds;
    __shared__ double sm[256];
    __shared__ double Hl[kHl];
    __shared__ CtlOut s_ctl;
    const CtrlHead *head = S.ctrl_snap;          // (taken by k_reduce_stats: block 0 rewrites S.ctrl while the others may not have started)
    if (blockIdx.x == 0) {
        __shared__ double Gall[kGall];
        finish_evaluation<false>(P, S, init, have_backsub, /*writer=*/true, Hl, Gall, sm, &s_ctl, head);
        __syncthreads();
        if (threadIdx.x == 0) S.ctrl->t_end = wall_clock64();
        __threadfence();
        __syncthreads();
        // head + the log entries written so far, 8-byte words (the host's copy is pinned, device-visible memory)
        const int n_log = min(max(__hip_atomic_load(&S.ctrl->n_log, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0), kMaxLog);
        const int words = (int)((sizeof(CtrlHead) + sizeof(IterLog) * (size_t)n_log) / 8);
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(S.ctrl);
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(host_ctrl);
        for (int i = threadIdx.x; i < words; i += 256) dst[i] = __hip_atomic_load(&src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    control_outcome(P, S, init, have_backsub, Hl, sm, &s_ctl, head);
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(s_ctl.cur) == 0) return;
    const int i0 = (blockIdx.x - 1) * 256 + threadIdx.x, n = (gridDim.x - 1) * 256;
    for (int i = i0; i < 6 * C; i += n) S.cam_rt[0][i] = S.cam_rt[1][i];
    for (int i = i0; i < 9 * C; i += n) S.intr[0][i] = S.intr[1][i];
    for (int i = i0; i < 6 * B; i += n) S.board_rt[0][i] = S.board_rt[1][i];
}
