// tscm_backsub.h -- stage 5, the back-substitution of the board steps and the candidate's per-view constants; its body
// also runs inside the fused reduced-solve launches (stage 4), which is why it is included in front of them.
#pragma once
// (included from tscm_kernels.h inside namespace tscm)

// Back-substitution of the board steps (SchurEliminator::BackSubstitute) AND the per-view constants of the candidate
// point (what k_view_prep computes for the initial point) in one launch.  A workgroup of NTH threads owns NTH / 8
// consecutive boards, whose views are consecutive record slots.  Small workgroups on purpose: the kernel streams the W
// region, a CU sustains ~20 GB/s of it, so the time is set by the CU with the most bytes -- thousands of small
// workgroups spread evenly, a few hundred large ones leave CUs with one or with two of them (measured: 2.3 TB/s).
//   phase A  q_b = sum_v W_v yhat[m_v]: 16 lanes per slot, lane a loads column a of the slot's W record (six adjacent doubles,
//            three 16-byte loads) straight into registers, multiplies by yhat[m_v][a] and the 16 lanes sum (DPP).  Round 5:
//            before, the records of a round were read flat into LDS and the columns taken from there -- two barriers and an LDS
//            round trip per round of 32 slots, with the next round's loads behind the first; tools/ubench_stream.hip: the column
//            pattern streams exactly as fast as the flat one (7.1 TB/s).  Everything of a round of 64 slots is requested at once
//   phase B  one lane per board: y_b = L^{-T} (z - L^{-1} S_b q_b);  delta_b = -s_b y_b;  candidate = x + delta
//            (sum_v Y_v yhat = L^{-1} S_b sum_v W_v yhat: one forward substitution per board);  the candidate rotations
//            R_c of the cameras are prepared by lanes of the second wave
//   phase C  one lane per view of these boards: board rotation columns, t_b and R_c dR_b/dw of the candidate, staged in
//            LDS and written as 256-byte records (vconst, see k_view_prep); workgroup 0 also writes the per-camera records
// grid ceil(B / (NTH / 8)) x NTH, dynamic LDS BsGeom<NTH>::kLds doubles
// NTH threads own NTH / 8 boards; a round of phase A is 32 slots = 2688 doubles of W (21 per thread at 128 threads, 10.5
// at 256: the last load of a thread is masked), the factor records are 7 doubles per thread.  Two geometries: 128
// threads / 16 boards (thousands of small workgroups: balanced on mid-size problems) and 256 threads / 32 boards for
// problems with more groups of 16 than fit the chip at once -- the serial phases B and C cost a workgroup the same ~5 us
// whatever its size, so larger workgroups halve their share per board.
constexpr int kBsTile = 64;        // views per round of phase C
template <int NTH> struct BsGeom {
    static constexpr int kBoards = NTH / 8;
    static constexpr int kPassSlots = NTH / 16;                                        // phase A: 16 lanes per slot
    static constexpr int kPasses = 4;                                                  // ... four passes per round: 24 doubles of W per thread
    static constexpr int kRoundSlots = kPasses * kPassSlots;                           // 64 slots at 256 threads, 32 at 128
    static constexpr int kLdsA = kRoundSlots * 6, kLdsB = kBoards * kFac, kLdsC = kBsTile * (kVFloatOff + 1);
    static constexpr int kLds = kLdsC > kLdsB ? (kLdsC > kLdsA ? kLdsC : kLdsA) : (kLdsB > kLdsA ? kLdsB : kLdsA);     // dynamic LDS, doubles
    static_assert(kBoards * kFac == 7 * NTH, "the factor records are 7 doubles per thread");
    static_assert(kBoards <= 64 && 64 + kMaxCam <= NTH, "lane roles of phase B: the boards in wave 0, the cameras from wave 1 on");
};

// epoch: 1, 2, ... = the number of fused launches of this solve so far, this one included (the host resets the
// counter to zero in front of every solve).  The arrival counter is MONOTONIC: a launch waits for epoch * producers,
// so late arrivals of a launch that was given up on can never be mistaken for this launch's.
// WAIT: the workgroup runs inside the reduced solve's launch (k_solve_reduced<..., true>, one GPU).  Everything that does
// not depend on the camera step -- the first round of W records, the factor records, the boards' poses -- is requested
// at once; then thread 0 waits for the solver's flag (y_flag = 2 * epoch + lin_fail, monotonic like the T counter and
// with the same time bound) while the solver workgroup works, alone on the chip otherwise.  What the solver wrote is
// written through (handoff_store) and read behind an acquire fence.
template <int NTH, bool WAIT>
__device__ __forceinline__ void backsub_body(const DevProblem &P, const DevState &S, int with_floats, const int blk, const int nblk, const int epoch, const int t_need)
{
    constexpr int kBsBoards = BsGeom<NTH>::kBoards, kBsThreads = NTH, kPassSlots = BsGeom<NTH>::kPassSlots, kPasses = BsGeom<NTH>::kPasses, kRoundSlots = BsGeom<NTH>::kRoundSlots;
    constexpr int kBsCamLane0 = 64;
    // head: control block and slot range in one round trip
    const int b0 = blk * kBsBoards;
    const int nbl = min(kBsBoards, P.B - b0);
    const int s0 = P.bv_ptr[b0], s1 = P.bv_ptr[b0 + nbl];                // the views of these boards: slots [s0, s1)
    const int ctrl_done = S.ctrl->done, cur = S.ctrl->cur;
    int fail = WAIT ? 0 : S.ctrl->lin_fail;
    if (ctrl_done) return;
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    double (*s_qv)[6] = reinterpret_cast<double (*)[6]>(dyn);     // [kRoundSlots][6] W yhat per slot of the round   phase A
    double *s_fac = dyn;                                   // [kBsBoards][kFac]   phase B
    double *st_all = dyn;                                  // [kBsTile][kVFloatOff + 1]  phase C
    __shared__ double s_q[kBsBoards][6], s_new[kBsBoards][6];
    __shared__ double s_yh[16 * kMaxCam];                  // phase A
    // candidate R_c (9) and t_c (3), phases B and C: in the space of s_yh, which phase A is done with.  The workgroup's
    // LDS (static + dynamic) has to stay under 32 KB: config 1's 1250 workgroups are then resident at once, five per CU;
    // 768 bytes more (s_rc on its own, round 3) made it four per CU, a second round of workgroups and 22 us for 17.8
    double (*s_rc)[12] = reinterpret_cast<double (*)[12]>(s_yh);
    static_assert(12 * kMaxCam <= 16 * kMaxCam, "s_rc aliases s_yh");
    __shared__ double sm[16];
    __shared__ int s_view[kBsTile];
    const int t = threadIdx.x;
    PHASE_STAMP(ts0);
    // ---- everything whose address is known is requested now ---------------------------------------------------------
    const int my_q0 = t < nbl ? P.bv_ptr[b0 + t] : 0, my_q1 = t < nbl ? P.bv_ptr[b0 + t + 1] : 0;
    // (phase C's view / board / camera of the first tile: used at the end)
    const int c_slot = min(s0 + t, max(s1 - 1, 0));
    const int c_view = s1 > s0 ? P.slot_view[c_slot] : 0, c_board = s1 > s0 ? P.slot_board[c_slot] : 0, c_cam = s1 > s0 ? P.slot_cam[c_slot] : 0;
    // (phase B's current pose and Jacobi scaling of this lane's board)
    double xb[6], sbv[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { xb[k] = t < nbl ? S.board_rt[cur][6 * (b0 + t) + k] : 0.0; sbv[k] = t < nbl ? S.s_b[6 * (b0 + t) + k] : 1.0; }
    // (phase B's factor records: the boards' records are contiguous, 7 doubles per thread)
    double facv[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) facv[j] = S.fac[(size_t)kFac * b0 + min(t + kBsThreads * j, nbl * kFac - 1)];
    if constexpr (!WAIT) { for (int i = t; i < P.n_pad; i += kBsThreads) s_yh[i] = S.yhat[i]; }
    if (t < kBsBoards * 6) (&s_q[0][0])[t] = 0.0;
    // the candidate's per-camera records (rotation, left-Jacobian vectors, intrinsics: write_camera_record): one camera
    // per workgroup, by the first lane of the second wave while the loads requested above are in flight -- a serial
    // chain of a few hundred operations that cost workgroup 0 4.6 us when it did all cameras after its board solves
    if constexpr (!WAIT) { if (t == 64) for (int m = blk; m < P.C; m += nblk) write_camera_record(S, cur ^ 1, m); }
    // ---- phase A -----------------------------------------------------------------------------------------------------
    {
        const int grp = t >> 4, a = t & 15;
        const __amdgpu_buffer_rsrc_t r_w = make_rsrc(S.rec[cur], sizeof(double) * (size_t)kRecW * P.V);      // (the W region only: a slot behind s1 - 1 is never addressed)
        constexpr unsigned BAD = 0xffffe000u;
        // column a of the W records of this lane's slot in each of the round's passes, and the slot's camera
        double w[kPasses][6];
        int camv[kPasses];
        auto request = [&](int rbase) {
#pragma unroll
            for (int j = 0; j < kPasses; ++j) {
                const int slot = rbase + kPassSlots * j + grp;
                const unsigned off = (a < kFA && slot < s1) ? 8u * ((unsigned)kRecW * (unsigned)slot + 6u * (unsigned)a) : BAD;
#pragma unroll
                for (int k = 0; k < 3; ++k) { const d2 v = buf_load_2f64(r_w, off, 16u * (unsigned)k); w[j][2 * k] = v[0]; w[j][2 * k + 1] = v[1]; }
                camv[j] = P.slot_cam[min(slot, max(s1 - 1, 0))];
            }
        };
        request(s0);
        if constexpr (WAIT) {
            __shared__ int s_flag;
            if (t == 0) {
                const long long t_start = wall_clock64();
                int f;
                while (((f = __hip_atomic_load(S.y_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 1) < epoch) {
                    __builtin_amdgcn_s_sleep(8);
                    if (wall_clock64() - t_start > kHandoffTimeoutTicks) { f = -1; break; }
                }
                if (f < 0) {             // the solver never reported: a device fault (see k_solve_reduced), not a failed step
                    __hip_atomic_store(&S.ctrl->fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&S.ctrl->term_type, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&S.ctrl->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                s_flag = f;
            }
            __syncthreads();
            // (no acquire fence: it is a `buffer_inv` per wave, 2,500 of them at config 4, served one after the other
            // by the XCDs' L2s -- 20 us.  The few values of the solver that this workgroup reads are read through.)
            if (s_flag < 0 || __hip_atomic_load(&S.ctrl->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
            fail = s_flag & 1;
            for (int i = t; i < P.n_pad; i += kBsThreads) s_yh[i] = handoff_load(&S.yhat[i]);
            // (the candidate's per-camera records are written by the solver workgroup once it has published the step)
        }
        for (int rbase = s0; rbase < s1; rbase += kRoundSlots) {
            const int rend = min(s1, rbase + kRoundSlots);
            __syncthreads();                                            // the previous round is done with s_qv (and s_yh is there)
#pragma unroll
            for (int j = 0; j < kPasses; ++j) {
                const int sl = kPassSlots * j + grp;                    // slot of the round
                const double yh = a < kFA ? s_yh[16 * camv[j] + a] : 0.0;
                double p[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    p[k] = (a < kFA ? w[j][k] : 0.0) * yh;
                    p[k] = row16_allsum(p[k]);
                }
                if (a == 0) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) s_qv[sl][k] = p[k];
                }
            }
            if (rbase + kRoundSlots < s1) request(rbase + kRoundSlots);      // (boards of more than two views: the next round's records while this one's sums are formed)
            __syncthreads();
            // per board, its views in slot order (deterministic)
            if (t < nbl) {
                for (int q = max(my_q0, rbase); q < min(my_q1, rend); ++q)
#pragma unroll
                    for (int k = 0; k < 6; ++k) s_q[t][k] += s_qv[q - rbase][k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 7; ++j) s_fac[t + kBsThreads * j] = facv[j];
        __syncthreads();
    }
    PHASE_STAMP(ts1);
    // ---- phase B: lanes 0 .. nbl-1 one board each; lanes 64 .. 64+C-1 the candidate camera rotations -- in the SECOND
    //      wave: as lanes of the first they ran after the board solves (a wave executes both sides of a branch) -----------
    double mb = 0.0, ss = 0.0;
    if (t < nbl) {
        const int b = b0 + t;
        if (my_q1 == my_q0 || fail) {
#pragma unroll
            for (int k = 0; k < 6; ++k) { S.board_rt[cur ^ 1][6 * b + k] = xb[k]; s_new[t][k] = xb[k]; }
        } else {
            const double *f = s_fac + kFac * t;
            double tt[6], y[6], pz[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double v = f[kFacC + i] * s_q[t][i];
#pragma unroll
                for (int k = 0; k < i; ++k) v -= f[kFacM + i * (i - 1) / 2 + k] * pz[k];
                pz[i] = v;
                tt[i] = f[kFacZ + i] - v;
            }
#pragma unroll
            for (int i = 5; i >= 0; --i) {
                double w = tt[i];
#pragma unroll
                for (int k = i + 1; k < 6; ++k) w -= f[kFacL + k * (k - 1) / 2 + i] * y[k];
                y[i] = w * f[kFacI + i];
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                mb += 0.5 * tt[k] * tt[k] + 0.5 * f[kFacD + k] * y[k] * y[k];
                const double x = xb[k];
                const double xn = x + (-(sbv[k] * y[k]));
                const double d = x - xn;
                ss += d * d;
                S.board_rt[cur ^ 1][6 * b + k] = xn;
                s_new[t][k] = xn;
            }
        }
    } else if (t >= kBsCamLane0 && t < kBsCamLane0 + P.C) {
        const int m = t - kBsCamLane0;
        double crt[3], Rc[9], dRc[27];
        double crt6[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) crt6[k] = WAIT ? handoff_load(&S.cam_rt[cur ^ 1][6 * m + k]) : S.cam_rt[cur ^ 1][6 * m + k];
        for (int k = 0; k < 3; ++k) crt[k] = crt6[k];
        rotation_and_derivatives(crt, Rc, dRc);
        for (int k = 0; k < 9; ++k) s_rc[m][k] = Rc[k];
        for (int k = 0; k < 3; ++k) s_rc[m][9 + k] = crt6[3 + k];

    }
    {
        double red[2] = { mb, ss }, mdummy = 0.0;
        block_reduce256<2>(red, mdummy, sm);       // (contains the barriers that publish s_new / s_rc and retire s_fac)
        if (t == 0) { S.bs_part[2 * blk] = red[0]; S.bs_part[2 * blk + 1] = red[1]; }
    }
    PHASE_STAMP(ts2);
    // ---- phase C: one lane per view of these boards, tiles of kBsTile views ------------------------------------------
    for (int base = s0; base < s1; base += kBsTile) {
        const int slot = base + t;
        int view = -1;
        if (t < kBsTile && slot < s1) {
            const bool first = base == s0;
            view = first ? c_view : P.slot_view[slot];
            const int bl = (first ? c_board : P.slot_board[slot]) - b0, m = first ? c_cam : P.slot_cam[slot];
            double rt[6], bc[kBoardConst];
#pragma unroll
            for (int k = 0; k < 6; ++k) rt[k] = s_new[bl][k];
            board_constants(rt, bc);
            double *o = st_all + (size_t)t * (kVFloatOff + 1);
            view_point_constants(s_rc[m], s_rc[m] + 9, bc, rt + 3, o);
            for (int k = 0; k < 6; ++k) {           // six 3-vectors d -> R_c d
                const double d0 = bc[6 + 3 * k], d1 = bc[6 + 3 * k + 1], d2 = bc[6 + 3 * k + 2];
                for (int r = 0; r < 3; ++r) o[9 + 3 * k + r] = s_rc[m][3 * r] * d0 + s_rc[m][3 * r + 1] * d1 + s_rc[m][3 * r + 2] * d2;
            }
            for (int k = kVConst; k < kVFloatOff; ++k) o[k] = 0.0;
        }
        // the records are indexed by device view (camera-major); a workgroup's slots map to scattered views, so the
        // staging tile is drained one record per 32 consecutive lanes: 256-byte contiguous pieces
        if (t < kBsTile) s_view[t] = view;
        __syncthreads();
        const int nrec = min(kBsTile, s1 - base);
        for (int e = t; e < nrec * kVFloatOff; e += kBsThreads) {
            const int v = e / kVFloatOff, k = e % kVFloatOff;
            S.vconst[(size_t)kVStride * s_view[v] + k] = st_all[(size_t)v * (kVFloatOff + 1) + k];
        }
        if (with_floats) {
            constexpr int kF = kVStride - kVFloatOff;
            for (int e = t; e < nrec * kF; e += kBsThreads) {
                const int v = e / kF, k = e % kF, j = 2 * k;
                const double *sv = st_all + (size_t)v * (kVFloatOff + 1);
                const float f0 = j < kVConst ? (float)sv[j] : 0.f, f1 = j + 1 < kVConst ? (float)sv[j + 1] : 0.f;
                S.vconst[(size_t)kVStride * s_view[v] + kVFloatOff + k] = __hiloint2double(__float_as_int(f1), __float_as_int(f0));
            }
        }
        __syncthreads();
    }
#ifdef TSCM_WAVE_TIMELINE
    if (threadIdx.x == 0 && S.ctrl->iteration == 5 && blk < kKtlGroups) {
        long long *o = g_phs + (size_t)kPhStamps * (kKtlGroups + blk);
        o[0] = ts0; o[1] = ts0; o[2] = ts1; o[3] = ts2; o[4] = wall_clock64(); o[5] = o[4]; o[6] = nbl; o[7] = 0;
    }
#endif
#ifdef TSCM_PHASE_PROFILE
    if (threadIdx.x == 0 && (blk == 0 || blk == 200))
        printf("backsub_prep wg %d: W.yhat %lld  board solve %lld  view constants %lld [10 ns]\n", blk, ts1 - ts0, ts2 - ts1, wall_clock64() - ts2);
#endif
}

template <int NTH>
__global__ __launch_bounds__(NTH) void k_backsub_prep(DevProblem P, DevState S, int with_floats)
{
    KTL(5);
    backsub_body<NTH, false>(P, S, with_floats, (int)blockIdx.x, (int)gridDim.x, 0, 0);
}
