// tscm_eval_gram16.h -- stage 1, the evaluation: the 16x16-tile Gram kernel k_eval_gram (the TSCM_EXEC_GRAM_16X16 path;
// the default kernel is k_eval_gram4, the fp32-Jacobian tier k_eval_gram_f32).
#pragma once
// (included from tscm_kernels.h inside namespace tscm)

// ---------------------------------------------------------------------------------------------
// THE HOT KERNEL: per-corner TSCM projection + analytic Jacobian + residual, then ALL Gram
// products of the 2 x 20 Jacobian block [E | F | r] from ONE 16x16 f64 MFMA tile per 4 rows:
//   * t_b columns are constant combinations of the t_c columns (J_tb = J_tc R_c): dropped from
//     the tile, recovered per view by a 3x3 multiply in the epilogue;
//   * (fx, fy) and (cx, cy) have disjoint row support: merged into f* and one*, separated again
//     by keeping the u-rows and the v-rows of the Jacobian in two accumulators.
//   -> 15 tile columns, v_mfma_f64_16x16x4_f64 count per view = 2*ceil(n/4) (28 for 54 corners)
//      instead of 3*ceil(2n/4) = 81 for the naive [E|F|r] padding.
// One wave per chunk of consecutive views of ONE camera, four such waves (same camera) per workgroup;
// lane = corner (coalesced SoA loads of u[], v[]); board points in LDS; the 27 per-view constants live
// one per lane in a VGPR pair (prefetched a view ahead) and are fetched with v_readlane, the 48
// per-camera constants come through the constant address space as scalar loads (SGPR operands);
// Jacobian columns are transposed through LDS (column-major, pitch 2*odd: conflict-free
// ds_read_b64) into MFMA operand layout.  The per-camera tile stays in registers for the chunk.
// All global traffic of the view loop uses buffer addressing; the record is written by 13
// unconditional stores.
// dynamic LDS: 16*rp + kCst + 2*n_points doubles (the kCst block is only used by k_eval_gram_f32).

constexpr int kGramDepth = 4;      // k-steps between an operand's request and the MFMA that consumes it
// Gram contraction of one row half of a view, full tile of KS k-steps: every operand is its OWN ds_read_b64 (serviced
// in two 32-lane groups with banks mod 64: conflict-free at a pitch of 2 * odd), requested D steps ahead of the MFMA
// that consumes it.  The compiler fuses neighbouring plain loads into ds_read2_b64, which is serviced in 16-lane groups
// with banks mod 32 -- two-way conflicts at this pitch, 16 LDS cycles instead of 4 per pair: the source of
// SQ_LDS_BANK_CONFLICT in round 2's counters -- and waits for each pair right after requesting it.  Hence inline
// assembly with explicit counts: LDS operations of a wave complete in order, so after lgkmcnt(n) everything but the n
// youngest requests has arrived whatever else (scalar loads included) is in flight.
template <int OFF>
__device__ __forceinline__ double ds_read_f64(unsigned addr)
{
    double v;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
template <int N>
__device__ __forceinline__ void lgkm_wait(double &v) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "n"(N)); }
__device__ __forceinline__ unsigned lds_addr(const double *p)
{
    return (unsigned)(size_t)(const __attribute__((address_space(3))) double *)p;
}
template <int KS, int D, bool ZERO_C, int T = 0>
__device__ __forceinline__ void gram_steps(unsigned addr, double (&a)[KS], d4 &acc)
{
    if constexpr (T < KS) {
        if constexpr (T + D < KS) a[T + D] = ds_read_f64<32 * (T + D)>(addr);
        lgkm_wait<(KS - 1 - T < D ? KS - 1 - T : D)>(a[T]);
        if constexpr (ZERO_C && T == 0) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[T], a[T], d4{ 0.0, 0.0, 0.0, 0.0 }, 0, 0, 0);
        else acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[T], a[T], acc, 0, 0, 0);
        gram_steps<KS, D, ZERO_C, T + 1>(addr, a, acc);
    }
}
template <int KS, int D, bool ZERO_C, int T = 0>
__device__ __forceinline__ void gram_prime(unsigned addr, double (&a)[KS])
{
    if constexpr (T < D && T < KS) { a[T] = ds_read_f64<32 * T>(addr); gram_prime<KS, D, ZERO_C, T + 1>(addr, a); }
}
template <int KS, bool ZERO_C>
__device__ __forceinline__ void gram_full(const double *fp, d4 &acc)
{
    constexpr int D = kGramDepth;
    const unsigned addr = lds_addr(fp);
    double a[KS];
    gram_prime<KS, D, ZERO_C>(addr, a);
    gram_steps<KS, D, ZERO_C>(addr, a, acc);
}

template <int RPC>   // RPC > 0: compile-time LDS pitch (HV = RPC - 2): all tile offsets become immediates
__global__ __launch_bounds__(256, 4) void k_eval_gram(DevProblem P, DevState S, int cand)
{
    // the control block is read together with the static chunk tables (one memory round trip, not two);
    // the early exit is taken right before the first view
    const int ctrl_done = S.ctrl->done, ctrl_cur = S.ctrl->cur;
#ifdef TSCM_WAVE_TIMELINE
    // profiling builds only (make variant VARIANT=T EXTRA=-DTSCM_WAVE_TIMELINE): start / end time and hardware slot of every wave of the
    // launches of LM iteration 5 into g_timeline; tscm_debug_wave_timeline copies it out, tools/wave_timeline.py groups
    // the waves by SIMD
    const long long tl_t0 = wall_clock64();
    const int tl_iter = S.ctrl->iteration;
#endif
    extern __shared__ __attribute__((aligned(16))) double lds_all[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: keeps chunk/view/cnt in SGPRs
    double *lds = lds_all + (size_t)wave * P.lds_wave;     // every wave works in its own LDS region
    const int RP = RPC > 0 ? RPC : P.rp, HV = RPC > 0 ? RPC - 2 : P.half;   // pitch = 2*odd >= HV: conflict-free ds_read_b64
    double *Fl = lds;                          // [kTcols][RP]: HV rows; holds the u-rows, then the v-rows
    double *cst = Fl + max(16 * RP, 512);      // [kCst]  (column 15 of Fl stays zero; 512 = final camera-tile exchange)
    double *bxy = cst + kCst;
    const int lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * 4 + wave;
    const int cam = P.chunk_cam[chunk];
    for (int i = lane; i < 2 * P.n_points; i += 64) bxy[i] = P.board_xy[i];
    const int vb = P.chunk_vb[chunk], ve = P.chunk_ve[chunk];
    const int col = lane & 15, kq = lane >> 4;
    d4 camU = { 0.0, 0.0, 0.0, 0.0 }, camV = { 0.0, 0.0, 0.0, 0.0 };
    // rows of lanes without a corner are kept at zero instead of being re-written every pass
    if (lane < HV) {
#pragma unroll
        for (int c = 0; c < 16; ++c) Fl[c * RP + lane] = 0.0;      // incl. the all-zero 16th tile column
    }
    int prev_nv = 0;                           // lanes [nv, prev_nv) hold stale rows of the previous pass
    // software prefetch: the next view's constants and first 64 observations are loaded while
    // the current view computes (one wave per SIMD-slot cannot hide HBM latency otherwise)
    double pf_u = 0.0, pf_v = 0.0;
    int warm = 0;                              // see the prefetch below
    if (ctrl_done) return;
    const int tgt = cand ? (ctrl_cur ^ 1) : ctrl_cur;
    const __amdgpu_buffer_rsrc_t r_rec = make_rsrc(S.rec[tgt], sizeof(double) * (size_t)kRec * P.V);
    // camera constants: read through the constant address space (uniform address, written by an earlier
    // kernel) -> scalar loads straight into SGPR operands, no v_readlane pair per use
    const cptr4 ccs = (cptr4)(S.cconst[tgt] + kCStride * cam);
    auto CC = [&](int k) { return ccs[k]; };                                          // camera constants (see k_view_prep)
    const RecLane rl = rec_lane(lane, (unsigned)P.V);
    const __amdgpu_buffer_rsrc_t r_vc = make_rsrc(S.vconst, sizeof(double) * (size_t)kVStride * P.V);
    const __amdgpu_buffer_rsrc_t r_u = make_rsrc(P.obs_u, sizeof(double) * (size_t)P.N), r_v = make_rsrc(P.obs_v, sizeof(double) * (size_t)P.N);
    // Per-view metadata (corner count, record slot) of a block of <= 64 views sits in lane registers and is
    // read with v_readlane; the observations of a camera's views are contiguous, so the offset is a running
    // sum.  No dependent global load -- and therefore no in-order vmcnt wait behind the previous view's
    // record stores -- is left inside the view loop.
    int off_next = vb < ve ? P.view_obs[vb] : 0;
    // Wave priority by progress.  The four waves of a SIMD share the fp64 pipe, and the arbiter serves the OLDEST wave
    // first: left alone they finish one after the other (46 / 57 / 68 / 79 us into the launch at config 4), and the last
    // ten microseconds of the kernel run on one wave per SIMD, whose dependent chains cannot fill the pipe.  A wave that
    // is further along in its chunk than its neighbours gives way: the priority falls from 3 to 0 over each half of
    // the chunk (eighths of its views, mod 4), so whoever is behind by an eighth outranks whoever is ahead, and the
    // four finish within 6 us of each other (59 / 61 / 63 / 65 us after the epilogue rewrite).  The assignment of views
    // to waves is untouched: the results are the same bits.  (The other rules of the A/B runs in profiles/r03_eval_gram_ab.txt
    // -- by phase: geometry high, MFMA low; by quarters of the chunk; no priorities at all -- lost to this one.)
    for (int vbase = vb; vbase < ve; vbase += 64) {
    const int vend = min(ve, vbase + 64);
    int m_cnt = 0, m_slot = 0;
    if (vbase + lane < vend) { m_cnt = P.view_count[vbase + lane]; m_slot = P.view_slot[vbase + lane]; }
    asm volatile("" : "+v"(m_cnt), "+v"(m_slot));       // the loads complete here, outside the view loop
    {
        const int c0n = __builtin_amdgcn_readlane(m_cnt, 0);
        if (lane < c0n) { pf_u = buf_load_f64(r_u, 8u * lane, 8u * (unsigned)off_next); pf_v = buf_load_f64(r_v, 8u * lane, 8u * (unsigned)off_next); }
    }
    for (int view = vbase; view < vend; ++view) {
        const int cnt = __builtin_amdgcn_readlane(m_cnt, view - vbase);
        const int off = off_next;
        off_next = off + cnt;
        wave_lds_fence();                       // previous view's epilogue has finished with LDS
        set_prio(3 - min(3, 8 * (view - vb) / max(1, ve - vb) % 4));
        const cptr4 vcs = (cptr4)(S.vconst + (size_t)kVStride * view);      // this view's 27 constants: scalar loads
        auto VC = [&](int k) { return vcs[k]; };
        d4 accU = { 0.0, 0.0, 0.0, 0.0 }, accV = { 0.0, 0.0, 0.0, 0.0 };
        for (int c0 = 0; c0 < cnt; c0 += 64) {
            const int j = c0 + lane;
            const bool valid = j < cnt;
            double *fu = Fl + lane;
            double fv[kTcols];                 // v-rows wait in registers until the u-rows have been consumed
            if (valid) {
                const double x = bxy[2 * j], y = bxy[2 * j + 1];
                // (RPC > 0: boards of <= 56 corners, always a single pass -- the load path below would otherwise put a
                // vmcnt(0) in front of the residual, i.e. a wait for the prefetch issued a few hundred cycles earlier)
                const bool later_pass = RPC == 0 && c0 != 0;
                const double ou = later_pass ? buf_load_f64(r_u, 8u * j, 8u * (unsigned)off) : pf_u, ov = later_pass ? buf_load_f64(r_v, 8u * j, 8u * (unsigned)off) : pf_v;
                // semantic column -> tile column of this kernel
                constexpr int tcol[15] = { kTcWb, kTcWb + 1, kTcWb + 2, tc_tc(0), tc_tc(1), tc_tc(2), kTcWc, kTcWc + 1, kTcWc + 2,
                                           kTcF, kTcOne, kTcXi, kTcLam, kTcAl, kTcR };
                corner_geometry(x, y, ou, ov, VC, CC, [&](int gc, double u, double v) { fu[tcol[gc] * RP] = u; fv[tcol[gc]] = v; });
            } else if (lane < prev_nv) {
#pragma unroll
                for (int c = 0; c < kTcols; ++c) fu[c * RP] = 0.0;
            }
            if (c0 == 0) {
                // Prefetch of the next view, issued once the current view's observations have been consumed: the
                // loads reuse the same registers (no copy that would have to wait for them), and everything
                // between here and their use at the top of the next view is four unconditional stores.
                // Always issued (the block's last view re-reads itself; lanes past the corner count read past
                // the end of the buffer, i.e. zero): unconditional loads keep the vmcnt bookkeeping exact.
                const int vn = min(view + 1, vend - 1);
                const int cn = view + 1 < vend ? __builtin_amdgcn_readlane(m_cnt, vn - vbase) : 0;
                // pull the next view's 256-byte constant record into the L2 with one tracked vector load (lanes
                // 0..3, one dword per 64-byte line): the scalar loads at the top of the next view then hit the L2
                warm = __builtin_amdgcn_raw_buffer_load_b32(r_vc, lane < 4 ? 64 * lane : (int)0xffffe000u, (int)(8u * (unsigned)kVStride * (unsigned)vn), 0);
                pf_u = buf_load_f64(r_u, lane < cn ? 8u * lane : 0xffffe000u, 8u * (unsigned)off_next);
                pf_v = buf_load_f64(r_v, lane < cn ? 8u * lane : 0xffffe000u, 8u * (unsigned)off_next);
            }
            wave_lds_fence();
            const int nv = min(64, cnt - c0);
            prev_nv = nv;
            const int ksteps = (nv + 3) >> 2;
            // rows past the last corner are zero, so the loops run in
            // pairs of k-steps; operands of the next pair are fetched while the current MFMAs issue
            const double *fp = Fl + col * RP + kq;      // lane (col, kq) feeds tile column col, row 4t + kq
            const int tmax = (HV >> 2) - 2;
            constexpr int KSF = RPC > 0 ? (RPC - 2) / 4 : 1;      // k-steps of a full tile
            const bool full_tile = RPC > 0 && ksteps == KSF;
            if (full_tile) gram_full<KSF, true>(fp, accU);
            else {
                double a0 = fp[0], a1 = fp[4];
                for (int t = 0; t < ksteps; t += 2) {
                    const int tn = min(t + 2, tmax);
                    const double n0 = fp[4 * tn], n1 = fp[4 * tn + 4];
                    accU = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, accU, 0, 0, 0);
                    accU = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, accU, 0, 0, 0);
                    a0 = n0; a1 = n1;
                }
            }
            wave_lds_fence();
            if (valid) {
#pragma unroll
                for (int c = 0; c < kTcols; ++c) fu[c * RP] = fv[c];
            }
            wave_lds_fence();
            if (full_tile) gram_full<KSF, true>(fp, accV);
            else {
                double a0 = fp[0], a1 = fp[4];
                for (int t = 0; t < ksteps; t += 2) {
                    const int tn = min(t + 2, tmax);
                    const double n0 = fp[4 * tn], n1 = fp[4 * tn + 4];
                    accV = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, accV, 0, 0, 0);
                    accV = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, accV, 0, 0, 0);
                    a0 = n0; a1 = n1;
                }
            }
            wave_lds_fence();
        }
        // The next view's constants are waited for HERE, a full MFMA phase after their load was issued and before
        // this view's record stores: on gfx9 loads and stores share vmcnt and may complete out of order, so any
        // wait for a load with stores in flight is a vmcnt(0) -- a wait placed right after the stores (the top
        // of the next view) would expose the whole store latency.  The geometry is done with cst by now.
        asm volatile("" :: "v"(warm));       // the warming load retires here, before this view's record stores
        camU += accU; camV += accV;
        store_view_record(r_rec, lane, accU, accV, ccs, (unsigned)__builtin_amdgcn_readlane(m_slot, view - vbase), rl);
    }
    }   // block of <= 64 views
#ifdef TSCM_WAVE_TIMELINE
    if (lane == 0 && tl_iter == 5 && cand && chunk < kTimelineWaves) {
        g_timeline[4 * chunk] = (long long)__builtin_amdgcn_s_getreg(63492);     // HW_ID
        g_timeline[4 * chunk + 1] = (long long)__builtin_amdgcn_s_getreg(6164);  // XCC_ID
        g_timeline[4 * chunk + 2] = tl_t0;
        g_timeline[4 * chunk + 3] = wall_clock64();
    }
#endif
    // the four waves of the workgroup (same camera) sum their tiles through LDS in a fixed order
    wave_lds_fence();
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) { lds[(kq + 4 * rg) * 16 + col] = camU[rg]; lds[256 + (kq + 4 * rg) * 16 + col] = camV[rg]; }
    __syncthreads();
    {
        const int t = threadIdx.x;
        const size_t st = P.lds_wave;
        double *part = S.campart + (size_t)512 * blockIdx.x;
        part[t] = (lds_all[t] + lds_all[st + t]) + (lds_all[2 * st + t] + lds_all[3 * st + t]);
        part[256 + t] = (lds_all[256 + t] + lds_all[st + 256 + t]) + (lds_all[2 * st + 256 + t] + lds_all[3 * st + 256 + t]);
    }
}
