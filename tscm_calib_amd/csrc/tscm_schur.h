// tscm_schur.h -- stage 3, the Schur complement: the boards' e-block factors, the camera-pair Gram tiles Y^T Y, their
// reduction into T, and the common tail of the reduced-system solvers.
#pragma once
// (included from tscm_kernels.h inside namespace tscm)

// ---------------------------------------------------------------------------------------------
// e-block factorisation (SchurEliminator, one 6x6 block per board): ONE LANE per board.
//   V = sum_views E^T E, Jacobi-scaled, damped with D^2 = clamp(diag)/radius, Cholesky L L^T.
// Reads only the E region of the records; writes the board's factor record (kFac doubles): everything the
// Schur-complement and back-substitution kernels need to re-derive Y = L^-1 S_b W column by column.
// grid ceil(B/256) x 256
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool chol6(const double M[21], double L[21])
{
    // packed lower: idx(i,j) = i(i+1)/2 + j; the diagonal slots hold 1 / L_jj
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = M[j * (j + 1) / 2 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        if (!(d > 0.0)) { ok = false; d = 1.0; }
        const double inv = fast_rsqrt(d);      // 1 / L_jj: only the inverse is ever used (forward and back substitution)
        L[j * (j + 1) / 2 + j] = inv;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = M[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            L[i * (i + 1) / 2 + j] = s * inv;
        }
    }
    return ok;
}

// Factor the damped, Jacobi-scaled 6x6 block of a board from M = sum_views E^T E (packed lower) and g = sum_views E^T r,
// and write the board's factor record (kFac doubles) to f (HBM or LDS).  Returns false if the block is not positive
// definite.
// A board whose pose block is constant (SetParameterBlockConstant) has no e-block: its record is all zeros, which makes
// Y = 0 (no Schur-complement contribution), z = 0 and the back-substituted step exactly 0.
__device__ __forceinline__ bool factor_core(double (&M)[21], const double (&g)[6], const double (&sb)[6], double radius, double dmin, double dmax, double *f,
                                            bool constant_block = false)
{
    if (constant_block) {
#pragma unroll
        for (int i = 0; i < kFac; ++i) f[i] = 0.0;
        return true;
    }
    double D2[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) M[i * (i + 1) / 2 + j] *= sb[i] * sb[j];
        D2[i] = fmin(fmax(M[i * (i + 1) / 2 + i], dmin), dmax) / radius;
        M[i * (i + 1) / 2 + i] += D2[i];
    }
    double L[21];
    const bool ok = chol6(M, L);
    // forward substitution in multiply-only form: y_i = c_i w_i - sum_{k<i} m_ik y_k
    double z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double il = L[i * (i + 1) / 2 + i];
        const double c = sb[i] * il;
        f[kFacC + i] = c;
        f[kFacI + i] = il;
        f[kFacD + i] = D2[i];
        double w = c * g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) {
            const double m = L[i * (i + 1) / 2 + k] * il;
            f[kFacM + i * (i - 1) / 2 + k] = m;
            f[kFacL + i * (i - 1) / 2 + k] = L[i * (i + 1) / 2 + k];
            w -= m * z[k];
        }
        z[i] = w;
        f[kFacZ + i] = w;
    }
    f[54] = 0.0; f[55] = 0.0;
    return ok;
}

// ... of board b with its views at slots [q0, q1), record to HBM
__device__ __forceinline__ void factor_board(const DevProblem &P, const DevState &S, int cur, double radius, double dmin, double dmax,
                                             int b, int q0, int q1)
{
    double sb[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) sb[i] = S.s_b[6 * b + i];
    double M[21], g[6] = { 0, 0, 0, 0, 0, 0 };
#pragma unroll
    for (int i = 0; i < 21; ++i) M[i] = 0.0;
    for (int q = q0; q < q1; ++q) {
        const double *E = rec_e(S.rec[cur], P.V, q), *W = rec_w(S.rec[cur], q), *Rc = S.cconst[cur] + kCStride * P.slot_cam[q];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) M[i * (i + 1) / 2 + j] += j < 3 ? E[6 * j + i] : tb_tb(W, Rc, i - 3, j - 3);
            g[i] += W[6 * kFR + i];
        }
    }
    if (!factor_core(M, g, sb, radius, dmin, dmax, S.fac + (size_t)kFac * b, P.board_const[b] != 0)) *S.fac_fail = 1;
}

// stand-alone factorisation of the boards seen by more than three cameras (their Gram products go through
// k_pair_gram); the others are factored inside k_schur_gram.   grid ceil(n_slow/256) x 256
__global__ __launch_bounds__(256) void k_schur_factor(DevProblem P, DevState S)
{
    if (S.ctrl->done) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n_slow) return;
    const int b = P.slow_boards[i];
    factor_board(P, S, S.ctrl->cur, S.ctrl->radius, S.ctrl->opt.min_lm_diagonal, S.ctrl->opt.max_lm_diagonal, b, P.bv_ptr[b], P.bv_ptr[b + 1]);
}

// e-block factorisation + Schur complement contributions  T(m_p, m_q) += Y_p^T Y_q  (views p <= q of one board,
// Y = L^-1 S_b W) in ONE launch.  Boards are grouped by their camera set ("signature"); one 4-wave workgroup per
// chunk of <= 64 boards of ONE signature, so the NV(NV+1)/2 16x16 tiles of a chunk map to fixed camera-pair blocks
// and stay in registers as MFMA accumulators.
//   phase 0a  16 lanes per board sum the E records of its views (contiguous: coalesced) into LDS, 16 boards per pass; in the
//             RIDE instantiation a pass whose boards all lie beyond the chunk's end requests nothing and stores nothing
//             (-0.3 us at config 4's 40 boards; the same two conditions cost the non-riding instantiation 0.85 us at
//             config 5, where no pass is ever empty -- this kernel's code is that touchy, HISTORY A.6 -- so it does without)
//   phase 0b  one lane per board: damped Cholesky -> the board's factor record, in LDS
//   (then the records leave for HBM -- the back-substitution needs them -- as one coalesced stream per board)
//   phase 1   the chunk's groups of FOUR boards are shared evenly among the four waves (schur_group_of: a chunk of 40
//             boards is 3, 3, 2, 2 groups, not 4, 4, 2, 0 -- the phase is bound by the SIMD's one fp64 pipe and lies on the
//             launch's critical path).
//             A wave takes four boards at a time: lane (a, kq) loads column a of the W records of board kq of the
//             group and runs the 21-FMA forward substitution with that board's multipliers (LDS).  The matrix core
//             contracts over k, and T is a sum over boards -- so the k index of v_mfma_f64_16x16x4 IS the board:
//             for each of the 6 rows r, one MFMA per tile adds sum_{4 boards} Y_p[r][i] Y_q[r][j].  No lane computes
//             anything twice and no operand has to be moved: 6 NT MFMAs and 27 NV FMAs per lane per four boards.
//             The next group's columns are requested before the MFMAs, which cover their latency.
// The four waves' tiles are summed in a fixed order through LDS: by VIRTUAL wave, so the bits do not depend on `rot` (tests: tscm_solver_debug_schur_rot).
// grid (chunks of this NV) x 256; a chunk has at most kChunkBoards boards (tscm_layout.h)


// the forward-substitution values of a board factored by k_schur_factor, wave-uniform through the constant address
// space (scalar loads): k_pair_gram
struct FacFwd { double m[15], c[6], z[6]; };
__device__ __forceinline__ void load_fac_fwd(const double *fac, int board, FacFwd &F)
{
    const cptr4 f = (cptr4)(fac + (size_t)kFac * board);
#pragma unroll
    for (int i = 0; i < 15; ++i) F.m[i] = f[kFacM + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) { F.c[i] = f[kFacC + i]; F.z[i] = f[kFacZ + i]; }
}

// One column of Y = L^-1 S_b W from the column of W.  Column kFR (the gradient column) of EVERY view of a board is
// z = L^-1 S_b (sum over the board's views of E^T r): the reduced right-hand side reads sum_b Y_v^T z from the
// diagonal camera blocks only.
__device__ __forceinline__ void y_column(const FacFwd &F, const double (&w)[6], bool grad_col, double (&y)[6])
{
    y[0] = F.c[0] * w[0];
    y[1] = F.c[1] * w[1] - F.m[0] * y[0];
    y[2] = F.c[2] * w[2] - F.m[1] * y[0] - F.m[2] * y[1];
    y[3] = F.c[3] * w[3] - F.m[3] * y[0] - F.m[4] * y[1] - F.m[5] * y[2];
    y[4] = F.c[4] * w[4] - F.m[6] * y[0] - F.m[7] * y[1] - F.m[8] * y[2] - F.m[9] * y[3];
    y[5] = F.c[5] * w[5] - F.m[10] * y[0] - F.m[11] * y[1] - F.m[12] * y[2] - F.m[13] * y[3] - F.m[14] * y[4];
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] = grad_col ? F.z[i] : y[i];
}

// ... as the two MFMA operands of a 6-row block of ONE board (k_pair_gram): K = 6 rows as two k-steps of 4 (rows 0..3,
// then rows 4, 5 and two zero rows); lane (a, kq) supplies row kq and row 4 + kq.
__device__ __forceinline__ void y_column_operands(const FacFwd &F, const double (&w)[6], bool grad_col, int kq, double &s0, double &s1)
{
    double y[6];
    y_column(F, w, grad_col, y);
    double y0 = y[0], y1 = y[1], y2 = y[2], y3 = y[3], y4 = y[4], y5 = y[5];
    // (register values, not an indexable array: a select chain over array elements is turned into a dynamic index,
    // and the array then lives in scratch)
    asm volatile("" : "+v"(y0), "+v"(y1), "+v"(y2), "+v"(y3), "+v"(y4), "+v"(y5));
    const bool lo = (kq & 1) == 0, first = kq < 2;
    const double a01 = lo ? y0 : y1, a23 = lo ? y2 : y3, a45 = lo ? y4 : y5;
    s0 = first ? a01 : a23;
    s1 = first ? a45 : 0.0;
}

// the t_b x t_c blocks (3 x 3, one per view) a board's factorisation needs to rebuild its t_b x t_b block, staged in
// LDS as r[3 * jc + l]; indexed like the W record they were taken from so that tb_tb serves both
struct RawTc {
    const double *r;
    __device__ __forceinline__ double operator[](int i) const { return r[3 * (i / 6 - kWcolTc) + (i % 6 - 3)]; }
};

// ctl = 1 (one GPU, <= 8 cameras) or 2 (communicator: the tiles are all-reduced in H_stage); this the only Schur kernel
// of the iteration: the evaluation in front of this launch
// has not been followed by its control step yet -- EVERY workgroup takes it here, in its head (finish_evaluation, LDS
// borrowed from the factor records), on the same inputs and to the same bits; workgroup 0 writes the results.  No
// launch, no hand-off and no single workgroup that the whole chip waits for: what k_reduce_control's last workgroup
// did in 10 us with 255 CUs idle happens here while nothing else could run anyway.
// With ctl the grid has one workgroup more: workgroup 0 writes the step's results (S.ctrl, H, the iteration log), publishes
// the outcome (S.ctl_pub, epoch = ctl_epoch) and does nothing else; workgroups 1 .. first_round - 1 -- those resident when the
// launch starts -- take the step themselves; the workgroups of LATER rounds of the grid (config 5 on one GPU: 1256 chunks,
// 2.5 rounds) start when a first-round workgroup has finished, long after workgroup 0, and read the published outcome:
// the step is paid once per launch, not once per round.
// RIDE (round 5; one GPU, a candidate's evaluation, a grid of ONE round): the reductions behind the evaluation -- k_reduce_stats' blocks,
// 5.2 us + a kernel boundary at config 4 in front of a kernel whose head waits for exactly their results -- ride in this launch.
// Workgroup j + 1 (j < n_stats = 16 C + ceil(B / 256)) takes reduction block j IN FRONT of its own chunk j (a grid of fewer chunks
// than blocks has workgroups that do nothing else); nothing is added to the grid, so everything is resident at once -- as extra
// workgroups the blocks pushed 132 chunks of config 4 into a second round, +5 us -- and the wait below cannot deadlock (the host
// checks max(blocks, chunks) + 1 <= resident workgroups and launches k_reduce_stats otherwise; a block that does not arrive within
// the hand-offs' time bound is a device fault and the solve is run again on separate launches: fault injection 3).  A block
// writes its results through (handoff_store, as it always did), the last block also the snapshot of the LM state, and counts
// itself in: S.stats_count, monotonic over the solve (stats_target = n_stats x the riding launches so far); the last arrival
// copies the count into S.stats_flag, a line of its own, which is what everybody polls -- 370 workgroups polling the COUNTER's line
// held the 143 read-modify-writes on it up by 4.5 us (and a workgroup keeps its slot until its atomic has returned).
// In front of the wait every workgroup requests what the control step reads that the blocks do not write (control_early) and
// then its chunk's RECORDS, from the buffer an accepted step makes current (S.ctrl->cur ^ 1: the state in front of the step;
// whoever reads it after the extra workgroup's commit, or finds the step rejected, asks again behind the step): the 34 MB stream
// while the blocks run.
// Behind the flag the step reads the snapshot (through the scalar cache, as always), two finished sums per thread and the
// statistics partials with PLAIN loads, not handoff_load (500 workgroups x 50 lines read through would queue at the memory side):
// every one of those lines is written by ONE workgroup in this launch (campart2: 256 bytes per block; st_part: a 128-byte line per
// block, kStStride; the snapshot) and by nobody else, nobody reads them in this launch before the flag (the instrumented build's
// scope reads S.ctrl instead of the snapshot for that reason), and the XCDs' L2s and the CUs' vector and scalar caches start a
// launch invalidated (what k_reduce_stats wrote has always reached the next launch's plain loads that way) -- so the first touch
// of a line from an XCD fetches what was written through, or hits the writer's own written-through copy.
template <int NV, bool RIDE = false>
__global__ __launch_bounds__(256, RIDE && NV <= 2 ? 2 : 1) void k_schur_gram(DevProblem P, DevState S, int chunk0, int ctl, int first_round, int ctl_epoch, int stats_target, int n_chunks, int rot)
{
#ifdef TSCM_WAVE_TIMELINE
    KtlScope ktl_scope(3, ctl && !RIDE ? S.ctrl_snap : static_cast<const CtrlHead *>(S.ctrl));      // (the snapshot: the writer workgroup advances S.ctrl while later rounds start)
#endif
    PHASE_STAMP(tsk);
    // head of the kernel: the control block and the chunk descriptor travel together (one memory round trip), every
    // other address follows from them arithmetically -- the second round trip already brings the data
    // (kCtlInit: the evaluation whose step is taken here is the solve's INITIAL one -- IterationZero: no back-substitution behind it,
    // the Jacobi scaling of the camera columns written by the extra workgroup)
    // (the bits of ctl: tscm_exec_plan.h; decoded by shifts, which is the code the kernel was tuned with)
    static_assert(kCtlInit == 1 << 2 && kCtlWithhold == 1 << 4 && (kCtlOneGpu | kCtlComm) == 3, "k_schur_gram's decode of ctl");
    const int ctl_init = (ctl >> 2) & 1, withhold = (ctl >> 4) & 1;      // (withhold: fault injection, tscm_solver_debug_withhold_handoff(s, 3))
    ctl &= 3;
    const int n_stats = RIDE ? P.C * kCamSl + S.n_st_blocks : 0;
    const int bid = (int)blockIdx.x;
    const bool extra = ctl != 0 && bid == 0;               // the workgroup that writes the control step's results, and nothing else
    const int jblk = ctl ? bid - 1 : bid;                  // (RIDE: reduction block jblk < n_stats in front of chunk jblk < n_chunks)
    const int cblk = RIDE ? min(max(jblk, 0), n_chunks - 1) : max(jblk, 0);
    const int4 desc = P.bc_desc[chunk0 + cblk];
    constexpr int NT = NV * (NV + 1) / 2;
    // what phase 0a gathers per board: sums over its views of E^T E_wb (18) and of E^T r (6), then per view the raw
    // 3 x 3 block t_b x t_c of W (9 NV): the t_b x t_b block is built from those in phase 0b with each view's R_c
    constexpr int NE = 24 + 9 * NV, NJ = (NE + 15) / 16;
    // (one block, so that the control step in the head can borrow all of it: facl first, 16-byte aligned)
    struct __attribute__((aligned(16))) Lds { double facl[kChunkBoards][kFac]; double sumE[kChunkBoards][NE]; double tiles[4][NT][256]; };
    __shared__ Lds lds_blk;
    double (&sumE)[kChunkBoards][NE] = lds_blk.sumE;
    double (&facl)[kChunkBoards][kFac] = lds_blk.facl;
    double (&tiles)[4][NT][256] = lds_blk.tiles;
    const int chunk = chunk0 + cblk;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int a = lane & 15, kq = lane >> 4;
    // phase 1's deal (tscm_layout.h): this wave plays virtual wave vw and takes the groups schur_group_of(nbd, vw, 0 .. 3)
    const int vw = schur_virtual_wave(wave, rot);
    const int c0 = desc.x, nbd = desc.y - desc.x, slot0 = desc.z;       // boards c0 .. c0 + nbd - 1 (<= kChunkBoards), views at slots slot0 + NV * i
    constexpr unsigned BAD = 0xffffe000u;
    double ev[4][NJ];
    double w[4][NV][6];
    // the boards of a chunk share their camera set: the rotation of view p's camera is chunk-uniform
    const double *Rcp[NV];
    auto request = [&](int cur_) {
        const __amdgpu_buffer_rsrc_t r_w = make_rsrc(S.rec[cur_], sizeof(double) * (size_t)kRec * P.V);
        // ---- requests: the pieces of the records of the boards this lane gathers (phase 0a), the W columns of the four
        //      groups of four boards its wave contracts (phase 1), the Jacobi scaling of the board it factors (phase 0b)
        {
            const int e = tid & 15;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                // entry e + 16 j of the list above: offset of its first term inside the allocation relative to the board's
                // first view, stride between the views' terms (0: a single term)
                const int idx = e + 16 * j;
                const int pv = idx < 24 ? 0 : (idx - 24) / 9, r9 = idx < 24 ? 0 : (idx - 24) % 9;
                const bool summed = idx < 24;
                const unsigned first = idx < 18 ? 8u * ((unsigned)kRecW * (unsigned)P.V + (unsigned)idx)
                                     : idx < 24 ? 8u * (unsigned)(6 * kFR + idx - 18)
                                     : 8u * (unsigned)(kRecW * pv + 6 * (kWcolTc + r9 / 3) + 3 + r9 % 3);
                const unsigned per_slot = idx < 18 ? 8u * kRecE : 8u * kRecW;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int bf = 16 * i + (tid >> 4);
                    const unsigned o0 = idx < NE && 16 * i < nbd ? first + per_slot * (unsigned)(slot0 + NV * min(bf, nbd - 1)) : BAD;
                    double acc = 0.0;
#pragma unroll
                    for (int p = 0; p < NV; ++p) acc += buf_load_f64(r_w, (p == 0 || summed) ? o0 : BAD, per_slot * (unsigned)p);
                    ev[i][j] = acc;
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int bg = 4 * schur_group_of(nbd, vw, g) + kq;             // (no such group: negative)
            const unsigned base = (a < 14 && bg >= 0 && bg < nbd) ? 8u * ((unsigned)kRecW * (unsigned)(slot0 + NV * bg) + 6u * (unsigned)a) : BAD;
#pragma unroll
            for (int p = 0; p < NV; ++p)
#pragma unroll
                for (int k = 0; k < 3; ++k) {          // column a of the view's W: six adjacent doubles
                    const d2 v = buf_load_2f64(r_w, base, 8u * (unsigned)(kRecW * p + 2 * k));
                    w[g][p][2 * k] = v[0]; w[g][p][2 * k + 1] = v[1];
                }
        }
#pragma unroll
        for (int p = 0; p < NV; ++p) Rcp[p] = S.cconst[cur_] + kCStride * P.slot_cam[slot0 + p];
    };
    int ctrl_done, cur;
    double radius, dmin, dmax;
#ifdef TSCM_WAVE_TIMELINE
    long long t_waited = 0, t_reduced = 0;
#endif
    if (RIDE && !extra && jblk < n_stats) {
        // a reduction block of the evaluation in front of this launch (k_reduce_stats' body; the candidate's evaluation) before
        // the workgroup's own chunk
        double *sm = reinterpret_cast<double *>(&lds_blk);
        const int blk = jblk, nc = P.C * kCamSl;
        if (blk == n_stats - 1 && threadIdx.x < sizeof(CtrlHead) / 8)
            __hip_atomic_store(&reinterpret_cast<unsigned long long *>(S.ctrl_snap)[threadIdx.x], reinterpret_cast<const unsigned long long *>(S.ctrl)[threadIdx.x],
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // (no look at ctrl->done first: a branch on a loaded value is a round trip in front of the block's own loads, and what a
        // finished solve's reductions write nobody reads)
        if (blk < nc) cam_reduce_block(P, S, blk, sm);
        else board_stats_block(P, S, /*cand=*/1, /*init=*/0, blk - nc, sm);
        PHASE_STAMP(tr1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the written-through results are complete, then the count (see "hand-offs")
        __syncthreads();
        PHASE_STAMP(tr2);
        if (threadIdx.x == 0 && !(withhold && blk == 1) && __hip_atomic_fetch_add(S.stats_count, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == stats_target - 1)
            __hip_atomic_store(S.stats_flag, stats_target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // the last one: everybody's results are complete
#ifdef TSCM_WAVE_TIMELINE
        t_reduced = wall_clock64();
        if (threadIdx.x == 0 && ktl_scope.on && blk < kKtlGroups) {
            long long *o = g_phs + (size_t)kPhStamps * (2 * kKtlGroups + blk);
            o[0] = tsk; o[1] = tr1; o[2] = tr2; o[3] = t_reduced; o[4] = blk < nc;
        }
#endif
        __syncthreads();                                          // (the LDS goes on to the requests' consumers)
    }
    if (RIDE && jblk >= n_chunks) return;                         // (a grid of fewer chunks than reduction blocks)
    // RIDE: the records are requested BEFORE the wait for the riding reductions and the control step, from the buffer an accepted
    // step makes current (S.ctrl->cur is the state in front of the step; whoever reads it after the extra workgroup's commit, or
    // sees the step rejected, asks again below): the 34 MB stream while the reductions run, the control step's own loads come
    // after it.  First-round workgroups only -- a later round finds the outcome published.
    int cur_spec = -1;
    ControlEarly early;
    if (RIDE && !extra && bid < first_round) {
        cur_spec = (S.ctrl->cur ^ 1) & 1;
        control_early(P, S, !ctl_init, early);          // (what the control step reads that the reductions do not write: ahead of the records)
        request(cur_spec);
    }
    if (ctl) {
        constexpr int kHl = 256 * kMaxCamLds + kScal + 8, kGall = 512 * kMaxCamLds;
        static_assert(sizeof(Lds) / sizeof(double) >= kHl + kGall + 256, "finish_evaluation's LDS (C <= 8) fits the kernel's block");
        static_assert(kChunkBoards * kFac >= kHl + 256, "control_outcome's LDS fits the factor records' space");
        __shared__ CtlOut s_ctl;
        double *scratch = reinterpret_cast<double *>(&lds_blk);
        // The LM state comes from the SNAPSHOT the reductions' launch took (k_reduce_stats): the extra workgroup of THIS
        // launch commits the advanced state to S.ctrl while the others may not even have started -- a workgroup that read
        // S.ctrl itself could find the step already taken and take it a second time.  Nobody writes the snapshot here.
        const CtrlHead *head = S.ctrl_snap;
        if (RIDE) {
            // the reductions ride in this launch: their results (and the snapshot) are there when all of them have counted themselves in
            // (a workgroup of a later round finds the count complete)
            __shared__ int s_late;
            if (threadIdx.x == 0) {
                const long long t_start = wall_clock64();
                int late = 0;
                while (__hip_atomic_load(S.stats_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < stats_target) {
                    __builtin_amdgcn_s_sleep(4);
                    if (wall_clock64() - t_start > kHandoffTimeoutTicks) { late = 1; break; }
                }
                if (late) {          // a device fault like any other late hand-off
                    __hip_atomic_store(&S.ctrl->fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&S.ctrl->term_type, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&S.ctrl->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                s_late = late;
            }
            __syncthreads();
            if (s_late) return;
        }
        PHASE_STAMP(tsw);
#ifdef TSCM_WAVE_TIMELINE
        t_waited = tsw;
#endif
        if (head->done) return;
        if (!extra && bid >= first_round) {
            // a later round of the grid: the outcome is published (or about to be)
            if (threadIdx.x == 0) {
                const long long t_start = wall_clock64();
                bool late = false;
                while (__hip_atomic_load(&S.ctl_pub->epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < ctl_epoch) {
                    __builtin_amdgcn_s_sleep(4);
                    if (wall_clock64() - t_start > kHandoffTimeoutTicks) { late = true; break; }
                }
                s_ctl.cur = __hip_atomic_load(&S.ctl_pub->cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s_ctl.done = __hip_atomic_load(&S.ctl_pub->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s_ctl.radius = handoff_load(&S.ctl_pub->radius);
                s_ctl.dmin = head->opt.min_lm_diagonal; s_ctl.dmax = head->opt.max_lm_diagonal;
                if (late) {          // workgroup 0 never reported: a device fault like a late hand-off of the fused solve launch
                    __hip_atomic_store(&S.ctrl->fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&S.ctrl->term_type, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&S.ctrl->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    s_ctl.done = 1;
                }
            }
        } else if (ctl == 2) {
            // communicator path: H_stage holds the all-reduced tiles and scalars -- k_control's work, by every workgroup
            ControlPre pre;
            control_prefetch(P, S, 0, pre, head);
            control_step(P, S, 0, pre, scratch, S.H_stage, S.H_stage + 256 * P.C, nullptr, /*writer=*/extra, &s_ctl);
        } else {
            if (extra) finish_evaluation<false>(P, S, ctl_init, !ctl_init, true, scratch, scratch + kHl, scratch + kHl + kGall, &s_ctl, head);
            else if (RIDE && cur_spec >= 0) control_outcome_late(P, S, ctl_init, early, scratch, scratch + kHl, &s_ctl, head);
            else control_outcome<false>(P, S, ctl_init, !ctl_init, scratch, scratch + kHl, &s_ctl, head);
        }
        if (extra) {
            // thread 0 took the serial part of the step and committed it: the outcome, written through, then the epoch
            if (threadIdx.x == 0) {
                __hip_atomic_store(&S.ctl_pub->cur, s_ctl.cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&S.ctl_pub->done, s_ctl.done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                handoff_store(&S.ctl_pub->radius, s_ctl.radius);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&S.ctl_pub->epoch, ctl_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
        }
        __syncthreads();
        // (wave-uniform by construction -- and the compiler has to know: `cur` selects the buffer descriptors)
        ctrl_done = __builtin_amdgcn_readfirstlane(s_ctl.done); cur = __builtin_amdgcn_readfirstlane(s_ctl.cur);
        radius = s_ctl.radius; dmin = s_ctl.dmin; dmax = s_ctl.dmax;
        __syncthreads();
    } else {
        ctrl_done = S.ctrl->done; cur = S.ctrl->cur;
        radius = S.ctrl->radius; dmin = S.ctrl->opt.min_lm_diagonal; dmax = S.ctrl->opt.max_lm_diagonal;
    }
    if (ctrl_done) return;
    PHASE_STAMP(ts0);
    if constexpr (RIDE) {
        if (cur != cur_spec) request(cur);
    } else {
        // (the same requests written out where they always were: this instantiation serves the grids of several rounds -- config 5 --
        // and inlined from the lambda above it came out 2.8 us slower there)
        const double *rec = S.rec[cur];
        // ---- requests: the pieces of the records of the boards this lane gathers (phase 0a), the W columns of the four
        //      groups of four boards its wave contracts (phase 1), the Jacobi scaling of the board it factors (phase 0b)
        const __amdgpu_buffer_rsrc_t r_w = make_rsrc(rec, sizeof(double) * (size_t)kRec * P.V);
        {
            const int e = tid & 15;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                // entry e + 16 j of the list above: offset of its first term inside the allocation relative to the board's
                // first view, stride between the views' terms (0: a single term)
                const int idx = e + 16 * j;
                const int pv = idx < 24 ? 0 : (idx - 24) / 9, r9 = idx < 24 ? 0 : (idx - 24) % 9;
                const bool summed = idx < 24;
                const unsigned first = idx < 18 ? 8u * ((unsigned)kRecW * (unsigned)P.V + (unsigned)idx)
                                     : idx < 24 ? 8u * (unsigned)(6 * kFR + idx - 18)
                                     : 8u * (unsigned)(kRecW * pv + 6 * (kWcolTc + r9 / 3) + 3 + r9 % 3);
                const unsigned per_slot = idx < 18 ? 8u * kRecE : 8u * kRecW;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int bf = 16 * i + (tid >> 4);
                    const unsigned o0 = idx < NE ? first + per_slot * (unsigned)(slot0 + NV * min(bf, nbd - 1)) : BAD;
                    double acc = 0.0;
#pragma unroll
                    for (int p = 0; p < NV; ++p) acc += buf_load_f64(r_w, (p == 0 || summed) ? o0 : BAD, per_slot * (unsigned)p);
                    ev[i][j] = acc;
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int bg = 4 * schur_group_of(nbd, vw, g) + kq;             // (no such group: negative)
            const unsigned base = (a < 14 && bg >= 0 && bg < nbd) ? 8u * ((unsigned)kRecW * (unsigned)(slot0 + NV * bg) + 6u * (unsigned)a) : BAD;
#pragma unroll
            for (int p = 0; p < NV; ++p)
#pragma unroll
                for (int k = 0; k < 3; ++k) {          // column a of the view's W: six adjacent doubles
                    const d2 v = buf_load_2f64(r_w, base, 8u * (unsigned)(kRecW * p + 2 * k));
                    w[g][p][2 * k] = v[0]; w[g][p][2 * k + 1] = v[1];
                }
        }
#pragma unroll
        for (int p = 0; p < NV; ++p) Rcp[p] = S.cconst[cur] + kCStride * P.slot_cam[slot0 + p];
    }
    double sb[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) sb[i] = tid < nbd ? S.s_b[6 * (c0 + tid) + i] : 1.0;
    const bool board_is_const = tid < nbd && P.board_const[c0 + tid] != 0;
    // ---- phase 0a: 16 lanes per board, 16 boards per pass ------------------------------------------------------------
    {
        const int e = tid & 15, grp = tid >> 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (RIDE && 16 * i >= nbd) break;                                // workgroup-uniform: a pass without boards (RIDE: see the head)
#pragma unroll
            for (int j = 0; j < NJ; ++j) if (e + 16 * j < NE) sumE[16 * i + grp][e + 16 * j] = ev[i][j];
        }
    }
    __syncthreads();
    PHASE_STAMP(ts1);
    // ---- phase 0b: one lane per board --------------------------------------------------------------------------------
    if (tid < nbd) {
        double M[21], g[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                if (j < 3) M[i * (i + 1) / 2 + j] = sumE[tid][6 * j + i];
                else {
                    double acc = 0.0;
#pragma unroll
                    for (int p = 0; p < NV; ++p) acc += tb_tb(RawTc{ &sumE[tid][24 + 9 * p] }, Rcp[p], i - 3, j - 3);
                    M[i * (i + 1) / 2 + j] = acc;
                }
            }
            g[i] = sumE[tid][18 + i];
        }
        if (!factor_core(M, g, sb, radius, dmin, dmax, facl[tid], board_is_const)) *S.fac_fail = 1;
    }
    __syncthreads();
    PHASE_STAMP(ts2);
    // the factor records leave for HBM (the back-substitution reads them): one contiguous stream for the chunk
    for (int i = tid; i < nbd * kFac; i += 256) S.fac[(size_t)kFac * c0 + i] = (&facl[0][0])[i];
    // ---- phase 1 ---------------------------------------------------------------------------------------------------------
    d4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = d4{ 0.0, 0.0, 0.0, 0.0 };
    const bool grad_col = a == kFR;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int grp = schur_group_of(nbd, vw, g);
        if (grp < 0) break;                                               // wave-uniform
        const int bg = 4 * grp + kq;
        const bool valid = bg < nbd;
        const int bl = min(bg, nbd - 1);
        FacFwd F;
#pragma unroll
        for (int i = 0; i < 15; ++i) F.m[i] = facl[bl][kFacM + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) { F.c[i] = facl[bl][kFacC + i]; F.z[i] = valid ? facl[bl][kFacZ + i] : 0.0; }
        double y[NV][6];
#pragma unroll
        for (int p = 0; p < NV; ++p) y_column(F, w[g][p], grad_col, y[p]);      // lanes without a board: w = 0, z = 0 -> y = 0
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            int t = 0;
#pragma unroll
            for (int p = 0; p < NV; ++p)
#pragma unroll
                for (int q = p; q < NV; ++q, ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[p][r], y[q][r], acc[t], 0, 0, 0);
        }
    }
    PHASE_STAMP(ts3);
    // D layout: lane (col = a, kq) holds rows kq + 4 r of column a -> tile entry [row][col]
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) tiles[vw][t][(kq + 4 * r) * 16 + a] = acc[t][r];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t)
        S.pairpart[(size_t)256 * P.bc_tile[6 * chunk + t] + tid] = (tiles[0][t][tid] + tiles[1][t][tid]) + (tiles[2][t][tid] + tiles[3][t][tid]);
#ifdef TSCM_WAVE_TIMELINE
    if (threadIdx.x == 0 && ktl_scope.on && (int)blockIdx.x < kKtlGroups) {
        long long *o = g_phs + (size_t)kPhStamps * blockIdx.x;
        o[0] = tsk; o[1] = ts0; o[2] = ts1; o[3] = ts2; o[4] = ts3; o[5] = wall_clock64(); o[6] = nbd; o[7] = (bid >= first_round ? 1 : 0) | ((RIDE && t_waited ? t_waited - tsk : 0) << 1) | ((RIDE && t_reduced ? t_reduced - tsk : 0) << 32);      // (bit 0: a later round; above: ticks until the riding reductions had arrived)
    }
#endif
#ifdef TSCM_PHASE_PROFILE
    if (threadIdx.x == 0 && (cblk == 0 || cblk == 200))
        printf("schur_gram wg %d: boards %d  head %lld  E sums %lld  factor %lld  gram %lld  tiles %lld [10 ns]\n", (int)blockIdx.x, nbd, ts0 - tsk, ts1 - ts0, ts2 - ts1, ts3 - ts2, wall_clock64() - ts3);
#endif
}

// Fallback for boards seen by more than three cameras: explicit list of view pairs, pre-sorted by
// camera-pair block; one 4-wave workgroup per chunk of pairs of a single block.   grid n_pchunks x 256
__global__ __launch_bounds__(256) void k_pair_gram(DevProblem P, DevState S)
{
    if (S.ctrl->done) return;
    __shared__ double red[4][256];
    const int pc = blockIdx.x;
    const int cur = S.ctrl->cur;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = lane & 15, kq = lane >> 4;
    d4 acc = { 0.0, 0.0, 0.0, 0.0 };
    for (int p = P.pc_begin[pc] + wave; p < P.pc_end[pc]; p += 4) {
        const double *Wi = rec_w(S.rec[cur], P.pair_i[p]), *Wj = rec_w(S.rec[cur], P.pair_j[p]);
        FacFwd F;
        load_fac_fwd(S.fac, __builtin_amdgcn_readfirstlane(P.pair_board[p]), F);     // p is wave-uniform
        double wi[6], wj[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) { wi[k] = a < 14 ? Wi[6 * a + k] : 0.0; wj[k] = a < 14 ? Wj[6 * a + k] : 0.0; }
        double i0, i1, j0, j1;
        y_column_operands(F, wi, a == kFR, kq, i0, i1);
        y_column_operands(F, wj, a == kFR, kq, j0, j1);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(i0, j0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(i1, j1, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][(kq + 4 * r) * 16 + a] = acc[r];
    __syncthreads();
    const int t = threadIdx.x;
    S.pairpart[(size_t)256 * P.pc_tile[pc] + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

// (kTEntries, kTSlices: tscm_exec_plan.h)
// block blk of a (n_bids * 256 / ENTRIES)-block grid of ENTRIES * kTSlices threads, partial tiles [cb, ce) of its
// camera-pair block; the summation order of an entry depends on kTSlices only, so every geometry produces the same bits
template <int ENTRIES>
__device__ __forceinline__ void t_reduce_block(const DevState &S, int bid, int part, int cb, int ce, double (*red)[ENTRIES])
{
    const int e = threadIdx.x % ENTRIES, slice = threadIdx.x / ENTRIES;
    const int entry = part * ENTRIES + e;
    const int per = (ce - cb + kTSlices - 1) / kTSlices;
    const int b0 = cb + slice * per, b1 = min(ce, b0 + per);
    // the partial tiles of one block are stored contiguously; eight loads in flight per thread, the ragged end
    // included (no dependent tail loop)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0, a6 = 0.0, a7 = 0.0;
    const double *src = S.pairpart + entry;
    for (int c = b0; c < b1; c += 8) {
        const double v0 = src[(size_t)256 * c];
        const double v1 = c + 1 < b1 ? src[(size_t)256 * (c + 1)] : 0.0;
        const double v2 = c + 2 < b1 ? src[(size_t)256 * (c + 2)] : 0.0;
        const double v3 = c + 3 < b1 ? src[(size_t)256 * (c + 3)] : 0.0;
        const double v4 = c + 4 < b1 ? src[(size_t)256 * (c + 4)] : 0.0;
        const double v5 = c + 5 < b1 ? src[(size_t)256 * (c + 5)] : 0.0;
        const double v6 = c + 6 < b1 ? src[(size_t)256 * (c + 6)] : 0.0;
        const double v7 = c + 7 < b1 ? src[(size_t)256 * (c + 7)] : 0.0;
        a0 += v0; a1 += v1; a2 += v2; a3 += v3; a4 += v4; a5 += v5; a6 += v6; a7 += v7;
    }
    red[slice][e] = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
    __syncthreads();
    if (slice == 0) {
        // tiles without a local partial (the pair is only seen on other ranks) are written as zeros
        double v[kTSlices];
#pragma unroll
        for (int q = 0; q < kTSlices; ++q) v[q] = red[q][e];
#pragma unroll
        for (int w = kTSlices / 2; w >= 1; w >>= 1)
#pragma unroll
            for (int q = 0; q < w; ++q) v[q] += v[q + w];
        handoff_store(&S.T[(size_t)256 * bid + entry], v[0]);      // (written through: the fused launch hands T over inside the launch)
    }
}
// grid (n_bids * 256 / kTEntries) x 1024: block (bid, part) sums kTEntries entries of the partial tiles that belong to
// one camera-pair block, the tile list split kTSlices ways across the threads of an entry (the kernel is a chain of
// memory round trips: the more of the list is in flight at once, the shorter it is)
__global__ __launch_bounds__(kTEntries * kTSlices) void k_T_reduce(DevProblem P, DevState S)
{
    if (S.ctrl->done) return;
    __shared__ double red[kTSlices][kTEntries];
    constexpr int kParts = 256 / kTEntries;
    const int bid = blockIdx.x / kParts;
    t_reduce_block<kTEntries>(S, bid, blockIdx.x % kParts, P.bid_part_ptr[bid], P.bid_part_ptr[bid + 1], red);
}

// T(i, j) for padded columns i, j of the camera side; the lower blocks are the transposed upper ones
__device__ __forceinline__ double load_T_lut(const DevProblem &P, const double *T, int i, int j)
{
    int lo = i >> 4, hi = j >> 4, a = i & 15, b = j & 15;
    if (lo > hi) { const int t = lo; lo = hi; hi = t; const int u = a; a = b; b = u; }
    const int tile = P.bid_lut[lo * P.C + hi];
    return tile >= 0 ? T[(size_t)256 * tile + a * 16 + b] : 0.0;
}

// Common end of the reduced-system solvers: yhat = S_c y (camera step = -yhat), the candidate camera parameters, and
// the camera part of the model cost change / step norm.  One thread per padded column (n_pad <= workgroup size in
// every variant).  The global operands of the tail -- the column's parameter and its row of H -- do not depend on
// the solution: tail_prefetch() issues their loads early (before the back-substitution where registers allow), so
// the tail itself waits for no memory.
struct TailOperands { double x, hg, hrow[kFA]; };
// (i: the padded column -- the calling thread's own unless another thread requests the operands for it)
__device__ __forceinline__ void tail_prefetch(const DevProblem &P, const DevState &S, int cur, const double *H, TailOperands &o, int i)
{
    o.x = 0.0; o.hg = 0.0;
#pragma unroll
    for (int b = 0; b < kFA; ++b) o.hrow[b] = 0.0;
    if (i < P.n_pad) {
        const int m = i >> 4, ai = i & 15;
        if (ai < 6) o.x = S.cam_rt[cur][6 * m + ai];
        else if (ai < 15) o.x = S.intr[cur][9 * m + (ai - 6)];
        if (ai < kFA) {
#pragma unroll
            for (int b = 0; b < kFA; ++b) o.hrow[b] = H[256 * m + ai * 16 + b];
            o.hg = H[256 * m + ai * 16 + kFR];
        }
    }
}
__device__ __forceinline__ void tail_prefetch(const DevProblem &P, const DevState &S, int cur, const double *H, TailOperands &o)
{
    tail_prefetch(P, S, cur, H, o, (int)threadIdx.x);
}
// yv: solution by padded column (LDS); s_sc, s_yh, s_act: LDS arrays of n_pad entries.  Every thread of the workgroup calls it.
// publish_epoch > 0: workgroups of this launch wait for the step (backsub_body<.., true>): yhat and the candidate camera
// parameters are written through, and once they are complete thread 0 sets y_flag = 2 * epoch + fail
__device__ __forceinline__ void reduced_solution_tail(const DevProblem &P, const DevState &S, int cur, int fail, const TailOperands &o,
                                                      const double *yv, const double *s_sc, double *s_yh, const unsigned char *s_act, double *sred,
                                                      int publish_epoch = 0)
{
    const int n = P.n_pad, i = threadIdx.x;
    const int m = i >> 4, ai = i & 15;
    double model = 0.0, stepsq = 0.0, yh = 0.0;
    if (i < n) {
        const bool act = s_act[i] && !fail;
        yh = act ? s_sc[i] * yv[i] : 0.0;
        handoff_store(&S.yhat[i], yh);
        s_yh[i] = yh;
        if (ai < kFA) {
            const double x = o.x;
            const double xn = x + (-yh);
            if (ai < 6) handoff_store(&S.cam_rt[cur ^ 1][6 * m + ai], xn); else handoff_store(&S.intr[cur ^ 1][9 * m + (ai - 6)], xn);
            const double d = x - xn; stepsq = d * d;
        } else if (ai < 15) {
            handoff_store(&S.intr[cur ^ 1][9 * m + (ai - 6)], o.x);   // b, c are inert
        }
    }
    if (publish_epoch > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (publish_epoch > 0 && i == 0) __hip_atomic_store(S.y_flag, 2 * publish_epoch + (fail ? 1 : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the candidate's per-camera records for the next evaluation: the waiting workgroups are busy now, this one is not.
    // (Plain loads: this workgroup wrote the parameters itself, through its own L2, and never had them in its L1.)
    if (publish_epoch > 0 && i >= 64 && i < 64 + P.C) write_camera_record(S, cur ^ 1, i - 64);
    // model_cam = yhat^T g_c - 1/2 yhat^T H_cc yhat   (block diagonal H_cc)
    if (i < n && ai < kFA && yh != 0.0) {
        double hy = 0.0;
#pragma unroll
        for (int b = 0; b < kFA; ++b) hy += o.hrow[b] * s_yh[m * 16 + b];
        model = yh * (o.hg - 0.5 * hy);
    }
    { double red[2] = { model, stepsq }, mdummy = 0.0; block_reduce256<2>(red, mdummy, sred); model = red[0]; stepsq = red[1]; }
    if (i == 0) { S.ctrl->model_cam = model; S.ctrl->stepsq_cam = stepsq; S.ctrl->lin_fail = fail; *S.fac_fail = 0; }
}
