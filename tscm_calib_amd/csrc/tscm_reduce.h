// tscm_reduce.h -- stage 2, behind the evaluation: the camera-tile and board-statistics reductions and the LM control step
// (accept / reject, trust-region radius, termination) on their results.
#pragma once
// (included from tscm_kernels.h inside namespace tscm)

// camera priors (tscm_spec.h: effective_priors): mean and weight per camera-side column, [C][16] each, the weight 0
// where the column is not free -- an argument of the PRIOR kernels alone
struct PriorArg { const double *mean, *weight; };
// The prior's part of raw entry e (of 512: half, tile row, tile column) of camera cam's tile at the target point: w_k on the
// diagonal entry of column k, w_k d_k on (k, kFR) and (kFR, k) -- the raw tile is kept full -- and sum w_k d_k^2 on (kFR, kFR), with
// d_k = x_k - mean_k.  camera_tile_entry adds the halves, so a term sits in ONE of them: GU where f_mask(a) & f_mask(b) & 1,
// else GV (fy, cy).  Columns in order: the same bits on every call
__device__ __forceinline__ double prior_raw_entry(const DevState &S, const PriorArg &pr, int cam, int e, int tgt)
{
    const int h = e >> 8, ta = (e >> 4) & 15, tb = e & 15;
    double v = 0.0;
    for (int k = 0; k < kFA; ++k) {
        const double w = pr.weight[16 * cam + k];
        if (!(w > 0.0)) continue;
        const double x = k < 6 ? S.cam_rt[tgt][6 * cam + k] : S.intr[tgt][9 * cam + (k - 6)];
        const double d = x - pr.mean[16 * cam + k];
        const int tk = f_tile(k), hk = (f_mask(k) & 1) ? 0 : 1;
        if (ta == kTcR && tb == kTcR) { if (h == 0) v += w * d * d; }
        else if (h != hk) continue;
        else if (ta == tk && tb == tk) v += w;
        else if ((ta == tk && tb == kTcR) || (ta == kTcR && tb == tk)) v += w * d;
    }
    return v;
}
// per-camera raw tile (GU | GV) reduction: one block per (camera, slice of 32 of the 512 raw entries).  Eight threads per
// entry take every eighth workgroup tile -- up to 32 loads per thread requested at once -- and are combined through LDS
// in a fixed order: campart2[cam][512] holds the finished sums (round 3; before: 16 groups of tiles per camera here and
// a second level in k_finalize_eval, 16 more dependent loads per thread in a kernel that is nothing but a latency chain)
// PRIOR: behind the fixed-order sum the thread that stores a raw entry adds that entry's prior term at the target point (cand: the
// candidate, as board_stats_block forms it); PRIOR = false is the code without priors, cam_reduce_block
template <bool PRIOR>
__device__ __forceinline__ void cam_reduce(const DevProblem &P, const DevState &S, int blk, double *sm /* 256 doubles */, int cand, const PriorArg &pr)
{
    const int cam = blk / kCamSl, sl = blk % kCamSl;
    int cb, ce;
    if (P.C <= kMaxCamLds) {
        cb = P.cam_wg[0]; ce = P.cam_wg[1];
#pragma unroll
        for (int q = 1; q < kMaxCamLds; ++q) { cb = cam >= q ? P.cam_wg[q] : cb; ce = cam >= q ? P.cam_wg[q + 1] : ce; }
    } else {
        cb = P.cam_chunk_ptr[cam]; ce = P.cam_chunk_ptr[cam + 1];
    }
    const int t = threadIdx.x, o = t & 31, ph = t >> 5;
    const double *src = S.campart + 32 * sl + o;
    double acc = 0.0;
    for (int base = cb + ph; base < ce; base += 256) {
        double v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) { const int c = base + 8 * u; v[u] = src[(size_t)512 * min(c, ce - 1)]; v[u] = c < ce ? v[u] : 0.0; }
#pragma unroll
        for (int w = 16; w >= 1; w >>= 1)
#pragma unroll
            for (int u = 0; u < w; ++u) v[u] += v[u + w];
        acc += v[0];
    }
    sm[t] = acc;
    __syncthreads();
    if constexpr (PRIOR) {
        if (t < 32) {
            const double sum = ((sm[t] + sm[32 + t]) + (sm[64 + t] + sm[96 + t])) + ((sm[128 + t] + sm[160 + t]) + (sm[192 + t] + sm[224 + t]));
            handoff_store(&S.campart2[(size_t)512 * cam + 32 * sl + t], sum + prior_raw_entry(S, pr, cam, 32 * sl + t, cand ? (S.ctrl->cur ^ 1) : S.ctrl->cur));
        }
    } else {
        if (t < 32)
            handoff_store(&S.campart2[(size_t)512 * cam + 32 * sl + t], ((sm[t] + sm[32 + t]) + (sm[64 + t] + sm[96 + t])) + ((sm[128 + t] + sm[160 + t]) + (sm[192 + t] + sm[224 + t])));
    }
    __syncthreads();
}
__device__ void cam_reduce_block(const DevProblem &P, const DevState &S, int blk, double *sm /* 256 doubles */) { cam_reduce<false>(P, S, blk, sm, 0, PriorArg{}); }

// deterministic block reductions (256 threads)
// Block reductions (256 threads; any multiple of 64 works): DPP butterfly inside each 16-lane row, two xor shuffles across the
// rows of a wave, one LDS exchange between the
// waves -- two barriers per call, several quantities at once (the previous LDS tree cost ten barriers per
// quantity: 1.5 us each on the single-block control paths).  Fixed order: bit-reproducible.
template <int NS>
__device__ __forceinline__ void block_reduce256(double (&sum)[NS], double &mx, double *sm)   // sm: >= 4 * (NS + 1) doubles
{
#pragma unroll
    for (int i = 0; i < NS; ++i) sum[i] = row16_allsum(sum[i]);
    mx = row16_allmax(mx);
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
#pragma unroll
        for (int i = 0; i < NS; ++i) sum[i] += __shfl_xor(sum[i], off);
        mx = fmax(mx, __shfl_xor(mx, off));
    }
    const int wave = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NS; ++i) sm[wave * (NS + 1) + i] = sum[i];
        sm[wave * (NS + 1) + NS] = mx;
    }
    __syncthreads();
    if (nw == 4) {
#pragma unroll
        for (int i = 0; i < NS; ++i) sum[i] = (sm[i] + sm[(NS + 1) + i]) + (sm[2 * (NS + 1) + i] + sm[3 * (NS + 1) + i]);
        mx = fmax(fmax(sm[NS], sm[(NS + 1) + NS]), fmax(sm[2 * (NS + 1) + NS], sm[3 * (NS + 1) + NS]));
    } else {                                    // other workgroup sizes (k_solve_reduced<4, 32>): waves in order
#pragma unroll
        for (int i = 0; i < NS; ++i) { double t = 0.0; for (int w = 0; w < nw; ++w) t += sm[w * (NS + 1) + i]; sum[i] = t; }
        double t = sm[NS];
        for (int w = 1; w < nw; ++w) t = fmax(t, sm[w * (NS + 1) + NS]);
        mx = t;
    }
    __syncthreads();
}
__device__ __forceinline__ double block_sum256(double v, double *sm)
{
    double s[1] = { v }, m = 0.0;
    block_reduce256<1>(s, m, sm);
    return s[0];
}
__device__ __forceinline__ double block_max256(double v, double *sm)
{
    double s[1] = { 0.0 }, m = v;
    block_reduce256<1>(s, m, sm);
    return m;
}

// per-board gradient / norm statistics of the evaluation target (and, at iteration 0, the
// Jacobi scaling of the board columns: s = 1/(1 + ||J_col||)).  grid ceil(B/256) x 256
__device__ void board_stats_block(const DevProblem &P, const DevState &S, int cand, int init, int blk, double *sm)
{
    const int tgt = cand ? (S.ctrl->cur ^ 1) : S.ctrl->cur;
    const int b = blk * 256 + threadIdx.x;
    double gmax = 0.0, gsq = 0.0, xsq = 0.0;
    if (b < P.B) {
        const int q0 = P.bv_ptr[b], q1 = P.bv_ptr[b + 1];
        if (q1 > q0 && !P.board_const[b]) {         // constant pose blocks are not part of the reduced program
            double g[6] = { 0, 0, 0, 0, 0, 0 }, dg[6] = { 0, 0, 0, 0, 0, 0 };
            // the gradient columns of up to four views per trip, requested together (a load inside a loop of unknown
            // length is one memory round trip per view); same order of additions
            for (int qb = q0; qb < q1; qb += 4) {
                double w[4][6];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double *G = rec_g(S.rec[tgt], P.V, min(qb + u, q1 - 1));
#pragma unroll
                    for (int i = 0; i < 6; ++i) w[u][i] = G[i];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int i = 0; i < 6; ++i) g[i] += qb + u < q1 ? w[u][i] : 0.0;
            }
            if (init) {                         // diag(E^T E) is only needed for the Jacobi scaling
                for (int q = q0; q < q1; ++q) {
                    const double *W = rec_w(S.rec[tgt], q);
                    const double *E = rec_e(S.rec[tgt], P.V, q), *Rc = S.cconst[tgt] + kCStride * P.slot_cam[q];
                    for (int i = 0; i < 3; ++i) { dg[i] += E[6 * i + i]; dg[3 + i] += tb_tb(W, Rc, i, i); }
                }
            }
            for (int i = 0; i < 6; ++i) {
                const double x = S.board_rt[tgt][6 * b + i];
                const double d = x - (x + (-g[i]));   // |x - Plus(x, -gradient)| like Ceres
                gmax = fmax(gmax, fabs(d)); gsq += d * d; xsq += x * x;
                if (init) S.s_b[6 * b + i] = S.ctrl->opt.jacobi_scaling ? 1.0 / (1.0 + sqrt(dg[i])) : 1.0;
            }
        } else if (init) {
            for (int i = 0; i < 6; ++i) S.s_b[6 * b + i] = 1.0;
        }
    }
    double red[2] = { gsq, xsq }, m = gmax;
    block_reduce256<2>(red, m, sm);
    const double s1 = red[0], s2 = red[1];
    if (threadIdx.x == 0) { handoff_store(&S.st_part[kStStride * blk], m); handoff_store(&S.st_part[kStStride * blk + 1], s1); handoff_store(&S.st_part[kStStride * blk + 2], s2); }
}

// one launch for the two independent post-evaluation reductions:
//   blocks [0, C*kCamSl)            sums of the per-workgroup camera tiles
//   blocks [C*kCamSl, +ceil(B/256)) per-board gradient / norm statistics (+ Jacobi scaling at iteration 0)
__global__ __launch_bounds__(256) void k_reduce_stats(DevProblem P, DevState S, int cand, int init)
{
    KTL(1);
    // snapshot of the LM state for the control step in the head of the next launch (k_schur_gram, DevState::ctrl_snap):
    // taken BEFORE the early exit, so that a finished -- or faulted -- solve is seen there as well
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x < sizeof(CtrlHead) / 8)
        reinterpret_cast<unsigned long long *>(S.ctrl_snap)[threadIdx.x] = reinterpret_cast<const unsigned long long *>(S.ctrl)[threadIdx.x];
    if (S.ctrl->done) return;
    __shared__ double sm[256];
    const int nc = P.C * kCamSl;
    if ((int)blockIdx.x < nc) cam_reduce_block(P, S, blockIdx.x, sm);
    else board_stats_block(P, S, cand, init, blockIdx.x - nc, sm);
}
// ... of a solve with camera priors (ExecPlan::priors) and of tscm_eval_normal_equations* with them: the same launch with the
// PRIOR camera-tile reduction.  A kernel of its own, not an instantiation of a shared body, and no k_reduce_control of this
// kind (plan_exec: k_finalize_eval and k_control follow instead): k_reduce_stats and k_reduce_control keep their code bit for
// bit only as they are written and instantiated once (tools/same_kernels.py)
__global__ __launch_bounds__(256) void k_reduce_stats_prior(DevProblem P, DevState S, int cand, int init, PriorArg pr)
{
    KTL(1);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x < sizeof(CtrlHead) / 8)
        reinterpret_cast<unsigned long long *>(S.ctrl_snap)[threadIdx.x] = reinterpret_cast<const unsigned long long *>(S.ctrl)[threadIdx.x];
    if (S.ctrl->done) return;
    __shared__ double sm[256];
    const int nc = P.C * kCamSl;
    if ((int)blockIdx.x < nc) cam_reduce<true>(P, S, blockIdx.x, sm, cand, pr);
    else board_stats_block(P, S, cand, init, blockIdx.x - nc, sm);
}

// H_stage = C camera tiles ([F|r]^T[F|r] from the raw u/v sums), then kScal scalars: [0] model_b [1] stepsq_b [2] xsq_b [3] gsq_b
// [4] e-block factorisation failures on this rank, then one slot per rank with that rank's board gradient max-norm
// (zero in the other ranks' slots): ONE sum all-reduce carries sums, the failure flag and the maximum.
// What the control step reads from memory that does NOT depend on the evaluation being finalised: the LM state and the
// target point's camera-side parameters, requested together with the first loads of the workgroup that runs the step.
struct ControlPre { CtrlHead c; double x[2]; bool free_param[2], grad_param[2]; };   // free_param: counts in |x|; grad_param: has a gradient
// what the kernel that runs the control step in its head goes on with (LDS, written by thread 0)
struct CtlOut { int cur, done; double radius, dmin, dmax; };
// `head`: where the LM state is read from -- S.ctrl where the calling workgroup is the only one that takes the step
// (k_reduce_control's last workgroup, k_control_tail, k_control), S.ctrl_snap where every workgroup of a launch takes it
// while one of them writes S.ctrl (k_schur_gram)
// ... split in two for a workgroup that has to WAIT for the evaluation's reductions first (k_schur_gram<NV, true>): what does not
// depend on them -- the parameters of both buffers, the camera flags, the back-substitution's partials (summed per thread) -- is
// requested in front of the wait, the LM state behind it
struct ControlEarly { double x0[2], x1[2]; int cls[2]; double mb, ss; };
__device__ __forceinline__ void control_early_params(const DevProblem &P, const DevState &S, ControlEarly &e)
{
    // (both parameter buffers and the camera flags are requested without waiting for `cur`: one round trip, not two)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = threadIdx.x + 256 * j;
        const int m = min(p >> 4, P.C - 1), a = p & 15;
        const int ia = a < 6 ? 6 * m + a : 9 * m + min(a - 6, 8);
        e.x0[j] = a < 6 ? S.cam_rt[0][ia] : S.intr[0][ia];
        e.x1[j] = a < 6 ? S.cam_rt[1][ia] : S.intr[1][ia];
        // (bounded for any block size: the last entry is column 15 of camera kMaxCam - 1, a padding column whose class is 0)
        e.cls[j] = P.col_ctl[min(p, 16 * kMaxCam - 1)];
    }
}
__device__ __forceinline__ void control_state(const DevProblem &P, int init, ControlPre &pre, const CtrlHead *head, const ControlEarly &e)
{
    // (the LM state through the scalar cache: wave-uniform, and when 500 workgroups take the step at once -- k_schur_gram's
    // head -- 2,000 waves x 22 vector loads of the same six cache lines queue up at one L2 channel)
    {
        static_assert(sizeof(CtrlHead) % 8 == 0, "copied in 8-byte words");
        typedef const unsigned long long __attribute__((address_space(4))) *cq4;
        const cq4 src = (cq4)(const void *)head;
        unsigned long long w[sizeof(CtrlHead) / 8];
#pragma unroll
        for (unsigned q = 0; q < sizeof(CtrlHead) / 8; ++q) w[q] = src[q];
        __builtin_memcpy(&pre.c, w, sizeof(CtrlHead));
    }
    const int tgt = init ? pre.c.cur : (pre.c.cur ^ 1);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = threadIdx.x + 256 * j;
        const int a = p & 15;
        const bool in = p < 16 * P.C && a < 15;
        pre.x[j] = in ? (tgt ? e.x1[j] : e.x0[j]) : 0.0;
        pre.free_param[j] = in & ((e.cls[j] & 1) != 0);
        pre.grad_param[j] = in & ((e.cls[j] & 2) != 0);
    }
}
__device__ __forceinline__ void control_prefetch(const DevProblem &P, const DevState &S, int init, ControlPre &pre, const CtrlHead *head)
{
    ControlEarly e;
    control_early_params(P, S, e);
    control_state(P, init, pre, head, e);
}

// ---------------------------------------------------------------------------------------------
// LM control (TrustRegionMinimizer + LevenbergMarquardtStrategy + TrustRegionStepEvaluator),
// one thread.  `init` = IterationZero; otherwise the tail of one loop iteration followed by
// FinalizeIterationAndCheckIfMinimizerCanContinue.
// ---------------------------------------------------------------------------------------------
// H: the (all-reduced) camera tiles, sc: the scalars behind them -- H_stage in global memory, or the LDS copy of the
// workgroup that formed them (k_reduce_control: stage_copy = H_stage, which then receives a copy as well)
// writer = false: the step is taken redundantly (k_schur_gram: every workgroup runs it in its head, on the same inputs,
// to the same bits -- no hand-off, no kernel of its own); only the writer touches global memory.  out: the new state for
// the calling workgroup.
__device__ void control_step(const DevProblem &P, const DevState &S, int init, const ControlPre &pre, double *sm, const double *H, const double *sc, double *stage_copy,
                             bool writer = true, CtlOut *out = nullptr)
{
    // The LM state is read ONCE (wide loads, one memory round trip -- by control_prefetch, at the head of the kernel),
    // advanced in registers and written back once: as individual fields in global memory the ~40 dependent loads and
    // stores of this function cost about half a microsecond each on the single thread that executes it.
    Ctrl &g = *S.ctrl;
    CtrlHead c = pre.c;
    const int t = threadIdx.x;
    if (out && t == 0) { out->cur = c.cur; out->done = c.done; out->radius = c.radius; out->dmin = c.opt.min_lm_diagonal; out->dmax = c.opt.max_lm_diagonal; }
    if (c.done) return;
    const Options &o = c.opt;
    const int tgt = init ? c.cur : (c.cur ^ 1);
    // camera-side norms |x - Plus(x, -g)|_inf, its 2-norm, |x|^2 and the cost, one thread per parameter
    double gmax_c = 0.0, gsq_c = 0.0, xsq_c = 0.0, cost = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {                       // (one pass up to 16 cameras, two up to kMaxCam)
        const int p = t + 256 * j;
        if (p >= 16 * P.C) break;
        const int m = p >> 4, a = p & 15;
        if (pre.free_param[j]) {
            const double x = pre.x[j];
            const double g = pre.grad_param[j] ? H[256 * m + a * 16 + kFR] : 0.0;   // b, c and held intrinsics: zero gradient (d = 0)
            const double d = x - (x + (-g));
            gmax_c = fmax(gmax_c, fabs(d)); gsq_c += d * d; xsq_c += x * x;
        }
        if (a == 15) cost += 0.5 * H[256 * m + kFR * 16 + kFR];
        if (init && writer && a < 15) {
            const double hii = (a < kFA) ? H[256 * m + a * 16 + a] : 0.0;
            S.s_c[p] = o.jacobi_scaling ? 1.0 / (1.0 + sqrt(hii)) : 1.0;
        }
        if (init && writer && a == 15) S.s_c[p] = 1.0;
    }
    KTLX(4, true);
    { double red[3] = { gsq_c, xsq_c, cost }; block_reduce256<3>(red, gmax_c, sm); gsq_c = red[0]; xsq_c = red[1]; cost = red[2]; }
    KTLX(5, true);
    // publish the staged (all-reduced) camera tiles as the target system's H -- behind the last barrier of this step: a
    // barrier with global stores in flight waits for their acknowledgement
    if (writer) {
#pragma unroll 8
        for (int i = t; i < 256 * P.C; i += 256) { const double h = H[i]; S.H[tgt][i] = h; if (stage_copy) stage_copy[i] = h; }
        if (stage_copy && t < kScal + P.world) stage_copy[256 * P.C + t] = sc[t];
    }
    if (t != 0) return;
    auto commit = [&]() {
        c.fin_count = 0;
        if (writer) static_cast<CtrlHead &>(g) = c;
        if (out) { out->cur = c.cur; out->done = c.done; out->radius = c.radius; }
    };
    double gmax_b = 0.0;
    for (int r = 0; r < P.world; ++r) gmax_b = fmax(gmax_b, sc[kScal + r]);
    const double gmax_t = fmax(gmax_c, gmax_b);
    if (sc[4] > 0.0) c.lin_fail = 1;          // an e-block factorisation failed on some rank: every rank rejects the step
    const double gnorm_t = sqrt(gsq_c + sc[3]);
    const double xnorm_t = sqrt(xsq_c + sc[2]);
    KTLX(6, true);

    IterLog it;
    const StepInput in = { cost, gmax_t, gnorm_t, xnorm_t, sc[0] + c.model_cam, sqrt(sc[1] + c.stepsq_cam) };
    if (lm_step(c, init, tgt, in, it) && writer && c.n_log <= kMaxLog) g.log[c.n_log - 1] = it;
    commit();
}

// raw (GU | GV) tile of one camera (G: 512 doubles in LDS) -> H layout: 14x14 [F | r]^T [F | r] in a 16x16 slot
__device__ __forceinline__ double camera_tile_entry(const double *G, int t)
{
    const int a = t >> 4, b = t & 15;
    double v = 0.0;
    if (a < 14 && b < 14) {
        const int ta = f_tile(a), tb = f_tile(b), m = f_mask(a) & f_mask(b);
        if (m & 1) v += G[ta * 16 + tb];
        if (m & 2) v += G[256 + ta * 16 + tb];
    }
    return v;
}

// the per-workgroup scalar partials of the back-substitution and of the board statistics -> the kScal + world scalars
// that follow the camera tiles in H_stage, written to `sc` (global or LDS; 256 threads; sm: block_reduce256 scratch).
// Every load is unconditional (clamped index, value masked): a load under `if (i < n)` is a branch with its own wait,
// and the eight + four of them in the ragged ends were twelve memory round trips in a row (5 us of the control
// workgroup's 10, tools/kernel_timeline.py).
// THROUGH: the board statistics were handed over inside this launch (handoff_store): read them the same way
// (the back-substitution's partials, summed per thread: written by the launch before -- no hand-off)
__device__ __forceinline__ void backsub_partials(const DevState &S, int have_backsub, double &mb, double &ss)
{
    const int t = threadIdx.x;
    mb = 0.0; ss = 0.0;
    if (have_backsub) {
        const d2 *bp = reinterpret_cast<const d2 *>(S.bs_part);
        const int n = S.n_bs_blocks;
        d2 a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = d2{ 0.0, 0.0 };
        for (int i = t; i < n; i += 8 * 256) {
            d2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = bp[min(i + 256 * u, n - 1)];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] += i + 256 * u < n ? v[u] : d2{ 0.0, 0.0 };
        }
        const d2 r = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
        mb = r[0]; ss = r[1];
    }
}
template <bool THROUGH>
__device__ __forceinline__ void reduce_scalar_partials_from(const DevProblem &P, const DevState &S, double mb, double ss, int lin_fail, double *sc, double *sm)
{
    const int t = threadIdx.x;
    double gm = 0.0, gs = 0.0, xs = 0.0;
    {
        const int n = S.n_st_blocks;
        double g4[4] = { 0, 0, 0, 0 }, s4[4] = { 0, 0, 0, 0 }, x4[4] = { 0, 0, 0, 0 };
        for (int i = t; i < n; i += 4 * 256) {
            double q[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const double *src = S.st_part + kStStride * (size_t)min(i + 256 * u, n - 1); q[u][0] = THROUGH ? handoff_load(src) : src[0]; q[u][1] = THROUGH ? handoff_load(src + 1) : src[1]; q[u][2] = THROUGH ? handoff_load(src + 2) : src[2]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) { const bool in = i + 256 * u < n; g4[u] = fmax(g4[u], in ? q[u][0] : 0.0); s4[u] += in ? q[u][1] : 0.0; x4[u] += in ? q[u][2] : 0.0; }
        }
        gm = fmax(fmax(g4[0], g4[1]), fmax(g4[2], g4[3])); gs = (s4[0] + s4[1]) + (s4[2] + s4[3]); xs = (x4[0] + x4[1]) + (x4[2] + x4[3]);
    }
    double red[4] = { mb, ss, gs, xs };
    block_reduce256<4>(red, gm, sm);
    mb = red[0]; ss = red[1]; gs = red[2]; xs = red[3];
    if (t == 0) {
        sc[0] = mb; sc[1] = ss; sc[2] = xs; sc[3] = gs; sc[4] = lin_fail ? 1.0 : 0.0; sc[5] = 0.0; sc[6] = 0.0; sc[7] = 0.0;
        for (int r = 0; r < P.world; ++r) sc[kScal + r] = r == P.rank ? gm : 0.0;
    }
}
template <bool THROUGH>
__device__ __forceinline__ void reduce_scalar_partials(const DevProblem &P, const DevState &S, int have_backsub, int lin_fail, double *sc, double *sm)
{
    double mb, ss;
    backsub_partials(S, have_backsub, mb, ss);
    reduce_scalar_partials_from<THROUGH>(P, S, mb, ss, lin_fail, sc, sm);
}

// camera tiles (raw u/v sums -> [F|r]^T[F|r]) into H_stage + reduction of the per-block scalar partials, for the paths
// with something between the evaluation and the control step (all-reduce: k_control follows) or without a control step
// (tscm_eval_normal_equations).  grid (C + 1) x 256, or C x 256 for the camera tiles alone.
__global__ __launch_bounds__(256) void k_finalize_eval(DevProblem P, DevState S, int have_backsub)
{
    KTL(2);
    const int done = S.ctrl->done, lin_fail = S.ctrl->lin_fail;
    if (done) return;
    __shared__ double sm[256];
    __shared__ double G[512];
    const int t = threadIdx.x;
    if ((int)blockIdx.x < P.C) {
        const int cam = blockIdx.x;
        G[t] = S.campart2[(size_t)512 * cam + t];
        G[256 + t] = S.campart2[(size_t)512 * cam + 256 + t];
        __syncthreads();
        S.H_stage[256 * cam + t] = camera_tile_entry(G, t);
    } else {
        reduce_scalar_partials<false>(P, S, have_backsub, lin_fail, S.H_stage + 256 * P.C, sm);
    }
}

// What is left of an evaluation once the camera-tile sums (campart2) and the scalar partials are complete: one batch of
// loads -- the 512 finished sums per camera, the partials, the LM state, the target point's camera parameters -- H in
// LDS, the control step on that copy.  Called by the last workgroup of k_reduce_control (writer), by k_control_tail,
// and by EVERY workgroup of k_schur_gram in its head (one of them the writer): the step is cheap, deterministic and
// needs no hand-off when everybody takes it.  Hl: 256 C + kScal + 8 doubles, Gall: 512 C, sm: 256 (LDS; C <= 8).
// THROUGH: the sums were handed over inside this launch (k_reduce_control); otherwise they come through a kernel boundary
// and plain loads let the L2s serve the 500 workgroups of k_schur_gram that all read the same 36 KB
template <bool THROUGH>
__device__ __forceinline__ void finish_evaluation(const DevProblem &P, const DevState &S, int init, int have_backsub, bool writer,
                                                  double *Hl, double *Gall, double *sm, CtlOut *out, const CtrlHead *head)
{
    const int t = threadIdx.x;
    ControlPre pre;
    control_prefetch(P, S, init, pre, head);
    double gu[kMaxCamLds], gv[kMaxCamLds];
#pragma unroll
    for (int m = 0; m < kMaxCamLds; ++m) {
        const int cam = min(m, P.C - 1);
        gu[m] = THROUGH ? handoff_load(&S.campart2[(size_t)512 * cam + t]) : S.campart2[(size_t)512 * cam + t];
        gv[m] = THROUGH ? handoff_load(&S.campart2[(size_t)512 * cam + 256 + t]) : S.campart2[(size_t)512 * cam + 256 + t];
    }
    double *scl = Hl + 256 * P.C;
    reduce_scalar_partials<THROUGH>(P, S, have_backsub, pre.c.lin_fail, scl, sm);
    KTLX(2, true);
    // (all cameras' raw tiles in LDS at once: one barrier, not two per camera)
#pragma unroll
    for (int m = 0; m < kMaxCamLds; ++m) if (m < P.C) { Gall[512 * m + t] = gu[m]; Gall[512 * m + 256 + t] = gv[m]; }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kMaxCamLds; ++m) if (m < P.C) Hl[256 * m + t] = camera_tile_entry(Gall + 512 * m, t);
    __syncthreads();
    KTLX(3, true);
    // (no global store up to here: a barrier behind one waits for its acknowledgement, a microsecond.  The control
    // step writes H -- and H_stage, for whoever reads the staged copy -- behind its own last barrier.)
    control_step(P, S, init, pre, sm, Hl, scl, S.H_stage, writer, out);
}

// The same step for a workgroup that only needs its OUTCOME (every workgroup of k_schur_gram but the extra one that
// writes): of H only the gradient column and the cost entry of each camera enter the step -- 15 entries per camera, two
// loads per thread straight from the finished sums instead of 16 KB through LDS and two barriers.  Hl: 256 C + kScal + 8.
// ... in two parts for k_schur_gram<NV, true>: control_early in front of the wait for the riding reductions, this behind it (the same
// loads, the same arithmetic in the same order: same bits)
__device__ __forceinline__ void control_early(const DevProblem &P, const DevState &S, int have_backsub, ControlEarly &e)
{
    control_early_params(P, S, e);
    backsub_partials(S, have_backsub, e.mb, e.ss);
}
__device__ __forceinline__ void control_outcome_late(const DevProblem &P, const DevState &S, int init, const ControlEarly &e, double *Hl, double *sm, CtlOut *out, const CtrlHead *head)
{
    const int t = threadIdx.x;
    ControlPre pre;
    control_state(P, init, pre, head, e);
    const int m = min(t >> 4, P.C - 1), a = t & 15;
    const int fa = min(a, 13), ta = f_tile(fa), tb = f_tile(kFR), mk = f_mask(fa) & f_mask(kFR);
    const double gu = S.campart2[(size_t)512 * m + ta * 16 + tb], gv = S.campart2[(size_t)512 * m + 256 + ta * 16 + tb];
    double *scl = Hl + 256 * P.C;
    reduce_scalar_partials_from<false>(P, S, e.mb, e.ss, pre.c.lin_fail, scl, sm);
    if (t < 16 * P.C && a < 14) Hl[256 * m + a * 16 + kFR] = ((mk & 1) ? gu : 0.0) + ((mk & 2) ? gv : 0.0);
    __syncthreads();
    control_step(P, S, init, pre, sm, Hl, scl, nullptr, /*writer=*/false, out);
}
// THROUGH: the finished sums and the board statistics were handed over inside this launch
template <bool THROUGH = false>
__device__ __forceinline__ void control_outcome(const DevProblem &P, const DevState &S, int init, int have_backsub, double *Hl, double *sm, CtlOut *out, const CtrlHead *head)
{
    const int t = threadIdx.x;
    ControlPre pre;
    control_prefetch(P, S, init, pre, head);
    // thread (camera m, a): H[m][a][kFR] for a < 14 (a = kFR = 13: the cost entry)
    const int m = min(t >> 4, P.C - 1), a = t & 15;
    const int fa = min(a, 13), ta = f_tile(fa), tb = f_tile(kFR), mk = f_mask(fa) & f_mask(kFR);
    const double *pu = &S.campart2[(size_t)512 * m + ta * 16 + tb], *pv = &S.campart2[(size_t)512 * m + 256 + ta * 16 + tb];
    const double gu = THROUGH ? handoff_load(pu) : *pu, gv = THROUGH ? handoff_load(pv) : *pv;
    double *scl = Hl + 256 * P.C;
    reduce_scalar_partials<THROUGH>(P, S, have_backsub, pre.c.lin_fail, scl, sm);
    if (t < 16 * P.C && a < 14) Hl[256 * m + a * 16 + kFR] = ((mk & 1) ? gu : 0.0) + ((mk & 2) ? gv : 0.0);
    __syncthreads();
    control_step(P, S, init, pre, sm, Hl, scl, nullptr, /*writer=*/false, out);
}

// One GPU: everything between the evaluation and the next Schur complement in ONE launch (round 3; before:
// k_reduce_stats, k_finalize_eval with a second reduction level, the control step in its last workgroup -- 6.6 + 16.4 us
// of an iteration of 131, every dependent load of these small kernels a cold round trip of 1-2 us).  The workgroups
// are k_reduce_stats' (camera-tile slices, board statistics); whichever arrives last (release -> counter -> acquire at
// agent scope, cdna guide G16) requests in ONE batch what is left -- the 512 finished sums per camera, the scalar
// partials, the LM state, the target point's camera parameters -- forms H_stage and runs the control step.
__global__ __launch_bounds__(256) void k_reduce_control(DevProblem P, DevState S, int cand, int init, int have_backsub)
{
    KTL(1);
    if (S.ctrl->done) return;
    __shared__ double sm[256];
    __shared__ int s_last;
    __shared__ double Hl[256 * kMaxCamLds + kScal + 8];
    __shared__ double Gall[512 * kMaxCamLds];
    const int t = threadIdx.x;
    const int nc = P.C * kCamSl;
    if ((int)blockIdx.x < nc) cam_reduce_block(P, S, blockIdx.x, sm);
    else board_stats_block(P, S, cand, init, blockIdx.x - nc, sm);
    // hand-off without an L2 write-back (handoff_store): the written-through results are complete, then the count
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        const int old = __hip_atomic_fetch_add(&S.ctrl->fin_count, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (old == (int)gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    KTLX(0, true);
    if (t == 0) __hip_atomic_store(&S.ctrl->fin_count, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // (buffer_inv: whatever else this workgroup reads from now on is current)
    __syncthreads();
    KTLX(1, true);
    finish_evaluation<true>(P, S, init, have_backsub, /*writer=*/true, Hl, Gall, sm, nullptr, S.ctrl);
    KTLX(8, true);
    KTLX_FLUSH();
}
