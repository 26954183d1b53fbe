// tscm_eval_gram4.h -- the dominant kernel with the Gram contraction on v_mfma_f64_4x4x4_4b_f64 (round 3).
//
// Same inputs, same outputs, same bits as k_eval_gram<58> (tscm_eval_gram16.h); what changes is the matrix instruction.
// Measured on gfx950 (tools/ubench_mfma64.hip, four waves per SIMD): v_mfma_f64_16x16x4_f64 occupies the fp64 pipe for
// ~90 clocks (2048 flop: 23 flop/clock/SIMD -- the 49 TFLOP/s ceiling bench.py reports), v_mfma_f64_4x4x4_4b_f64 for
// ~12.5 clocks (4 blocks of 4x4x4 = 512 flop: 41 flop/clock/SIMD), and the 16x16 tile computes every off-diagonal
// block of the symmetric Gram twice.  With the 16 tile columns in four groups of four, the ten block pairs (I <= J)
// fit THREE 4x4x4 instructions per four rows (twelve block slots): 37.5 clocks instead of 90.
//
// Operand layout of the instruction (tools/probe_mfma4x4.hip): lane l: k = l / 16, block = (l % 16) / 4, A_b[i][k] with
// i = l % 4, B_b[k][j] with j = l % 4; result D_b[i][j] in lane 16 i + 4 b + j.  So lane (c = l % 16, k = l / 16)
// supplies element (tile column c, row 4 t + k) as A operand -- the vector N the 16x16 kernel reads -- block b of the
// result holds rows of column group b, and the B operand decides which column group they meet:
//   q0  B = N                         pairs (0,0) (1,1) (2,2) (3,3)
//   q1  B = N rotated by one group     pairs (0,1) (1,2) (2,3) (3,0)
//   q2  B = groups [2, 3, 1, 1]        pairs (0,2) (1,3) (2,1) (3,1)
// i.e. all ten unordered pairs, and every pair (b, 1) with the column group of the t_c columns as the COLUMN group:
// there the three t_c entries of a tile column sit in the three adjacent lanes of a quad, and the t_b rows
// (J_tb = J_tc R_c) are three quad-broadcast DPP moves and three FMAs per register -- no LDS crossbar, no cross-row move.
// Entries of the 4x4x4 result are bit-identical to those of the 16x16x4 tile (tools/check_mfma4x4.hip), the epilogue
// performs the same operations in the same order, and the camera tile is handed on in the 16x16 layout and column
// numbering of k_eval_gram: the whole solve is bit-identical (tools/regress_bits.py).
//
// Tile columns here (groups of four):  0-2 w_b, 3 r | 4-6 t_c, 7 alpha | 8-10 w_c, 11 f* | 12 one*, 13 xi, 14 lambda, 15 zero.
// A chunk of a camera whose pose block is constant, in a solve's launch (the constant-pose path, CP below):
//                                       0-2 w_b, 3 r | 4-6 t_c, 7 alpha | 8-11 never written: zero | 12 one*, 13 xi, 14 lambda, 15 f*
// -- three groups, six pairs, TWO instructions per four rows, no w_c block in the geometry (g4_live, kG4FCp).
// LDS tile: element (k-step t, column c, row k) at double t * 68 + 4 c + (k ^ 2 (c >> 3)):
//   * the three operand vectors are conflict-free ds_read_b64 (32-lane groups, banks mod 64: columns c and c + 8 would
//     share a bank pair, the xor puts them on complementary halves);
//   * a corner's lane writes row (t, k) = (lane / 4, lane % 4) of a column: 16 lanes x 8 bytes on 32 distinct banks
//     (k-step stride 68 doubles = 8 dwords mod 32).
//
// Every board size (round 6; rounds 3-5: boards of 49..56 corners only, everything else ran k_eval_gram<0>).  A pass holds
// 4 KS <= 56 rows, KS a template parameter, so a board of n <= 56 corners issues exactly ceil(n / 4) k-steps (6 x 5: 8, not
// 14 zero-padded ones); larger boards -- the reference's own 11 x 8 (main.cpp:190-191) -- take ceil(n / 56) BALANCED passes
// per view (88 = 2 x 44 -> KS = 11), the accumulators carried across the passes, one epilogue per view (MULTI).  The
// corners of a pass are a multiple of four, so the k-steps of a view contract the same groups of four rows in the same
// order as k_eval_gram<0>'s 64-row passes do: same bits.
#pragma once
// (included from tscm_kernels.h inside namespace tscm)

constexpr int kG4Stride = 68;                   // doubles per k-step of the tile
// (kG4MaxKS, g4_plan: tscm_exec_plan.h, next to plan_gram: the fp32-Jacobian tier's kernel runs on the same pass plan)
// doubles of LDS per wave: the tile (>= the 512-double camera-tile exchange), then the board points
__host__ __device__ constexpr int g4_tile_doubles(int ks) { return ks * kG4Stride > 512 ? ks * kG4Stride : 512; }
__host__ __device__ inline int eval_gram4_lds_doubles(int n_points, int ks) { return g4_tile_doubles(ks) + 2 * n_points; }

// tile columns of this kernel
constexpr int kG4Wb = 0, kG4R = 3, kG4Tc = 4, kG4Al = 7, kG4Wc = 8, kG4F = 11, kG4One = 12, kG4Xi = 13, kG4Lam = 14;
// ... -> tile column of k_eval_gram (the camera tile is handed on in that numbering)
__device__ __forceinline__ constexpr int g4_old_col(int c)
{
    return c < 3 ? kTcWb + c : c == 3 ? kTcR : c < 7 ? tc_tc(c - 4) : c == 7 ? kTcAl : c < 11 ? kTcWc + (c - 8) : c == 11 ? kTcF
         : c == 12 ? kTcOne : c == 13 ? kTcXi : c == 14 ? kTcLam : 15;
}
// ... -> W column (F index) of the record; f* / one* are the first of a (u-part, v-part) pair; -1: none (w_b, zero)
__device__ __forceinline__ constexpr int g4_wcol(int c)
{
    return c < 3 ? -1 : c == 3 ? kFR : c < 7 ? kWcolTc + (c - 4) : c == 7 ? 12 : c < 11 ? c - 8 : c == 11 ? 6 : c == 12 ? 8 : c == 13 ? 10 : c == 14 ? 11 : -1;
}
// column group block b of the result meets in instruction q
__device__ __forceinline__ constexpr int g4_cgroup(int b, int q) { return q == 0 ? b : q == 1 ? ((b + 1) & 3) : (b == 0 ? 2 : b == 1 ? 3 : 1); }
__device__ __forceinline__ int g4_elem(int c, int k) { return 4 * c + (k ^ ((c >> 3) << 1)); }     // within a k-step

// The constant-pose path (CP): a chunk is one camera, and a camera whose pose block is held constant has no pose column in
// the reduced system (plan_columns), so a solve's launch (ExecPlan::skip_const_pose) takes such a chunk's waves down a
// path without the w_c columns.  Same tile addresses; f* moves from column 11 into the zero column 15, columns 8-11 are
// never written and stay zero.  Three groups are left -- 0 (w_b, r), 1 (t_c, alpha), 3' (one*, xi, lambda, f*) -- and their
// six pairs fit TWO instructions per four rows.  A = N in blocks 0, 1, 3; the lanes of the idle block 2 read group 3':
//   q0  B = N in blocks 0, 1, 3, group 0 in block 2       pairs (0,0) (1,1) (3',0) (3',3')
//   q1  B = group 1 (t_c) in every block                   pairs (0,1) (1,1) (3',1) (3',1)
// Every pair that meets the t_c group has it as the column group, as on the full path, and block 2 of q0 holds what block
// 3 of the full path's q1 holds (rows one*, xi, lambda x columns w_b) plus the f* row of its q2 block 0, transposed: the
// same products summed in the same order, the same bits.
constexpr int kG4FCp = 15;                      // tile column of f* on the constant-pose path
// (kChunkConstPose, kChunkCamMask, kEvalCand, kEvalSkipConst: tscm_dev.h)
template <bool CP> __device__ __forceinline__ constexpr bool g4_live(int c) { return CP ? (c < 8 || c >= 12) : c < kTcols; }   // columns a corner writes
template <bool CP> __device__ __forceinline__ constexpr int g4_old_col_of(int c) { return CP && c == kG4FCp ? kTcF : g4_old_col(c); }
// W column of member i of group 3' (one*, xi, lambda, f*); one* and f* are the first of a (u-part, v-part) pair
__device__ __forceinline__ constexpr int g4_wcol_cp(int i) { return i == 0 ? 8 : i == 1 ? 10 : i == 2 ? 11 : 6; }

// one k-step: three operand vectors, three instructions (NQ = 2, the constant-pose path: n is A of both, r and b their B);
// operands requested D k-steps ahead
template <int KS, int D, bool ACC, int NQ, int T = 0>
__device__ __forceinline__ void gram4_steps(unsigned aN, unsigned aR, unsigned aB, double (&n)[KS], double (&r)[KS], double (&b)[KS], double (&acc)[NQ])
{
    if constexpr (T < KS) {
        if constexpr (T + D < KS) {
            n[T + D] = ds_read_f64<8 * kG4Stride * (T + D)>(aN);
            r[T + D] = ds_read_f64<8 * kG4Stride * (T + D)>(aR);
            b[T + D] = ds_read_f64<8 * kG4Stride * (T + D)>(aB);
        }
        constexpr int newer = 3 * (KS - 1 - T < D ? KS - 1 - T : D);      // requests younger than this k-step's three
        lgkm_wait<newer + 2>(n[T]);
        if constexpr (NQ == 3) {
            if constexpr (T == 0 && !ACC) acc[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(n[T], n[T], 0.0, 0, 0, 0);
            else acc[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(n[T], n[T], acc[0], 0, 0, 0);
        }
        lgkm_wait<newer + 1>(r[T]);
        if constexpr (T == 0 && !ACC) acc[NQ - 2] = __builtin_amdgcn_mfma_f64_4x4x4f64(n[T], r[T], 0.0, 0, 0, 0);
        else acc[NQ - 2] = __builtin_amdgcn_mfma_f64_4x4x4f64(n[T], r[T], acc[NQ - 2], 0, 0, 0);
        lgkm_wait<newer>(b[T]);
        if constexpr (T == 0 && !ACC) acc[NQ - 1] = __builtin_amdgcn_mfma_f64_4x4x4f64(n[T], b[T], 0.0, 0, 0, 0);
        else acc[NQ - 1] = __builtin_amdgcn_mfma_f64_4x4x4f64(n[T], b[T], acc[NQ - 1], 0, 0, 0);
        gram4_steps<KS, D, ACC, NQ, T + 1>(aN, aR, aB, n, r, b, acc);
    }
}
template <int KS, int D, int T = 0>
__device__ __forceinline__ void gram4_prime(unsigned aN, unsigned aR, unsigned aB, double (&n)[KS], double (&r)[KS], double (&b)[KS])
{
    if constexpr (T < D && T < KS) {
        n[T] = ds_read_f64<8 * kG4Stride * T>(aN);
        r[T] = ds_read_f64<8 * kG4Stride * T>(aR);
        b[T] = ds_read_f64<8 * kG4Stride * T>(aB);
        gram4_prime<KS, D, T + 1>(aN, aR, aB, n, r, b);
    }
}
// ACC: the accumulators carry the earlier passes of the view (otherwise the first k-step starts from C = 0)
template <int KS, bool ACC, int NQ>
__device__ __forceinline__ void gram4_full(unsigned aN, unsigned aR, unsigned aB, double (&acc)[NQ])
{
    constexpr int D = KS < 2 ? KS : 2;      // (round 5: 1, 2, 3 and 4 k-steps ahead measure the same to 0.1 us -- the MFMA phases do not wait for the LDS)
    double n[KS], r[KS], b[KS];
    gram4_prime<KS, D>(aN, aR, aB, n, r, b);
    gram4_steps<KS, D, ACC, NQ>(aN, aR, aB, n, r, b, acc);
}

// t_b entry of this lane's quad: lanes j = 0, 1, 2 of a quad hold the t_c0, t_c1, t_c2 entries of one tile column; lane
// j = l gets R_c[0][l] x0 + R_c[1][l] x1 + R_c[2][l] x2 in the operation order of store_view_record (c_m = R_c[m][l])
__device__ __forceinline__ double quad_tb(double x, double c0, double c1, double c2)
{
    const double x0 = dpp_f64<0x00>(x), x1 = dpp_f64<0x55>(x), x2 = dpp_f64<0xAA>(x);
    return fma(c2, x2, fma(c0, x0, c1 * x1));
}

// `take` in the lanes of the DPP rows ROW (bit i: lanes 16 i .. 16 i + 15) and banks BANK (bit b: lanes 4 b .. 4 b + 3 of a row),
// `keep` in the others: two masked identity moves
template <int ROW, int BANK>
__device__ __forceinline__ double lane_pick(double keep, double take)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(keep), __double2loint(take), 0xE4, ROW, BANK, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(keep), __double2hiint(take), 0xE4, ROW, BANK, false);
    return __hiloint2double(hi, lo);
}

// KS: k-steps of a pass (4 KS rows >= the corners of a pass); MULTI: boards of more than 56 corners, P.g4_per corners per pass;
// ROBUST: a loss L (robust_rho): every entry a corner puts into the tile, r column included, is scaled by w = sqrt(rho'), and
// the cost entry of the camera tile is the lanes' fp64 sum of rho instead of the contraction r^T r.  L is not read
// by the ROBUST = false instantiations, which compile to the code they had before the switch existed.
// WEIGHTED (with ROBUST): corner weights P.obs_w -- the weight is fetched like the observation it belongs to (pf_w
// beside pf_u / pf_v, through a buffer resource: a lane past the end reads 0) and enters robust_rho<true>, which also takes
// kind kLossNone; rho_sum is then sum(omega rho).  The other instantiations compile to the code they had before.
// CP: the constant-pose path (above).  The kernel below takes the first trip of the head -- cd: the chunk's descriptor,
// ctrl_done, ctrl_cur: the control block, my_xy: the lane's board point -- and then one wave-uniform branch into the
// instantiation of its chunk; cand: 0 or 1.
template <int KS, bool MULTI, bool ROBUST, bool CP, bool WEIGHTED = false>
__device__ __forceinline__ void eval_gram4_wave(const DevProblem &P, const DevState &S, const int cand, const LossArg &L, const v4i cd,
                                                const int ctrl_done, const int ctrl_cur, const d2 my_xy)
{
    static_assert(KS >= 1 && KS <= kG4MaxKS, "a pass holds at most 56 rows");
    static_assert(ROBUST || !WEIGHTED, "the weight enters where the loss does");
    constexpr int kTile = g4_tile_doubles(KS);
    constexpr int NQ = CP ? 2 : 3;              // instructions per four rows
#ifdef TSCM_WAVE_TIMELINE
    const long long tl_t0 = wall_clock64();
    const int tl_iter = S.ctrl->iteration;
    long long tl_ph[5] = { 0, 0, 0, 0, 0 };      // shader clocks per phase, summed over the chunk: geometry, MFMA u, copy, MFMA v, epilogue
    // wall-clock stamps (10 ns) of this wave: [0] view loop reached, [1] first MFMA, [2] the wave's very end (camera tile handed
    // on; written at the end of the kernel), [3] last record stored, [4 + i] start of view i (i < kTlViews)
    long long tl_w[4] = { 0, 0, 0, 0 };
    int tl_nv = 0;
#define TL_STAMP(var) const long long var = (long long)__builtin_readcyclecounter()
#define TL_ADD(k, a, b) tl_ph[k] += (b) - (a)
#else
#define TL_STAMP(var)
#define TL_ADD(k, a, b)
#endif
    extern __shared__ __attribute__((aligned(16))) double lds_all[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lds_wave = eval_gram4_lds_doubles(P.n_points, KS);
    double *lds = lds_all + (size_t)wave * lds_wave;
    double *Fl = lds;                          // the tile: holds the u-rows, then the v-rows
    double *bxy = lds + kTile;
    const int lane = threadIdx.x & 63;
#ifdef TSCM_WAVE_TIMELINE
    const int chunk = blockIdx.x * 4 + wave;
#endif
    // Head in TWO dependent round trips (round 5; it was six: control block | board points, twice | view range | camera
    // constants | view metadata | observations -- 7 us from a wave's start to its first MFMA, with every wave of the chip in
    // the same place at the same time).  Trip 1, scalar: the control block and the chunk's 16-byte descriptor; vector: the
    // lane's board point.  Trip 2, everything that hangs on the descriptor at once: R_c, the metadata of the chunk's first
    // 64 views, the first view's observations (all 64 lanes: a lane without a corner reads the next view's value or, past
    // the end, zero -- the offset is in the vector operand, which the range check covers -- and never uses it), and one dword of every 64-byte line of the first view's and of the camera's
    // constants through the SCALAR cache, so that the geometry's scalar loads hit there.
    const int cam = cd[0] & kChunkCamMask, vb = cd[1], ve = cd[2];
    double *const cc_buf[2] = { S.cconst[0], S.cconst[1] };
    double *const rec_buf[2] = { S.rec[0], S.rec[1] };
    double camU[NQ] = {}, camV[NQ] = {};
    for (int i = lane; i < KS * kG4Stride; i += 64) Fl[i] = 0.0;     // rows of lanes without a corner, the zero column, the padding
    int prev_nv = 0;
    double pf_u = 0.0, pf_v = 0.0;
    double pf_w = 0.0;                          // WEIGHTED: the weight of the corner of pf_u / pf_v
    int warm = 0;
    double rho_sum = 0.0;                       // ROBUST: this lane's share of sum(rho), fp64
    if (ctrl_done) return;
    const int tgt = cand ? (ctrl_cur ^ 1) : ctrl_cur;
    const __amdgpu_buffer_rsrc_t r_rec = make_rsrc(tgt ? rec_buf[1] : rec_buf[0], sizeof(double) * (size_t)kRec * P.V);
    const cptr4 ccs = (cptr4)((tgt ? cc_buf[1] : cc_buf[0]) + kCStride * cam);
    auto CC = [&](int k) { return ccs[k]; };
    const __amdgpu_buffer_rsrc_t r_vc = make_rsrc(S.vconst, sizeof(double) * (size_t)kVStride * P.V);
    const __amdgpu_buffer_rsrc_t r_u = make_rsrc(P.obs_u, sizeof(double) * (size_t)P.N), r_v = make_rsrc(P.obs_v, sizeof(double) * (size_t)P.N);
    const __amdgpu_buffer_rsrc_t r_w = WEIGHTED ? make_rsrc(P.obs_w, sizeof(double) * (size_t)P.N) : r_u;
    int off_next = cd[3];
    int m_cnt0 = 0, m_slot0 = 0;
    if (vb + lane < min(ve, vb + 64)) { m_cnt0 = P.view_count[vb + lane]; m_slot0 = P.view_slot[vb + lane]; }
    if (vb < ve) { pf_u = buf_load_f64(r_u, 8u * ((unsigned)off_next + lane), 0); pf_v = buf_load_f64(r_v, 8u * ((unsigned)off_next + lane), 0); }
    if constexpr (WEIGHTED) { if (vb < ve) pf_w = buf_load_f64(r_w, 8u * ((unsigned)off_next + lane), 0); }
    // the scalar cache's lines of the first view's 27 constants (4 lines) and of the camera's 48 (6 lines); retired in front of the loop
    typedef const int __attribute__((address_space(4))) *cptr4i;
    const cptr4i vc0 = (cptr4i)(S.vconst + (size_t)kVStride * min(vb, P.V - 1)), cc0 = (cptr4i)ccs;
    // (as dwords on purpose: the same words loaded as doubles are merged with the geometry's own loads of them, which moves
    // contraction decisions in the geometry and with them the last bits of 8 of the 13 fingerprints of tools/regress_bits.py)
    const int kw0 = vc0[0], kw1 = vc0[16], kw2 = vc0[32], kw3 = vc0[48], kw4 = cc0[16], kw5 = cc0[32], kw6 = cc0[48], kw7 = cc0[64], kw8 = cc0[80];
    // ---- lane roles ------------------------------------------------------------------------------------------------
    // as a corner: row (t, k) of the tile
    double *fu_lo = Fl + (lane >> 2) * kG4Stride + (lane & 3), *fu_hi = Fl + (lane >> 2) * kG4Stride + ((lane & 3) ^ 2);
    // as an MFMA lane: k = i = lane / 16, c16 = 4 b + j
    const int li = lane >> 4, c16 = lane & 15, lb = c16 >> 2, lj = c16 & 3;
    const unsigned lds0 = lds_addr(Fl);
    // (CP: aN the A operand of both instructions, aR and aB their B operands)
    const unsigned aN = lds0 + 8u * (unsigned)g4_elem(CP && lb == 2 ? 12 + lj : c16, li);
    const unsigned aR = lds0 + 8u * (unsigned)g4_elem(CP ? (lb == 2 ? lj : c16) : (c16 + 4) & 15, li);
    const unsigned aB = lds0 + 8u * (unsigned)g4_elem(CP ? 4 + lj : 4 * g4_cgroup(lb, 2) + lj, li);
    // R_c[m][j] of this lane's quad position (t_b rows), fixed for the chunk
    const double rc0 = lj == 0 ? ccs[0] : lj == 1 ? ccs[1] : ccs[2];
    const double rc1 = lj == 0 ? ccs[3] : lj == 1 ? ccs[4] : ccs[5];
    const double rc2 = lj == 0 ? ccs[6] : lj == 1 ? ccs[7] : ccs[8];
    // record offsets of this lane's entries in the seven stores of a view (bytes inside the view's W / E record; lanes
    // without an entry store past the end of the buffer).  Columns by group: see g4_wcol.
    constexpr unsigned BAD = 0xffffe000u;
    unsigned o1e = BAD, o1w = BAD, o2 = BAD, o3e = BAD, o4 = BAD, o5 = BAD, o6 = BAD, o7a = BAD, o7b = BAD;
    {
        const int b = lb, j = lj, i = li;
        auto W = [](int wcol, int row) { return 8u * (unsigned)(6 * wcol + row); };
        const int f1 = g4_wcol(4 + i), f1j = g4_wcol(4 + j), f2 = g4_wcol(8 + i), f2j = g4_wcol(8 + j), f3 = g4_wcol(12 + i);
        if (b == 0 && j < 3 && i < 3) { o1e = 8u * (unsigned)(6 * j + i); o3e = 8u * (unsigned)(6 * i + 3 + j); }
        if (b == 0 && j == 3 && i < 3) { o1w = W(kFR, i); o7a = 8u * (unsigned)i; }                 // w_b rows x r (and once more in the G region)
        if (b == 1 && j < 3) o1w = W(f1, 3 + j);                             // t_b rows x (t_c | alpha)
        if (b == 0 && i < 3) o2 = W(f1j, i);                                 // w_b rows x (t_c | alpha)
        if (b == 0 && i == 3 && j < 3) { o2 = W(kFR, 3 + j); o7b = 8u * (unsigned)(3 + j); }       // t_b rows x r (G region)
        if constexpr (CP) {
            // seven stores (o5, o6 unused): o2 also takes the rows of group 3' -- block 2 x w_b (held transposed), block 3 x t_b --,
            // the u-part where the row is one* or f*, and o4 their v-part in the next record column (cy, fy)
            const int f3c = g4_wcol_cp(i);
            if (b == 2 && j < 3) o2 = W(f3c, j);
            if (b == 3 && j < 3) o2 = W(f3c, 3 + j);
            if (b == 2 && j < 3 && (i == 0 || i == 3)) o4 = W(f3c + 1, j);
            if (b == 3 && j < 3 && (i == 0 || i == 3)) o4 = W(f3c + 1, 3 + j);
        } else {
        if (b == 3 && j < 3 && i < 3) o2 = W(f3, j);                         // w_b rows x (one* | xi | lambda), held transposed
        if (b == 0 && i < 3) o4 = W(f2j, i);                                 // w_b rows x (w_c | f*)
        if (b == 2 && j < 3) o4 = W(f2, 3 + j);                              // t_b rows x (w_c | f*)
        if (b == 3 && j < 3 && i < 3) o4 = W(f3, 3 + j);                     // t_b rows x (one* | xi | lambda)
        if (b == 3 && i == 0 && j < 3) { o5 = W(9, j); o6 = W(9, 3 + j); }   // v-row parts: cy
        if (b == 0 && j == 3 && i < 3) o6 = W(7, i);                         // ... fy
        if (b == 2 && i == 3 && j < 3) o6 = W(7, 3 + j);
        }
    }
    // (the E and G regions' start goes into the lane's own offset, once: two scalar registers and two additions per view less)
    {
        const unsigned baseE = 8u * (unsigned)kRecW * (unsigned)P.V, baseG = 8u * (unsigned)(kRecW + kRecE) * (unsigned)P.V;
        if (o1e != BAD) { o1e += baseE; o3e += baseE; }
        if (o7a != BAD) o7a += baseG;
        if (o7b != BAD) o7b += baseG;
    }
    if (lane < P.n_points) *reinterpret_cast<d2 *>(bxy + 2 * lane) = my_xy;
    if constexpr (MULTI) {
        for (int j = lane + 64; j < P.n_points; j += 64) *reinterpret_cast<d2 *>(bxy + 2 * j) = *reinterpret_cast<const d2 *>(P.board_xy + 2 * j);
    }
    const int per = MULTI ? P.g4_per : 4 * KS;          // corners of a pass
    asm volatile("" :: "s"(kw0), "s"(kw1), "s"(kw2), "s"(kw3), "s"(kw4), "s"(kw5), "s"(kw6), "s"(kw7), "s"(kw8));
#ifdef TSCM_WAVE_TIMELINE
    tl_w[0] = wall_clock64();
    const bool tl_on = lane == 0 && tl_iter == 5 && cand && chunk < kTimelineWaves;
#endif
    const int prio_n = max(1, ve - vb);
    int prio_q = 0, prio_rem = 0;
    for (int vbase = vb; vbase < ve; vbase += 64) {
    const int vend = min(ve, vbase + 64);
    int m_cnt = 0, m_slot = 0;
    if (vbase == vb) { m_cnt = m_cnt0; m_slot = m_slot0; }
    else {
        if (vbase + lane < vend) { m_cnt = P.view_count[vbase + lane]; m_slot = P.view_slot[vbase + lane]; }
        pf_u = buf_load_f64(r_u, 8u * ((unsigned)off_next + lane), 0); pf_v = buf_load_f64(r_v, 8u * ((unsigned)off_next + lane), 0);
        if constexpr (WEIGHTED) pf_w = buf_load_f64(r_w, 8u * ((unsigned)off_next + lane), 0);
    }
    asm volatile("" : "+v"(m_cnt), "+v"(m_slot));
    for (int view = vbase; view < vend; ++view) {
        const int cnt = __builtin_amdgcn_readlane(m_cnt, view - vbase);
        const int off = off_next;               // (MULTI: the later passes' observations)
        off_next += cnt;
        wave_lds_fence();                       // the previous view's MFMA phase has finished with the tile
        // priority by progress: see k_eval_gram.  Short chunks (round 5): the last three views step down 3 | 2 | 1 (geometry), 0 (the
        // rest of the last view), so that the four waves of a SIMD -- served oldest first among equals -- enter the last
        // equal-priority stretch half a view apart, not a view and a quarter: -0.4 us at 10 views per wave; at 40 the stretch is a
        // twentieth of the chunk either way and the wrap of the levels in front of it costs more than it brings (+1.6 us)
        const int left = ve - 1 - view;
        const bool tail_steps = left <= 2 && ve - vb <= 16;
        set_prio(tail_steps ? left + 1 : 3 - (prio_q & 3));
        // eighths of the chunk behind this view, prio_q = floor(8 (view - vb) / prio_n), counted up instead of divided out per view
        // (the empty asm keeps the compiler from turning the count back into a division)
        for (prio_rem += 8; prio_rem >= prio_n; prio_rem -= prio_n) { ++prio_q; asm volatile("" : "+s"(prio_q)); }
#ifdef TSCM_WAVE_TIMELINE
        if (tl_on && tl_nv < kTlViews) g_tlv[(size_t)(4 + kTlViews) * chunk + 4 + tl_nv] = wall_clock64();
        ++tl_nv;
#endif
        const cptr4 vcs = (cptr4)(S.vconst + (size_t)kVStride * view);
        auto VC = [&](int k) { return vcs[k]; };
        double accU[NQ] = {}, accV[NQ] = {};
        int pbv = 0;                            // first corner of the pass (MULTI)
        do {
        const int pb = MULTI ? pbv : 0;
        TL_STAMP(ts0);
        if constexpr (MULTI) { if (pb) wave_lds_fence(); }      // ... and so has the previous pass's
        const int nv = MULTI ? min(per, cnt - pb) : cnt;         // corners of this pass
        const bool valid = lane < nv;
        double fv[16];                          // v-rows wait in registers until the u-rows have been consumed (index = tile column)
        auto PUT = [&](int c, double u, double v) { (c < 8 ? fu_lo : fu_hi)[4 * c] = u; fv[c] = v; };
        if (valid) {
            const double x = bxy[2 * (pb + lane)], y = bxy[2 * (pb + lane) + 1];
            // semantic column -> tile column of this kernel
            constexpr int tcol[15] = { kG4Wb, kG4Wb + 1, kG4Wb + 2, kG4Tc, kG4Tc + 1, kG4Tc + 2, kG4Wc, kG4Wc + 1, kG4Wc + 2,
                                       CP ? kG4FCp : kG4F, kG4One, kG4Xi, kG4Lam, kG4Al, kG4R };
            if constexpr (ROBUST) {
                // the corner's weight from its residual first (corner_residual: the same operations corner_geometry starts
                // with, merged with them by the compiler), then every entry scaled as it is handed out
                double ru, rv, rho, w;
                corner_residual(x, y, pf_u, pf_v, VC, CC, ru, rv);
                robust_rho<WEIGHTED>(L, ru * ru + rv * rv, rho, w, pf_w);
                rho_sum += rho;
                corner_geometry<!CP, WEIGHTED>(x, y, pf_u, pf_v, VC, CC, [&](int gc, double u, double v) { PUT(tcol[gc], w * u, w * v); });
            } else {
                corner_geometry<!CP>(x, y, pf_u, pf_v, VC, CC, [&](int gc, double u, double v) { PUT(tcol[gc], u, v); });
            }
        }
        // rows of lanes that lost their corner: only behind a view (pass) that had more corners -- with the same count from view to
        // view, the usual chunk, the wave skips this on a scalar compare
        if (nv < prev_nv) {
            if (!valid && lane < prev_nv) {
#pragma unroll
                for (int c = 0; c < 16; ++c) if (g4_live<CP>(c)) (c < 8 ? fu_lo : fu_hi)[4 * c] = 0.0;
            }
        }
        {
            // prefetch of the next view (see k_eval_gram): observations, and the constant record into the L2.  All 64 lanes load: a
            // lane without a corner there reads the value of the view behind it and never uses it (selecting the lanes cost a
            // readlane, a compare and a select per view; the ten idle lanes of a 54-corner view touch the next 80 bytes a view early,
            // and the kernel's measured reads went from 46.9 to 50.9 MB per launch at config 4 with it -- 2.4 us faster all the same).  The whole offset is in the
            // VECTOR operand, the one the descriptor's range check covers: past the end of the array a lane reads zero
            const int vn = min(view + 1, vend - 1);
            if (!MULTI || pb == 0) warm = __builtin_amdgcn_raw_buffer_load_b32(r_vc, lane < 4 ? 64 * lane : (int)0xffffe000u, (int)(8u * (unsigned)kVStride * (unsigned)vn), 0);
            // MULTI: the next pass of this view, or the first pass of the next one
            const bool more = MULTI && pb + per < cnt;
            const unsigned noff = more ? (unsigned)(off + pb + per) : (unsigned)off_next;
            pf_u = buf_load_f64(r_u, 8u * (noff + lane), 0);
            pf_v = buf_load_f64(r_v, 8u * (noff + lane), 0);
            if constexpr (WEIGHTED) pf_w = buf_load_f64(r_w, 8u * (noff + lane), 0);
        }
        prev_nv = MULTI ? min(per, max(cnt - pb, 0)) : cnt;
        wave_lds_fence();
        if (tail_steps && left == 0) set_prio(0);
        TL_STAMP(ts1);
#ifdef TSCM_WAVE_TIMELINE
        if (tl_nv == 1) tl_w[1] = wall_clock64();
#endif
        gram4_full<KS, MULTI, NQ>(aN, aR, aB, accU);
        wave_lds_fence();
        TL_STAMP(ts2);
        if (valid) {
#pragma unroll
            for (int c = 0; c < 16; ++c) if (g4_live<CP>(c)) (c < 8 ? fu_lo : fu_hi)[4 * c] = fv[c];
        }
        wave_lds_fence();
        TL_STAMP(ts3);
        gram4_full<KS, MULTI, NQ>(aN, aR, aB, accV);
        TL_STAMP(ts4);
        TL_ADD(0, ts0, ts1); TL_ADD(1, ts1, ts2); TL_ADD(2, ts2, ts3); TL_ADD(3, ts3, ts4);
        pbv += per;
        } while (MULTI && pbv < cnt);
        TL_STAMP(ts4e);
        asm volatile("" :: "v"(warm));       // the warming load retires here, before this view's record stores
#pragma unroll
        for (int q = 0; q < NQ; ++q) { camU[q] += accU[q]; camV[q] += accV[q]; }
        // ---- epilogue: the view's record (same values, same operation order as store_view_record) ------------------
        {
            const unsigned slot = (unsigned)__builtin_amdgcn_readlane(m_slot, view - vbase);
            const unsigned offW = 8u * (unsigned)kRecW * slot, offE = 8u * (unsigned)kRecE * slot, offG = 8u * (unsigned)kRecG * slot;
            if constexpr (CP) {
            // The same scheme as below with two tiles.  The t_b rows: block 1 stores those of T0 (o1w), blocks 0 and 3 those of
            // T1; the rows of group 3' are T0 in block 2 (x w_b) and tb(T1) in block 3 (x t_b), and their rows 0 (one*) and 3 (f*)
            // leave as u-part and v-part = total - u-part.  The W columns of w_c and their E^T-side rows are not written: both
            // record buffers are zero from the solver's creation on.
            const double T0 = accU[0] + accV[0], T1 = accU[1] + accV[1];
            const double X = lane_pick<0xF, 0x2>(T1, T0);
            const double tbX = quad_tb(X, rc0, rc1, rc2), tbU1 = quad_tb(accU[1], rc0, rc1, rc2);
            buf_store_f64(r_rec, o1e, offE, T0);
            buf_store_f64(r_rec, o7a, offG, T0);
            // Z: the total, ZU: the u-part of what blocks 2 and 3 store (Z in block 0: its t_b rows)
            const double Z = lane_pick<0xF, 0x9>(T0, tbX), ZU = lane_pick<0xF, 0x8>(accU[0], tbU1);
            buf_store_f64(r_rec, o4, offW, Z - ZU);
            buf_store_f64(r_rec, o1w, offW, lane_pick<0xF, 0x2>(T0, tbX));
            // o2: block 0 rows 0-2 T1, row 3 its t_b rows; blocks 2 and 3 rows 1, 2 the total, rows 0, 3 the u-part
            buf_store_f64(r_rec, o2, offW, lane_pick<0x9, 0xC>(lane_pick<0x7, 0x1>(Z, T1), ZU));
            buf_store_f64(r_rec, o3e, offE, tbX);
            buf_store_f64(r_rec, o7b, offG, tbX);
            } else {
            const double T0 = accU[0] + accV[0], T1 = accU[1] + accV[1], T2 = accU[NQ - 1] + accV[NQ - 1];
            // A lane's block b is its DPP bank and its row i its DPP row: every choice by (b, i) below is a pair of masked moves
            // (lane_pick) -- no compare, no mask in an SGPR pair.  The t_b rows: block 1 stores those of T0 (o1w), block 0 those of
            // T1 (o2, o3e, o7b), blocks 2 and 3 those of T2 (o4, o6), so ONE quad_tb of the block's own T serves all three; the
            // products and FMAs of a stored value are the ones quad_tb(T0 | T1 | T2) performed for it.
            const double X = lane_pick<0xF, 0x1>(lane_pick<0xF, 0x2>(T2, T0), T1);
            const double tbX = quad_tb(X, rc0, rc1, rc2), tbU2 = quad_tb(accU[NQ - 1], rc0, rc1, rc2);
            // (a pick overwrites its `keep` operand: each one below is the last use of that value, so none costs a copy)
            buf_store_f64(r_rec, o1e, offE, T0);
            buf_store_f64(r_rec, o7a, offG, T0);          // E^T r once more, compact (k_reduce_stats reads it there)
            buf_store_f64(r_rec, o1w, offW, lane_pick<0xF, 0x2>(T0, tbX));
            buf_store_f64(r_rec, o5, offW, T1 - accU[1]);
            // o2: T1; row 3 (of block 0: the other blocks store nothing from it) the t_b rows; row 0 of block 3 the u-part
            buf_store_f64(r_rec, o2, offW, lane_pick<0x1, 0x8>(lane_pick<0x8, 0xF>(T1, tbX), accU[1]));
            buf_store_f64(r_rec, o3e, offE, tbX);
            buf_store_f64(r_rec, o7b, offG, tbX);
            const double a4 = lane_pick<0xF, 0xE>(T2, tbX), u4 = lane_pick<0xF, 0x1>(tbU2, accU[NQ - 1]);
            // the lanes that store the u-part through o4 are the lanes with an entry in o6 (which takes the v-part, a4 - u4)
            buf_store_f64(r_rec, o4, offW, (int)o6 >= 0 ? u4 : a4);
            buf_store_f64(r_rec, o6, offW, a4 - u4);
            }
        }
#ifdef TSCM_WAVE_TIMELINE
        { TL_STAMP(ts5); TL_ADD(4, ts4e, ts5); }
        if (view + 1 == ve) tl_w[3] = wall_clock64();
#endif
    }
    }   // block of <= 64 views
#ifdef TSCM_WAVE_TIMELINE
    if (lane == 0 && tl_iter == 5 && cand && chunk < kTimelineWaves) {
        g_timeline[4 * chunk] = (long long)__builtin_amdgcn_s_getreg(63492);
        g_timeline[4 * chunk + 1] = (long long)__builtin_amdgcn_s_getreg(6164);
        g_timeline[4 * chunk + 2] = tl_t0;
        g_timeline[4 * chunk + 3] = wall_clock64();
        for (int k = 0; k < 5; ++k) g_phase[5 * chunk + k] = tl_ph[k];
        for (int k = 0; k < 4; ++k) g_tlv[(size_t)(4 + kTlViews) * chunk + k] = tl_w[k];
    }
#endif
    if constexpr (ROBUST) {
        // the cost entry (r, r) -- tile column 3 with itself: block 0 of q0, lane 16 * 3 + 3 -- is sum(rho), not sum(rho' s)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) rho_sum += __shfl_xor(rho_sum, o);
        if (lane == 16 * kG4R + kG4R) { camU[0] = rho_sum; camV[0] = 0.0; }
    }
    // the camera tile leaves in the 16x16 layout and column numbering of k_eval_gram (both triangles: every entry is
    // written by the lane that holds it and, mirrored, by the same lane; the doubly held pairs carry the same bits)
    wave_lds_fence();
    if constexpr (CP) {
        // ... with zeros in the rows and columns of w_c
        for (int i = lane; i < 512; i += 64) lds[i] = 0.0;
        wave_lds_fence();
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int rg = CP && lb == 2 ? 3 : lb, cg = !CP ? g4_cgroup(lb, q) : q == 1 ? 1 : lb == 2 ? 0 : lb;
        const int r = g4_old_col_of<CP>(4 * rg + li), c = g4_old_col_of<CP>(4 * cg + lj);
        lds[16 * r + c] = camU[q]; lds[16 * c + r] = camU[q];
        lds[256 + 16 * r + c] = camV[q]; lds[256 + 16 * c + r] = camV[q];
    }
    __syncthreads();
    {
        const int t = threadIdx.x;
        const size_t st = lds_wave;
        double *part = S.campart + (size_t)512 * blockIdx.x;
        part[t] = (lds_all[t] + lds_all[st + t]) + (lds_all[2 * st + t] + lds_all[3 * st + t]);
        part[256 + t] = (lds_all[256 + t] + lds_all[st + 256 + t]) + (lds_all[2 * st + 256 + t] + lds_all[3 * st + 256 + t]);
    }
#ifdef TSCM_WAVE_TIMELINE
    if (lane == 0 && tl_iter == 5 && cand && chunk < kTimelineWaves) g_tlv[(size_t)(4 + kTlViews) * chunk + 2] = wall_clock64();     // [2]: the wave's very end (camera tile handed on)
#endif
}

// the kernels below: the first trip of the head, then one wave-uniform branch into the instantiation of the wave's chunk
template <int KS, bool MULTI, bool ROBUST, bool WEIGHTED>
__device__ __forceinline__ void eval_gram4_kernel(const DevProblem &P, const DevState &S, const int cand, const LossArg &L)
{
    KTL(0);
    const int ctrl_done = S.ctrl->done, ctrl_cur = S.ctrl->cur;
    const int chunk = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const v4i cd = *(const v4i __attribute__((address_space(4))) *)(const void *)(P.chunk_desc + chunk);
    const d2 my_xy = *reinterpret_cast<const d2 *>(P.board_xy + 2 * min((int)(threadIdx.x & 63), P.n_points - 1));
    // one camera per chunk and whole workgroups per camera (plan_layout): the branch is uniform in the workgroup
#ifndef TSCM_G4_FULL_PATH
    if ((cand & kEvalSkipConst) && (cd[0] & kChunkConstPose)) eval_gram4_wave<KS, MULTI, ROBUST, true, WEIGHTED>(P, S, cand & kEvalCand, L, cd, ctrl_done, ctrl_cur, my_xy);
    else
#endif
        eval_gram4_wave<KS, MULTI, ROBUST, false, WEIGHTED>(P, S, cand & kEvalCand, L, cd, ctrl_done, ctrl_cur, my_xy);
}

// KS: k-steps of a pass; MULTI, ROBUST: see eval_gram4_wave.  cand: kEvalCand | kEvalSkipConst.
template <int KS, bool MULTI, bool ROBUST = false>
__global__ __launch_bounds__(256, 4) void k_eval_gram4(DevProblem P, DevState S, int cand, LossArg L)
{
    eval_gram4_kernel<KS, MULTI, ROBUST, false>(P, S, cand, L);
}

// ... with corner weights (P.obs_w; L.kind may be kLossNone): the WEIGHTED instantiation
template <int KS, bool MULTI>
__global__ __launch_bounds__(256, 4) void k_eval_gram4_weighted(DevProblem P, DevState S, int cand, LossArg L)
{
    eval_gram4_kernel<KS, MULTI, true, true>(P, S, cand, L);
}
