// tscm_dev.h -- what every stage of an LM iteration shares on the device: the record and tile constants, buffer and lane
// helpers, the problem / state structs the kernels take by value, and the in-launch hand-off loads and stores.
#pragma once
// (included inside namespace tscm: from tscm_kernels.h, and from tscm_mono_batch.hip)

// the view record regions kRecW / kRecE / kRecG and the rig limits kMaxCamLds / kMaxCam / kSmallBids: tscm_layout.h
// the operand map of k_solve_reduced (kMap*, kSolveMapSlots, kMapOne): tscm_columns.h
static_assert(kColFree == kFA && kColGrad == kFR, "tscm_columns.h plans the columns of tscm_math.h's camera tile");
constexpr int kWcolTc = 3;         // W columns of t_c: F index 3, 4, 5 (the gradient column E^T r is F index kFR = 13)
// per-board factor record (doubles)
constexpr int kFac = 56;
constexpr int kFacM = 0;           // [15] L_ik / L_ii, i > k, packed i (i - 1) / 2 + k
constexpr int kFacC = 15;          // [6]  s_i / L_ii
constexpr int kFacL = 21;          // [15] L_ik, same packing (back-substitution)
constexpr int kFacI = 36;          // [6]  1 / L_ii
constexpr int kFacZ = 42;          // [6]  z = L^-1 S_b E^T r
constexpr int kFacD = 48;          // [6]  D^2 (damping of the scaled block)
constexpr int kTcols = 15;         // columns of the single MFMA Gram tile (see k_eval_gram)
// Tile columns (= tile rows): 0-2 w_b | 3 t_c0 | 4-6 w_c | 7 t_c1 | 8 f* | 9 one* | 10 xi | 11 t_c2 | 12 lambda | 13 alpha |
// 14 r | 15 zero.  The accumulator of v_mfma_f64_16x16x4 keeps rows kq + 4 * reg of column col in lane (col, kq): with
// the t_c rows at 3, 7, 11 ONE lane (kq = 3) holds all three of them in registers 0, 1, 2 -- the t_b rows
// (J_tb = J_tc R_c) are nine FMAs with scalar operands there, no cross-lane traffic -- and the w_b rows 0, 1, 2 sit in
// register 0 of the lanes kq = 0, 1, 2.
constexpr int kTcWb = 0, kTcWc = 4, kTcF = 8, kTcOne = 9, kTcXi = 10, kTcLam = 12, kTcAl = 13, kTcR = 14;
__host__ __device__ constexpr int tc_tc(int j) { return 3 + 4 * j; }
// word 0 of a chunk descriptor (DevProblem::chunk_desc): the camera, and whether its pose block is constant
constexpr int kChunkConstPose = 1 << 30, kChunkCamMask = kChunkConstPose - 1;
// bits of the Gram kernels' `cand` argument: the candidate point; k_eval_gram4 only: chunks of a constant-pose camera form no
// w_c columns (ExecPlan::skip_const_pose)
constexpr int kEvalCand = 1, kEvalSkipConst = 2;
constexpr int kVConst = 27;        // per-view constants: R_c r1, R_c r2, R_c t_b + t_c (board point -> camera frame in two FMAs per
                                   // component), then R_c dR_b/dw_k [:,0:2]
constexpr int kCConst = 48;        // per-camera constants: [0,9) R_c, [9,12) t_c, [12,21) a_k (dR_c/dw_k = [a_k]x R_c), [21,24) w if the
                                   // rotation is in the small-angle branch else 0, [24] 1 / 0 for that branch, [39,47) fx fy cx cy xi lambda
                                   // beta 1/(1-alpha)^2   (camera_rotation_constants, tscm_math.h)
constexpr int kCStride = 72;       // doubles per camera record in cconst: 48 doubles, then the same 48 values as floats
constexpr int kCst = 80;           // LDS constant block: [0,27) view, [27,75) camera
constexpr int kScal = 8;           // scalars appended to H_stage
constexpr int kStStride = 16;      // doubles between the board-statistics partials of two workgroups: a 128-byte line each (written by ONE workgroup: see k_schur_gram<NV, true>)

constexpr int kVStride = 48;      // doubles per view record in vconst: 27 doubles (+5 pad), then at byte 256 the same 27 values as
                                  // floats (read by the fp32-Jacobian kernel): 384 bytes
constexpr int kVFloatOff = 32;    // offset of the float copy, in doubles

// LDS hand-off inside ONE wave (64-thread workgroups): DS operations of a wave are serviced in
// issue order, so no s_barrier / vmcnt(0) drain is needed -- only the compiler must keep the
// program order of the LDS accesses.  (__syncthreads() would also drain the global prefetches.)
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Buffer addressing (SGPR descriptor + 32-bit VGPR offset + SGPR offset): the hot kernels keep no 64-bit
// per-lane addresses in registers.  Out-of-range offsets are dropped / read as zero by the hardware.
typedef int v2i __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *p, size_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)(bytes > 0xffffffffull ? 0xffffffffu : (unsigned)bytes), 0x00020000);
}
__device__ __forceinline__ double buf_load_f64(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0));
}
// cache policy of the record stores: 0 (the default policy).  sc1 (16: written through) takes 0.7 us off the Gram kernel and nothing
// off the iteration, and WRITE_SIZE goes from 33.6 to 59.7 MB per launch (partial lines are no longer merged in the L2); nt (2)
// costs the consumers more than it saves the producer: both measured, neither kept
__device__ __forceinline__ void buf_store_f64(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, double v)
{
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i, v), r, (int)voff, (int)soff, 0);
}

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ d2 buf_load_2f64(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    return __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ void buf_store_2f64(__amdgpu_buffer_rsrc_t r, unsigned voff, double a, double b)
{
    const d2 v = { a, b };
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r, (int)voff, 0, 0);
}

// Wave priority of the Gram kernels (the rule: see k_eval_gram; s_setprio takes an immediate, p is wave-uniform)
__device__ __forceinline__ void set_prio(int p)
{
    switch (p & 3) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
    }
}

// record regions (V = views of this rank)
__device__ __forceinline__ const double *rec_w(const double *rec, int slot) { return rec + (size_t)kRecW * slot; }
__device__ __forceinline__ const double *rec_e(const double *rec, int V, int slot) { return rec + (size_t)kRecW * V + (size_t)kRecE * slot; }
__device__ __forceinline__ const double *rec_g(const double *rec, int V, int slot) { return rec + (size_t)(kRecW + kRecE) * V + (size_t)kRecG * slot; }

struct Ctrl : CtrlHead {
    IterLog log[kMaxLog];
};

// the problem on the device: the tables of tscm_layout.h's Layout (plan_layout), uploaded by tscm_solver_create_sharded
struct DevProblem {
    int C, B, n_points, V, N, n_pad;
    int n_chunks, n_pchunks, n_bids;
    int rp, half;                      // LDS pitch (doubles) and rows of the Jacobian tile
    int lds_wave;                      // doubles of LDS per wave of k_eval_gram
    const double *board_xy;
    const int *view_cam, *view_board, *view_obs, *view_count;
    const double *obs_u, *obs_v;
    const double *obs_w;               // [N] corner weights in the order of obs_u / obs_v, NULL = none (tscm_solver_set_corner_weights);
                                       // read by the weighted Gram instantiations and k_reproj_error<true> only
    const int *chunk_vb, *chunk_ve, *chunk_cam, *cam_chunk_ptr;
    const int4 *chunk_desc;            // per chunk of the Gram kernels: camera, first view, end view, observation offset of the first view
    const int *bv_ptr;                 // board -> range of view SLOTS (records are stored board-major)
    const int *view_slot, *slot_cam;   // device view -> slot ; slot -> camera
    const int *slot_view, *slot_board; // slot -> device view ; slot -> board
    const int *slow_boards;            // boards seen by more than three cameras (factored by k_schur_factor, Gram by k_pair_gram)
    int n_slow;
    const int *pair_i, *pair_j;
    const int *pc_begin, *pc_end, *pc_tile;
    const int *bid_part_ptr;                   // per camera-pair block: contiguous range of its partial tiles in pairpart
    const int *pair_board;                     // board of each fallback view pair
    const int *bc_tile;                        // board chunks: tile ids [chunk*6 + t]
    const int4 *bc_desc;                       // ... and per chunk one 16-byte record: first board, end board, first slot, views per board
                                               // (device boards are numbered in signature order: a chunk's boards AND slots are contiguous)
    int n_bchunks, n_tiles;
    const unsigned char *col_ctl;      // [kMaxCam * 16] per padded camera-side parameter, for the control step: bit 0 = it counts in |x| (its
                                       // block is part of the program), bit 1 = it is a tangent coordinate (has a gradient); 0 past n_pad
    const unsigned char *board_const;  // [B] device board: pose block held constant (tscm_problem.board_pose_constant)
    const unsigned char *col_active;   // [n_pad] 1 = column is a free camera-side parameter
    const int *act_map;                // [n_pad] compact index -> padded column (first n_act entries)
    int n_act;
    // the compact numbering of the free camera-side columns from kernel arguments for k_solve_reduced (<= kMaxCamLds cameras): the
    // free columns of camera q are compact [cam_pre[q], cam_pre[q + 1]) = padded 16 q + the set bits of cam_free[q] in ascending
    // order (cam_pre[q] = n_act from q = C on).  Without held intrinsics the set bits are contiguous; with them the
    // block of a camera has holes
    int cam_pre[9];
    unsigned short cam_free[8];
    unsigned long long pair_mask;      // bit mi * 8 + mj: the camera pair shares a board (its tile of T follows by a population count)
    const int4 *solve_map;             // [kSolveMapSlots / 4][256] operand offsets of every thread of k_solve_reduced (plan_solve_map)
    const int4 *solve_ext;             // [256] { kind, ri, cj, i }: the e-row and solution tiles of k_solve_reduced (plan_solve_ext)
    int solve_ext_on;                  // 1: those tiles take part and the solution falls out of the factor; 0: back-substitution (fallback plan, fp32-Jacobian tier, debug setter)
    int cam_wg[9];                     // cam_chunk_ptr by value for rigs of <= kMaxCamLds cameras (k_reduce_control: no index load in front of the tiles)
    // frame sharding (tscm_solver_create_sharded): this rank / number of ranks; 0 / 1 on a single GPU
    int rank, world;
    // T is stored compact: one 16x16 tile per camera-pair block (mi <= mj) that ANY rank contributes to, numbered in
    // lexicographic (mi, mj) order -- the same list on every rank, so the all-reduce is over n_bids * 256 doubles
    // and every tile is rewritten in full each iteration.
    const short *bid_lut;              // [C*C] tile of block (mi, mj), mi <= mj; -1 = no board is seen by both
    int bid_part_small[kSmallBids + 1]; // bid_part_ptr by value (rigs of <= kMaxCamLds cameras: no memory round trip in front of the partial tiles)
    int g4_per;                        // k_eval_gram4<KS, true>: corners of a pass (boards of more than 56 corners: g4_plan)
};

struct DevState {
    double *cam_rt[2], *intr[2], *board_rt[2];
    double *board_pc, *cam_pc;
    double *vconst;
    double *cconst[2];                 // per-camera constants of the point the records of the same index were evaluated at
    double *rec[2];
    double *campart, *campart2;
    double *H[2], *H_stage;
    double *s_b, *s_c;
    double *fac;                       // [B][kFac] e-block factors
    double *pairpart, *T;
    int *t_count;                      // arrival counter of the fused T reduction + reduced solve (k_solve_reduced<..., true>)
    int *fac_fail;                     // set by an e-block factorisation that failed (k_schur_gram / k_schur_factor); read and cleared by the reduced
                                       // solve (outside the control block: the control step may rewrite that block while the factorisations run)
    int *y_flag;                       // 2 * epoch + lin_fail once the camera step of that fused launch is written (backsub_body<.., true> waits for it)
    double *yhat;
    double *Abig;                      // compact reduced system + rhs row in 16x16 blocks, rigs of more than kMaxCamLds cameras only
    double *bs_part, *st_part;
    int n_bs_blocks, n_st_blocks;
    Ctrl *ctrl;
    CtrlHead *ctrl_snap;               // copy of the control block's head taken by k_reduce_stats: what the control step in the head of the
                                       // NEXT launch (k_schur_gram, every workgroup) reads while that launch's writer workgroup advances `ctrl`
    int *stats_count, *stats_flag;     // k_schur_gram<NV, true>: arrivals of its reduction workgroups, counted over the solve; the count the last arrival of a launch
                                       // found, in a line of its own (what the waiting workgroups poll: loads there, read-modify-writes here)
    struct CtlPub *ctl_pub;            // outcome of that step, published by the writer workgroup for the workgroups of later rounds of the grid
};
// epoch: number of control steps taken in k_schur_gram's head in this solve so far (monotonic, zeroed by k_begin_solve)
struct CtlPub { int epoch, cur, done, pad; double radius; };

// All-reduce over the 16 lanes of a DPP row without the LDS crossbar: a butterfly of quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_half_mirror and row_mirror (after the first two steps every lane of a quad holds the quad's value, so
// the mirrored partner is as good as the xor partner).  A VALU move per 32-bit half and step, a few clocks of latency
// each, against ~100 ns per ds_bpermute round trip of __shfl_xor.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row16_allsum(double v)
{
    v += dpp_f64<0xB1>(v); v += dpp_f64<0x4E>(v); v += dpp_f64<0x141>(v); v += dpp_f64<0x140>(v);
    return v;
}
__device__ __forceinline__ double row16_allmax(double v)
{
    v = fmax(v, dpp_f64<0xB1>(v)); v = fmax(v, dpp_f64<0x4E>(v)); v = fmax(v, dpp_f64<0x141>(v)); v = fmax(v, dpp_f64<0x140>(v));
    return v;
}

// Device-side hand-offs (many producer workgroups -> the workgroup that consumes their results in the SAME launch).
// The textbook form -- plain stores, release fence, counter; counter, acquire fence, plain loads -- makes every producer
// issue a `buffer_wbl2` (the agent-scope release fence writes its XCD's L2 back).  Measured with tools/kernel_timeline.py:
// with the fences the producers of k_reduce_control ended 4.9 us (143 workgroups, config 4) and 16 us (441, config 5)
// after the kernel's first start, whatever they computed.  Here the handed-over values are written THROUGH instead
// (agent-scope stores: `global_store ... sc1`), a producer waits for their completion (`s_waitcnt vmcnt(0)`, then the
// workgroup barrier) and only then counts itself in; the consumer reads them with agent-scope loads (`sc1`: not from its
// own XCD's L2).  No L2 write-back anywhere: 4.0 / 6-8 us, the iteration 130.1 -> 127.9 us (config 4), 393.8 -> 381.2
// (config 5), same bits.  Everything else a kernel writes stays an ordinary store and reaches the next kernel through
// the kernel boundary as before.  (Counting the arrivals in two levels, sixteen workgroups per counter, was slower:
// contention on the single counter is not what the producers wait for.)
//
// What the ordering rests on.  EVERY handed-over location is written with an agent-scope atomic store and read with an
// agent-scope atomic load -- no plain access to it on either side inside the launch that hands it over -- so in the
// language's terms there is no data race; what the relaxed orders leave open is only the ORDER between the data and the
// flag.  That order is supplied by the machine, in the way the AMDGPU back-end itself implements a release on
// gfx942 / gfx950 ("buffer_wbl2 sc1; s_waitcnt vmcnt(0)" in front of the flag's store): the write-back is there for PLAIN
// stores that may still sit in the XCD's L2; an sc1 store is written through, and its vmcnt slot is returned when the write
// has reached the level all XCDs share.  `s_waitcnt vmcnt(0)` + workgroup barrier + flag is therefore the release
// sequence minus the part that has nothing to do here.  On the consumer side the sc1 loads do not hit in the L1 / the
// XCD's L2, so no `buffer_inv` is needed for THESE loads (an acquire fence would issue one per wave: 20 us for the 2,500
// waves that wait for the camera step).  This is a property of the gfx942 / gfx950 cache hierarchy, not of HIP:
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "the in-launch hand-offs (handoff_store / handoff_load) rely on gfx942 / gfx950 sc1 write-through semantics: re-derive them for this target"
#endif
// The locations handed over inside a launch -- a new read of producer-written data in a waiting workgroup MUST go
// through handoff_load, a new write of consumer-read data through handoff_store:
//   T[n_bids][256]                    t_reduce_block (T producers)        -> k_solve_nd, solver workgroup        flag: t_count
//   yhat[n_pad]                       reduced_solution_tail (solver)      -> backsub_body<.., true>              flag: y_flag
//   cam_rt[cur^1], intr[cur^1]        reduced_solution_tail (solver)      -> backsub_body<.., true> (phase B)    flag: y_flag
//   ctrl->done / fault / term_type    solver or a waiting workgroup (late hand-off) -> waiting workgroups        (atomics both sides)
//   campart2[C][512], st_part[..][3]  cam_reduce_block / board_stats_block -> k_reduce_control's last workgroup  flag: ctrl->fin_count
//   campart2, st_part, ctrl_snap      the reduction blocks riding in k_schur_gram<NV, true> -> every workgroup's control step   flag: stats_flag
//                                     (read with PLAIN loads behind the flag: single-writer lines, see k_schur_gram)
// (the solver workgroup ALSO reads cam_rt / intr of the candidate with plain loads in write_camera_record: its own
// written-through stores, program order within one workgroup, never cached in its L1 before).
// A hand-off that has not come after this long is a device fault, not a numerical event: the solver workgroup sets the
// sticky ctrl->fault together with ctrl->done (every later kernel of the stream exits at once) and the host returns
// TSCM_E_HIP.  s_memrealtime ticks: 100 MHz whatever the shader clock does.
constexpr long long kHandoffTimeoutTicks = 50 * 1000 * 1000;          // 0.5 s
__device__ __forceinline__ void handoff_store(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double handoff_load(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
