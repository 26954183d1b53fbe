// tscm_prep.h -- stage 0 of an LM iteration: the pose, per-view and per-camera constants of the point that is evaluated
// next (k_pose_prep, k_view_prep; the back-substitution writes the same records for a candidate).
#pragma once
// (included from tscm_kernels.h inside namespace tscm)

// ---------------------------------------------------------------------------------------------
// pose constants of the evaluation target (rotations and their derivatives; the two sincos
// per pose are hoisted out of the per-corner work).  grid: ceil((B + C)/256) x 256
// ---------------------------------------------------------------------------------------------
__global__ void k_pose_prep(DevProblem P, DevState S, int cand)
{
    if (S.ctrl->done) return;
    const int tgt = cand ? (S.ctrl->cur ^ 1) : S.ctrl->cur;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.B) {
        double rt[6], out[kBoardConst];
        for (int k = 0; k < 6; ++k) rt[k] = S.board_rt[tgt][6 * i + k];
        board_constants(rt, out);
        for (int k = 0; k < kBoardConst; ++k) S.board_pc[(size_t)kBoardConst * i + k] = out[k];
    } else if (i < P.B + P.C) {
        const int m = i - P.B;
        double rt[6], out[kCamConst];
        for (int k = 0; k < 6; ++k) rt[k] = S.cam_rt[tgt][6 * m + k];
        camera_constants(rt, out);
        for (int k = 0; k < kCamConst; ++k) S.cam_pc[kCamConst * m + k] = out[k];
    }
}

__device__ __forceinline__ void load_view_const(const DevProblem &P, const DevState &S, int tgt, int cam, int board, ViewConst &vc)
{
    const double *bp = S.board_pc + (size_t)kBoardConst * board;
    for (int k = 0; k < 3; ++k) { vc.r1[k] = bp[k]; vc.r2[k] = bp[3 + k]; vc.tb[k] = S.board_rt[tgt][6 * board + 3 + k]; }
    for (int k = 0; k < 3; ++k) for (int q = 0; q < 6; ++q) vc.db[k][q] = bp[6 + 6 * k + q];
    const double *cp = S.cam_pc + kCamConst * cam;
    for (int k = 0; k < 9; ++k) vc.Rc[k] = cp[k];
    for (int k = 0; k < 27; ++k) vc.dRc[k] = cp[9 + k];
    for (int k = 0; k < 3; ++k) vc.tc[k] = S.cam_rt[tgt][6 * cam + 3 + k];
    const double *I = S.intr[tgt] + 9 * cam;
    vc.fx = I[0]; vc.fy = I[1]; vc.cx = I[2]; vc.cy = I[3]; vc.xi = I[4]; vc.lam = I[5]; vc.al = I[6];
}

// ---------------------------------------------------------------------------------------------
// per-view / per-camera constants of the evaluation target in the form the hot kernel consumes.
// grid ceil((V + C)/128) x 128.
//   vconst[view][32]: r1(3) r2(3) t_b(3), then for k=0..2: R_c dR_b/dw_k[:,0] (3), R_c dR_b/dw_k[:,1] (3); 5 pad
//   cconst[cam] : R_c(9) t_c(3) dR_c/dw_k (27) fx fy cx cy xi lambda beta=alpha/(1-alpha) 1/(1-alpha)^2
// ---------------------------------------------------------------------------------------------
// the first nine per-view constants: the board point (x, y, 0) in the camera frame is x m1 + y m2 + t
__device__ __forceinline__ void view_point_constants(const double Rc[9], const double *tc, const double *bc /* r1, r2 */, const double *tb, double *o)
{
    for (int r = 0; r < 3; ++r) {
        o[r] = Rc[3 * r] * bc[0] + Rc[3 * r + 1] * bc[1] + Rc[3 * r + 2] * bc[2];
        o[3 + r] = Rc[3 * r] * bc[3] + Rc[3 * r + 1] * bc[4] + Rc[3 * r + 2] * bc[5];
        o[6 + r] = (Rc[3 * r] * tb[0] + Rc[3 * r + 1] * tb[1] + Rc[3 * r + 2] * tb[2]) + tc[r];
    }
}

// the per-camera record of the evaluation target (doubles, then the same values as floats)
__device__ __forceinline__ void write_camera_record(const DevState &S, int tgt, int m, const double *cam_rt, const double *intr)
{
    double crt[3], Rc[9], a[9], wsm[3];
    for (int k = 0; k < 3; ++k) crt[k] = cam_rt[6 * m + k];
    const int small = camera_rotation_constants(crt, Rc, a, wsm);
    double *o = S.cconst[tgt] + kCStride * m;
    for (int k = 0; k < 9; ++k) o[k] = Rc[k];
    for (int k = 0; k < 3; ++k) o[9 + k] = cam_rt[6 * m + 3 + k];
    for (int k = 0; k < 9; ++k) o[12 + k] = a[k];
    for (int k = 0; k < 3; ++k) o[21 + k] = wsm[k];
    o[24] = small ? 1.0 : 0.0;
    for (int k = 25; k < 39; ++k) o[k] = 0.0;
    double I[7];
    for (int k = 0; k < 7; ++k) I[k] = intr[9 * m + k];
    for (int k = 0; k < 6; ++k) o[39 + k] = I[k];
    const double oma = 1.0 - I[6];
    o[45] = I[6] / oma;
    o[46] = 1.0 / (oma * oma);
    o[47] = 0.0;
    float *of = reinterpret_cast<float *>(o + kCConst);
    for (int k = 0; k < kCConst; ++k) of[k] = (float)o[k];
}
__device__ __forceinline__ void write_camera_record(const DevState &S, int tgt, int m) { write_camera_record(S, tgt, m, S.cam_rt[tgt], S.intr[tgt]); }

// (the point's parameters come from explicit arrays: buffer `tgt` -- or, in the first launch of a solve, the registered start point)
__device__ __forceinline__ void view_prep_body(const DevProblem &P, const DevState &S, int tgt, int with_floats, const double *cam_rt, const double *intr, const double *board_rt)
{
    __shared__ double st[kVPrepThreads][kVFloatOff + 1];    // the 27 (+5 pad) doubles of thread t in row t (pitch 33: conflict-free both ways)
    const int t = threadIdx.x;
    const int i = blockIdx.x * kVPrepThreads + t;
    if (i < P.V) {
        // self-contained (rotations recomputed per view: cheaper than a second launch + round trip)
        const int b = P.view_board[i], m = P.view_cam[i];
        double rt[6], bc[kBoardConst], Rc[9], dRc[27];
        for (int k = 0; k < 6; ++k) rt[k] = board_rt[6 * b + k];
        board_constants(rt, bc);
        double crt[3];
        for (int k = 0; k < 3; ++k) crt[k] = cam_rt[6 * m + k];
        rotation_and_derivatives(crt, Rc, dRc);
        double *o = st[t];
        view_point_constants(Rc, cam_rt + 6 * m + 3, bc, rt + 3, o);
        for (int k = 0; k < 6; ++k) {           // six 3-vectors d -> R_c d
            const double d0 = bc[6 + 3 * k], d1 = bc[6 + 3 * k + 1], d2 = bc[6 + 3 * k + 2];
            for (int r = 0; r < 3; ++r) o[9 + 3 * k + r] = Rc[3 * r] * d0 + Rc[3 * r + 1] * d1 + Rc[3 * r + 2] * d2;
        }
        for (int k = kVConst; k < kVFloatOff; ++k) o[k] = 0.0;
    } else if (i < P.V + P.C) {
        write_camera_record(S, tgt, i - P.V, cam_rt, intr);
    }
    __syncthreads();
    // the block's records leave as one contiguous, coalesced stream: vconst[view][32]
    const int v0 = blockIdx.x * kVPrepThreads;
    const int nv = min(kVPrepThreads, P.V - v0);
    for (int e = t; e < nv * kVFloatOff; e += kVPrepThreads) {                 // compile-time divisors: shifts
        const int v = e / kVFloatOff, k = e % kVFloatOff;
        S.vconst[(size_t)kVStride * (v0 + v) + k] = st[v][k];
    }
    if (with_floats) {
        // the float half of a record (the same 27 values as floats, two per double slot) is only written for
        // the fp32-Jacobian kernel
        constexpr int kF = kVStride - kVFloatOff;
        for (int e = t; e < nv * kF; e += kVPrepThreads) {
            const int v = e / kF, k = e % kF, j = 2 * k;
            const float f0 = j < kVConst ? (float)st[v][j] : 0.f, f1 = j + 1 < kVConst ? (float)st[v][j + 1] : 0.f;
            S.vconst[(size_t)kVStride * (v0 + v) + kVFloatOff + k] = __hiloint2double(__float_as_int(f1), __float_as_int(f0));
        }
    }
}

__global__ __launch_bounds__(kVPrepThreads) void k_view_prep(DevProblem P, DevState S, int cand, int with_floats)
{
    if (S.ctrl->done) return;
    const int tgt = cand ? (S.ctrl->cur ^ 1) : S.ctrl->cur;
    view_prep_body(P, S, tgt, with_floats, S.cam_rt[tgt], S.intr[tgt], S.board_rt[tgt]);
}
