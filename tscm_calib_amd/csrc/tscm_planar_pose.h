// tscm_planar_pose.h -- the planar pose fit behind estimate_extrinsic (TS.cpp:170-203), once, for k_estimate_extrinsic (one
// thread per view, all corners) and for the refit of k_estimate_extrinsic_ransac (one wave per view, the winner's inliers).
// cv::solvePnPRansac (external, randomised) is replaced by the deterministic planar PnP its iterative method performs on an
// all-inlier set: DLT homography (Hartley-normalised board points, h33 = 1, 8x8 normal equations), pose from the columns,
// polar orthonormalisation, Gauss-Newton on the 6 pose parameters with the analytic Jacobian.
// The two callers differ in the corners that take part (an accessor) and in how a sum over corners is formed (a lane
// policy); nothing here branches on the caller.  Plain C++17 on the host (tests/native/planar_pose_check.cpp runs it there).
#ifndef TSCM_PLANAR_POSE_H
#define TSCM_PLANAR_POSE_H

#include "../../include/tscm/tscm.h"
#include "tscm_math.h"

// Products are fused with sums only where one expression writes a * b + c, as the front end decides from this text: with
// hipcc's default (contract = fast) the back end fuses across statements, by what else it finds in the basic block, and the
// instantiations of one kernel then differ in their last bits.
#ifdef __HIPCC__
#pragma clang fp contract(on)
#endif

namespace tscm {

// Offsets inside a per-view stage record that both kernels and the host unpacking share.  T has its own offset per kernel.
constexpr int kStageH = 18, kStagePose0 = 27, kStagePose = 33, kStageSteps = 39;

// Lane policies: where a lane starts in the corner order, its stride, and how its partial becomes the sum.
struct SerialLanes {                                  // one thread walks every corner
    static TSCM_HD int first() { return 0; }
    static TSCM_HD int stride() { return 1; }
    static TSCM_HD double sum(double x) { return x; }
};
#ifdef __HIPCC__
struct WaveLanes {                                    // corner order i = lane, lane + 64, ...
    static __device__ __forceinline__ int first() { return threadIdx.x; }
    static __device__ __forceinline__ int stride() { return 64; }
    // sum over the wave in a fixed tree; every lane receives the same bits
    static __device__ __forceinline__ double sum(double x)
    {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        return x;
    }
};
#endif

// Cholesky solve in place; reads the lower triangle of A only
template <int NN>
TSCM_HD bool chol_solve(double *A, double *b)
{
    for (int j = 0; j < NN; ++j) {
        double d = A[j * NN + j];
        for (int k = 0; k < j; ++k) d -= A[j * NN + k] * A[j * NN + k];
        if (!(d > 0.0)) return false;
        d = sqrt(d);
        A[j * NN + j] = d;
        for (int i = j + 1; i < NN; ++i) {
            double s = A[i * NN + j];
            for (int k = 0; k < j; ++k) s -= A[i * NN + k] * A[j * NN + k];
            A[i * NN + j] = s / d;
        }
    }
    for (int i = 0; i < NN; ++i) { double s = b[i]; for (int k = 0; k < i; ++k) s -= A[i * NN + k] * b[k]; b[i] = s / A[i * NN + i]; }
    for (int i = NN - 1; i >= 0; --i) { double s = b[i]; for (int k = i + 1; k < NN; ++k) s -= A[k * NN + i] * b[k]; b[i] = s / A[i * NN + i]; }
    return true;
}

// orthogonal polar factor by Newton iteration X <- (X + X^-T) / 2, then the angle-axis vector (cv::Rodrigues)
TSCM_HD void rotation_vector(const double *Min, double *rv)
{
    double X[9];
    for (int i = 0; i < 9; ++i) X[i] = Min[i];
    for (int it = 0; it < 50; ++it) {
        const double c00 = X[4] * X[8] - X[5] * X[7], c01 = X[5] * X[6] - X[3] * X[8], c02 = X[3] * X[7] - X[4] * X[6];
        const double c10 = X[2] * X[7] - X[1] * X[8], c11 = X[0] * X[8] - X[2] * X[6], c12 = X[1] * X[6] - X[0] * X[7];
        const double c20 = X[1] * X[5] - X[2] * X[4], c21 = X[2] * X[3] - X[0] * X[5], c22 = X[0] * X[4] - X[1] * X[3];
        const double det = X[0] * c00 + X[1] * c01 + X[2] * c02;
        const double cof[9] = { c00, c01, c02, c10, c11, c12, c20, c21, c22 };
        double diff = 0.0;
        for (int i = 0; i < 9; ++i) { const double y = 0.5 * (X[i] + cof[i] / det); diff = fmax(diff, fabs(y - X[i])); X[i] = y; }
        if (diff < 1e-16) break;
    }
    double rx = X[7] - X[5], ry = X[2] - X[6], rz = X[3] - X[1];
    const double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (X[0] + X[4] + X[8] - 1.0) * 0.5;
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    double theta = acos(c);
    if (s < 1e-5) {
        if (c > 0) { rv[0] = rv[1] = rv[2] = 0.0; return; }
        double t = (X[0] + 1.0) * 0.5;
        rx = sqrt(fmax(t, 0.0));
        t = (X[4] + 1.0) * 0.5;
        ry = sqrt(fmax(t, 0.0)) * (X[1] < 0 ? -1.0 : 1.0);
        t = (X[8] + 1.0) * 0.5;
        rz = sqrt(fmax(t, 0.0)) * (X[2] < 0 ? -1.0 : 1.0);
        if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && ((X[5] > 0) != (ry * rz > 0))) rz = -rz;
        theta /= sqrt(rx * rx + ry * ry + rz * rz);
        rv[0] = rx * theta; rv[1] = ry * theta; rv[2] = rz * theta;
    } else {
        const double vth = theta / (2.0 * s);
        rv[0] = rx * vth; rv[1] = ry * vth; rv[2] = rz * vth;
    }
}

// transform T = R2 * R1 turning the camera towards the board's reference corner at pixel (u, v)  (:175-187)
TSCM_HD void look_at_turn(const double I[9], double u, double v, double T[9])
{
    double p[3];
    unproject_pixel(I, u, v, p);
    const double alpha = atan2(p[0], p[2]), beta = asin(p[1]);
    const double ca = cos(alpha), sa = sin(alpha), cb = cos(beta), sb = sin(beta);
    T[0] = ca; T[1] = 0.0; T[2] = -sa;
    T[3] = -sb * sa; T[4] = cb; T[5] = -sb * ca;
    T[6] = cb * sa; T[7] = sb; T[8] = cb * ca;
}

// the corner at pixel (u, v): un-projected, turned by T and divided by its depth Z in the turned frame
TSCM_HD void turned_corner(const double I[9], const double T[9], double u, double v, double &x, double &y, double &Z)
{
    double q[3];
    unproject_pixel(I, u, v, q);
    const double X = T[0] * q[0] + T[1] * q[1] + T[2] * q[2], Y = T[3] * q[0] + T[4] * q[1] + T[5] * q[2];
    Z = T[6] * q[0] + T[7] * q[1] + T[8] * q[2];
    x = X / Z; y = Y / Z;
}

// Rt = transform^T [r1 r2 t]  (:195-200)
TSCM_HD void compose_rt(const double T[9], const double R[9], const double t[3], double o[9])
{
    for (int r = 0; r < 3; ++r) {
        o[3 * r] = T[r] * R[0] + T[3 + r] * R[3] + T[6 + r] * R[6];
        o[3 * r + 1] = T[r] * R[1] + T[3 + r] * R[4] + T[6 + r] * R[7];
        o[3 * r + 2] = T[r] * t[0] + T[3 + r] * t[1] + T[6 + r] * t[2];
    }
}

// The fit of the m corners for which corner(i, x, y) is true (x, y: the turned, normalised corner i) to the board points
// worlds [n][3]: returns the TSCM_EXTRINSIC_* exit code, and from TSCM_EXTRINSIC_CONVERGED on the pose in (rv, t).  Every
// sum over corners is a lane's partial in the order of `lanes`, then lanes.sum: a run gives the same bits every time.  The
// 8x8 and 6x6 systems are solved by every lane on identical values.  stage: the caller's stage record, written at the
// shared offsets as far as the fit gets, or NULL (in a wave: all lanes but the one that records).
template <class Lanes, class Corner>
TSCM_HD int fit_planar_pose(Lanes lanes, Corner corner, int m, const double *worlds, int n, double *stage, double rv[3], double t[3])
{
    const int i0 = lanes.first(), di = lanes.stride();
    // Hartley normalisation of the board points
    double cx = 0, cy = 0, md = 0;
    for (int i = i0; i < n; i += di)
        if (double x, y; corner(i, x, y)) { cx += worlds[3 * i]; cy += worlds[3 * i + 1]; }
    cx = lanes.sum(cx) / m; cy = lanes.sum(cy) / m;
    for (int i = i0; i < n; i += di)
        if (double x, y; corner(i, x, y)) { const double dx = worlds[3 * i] - cx, dy = worlds[3 * i + 1] - cy; md += sqrt(dx * dx + dy * dy); }
    md = lanes.sum(md) / m;
    if (!(md > 0.0)) return TSCM_EXTRINSIC_DEGENERATE_BOARD;
    const double s = sqrt(2.0) / md;
    // DLT: 8x8 normal equations, the lower triangle of A (all that chol_solve reads) and b
    double A[64], b[8];
    for (int i = 0; i < 64; ++i) A[i] = 0.0;
    for (int i = 0; i < 8; ++i) b[i] = 0.0;
    for (int i = i0; i < n; i += di) {
        double x, y;
        if (!corner(i, x, y)) continue;
        const double X = (worlds[3 * i] - cx) * s, Y = (worlds[3 * i + 1] - cy) * s;
        const double r1[8] = { X, Y, 1, 0, 0, 0, -x * X, -x * Y }, r2[8] = { 0, 0, 0, X, Y, 1, -y * X, -y * Y };
        for (int a = 0; a < 8; ++a) {
            for (int c = 0; c <= a; ++c) A[8 * a + c] += r1[a] * r1[c] + r2[a] * r2[c];
            b[a] += r1[a] * x + r2[a] * y;
        }
    }
    for (int a = 0; a < 8; ++a) {
        for (int c = 0; c <= a; ++c) A[8 * a + c] = lanes.sum(A[8 * a + c]);
        b[a] = lanes.sum(b[a]);
    }
    if (!chol_solve<8>(A, b)) return TSCM_EXTRINSIC_DLT_FAILED;
    const double Hn[9] = { b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], 1.0 };
    double H[9];
    for (int r = 0; r < 3; ++r) {
        H[3 * r] = Hn[3 * r] * s; H[3 * r + 1] = Hn[3 * r + 1] * s;
        H[3 * r + 2] = Hn[3 * r + 2] - s * (Hn[3 * r] * cx + Hn[3 * r + 1] * cy);
    }
    if (stage)
        for (int i = 0; i < 9; ++i) stage[kStageH + i] = H[i];
    const double n1 = sqrt(H[0] * H[0] + H[3] * H[3] + H[6] * H[6]), n2 = sqrt(H[1] * H[1] + H[4] * H[4] + H[7] * H[7]);
    if (!(n1 > 0.0) || !(n2 > 0.0)) return TSCM_EXTRINSIC_ZERO_COLUMN;
    double lam = 2.0 / (n1 + n2);
    if (H[8] < 0) lam = -lam;
    double M[9];
    for (int r = 0; r < 3; ++r) { M[3 * r] = lam * H[3 * r]; M[3 * r + 1] = lam * H[3 * r + 1]; t[r] = lam * H[3 * r + 2]; }
    M[2] = M[3] * M[7] - M[6] * M[4]; M[5] = M[6] * M[1] - M[0] * M[7]; M[8] = M[0] * M[4] - M[3] * M[1];
    rotation_vector(M, rv);
    if (stage)
        for (int i = 0; i < 3; ++i) { stage[kStagePose0 + i] = rv[i]; stage[kStagePose0 + 3 + i] = t[i]; }
    // Gauss-Newton on (rv, t), analytic Jacobian
    double R[9], dR[27];
    int steps = 0;
    int exit_code = TSCM_EXTRINSIC_ITERATION_CAP;
    for (int it = 0; it < 10; ++it) {
        rotation_and_derivatives(rv, R, dR);
        double JtJ[36], Jtr[6];                                             // lower triangle, as for the DLT
        for (int i = 0; i < 36; ++i) JtJ[i] = 0.0;
        for (int i = 0; i < 6; ++i) Jtr[i] = 0.0;
        for (int i = i0; i < n; i += di) {
            double x, y;
            if (!corner(i, x, y)) continue;
            const double wx = worlds[3 * i], wy = worlds[3 * i + 1];
            const double PX = R[0] * wx + R[1] * wy + t[0], PY = R[3] * wx + R[4] * wy + t[1], PZ = R[6] * wx + R[7] * wy + t[2];
            const double iz = 1.0 / PZ, rx = PX * iz - x, ry = PY * iz - y;
            double J[2][6];
            for (int q = 0; q < 3; ++q) {                                   // d P / d w_q = dR_q (wx, wy, 0)
                const double dX = dR[9 * q] * wx + dR[9 * q + 1] * wy, dY = dR[9 * q + 3] * wx + dR[9 * q + 4] * wy, dZ = dR[9 * q + 6] * wx + dR[9 * q + 7] * wy;
                J[0][q] = (dX - PX * iz * dZ) * iz; J[1][q] = (dY - PY * iz * dZ) * iz;
            }
            J[0][3] = iz; J[0][4] = 0.0; J[0][5] = -PX * iz * iz;
            J[1][3] = 0.0; J[1][4] = iz; J[1][5] = -PY * iz * iz;
            for (int a = 0; a < 6; ++a) {
                for (int c = 0; c <= a; ++c) JtJ[6 * a + c] += J[0][a] * J[0][c] + J[1][a] * J[1][c];
                Jtr[a] += J[0][a] * rx + J[1][a] * ry;
            }
        }
        for (int a = 0; a < 6; ++a) {
            for (int c = 0; c <= a; ++c) JtJ[6 * a + c] = lanes.sum(JtJ[6 * a + c]);
            Jtr[a] = lanes.sum(Jtr[a]);
        }
        for (int a = 0; a < 6; ++a) JtJ[7 * a] *= 1.0 + 1e-12;
        if (!chol_solve<6>(JtJ, Jtr)) { exit_code = TSCM_EXTRINSIC_GN_CHOLESKY; break; }    // the iterate before the break is kept
        double step = 0.0;
        for (int a = 0; a < 3; ++a) { rv[a] -= Jtr[a]; t[a] -= Jtr[3 + a]; step += Jtr[a] * Jtr[a] + Jtr[3 + a] * Jtr[3 + a] / fmax(1.0, t[a] * t[a]); }
        ++steps;
        if (step < 1e-24) { exit_code = TSCM_EXTRINSIC_CONVERGED; break; }
    }
    if (stage) {
        for (int i = 0; i < 3; ++i) { stage[kStagePose + i] = rv[i]; stage[kStagePose + 3 + i] = t[i]; }
        stage[kStageSteps] = steps;
    }
    return exit_code;
}

}  // namespace tscm

#ifdef __HIPCC__
#pragma clang fp contract(fast)     // hipcc's default, for the code that includes this header
#endif

#endif
