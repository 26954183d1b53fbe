// tscm_view_gain.hip -- next-best view (tscm.h: tscm_view_gain): how much of the camera covariance of
// tscm_covariance a hypothetical view of the board removes, for many candidate board poses at once.
//
//   k_view_prepare  one workgroup (one wave) per distinct (camera_a, camera_b) among the candidates: gathers Sigma_theta from
//                   the 15-wide cam_cov, scales it to unit diagonal, factors it (columns that are not free skipped) and
//                   leaves G = D G~ and Q_theta = (Sigma diag(w) Sigma)_theta,theta, both [26][26], and a pivot flag.
//   k_view_gain<N>  one workgroup of one wave per candidate, N = 13 (one camera) or 26 (a pair).  Lanes run over corners in
//                   passes of 64: projection, visibility (counted by ballot) and the 2 x 19 rows [E | F] into LDS; the 190
//                   entries of the rows' 19 x 19 Gram triangle -- B' (21), W' (78) and C' (91) of the camera -- are owned by
//                   one lane each, three to a lane, and summed in corner order.  The 6 x 6 factor of B' is redundant in every
//                   lane's registers; Delta S, G (later Y), T = Delta S G and M = I + G^T T (later its Cholesky factor) are
//                   LDS tiles of odd pitch in the space the rows leave; entries of a product are dealt over the 64 lanes,
//                   the triangular solves, K and the trace run one column to a lane.  No trip count depends on data other
//                   than n_points and N.
//   k_view_apply    Sigma' = Sigma - Sigma[:, theta] K Sigma[theta, :] of one candidate, one thread per element of the lower
//                   triangle (its mirror is the same double), the sums over theta ascending.
// project_jacobian is a second copy of the one in tscm_uncertainty.hip: moving it into a shared header would have had to
// leave k_uncertainty's code object unchanged, and a copy guarantees that.
// All fp64, no floating-point atomics, every sum in a fixed order: two calls give the same bytes, and a candidate's bytes do
// not depend on its place in the batch.  Every index comes from arguments the host checked.
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_host.h"
#include "tscm_math.h"

#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

using namespace tscm;

namespace {

constexpr int kVgWave = 64;
constexpr int kVgTheta = kFA;                    // 13 columns of a camera: pose 6, intrinsics 7
constexpr int kVgMax = 2 * kVgTheta;             // 26
constexpr int kVgCam = 15;                       // a camera's width in cam_cov
constexpr int kVgRow = kE + kVgTheta;            // 19: a corner's row [E | F]
constexpr int kVgTri = kVgRow * (kVgRow + 1) / 2;   // 190 entries of the rows' Gram triangle
constexpr int kVgRowPitch = 2 * kVgRow + 1;      // 39 doubles per corner (u row, v row, pad: odd, so 32 lanes hit 32 banks)
constexpr int kVgOwn = (kVgTri + kVgWave - 1) / kVgWave;   // 3 entries to a lane
constexpr int kVgPrepStride = kVgMax * kVgMax;   // G and Q of a pair, pitch 26

thread_local double g_last_kernel_seconds = 0.0;

struct VgCandidate { int a, b, pair, pad; double rt[6]; };

struct ProjJ {
    double u, v, k, mx, my;
    double a[6];
    double gu[3], gv[3];
};

// The functor's projection and its derivatives, operation by operation as tscm_uncertainty.hip has them.
__device__ __forceinline__ void project_jacobian(const double *I, double X, double Y, double Z, ProjJ &o)
{
    const double fx = I[0], fy = I[1], cx = I[2], cy = I[3], xi = I[4], lam = I[5], al = I[6];
    const double rho2 = X * X + Y * Y;
    const double d1 = sqrt(rho2 + Z * Z);
    const double z1 = Z + xi * d1;
    const double d2 = sqrt(rho2 + z1 * z1);
    const double z2 = z1 + lam * d2;
    const double d3 = sqrt(rho2 + z2 * z2);
    const double oma = 1.0 - al;
    const double beta = al / oma;
    const double k = z2 + beta * d3;
    const double ik = 1.0 / k;
    const double mx = X * ik, my = Y * ik;
    o.k = k; o.mx = mx; o.my = my;
    o.u = fx * mx + cx;
    o.v = fy * my + cy;
    const double id1 = 1.0 / d1, id2 = 1.0 / d2, id3 = 1.0 / d3;
    const double c1 = 1.0 + xi * Z * id1;
    const double c2 = 1.0 + lam * z1 * id2;
    const double c3 = 1.0 + beta * z2 * id3;
    const double q = beta * id3 + c3 * (lam * id2 + c2 * xi * id1);
    const double kz = c1 * c2 * c3;
    const double fxk = fx * ik, fyk = fy * ik;
    o.a[0] = fxk * (1.0 - X * mx * q); o.a[1] = -fxk * mx * Y * q;        o.a[2] = -fxk * mx * kz;
    o.a[3] = -fyk * my * X * q;        o.a[4] = fyk * (1.0 - Y * my * q); o.a[5] = -fyk * my * kz;
    const double hu = fxk * mx, hv = fyk * my;
    const double kxi = c3 * c2 * d1, klam = c3 * d2, kal = d3 / (oma * oma);
    o.gu[0] = -(hu * kxi);  o.gv[0] = -(hv * kxi);
    o.gu[1] = -(hu * klam); o.gv[1] = -(hv * klam);
    o.gu[2] = -(hu * kal);  o.gv[2] = -(hv * kal);
}

__device__ __forceinline__ int tri_index(int p, int q) { return p >= q ? p * (p + 1) / 2 + q : q * (q + 1) / 2 + p; }

// row of cam_cov of theta column i of the pair (a, b)
__device__ __forceinline__ int theta_row(int i, int a, int b) { return kVgCam * (i < kVgTheta ? a : b) + (i < kVgTheta ? i : i - kVgTheta); }

// In-place lower Cholesky factor of the n x n tile A (pitch P) by one wave, left-looking: at column j lane i forms
// s_i = A_ij - sum_{k<j} L_ik L_jk (k ascending) and divides by the root of lane j's s.  skip (may be NULL): columns that
// are left out, zero in the factor.  Returns false if a pivot of a column that is not skipped was not > 0.
template <int P>
__device__ __forceinline__ bool wave_cholesky(double *A, int n, const unsigned char *skip, int lane)
{
    bool ok = true;
    for (int j = 0; j < n; ++j) {
        double s = 0.0;
        if (lane < n && lane >= j) {
            s = A[lane * P + j];
            for (int k = 0; k < j; ++k) s -= A[lane * P + k] * A[j * P + k];
        }
        const double piv = __shfl(s, j, kVgWave);
        __syncthreads();
        if (skip && skip[j]) {
            if (lane < n && lane >= j) A[lane * P + j] = 0.0;
        } else {
            if (!(piv > 0.0)) ok = false;
            const double d = sqrt(piv);
            if (lane < n && lane >= j) A[lane * P + j] = lane == j ? d : s / d;
        }
        __syncthreads();
    }
    return ok;
}

// pairs [n_pairs][2]; G, Q [n_pairs][26][26]; pair_bad [n_pairs]
__global__ __launch_bounds__(kVgWave) void k_view_prepare(const double *__restrict__ cam_cov, const double *__restrict__ weights, int n15,
                                                          const int *__restrict__ pairs, double *__restrict__ Gout, double *__restrict__ Qout,
                                                          int *__restrict__ pair_bad)
{
    constexpr int P = kVgMax + 1;
    __shared__ double sA[kVgMax * P];
    __shared__ double sD[kVgMax];
    __shared__ unsigned char sSkip[kVgMax];
    const int lane = threadIdx.x, pr = blockIdx.x;
    const int a = pairs[2 * pr], b = pairs[2 * pr + 1];
    const int n = a != b ? kVgMax : kVgTheta;
    if (lane < n) {
        const size_t r = (size_t)theta_row(lane, a, b);
        const double v = cam_cov[r * n15 + r];
        sSkip[lane] = v == 0.0 ? 1 : 0;
        sD[lane] = sqrt(v);
    }
    __syncthreads();
    for (int e = lane; e < n * n; e += kVgWave) {
        const int i = e / n, j = e % n;
        const int ri = theta_row(i, a, b), rj = theta_row(j, a, b);
        const double v = ri >= rj ? cam_cov[(size_t)ri * n15 + rj] : cam_cov[(size_t)rj * n15 + ri];
        sA[i * P + j] = (sSkip[i] || sSkip[j]) ? 0.0 : (i == j ? 1.0 : v / (sD[i] * sD[j]));
    }
    __syncthreads();
    const bool ok = wave_cholesky<P>(sA, n, sSkip, lane);
    double *G = Gout + (size_t)kVgPrepStride * pr, *Q = Qout + (size_t)kVgPrepStride * pr;
    for (int e = lane; e < kVgPrepStride; e += kVgWave) {
        const int i = e / kVgMax, j = e % kVgMax;
        double g = 0.0, q = 0.0;
        if (i < n && j < n) {
            if (i >= j) g = sD[i] * sA[i * P + j];
            // Q_ij = sum_k Sigma[theta_i, k] w_k Sigma[k, theta_j] over all 15 C columns, k ascending
            const int ri = theta_row(i, a, b), rj = theta_row(j, a, b);
            for (int k = 0; k < n15; ++k) {
                double w;
                if (weights) w = weights[k];
                else { const double skk = cam_cov[(size_t)k * n15 + k]; w = skk > 0.0 ? 1.0 / skk : 0.0; }
                const double sik = ri >= k ? cam_cov[(size_t)ri * n15 + k] : cam_cov[(size_t)k * n15 + ri];
                const double skj = rj >= k ? cam_cov[(size_t)rj * n15 + k] : cam_cov[(size_t)k * n15 + rj];
                q += (sik * w) * skj;
            }
        }
        G[e] = g;
        Q[e] = q;
    }
    if (lane == 0) pair_bad[pr] = ok ? 0 : 1;
}

// the LDS of k_view_gain<N>, in doubles
template <int N>
struct VgLds {
    static constexpr int P = (N % 2 == 0) ? N + 1 : N;     // odd pitch
    static constexpr int kTile = N * P;
    static constexpr int kRows = kVgWave * kVgRowPitch;     // the corner rows; dead once the Gram sums are done
    static constexpr int kMat = 4 * kTile;                  // Delta S, G (later Y), T, M (later L)
    static constexpr int kShared = kRows > kMat ? kRows : kMat;
    static constexpr int kGram = kShared;                   // [2][190] Gram triangle of each camera's rows
    static constexpr int kB = kGram + 2 * kVgTri;           // [21] B'
    static constexpr int kZ = kB + 21 + 1;                  // [6][N] Z = Lb^-1 W'
    static constexpr int kConst = kZ + kE * N;              // board R, dR (36), cameras R, dR (2 x 36), t and I (2 x 10)
    static constexpr int kVec = kConst + 36 + 72 + 20;      // [N] per-column trace terms
    static constexpr int kTotal = kVec + N;
};

// list [count]: the candidates with this N.  K (may be NULL): [N][N] of the one candidate of an apply call.
template <int N>
__global__ __launch_bounds__(kVgWave) void k_view_gain(const double *__restrict__ cam_rt, const double *__restrict__ intr,
                                                       const double *__restrict__ board_xy, int n_points, const int *__restrict__ image_size,
                                                       double border, int min_corners, const VgCandidate *__restrict__ cand,
                                                       const int *__restrict__ list, const double *__restrict__ Gprep,
                                                       const double *__restrict__ Qprep, const int *__restrict__ pair_bad,
                                                       double *__restrict__ gains, int *__restrict__ n_visible, int *__restrict__ flags,
                                                       double *__restrict__ Kout)
{
    using L = VgLds<N>;
    constexpr int P = L::P;
    constexpr int kCams = N / kVgTheta;
    __shared__ double sm[L::kTotal];
    double *sRows = sm, *sS = sm, *sG = sm + L::kTile, *sT = sm + 2 * L::kTile, *sM = sm + 3 * L::kTile;
    double *sGram = sm + L::kGram, *sB = sm + L::kB, *sZ = sm + L::kZ, *sC = sm + L::kConst, *sVec = sm + L::kVec;
    const int lane = threadIdx.x;
    const int ci = list[blockIdx.x];
    const VgCandidate cd = cand[ci];
    const int cams[2] = { cd.a, cd.b };

    // rotations: lane 0 the board's, lanes 1 and 2 the cameras'; lanes 8.. their translations and intrinsics
    if (lane <= kCams) {
        double w[3];
        if (lane == 0) { w[0] = cd.rt[0]; w[1] = cd.rt[1]; w[2] = cd.rt[2]; }
        else { const int m = cams[lane - 1]; w[0] = cam_rt[6 * m]; w[1] = cam_rt[6 * m + 1]; w[2] = cam_rt[6 * m + 2]; }
        rotation_and_derivatives(w, sC + 36 * lane, sC + 36 * lane + 9);
    }
    if (lane >= 8 && lane < 8 + 10 * kCams) {
        const int c = (lane - 8) / 10, j = (lane - 8) % 10, m = cams[c];
        sC[108 + 10 * c + j] = j < 3 ? cam_rt[6 * m + 3 + j] : intr[9 * m + j - 3];
    }
    __syncthreads();

    // the lane's entries of the 19 x 19 triangle
    int ep[kVgOwn], eq[kVgOwn];
#pragma unroll
    for (int t = 0; t < kVgOwn; ++t) {
        const int e = lane + kVgWave * t;
        int p = 0;
        for (int r = 1; r < kVgRow; ++r) p += (r * (r + 1) / 2 <= e) ? 1 : 0;
        ep[t] = e < kVgTri ? p : 0;
        eq[t] = e < kVgTri ? e - p * (p + 1) / 2 : 0;
    }

    const double *Rb = sC, *dRb = sC + 9;
    const int passes = (n_points + kVgWave - 1) / kVgWave;
    int nvis[2] = { 0, 0 };
    bool contrib[2] = { false, false };
    double accB = 0.0;                                           // the lane's entry of B' (lanes 0..20), over both cameras
    for (int c = 0; c < kCams; ++c) {
        const double *Rm = sC + 36 * (c + 1), *dRm = Rm + 9, *tm = sC + 108 + 10 * c, *Im = tm + 3;
        const double umax = (double)(image_size[2 * cams[c]] - 1) - border, vmax = (double)(image_size[2 * cams[c] + 1] - 1) - border;
        double acc[kVgOwn];
        acc[0] = accB;
#pragma unroll
        for (int t = 1; t < kVgOwn; ++t) acc[t] = 0.0;
        if (lane >= 21) acc[0] = 0.0;
        int count = 0;
        for (int pass = 0; pass < passes; ++pass) {
            const int j = pass * kVgWave + lane;
            double row[2 * kVgRow];
#pragma unroll
            for (int i = 0; i < 2 * kVgRow; ++i) row[i] = 0.0;
            bool vis = false;
            if (j < n_points) {
                const double x = board_xy[2 * j], y = board_xy[2 * j + 1];
                const double P0 = Rb[0] * x + Rb[1] * y + cd.rt[3], P1 = Rb[3] * x + Rb[4] * y + cd.rt[4], P2 = Rb[6] * x + Rb[7] * y + cd.rt[5];
                const double X = Rm[0] * P0 + Rm[1] * P1 + Rm[2] * P2 + tm[0];
                const double Y = Rm[3] * P0 + Rm[4] * P1 + Rm[5] * P2 + tm[1];
                const double Z = Rm[6] * P0 + Rm[7] * P1 + Rm[8] * P2 + tm[2];
                ProjJ pj;
                project_jacobian(Im, X, Y, Z, pj);
                vis = pj.k > 0.0 && pj.u >= border && pj.u <= umax && pj.v >= border && pj.v <= vmax;
                if (vis) {
                    double AR[6];
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int q = 0; q < 3; ++q) AR[3 * e + q] = pj.a[3 * e] * Rm[q] + pj.a[3 * e + 1] * Rm[3 + q] + pj.a[3 * e + 2] * Rm[6 + q];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double *Dk = dRb + 9 * k;
                        const double g0 = Dk[0] * x + Dk[1] * y, g1 = Dk[3] * x + Dk[4] * y, g2 = Dk[6] * x + Dk[7] * y;
                        row[k] = AR[0] * g0 + AR[1] * g1 + AR[2] * g2;
                        row[kVgRow + k] = AR[3] * g0 + AR[4] * g1 + AR[5] * g2;
                        row[3 + k] = AR[k];
                        row[kVgRow + 3 + k] = AR[3 + k];
                        const double *Mk = dRm + 9 * k;
                        const double h0 = Mk[0] * P0 + Mk[1] * P1 + Mk[2] * P2, h1 = Mk[3] * P0 + Mk[4] * P1 + Mk[5] * P2, h2 = Mk[6] * P0 + Mk[7] * P1 + Mk[8] * P2;
                        row[kE + k] = pj.a[0] * h0 + pj.a[1] * h1 + pj.a[2] * h2;
                        row[kVgRow + kE + k] = pj.a[3] * h0 + pj.a[4] * h1 + pj.a[5] * h2;
                        row[kE + 3 + k] = pj.a[k];
                        row[kVgRow + kE + 3 + k] = pj.a[3 + k];
                        row[kE + 10 + k] = pj.gu[k];
                        row[kVgRow + kE + 10 + k] = pj.gv[k];
                    }
                    row[kE + 6] = pj.mx;           // fx
                    row[kVgRow + kE + 7] = pj.my;  // fy
                    row[kE + 8] = 1.0;             // cx
                    row[kVgRow + kE + 9] = 1.0;    // cy
                }
            }
            count += __popcll(__ballot(vis));
            __syncthreads();                                     // the previous pass's sums have read the rows
#pragma unroll
            for (int i = 0; i < 2 * kVgRow; ++i) sRows[lane * kVgRowPitch + i] = row[i];
            __syncthreads();
#pragma unroll
            for (int t = 0; t < kVgOwn; ++t) {
                double s = acc[t];
                const int p = ep[t], q = eq[t];
                for (int r = 0; r < kVgWave; ++r) {
                    const double *rr = sRows + r * kVgRowPitch;
                    s += rr[p] * rr[q];
                    s += rr[kVgRow + p] * rr[kVgRow + q];
                }
                acc[t] = s;
            }
        }
        nvis[c] = count;
        contrib[c] = count >= min_corners;
        if (contrib[c]) { if (lane < 21) accB = acc[0]; }
        else {
#pragma unroll
            for (int t = 0; t < kVgOwn; ++t) acc[t] = 0.0;
        }
#pragma unroll
        for (int t = 0; t < kVgOwn; ++t) {
            const int e = lane + kVgWave * t;
            if (e < kVgTri) sGram[kVgTri * c + e] = acc[t];
        }
    }
    if (lane < 21) sB[lane] = accB;
    __syncthreads();

    const bool any = contrib[0] || contrib[1];
    unsigned fl = (contrib[0] ? 1u : 0u) | (contrib[1] ? 2u : 0u);
    double g_logdet = 0.0, g_trace = 0.0;
    bool ok = true;
    if (any) {                                                   // uniform over the wave
        const int pr = cd.pair;
        ok = pair_bad[pr] == 0;
        // B' = Lb Lb^T in every lane's registers
        double Lb[21];
#pragma unroll
        for (int i = 0; i < 21; ++i) Lb[i] = sB[i];
#pragma unroll
        for (int j = 0; j < kE; ++j) {
            double d = Lb[j * (j + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) d -= Lb[j * (j + 1) / 2 + k] * Lb[j * (j + 1) / 2 + k];
            if (!(d > 0.0)) ok = false;
            d = sqrt(d);
            Lb[j * (j + 1) / 2 + j] = d;
#pragma unroll
            for (int i = j + 1; i < kE; ++i) {
                double s = Lb[i * (i + 1) / 2 + j];
#pragma unroll
                for (int k = 0; k < j; ++k) s -= Lb[i * (i + 1) / 2 + k] * Lb[j * (j + 1) / 2 + k];
                Lb[i * (i + 1) / 2 + j] = s / d;
            }
        }
        // Z = Lb^-1 W', a column to a lane; W'[i][col] is entry (6 + col, i) of the column's camera
        if (lane < N) {
            const int c = lane / kVgTheta, col = lane % kVgTheta;
            double z[kE];
#pragma unroll
            for (int i = 0; i < kE; ++i) {
                double s = sGram[kVgTri * c + tri_index(kE + col, i)];
#pragma unroll
                for (int k = 0; k < i; ++k) s -= Lb[i * (i + 1) / 2 + k] * z[k];
                z[i] = s / Lb[i * (i + 1) / 2 + i];
                sZ[i * N + lane] = z[i];
            }
        }
        __syncthreads();
        // Delta S = C' - Z^T Z, and G of the pair
        for (int e = lane; e < N * N; e += kVgWave) {
            const int i = e / N, j = e % N;
            const int bi = i / kVgTheta, bj = j / kVgTheta;
            double s = bi == bj ? sGram[kVgTri * bi + tri_index(kE + i % kVgTheta, kE + j % kVgTheta)] : 0.0;
#pragma unroll
            for (int k = 0; k < kE; ++k) s -= sZ[k * N + i] * sZ[k * N + j];
            sS[i * P + j] = s;
            sG[i * P + j] = Gprep[(size_t)kVgPrepStride * pr + i * kVgMax + j];
        }
        __syncthreads();
        // T = Delta S G
        for (int e = lane; e < N * N; e += kVgWave) {
            const int i = e / N, j = e % N;
            double s = 0.0;
            for (int k = 0; k < N; ++k) s += sS[i * P + k] * sG[k * P + j];
            sT[i * P + j] = s;
        }
        __syncthreads();
        // M = I + G^T T
        for (int e = lane; e < N * N; e += kVgWave) {
            const int i = e / N, j = e % N;
            double s = i == j ? 1.0 : 0.0;
            for (int k = 0; k < N; ++k) s += sG[k * P + i] * sT[k * P + j];
            sM[i * P + j] = s;
        }
        __syncthreads();
        if (!wave_cholesky<P>(sM, N, nullptr, lane)) ok = false;
        // Y = L^-1 T^T, a column to a lane, into G's tile
        double *sY = sG;
        if (lane < N) {
            for (int j = 0; j < N; ++j) {
                double s = sT[lane * P + j];
                for (int k = 0; k < j; ++k) s -= sM[j * P + k] * sY[k * P + lane];
                sY[j * P + lane] = s / sM[j * P + j];
            }
        }
        __syncthreads();
        // K = Delta S - Y^T Y and the lane's column of tr(K Q)
        if (lane < N) {
            double t = 0.0;
            for (int i = 0; i < N; ++i) {
                double s = sS[i * P + lane];
                for (int k = 0; k < N; ++k) s -= sY[k * P + i] * sY[k * P + lane];
                t += s * Qprep[(size_t)kVgPrepStride * pr + i * kVgMax + lane];
                if (Kout) Kout[i * N + lane] = s;
            }
            sVec[lane] = t;
        }
        __syncthreads();
        for (int k = 0; k < N; ++k) {
            g_logdet += log(sM[k * P + k]);
            g_trace += sVec[k];
        }
        g_logdet *= 2.0;
        if (!ok) {
            fl |= 8u;
            g_logdet = __builtin_nan("");
            g_trace = __builtin_nan("");
        }
    }
    if (!(fl & 8u) && isfinite(g_logdet) && isfinite(g_trace)) fl |= 4u;
    if (lane == 0) {
        gains[2 * ci] = g_logdet;
        gains[2 * ci + 1] = g_trace;
        n_visible[2 * ci] = nvis[0];
        n_visible[2 * ci + 1] = nvis[1];
        flags[ci] = (int)fl;
    }
}

// out [n15][n15]: thread e owns the element (r, c), r >= c, of the lower triangle and writes its mirror too
__global__ __launch_bounds__(256) void k_view_apply(const double *__restrict__ cam_cov, int n15, int a, int b, int n, const double *__restrict__ K,
                                                    double *__restrict__ out)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)n15 * (n15 + 1) / 2;
    if (e >= total) return;
    int r = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while ((long long)r * (r + 1) / 2 > e) --r;
    while ((long long)(r + 1) * (r + 2) / 2 <= e) ++r;
    const int c = (int)(e - (long long)r * (r + 1) / 2);
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        const int ti = theta_row(i, a, b);
        double p = 0.0;                                          // (K Sigma[theta, c])_i
        for (int j = 0; j < n; ++j) {
            const int tj = theta_row(j, a, b);
            const double sjc = tj >= c ? cam_cov[(size_t)tj * n15 + c] : cam_cov[(size_t)c * n15 + tj];
            p += K[i * n + j] * sjc;
        }
        const double sri = r >= ti ? cam_cov[(size_t)r * n15 + ti] : cam_cov[(size_t)ti * n15 + r];
        s += sri * p;
    }
    const double v = cam_cov[(size_t)r * n15 + c] - s;
    out[(size_t)r * n15 + c] = v;
    out[(size_t)c * n15 + r] = v;
}

int invalid(const std::string &msg) { return tscm_set_error(TSCM_E_INVALID, msg); }

bool all_finite(const double *x, size_t n, size_t *where)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) { *where = i; return false; }
    return true;
}

// the checks of both entry points, in the order tscm.h lists them
int check_args(int n_cameras, const double *cam_rt, const double *intr, const double *cam_cov, const double *weights, int n_points, const double *board_xy,
               const int *image_size, const tscm_view_gain_params *params, const tscm_view_candidate *candidates, int n_candidates, const double *gain_logdet,
               const double *gain_trace, const int *n_visible, const int *flags)
{
    if (!cam_rt) return invalid("cam_rt is NULL");
    if (!intr) return invalid("intr is NULL");
    if (!cam_cov) return invalid("cam_cov is NULL");
    if (!board_xy) return invalid("board_xy is NULL");
    if (!image_size) return invalid("image_size is NULL");
    if (!params) return invalid("params is NULL");
    if (!candidates) return invalid("candidates is NULL");
    if (!gain_logdet) return invalid("gain_logdet is NULL");
    if (!gain_trace) return invalid("gain_trace is NULL");
    if (!n_visible) return invalid("n_visible is NULL");
    if (!flags) return invalid("flags is NULL");
    if (int rc = check_struct_size(params, "tscm_view_gain_params")) return rc;
    if (n_cameras < 1 || n_cameras > 32) return invalid("n_cameras " + std::to_string(n_cameras) + " outside 1..32");
    if (n_points < 1 || n_points > 1024) return invalid("n_points " + std::to_string(n_points) + " outside 1..1024");
    if (n_candidates <= 0) return invalid("n_candidates " + std::to_string(n_candidates) + " <= 0");
    if (n_candidates > (1 << 24)) return invalid("n_candidates " + std::to_string(n_candidates) + " above 2^24");
    if (!std::isfinite(params->border) || params->border < 0.0) return invalid("params: border must be finite and >= 0");
    if (params->min_corners < 4) return invalid("params: min_corners " + std::to_string(params->min_corners) + " < 4");
    size_t at = 0;
    if (!all_finite(cam_rt, (size_t)6 * n_cameras, &at)) return invalid("cam_rt[" + std::to_string(at) + "] is not finite");
    for (int m = 0; m < n_cameras; ++m)
        if (!all_finite(intr + 9 * m, 7, &at)) return invalid("intr[" + std::to_string(9 * m + at) + "] is not finite");
    if (!all_finite(board_xy, (size_t)2 * n_points, &at)) return invalid("board_xy[" + std::to_string(at) + "] is not finite");
    for (int m = 0; m < 2 * n_cameras; ++m)
        if (image_size[m] <= 0) return invalid("image_size[" + std::to_string(m) + "] = " + std::to_string(image_size[m]) + " is not positive");
    if (weights)
        for (int k = 0; k < kVgCam * n_cameras; ++k)
            if (!std::isfinite(weights[k]) || weights[k] < 0.0) return invalid("weights[" + std::to_string(k) + "] must be finite and >= 0");
    for (int i = 0; i < n_candidates; ++i) {
        const tscm_view_candidate &q = candidates[i];
        const std::string where = "candidates[" + std::to_string(i) + "]: ";
        if (q.camera_a < 0 || q.camera_a >= n_cameras) return invalid(where + "camera_a " + std::to_string(q.camera_a) + " out of range");
        if (q.camera_b < 0 || q.camera_b >= n_cameras) return invalid(where + "camera_b " + std::to_string(q.camera_b) + " out of range");
        if (!all_finite(q.board_rt, 6, &at)) return invalid(where + "board_rt[" + std::to_string(at) + "] is not finite");
    }
    return 0;
}

// both entry points; cam_cov_out != NULL: the apply call (n_candidates == 1)
int run(int n_cameras, const double *cam_rt, const double *intr, const double *cam_cov, const double *weights, int n_points, const double *board_xy,
        const int *image_size, const tscm_view_gain_params *params, const tscm_view_candidate *candidates, int n_candidates, int device, const char *who,
        double *gain_logdet, double *gain_trace, int *n_visible, int *flags, double *cam_cov_out)
{
    if (int rc = select_device(device, who)) return rc;
    const int C = n_cameras, R = n_candidates, n15 = kVgCam * C;
    std::map<std::pair<int, int>, int> index;
    std::vector<int> pairs;
    std::vector<VgCandidate> cand(R);
    std::vector<int> list[2];
    for (int i = 0; i < R; ++i) {
        const tscm_view_candidate &q = candidates[i];
        const auto key = std::make_pair(q.camera_a, q.camera_b);
        auto it = index.find(key);
        if (it == index.end()) {
            it = index.emplace(key, (int)index.size()).first;
            pairs.push_back(q.camera_a);
            pairs.push_back(q.camera_b);
        }
        cand[i].a = q.camera_a; cand[i].b = q.camera_b; cand[i].pair = it->second; cand[i].pad = 0;
        std::memcpy(cand[i].rt, q.board_rt, sizeof(double) * 6);
        list[q.camera_a != q.camera_b ? 1 : 0].push_back(i);
    }
    const int n_pairs = (int)index.size();
    DeviceMem mem;
    EventSpan span;
    const double *d_rt = nullptr, *d_intr = nullptr, *d_cov = nullptr, *d_w = nullptr, *d_xy = nullptr;
    const int *d_size = nullptr, *d_pairs = nullptr, *d_list[2] = { nullptr, nullptr };
    const VgCandidate *d_cand = nullptr;
    double *d_G = nullptr, *d_Q = nullptr, *d_gains = nullptr, *d_K = nullptr, *d_out = nullptr;
    int *d_bad = nullptr, *d_nvis = nullptr, *d_flags = nullptr;
    HIP_TRY(mem.upload(&d_rt, cam_rt, (size_t)6 * C));
    HIP_TRY(mem.upload(&d_intr, intr, (size_t)9 * C));
    HIP_TRY(mem.upload(&d_cov, cam_cov, (size_t)n15 * n15));
    if (weights) HIP_TRY(mem.upload(&d_w, weights, (size_t)n15));
    HIP_TRY(mem.upload(&d_xy, board_xy, (size_t)2 * n_points));
    HIP_TRY(mem.upload(&d_size, image_size, (size_t)2 * C));
    HIP_TRY(mem.upload(&d_pairs, pairs));
    HIP_TRY(mem.upload(&d_cand, cand));
    for (int t = 0; t < 2; ++t) HIP_TRY(mem.upload(&d_list[t], list[t]));
    HIP_TRY(mem.alloc(&d_G, (size_t)kVgPrepStride * n_pairs));
    HIP_TRY(mem.alloc(&d_Q, (size_t)kVgPrepStride * n_pairs));
    HIP_TRY(mem.alloc(&d_bad, (size_t)n_pairs));
    HIP_TRY(mem.alloc(&d_gains, (size_t)2 * R));
    HIP_TRY(mem.alloc(&d_nvis, (size_t)2 * R));
    HIP_TRY(mem.alloc(&d_flags, (size_t)R));
    if (cam_cov_out) {
        HIP_TRY(mem.alloc(&d_K, (size_t)kVgPrepStride));
        HIP_TRY(mem.alloc(&d_out, (size_t)n15 * n15));
    }
    HIP_TRY(span.create(3));
    HIP_TRY(span.mark(0));
    hipLaunchKernelGGL(k_view_prepare, dim3(n_pairs), dim3(kVgWave), 0, 0, d_cov, d_w, n15, d_pairs, d_G, d_Q, d_bad);
    if (!list[0].empty())
        hipLaunchKernelGGL(k_view_gain<kVgTheta>, dim3((unsigned)list[0].size()), dim3(kVgWave), 0, 0, d_rt, d_intr, d_xy, n_points, d_size, params->border,
                           params->min_corners, d_cand, d_list[0], d_G, d_Q, d_bad, d_gains, d_nvis, d_flags, d_K);
    if (!list[1].empty())
        hipLaunchKernelGGL(k_view_gain<kVgMax>, dim3((unsigned)list[1].size()), dim3(kVgWave), 0, 0, d_rt, d_intr, d_xy, n_points, d_size, params->border,
                           params->min_corners, d_cand, d_list[1], d_G, d_Q, d_bad, d_gains, d_nvis, d_flags, d_K);
    double stage[2] = { 0.0, 0.0 }, seconds = 0.0;
    HIP_TRY(span.finish(1, stage, &seconds));
    std::vector<double> gains((size_t)2 * R);
    HIP_TRY(hipMemcpy(gains.data(), d_gains, sizeof(double) * gains.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n_visible, d_nvis, sizeof(int) * 2 * (size_t)R, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(flags, d_flags, sizeof(int) * (size_t)R, hipMemcpyDeviceToHost));
    for (int i = 0; i < R; ++i) { gain_logdet[i] = gains[2 * (size_t)i]; gain_trace[i] = gains[2 * (size_t)i + 1]; }
    if (cam_cov_out) {
        const size_t nn = (size_t)n15 * n15;
        if (flags[0] & 8) {
            for (size_t i = 0; i < nn; ++i) cam_cov_out[i] = std::nan("");
        } else if (!(flags[0] & 3)) {
            std::memcpy(cam_cov_out, cam_cov, sizeof(double) * nn);
        } else {
            const int a = candidates[0].camera_a, b = candidates[0].camera_b;
            const long long total = (long long)n15 * (n15 + 1) / 2;
            HIP_TRY(span.mark(1));
            hipLaunchKernelGGL(k_view_apply, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, d_cov, n15, a, b, a != b ? kVgMax : kVgTheta, d_K, d_out);
            double more = 0.0;
            HIP_TRY(span.finish(2, stage, &more));
            seconds += stage[1];
            HIP_TRY(hipMemcpy(cam_cov_out, d_out, sizeof(double) * nn, hipMemcpyDeviceToHost));
        }
    }
    g_last_kernel_seconds = seconds;
    return 0;
}

}  // namespace

extern "C" int tscm_view_gain(int n_cameras, const double *cam_rt, const double *intr, const double *cam_cov, const double *weights, int n_points,
                              const double *board_xy, const int *image_size, const tscm_view_gain_params *params, const tscm_view_candidate *candidates,
                              int n_candidates, int device, double *gain_logdet, double *gain_trace, int *n_visible, int *flags)
{
    g_last_kernel_seconds = 0.0;
    if (int rc = check_args(n_cameras, cam_rt, intr, cam_cov, weights, n_points, board_xy, image_size, params, candidates, n_candidates, gain_logdet, gain_trace,
                            n_visible, flags))
        return rc;
    return run(n_cameras, cam_rt, intr, cam_cov, weights, n_points, board_xy, image_size, params, candidates, n_candidates, device, "tscm_view_gain", gain_logdet,
               gain_trace, n_visible, flags, nullptr);
}

extern "C" int tscm_view_gain_apply(int n_cameras, const double *cam_rt, const double *intr, const double *cam_cov, const double *weights, int n_points,
                                    const double *board_xy, const int *image_size, const tscm_view_gain_params *params, const tscm_view_candidate *candidate,
                                    int device, double *gain_logdet, double *gain_trace, int *n_visible, int *flags, double *cam_cov_out)
{
    g_last_kernel_seconds = 0.0;
    if (!candidate) return invalid("candidate is NULL");
    if (!cam_cov_out) return invalid("cam_cov_out is NULL");
    if (int rc = check_args(n_cameras, cam_rt, intr, cam_cov, weights, n_points, board_xy, image_size, params, candidate, 1, gain_logdet, gain_trace, n_visible,
                            flags))
        return rc;
    return run(n_cameras, cam_rt, intr, cam_cov, weights, n_points, board_xy, image_size, params, candidate, 1, device, "tscm_view_gain_apply", gain_logdet,
               gain_trace, n_visible, flags, cam_cov_out);
}

extern "C" double tscm_view_gain_seconds(void) { return g_last_kernel_seconds; }
