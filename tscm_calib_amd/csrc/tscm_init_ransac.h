// tscm_init_ransac.h -- k_estimate_extrinsic_ransac: the consensus search and masked refit behind
// tscm_estimate_extrinsic_ransac (definition: tscm.h, "outlier-tolerant pose initialisation").  One wave per view:
//   setup   lanes over corners: un-project, turn, keep u, v, x, y (4 doubles) and the usable flag of every corner in LDS;
//   search  lane = hypothesis, rounds of 64: integer sample, closed-form homography in registers, one walk over the
//           LDS corners (every lane reads the same corner: a broadcast), running best (score, h), butterfly reduction;
//   refit   lanes over the winner's inliers: tscm_planar_pose.h's fit with the wave's lane policy, every sum of the DLT and
//           of each Gauss-Newton step a per-lane partial in corner order i = lane, lane + 64, ... followed by the same xor
//           butterfly.  The 8x8 and 6x6 systems are factored by every lane on identical values: the time of one lane, and
//           no broadcast of the solution.
#pragma once

#include "tscm_planar_pose.h"

namespace {

constexpr int kRansacMaxPoints = 1024;       // 32 x 32 corners (kMaxBoardW squared): 34 KiB of LDS at the cap
constexpr int kRansacMaxHypotheses = 4096;
// per-view stage record of the STAGES instantiation: T | H_best | H_refit | rv0 t0 | rv t | GN steps | rms_px
constexpr int kRansacRec = 41, kRansacT = 0, kRansacHBest = 9, kRansacRmsPx = 40;

// MurmurHash3's 32-bit finaliser (fmix32)
__device__ __forceinline__ unsigned ransac_mix(unsigned h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// draw d of hypothesis h of view k: position d + ((word * (n - d)) >> 32) of a partial Fisher-Yates shuffle of 0 .. n-1.
// The shuffled array is never formed: mp/mv record the at most 4 positions a swap has written.
__device__ __forceinline__ void ransac_sample(unsigned seed, unsigned k, unsigned h, int n, int s[4])
{
    const unsigned base = ransac_mix(ransac_mix(ransac_mix(seed + 0x9e3779b9u) + k) + h);
    int mp[4], mv[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const unsigned r = ransac_mix(base + (unsigned)d);
        const int j = d + (int)(((unsigned long long)r * (unsigned)(n - d)) >> 32);
        int vj = j, vd = d;
#pragma unroll
        for (int e = 0; e < d; ++e) {
            if (mp[e] == j) vj = mv[e];
            if (mp[e] == d) vd = mv[e];
        }
        s[d] = vj; mp[d] = j; mv[d] = vd;
    }
}

// three of the four lattice points (i mod w, i div w) on one line
__device__ __forceinline__ bool ransac_collinear(const int s[4], int board_w)
{
    int cx[4], cy[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { cx[j] = s[j] % board_w; cy[j] = s[j] / board_w; }
    bool any = false;
#pragma unroll
    for (int skip = 0; skip < 4; ++skip) {
        const int a = skip == 0 ? 1 : 0, b = skip <= 1 ? 2 : 1, c = skip <= 2 ? 3 : 2;
        any |= (cx[b] - cx[a]) * (cy[c] - cy[a]) - (cy[b] - cy[a]) * (cx[c] - cx[a]) == 0;
    }
    return any;
}

// c_j = p_{j+1} x p_{j+2} (j cyclic over the first three points, p = (X, Y, 1)) and lam_j = c_j . p_4
__device__ __forceinline__ void ransac_basis(const double px[4], const double py[4], double c[9], double lam[3])
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int a = (j + 1) % 3, b = (j + 2) % 3;
        c[3 * j] = py[a] - py[b]; c[3 * j + 1] = px[b] - px[a]; c[3 * j + 2] = px[a] * py[b] - px[b] * py[a];
        lam[j] = c[3 * j] * px[3] + c[3 * j + 1] * py[3] + c[3 * j + 2];
    }
}

// H = sum_j g_j q_j c_j^T, g_j = mu_j lam_{j+1} lam_{j+2}: the map through the two projective bases (board points p
// with c, lam; normalised corners q with mu), negated where it sends the first sampled board point behind the camera
__device__ __forceinline__ void ransac_homography(const double X[4], const double Y[4], const double x[4], const double y[4], double H[9])
{
    double c[9], lam[3], d[9], mu[3];
    ransac_basis(X, Y, c, lam);
    ransac_basis(x, y, d, mu);
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double g = mu[j] * (lam[(j + 1) % 3] * lam[(j + 2) % 3]);
        const double q[3] = { g * x[j], g * y[j], g };
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) H[3 * r + cc] += q[r] * c[3 * j + cc];
    }
    if (H[6] * X[0] + H[7] * Y[0] + H[8] < 0.0)
#pragma unroll
        for (int i = 0; i < 9; ++i) H[i] = -H[i];
}

// the score's test of one corner: usable, in front, and within thr2 = threshold_px^2 of the pixel through the full model
__device__ __forceinline__ bool ransac_inlier(const double *H, const double *T, const double *I, double X, double Y, double u, double v, bool usable, double thr2)
{
    const double a = H[0] * X + H[1] * Y + H[2], b = H[3] * X + H[4] * Y + H[5], w = H[6] * X + H[7] * Y + H[8];
    if (!(usable && w > 0.0)) return false;
    const double xn = a / w, yn = b / w;
    const double rx = T[0] * xn + T[3] * yn + T[6], ry = T[1] * xn + T[4] * yn + T[7], rz = T[2] * xn + T[5] * yn + T[8];   // T^T (xn, yn, 1)
    double pu, pv;
    tscm::project_point(I, rx, ry, rz, pu, pv);
    const double du = u - pu, dv = v - pv;
    return du * du + dv * dv <= thr2;
}

__device__ __forceinline__ void ransac_sampled_homography(unsigned seed, int k, int h, int n, const double *__restrict__ worlds, const double *sx, const double *sy, double H[9])
{
    int s[4];
    ransac_sample(seed, (unsigned)k, (unsigned)h, n, s);
    double X[4], Y[4], x[4], y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { X[j] = worlds[3 * s[j]]; Y[j] = worlds[3 * s[j] + 1]; x[j] = sx[s[j]]; y[j] = sy[s[j]]; }
    ransac_homography(X, Y, x, y, H);
}

// grid = views, block = one wave, dynamic LDS = 34 n bytes (rounded up to 8).  inlier [V][n] arrives zeroed, samples /
// score arrive as -1 and the stage records as NaN; Rt holds the caller's values.  STAGES = false: samples, score, winner
// and stage are not touched.
template <bool STAGES>
__global__ __launch_bounds__(64) void k_estimate_extrinsic_ransac(const double *__restrict__ intr, const double *__restrict__ pu, const double *__restrict__ pv,
                                                                  const int *__restrict__ count, const double *__restrict__ worlds, int n, int board_w,
                                                                  double thr2, int n_hyp, int min_inliers, unsigned seed,
                                                                  double *__restrict__ Rt_out, unsigned char *__restrict__ inlier, int *__restrict__ n_inliers,
                                                                  int *__restrict__ code_out, int *__restrict__ samples, int *__restrict__ score_out,
                                                                  int *__restrict__ winner_out, double *__restrict__ stage_out)
{
    extern __shared__ double sm[];
    double *su = sm, *sv = sm + n, *sx = sm + 2 * n, *sy = sm + 3 * n;
    unsigned char *sok = reinterpret_cast<unsigned char *>(sm + 4 * n), *smask = sok + n;
    const int k = blockIdx.x, lane = threadIdx.x;
    double *stage = STAGES ? stage_out + (size_t)kRansacRec * k : nullptr;
    auto leave = [&](int code, int inl) {
        if (lane == 0) { code_out[k] = code; n_inliers[k] = inl; }
    };
    if (STAGES && lane == 0) winner_out[k] = -1;
    if (count[k] == 0) { leave(TSCM_EXTRINSIC_NO_BOARD, 0); return; }
    double I[9];
    for (int i = 0; i < 9; ++i) I[i] = intr[i];
    const double *u = pu + (size_t)k * n, *v = pv + (size_t)k * n;
    const int ref = n / 2 - board_w / 2 - 1;
    double T[9];
    tscm::look_at_turn(I, u[ref], v[ref], T);
    if (STAGES && lane == 0)
        for (int i = 0; i < 9; ++i) stage[kRansacT + i] = T[i];
    // ---- setup: lanes over corners
    for (int i = lane; i < n; i += 64) {
        const double ui = u[i], vi = v[i];
        double x, y, Z;
        tscm::turned_corner(I, T, ui, vi, x, y, Z);
        su[i] = ui; sv[i] = vi; sx[i] = x; sy[i] = y;
        sok[i] = isfinite(ui) && isfinite(vi) && isfinite(x) && isfinite(y) && Z > 0.0;
    }
    __syncthreads();
    // ---- search: lane = hypothesis
    int best_s = -2, best_h = 0x7fffffff;
    for (int h0 = 0; h0 < n_hyp; h0 += 64) {
        const int h = h0 + lane;
        if (h >= n_hyp) continue;
        int s[4];
        ransac_sample(seed, (unsigned)k, (unsigned)h, n, s);
        const bool ok = sok[s[0]] && sok[s[1]] && sok[s[2]] && sok[s[3]] && !ransac_collinear(s, board_w);
        int sc = -1;
        if (ok) {
            double X[4], Y[4], x[4], y[4], H[9];
#pragma unroll
            for (int j = 0; j < 4; ++j) { X[j] = worlds[3 * s[j]]; Y[j] = worlds[3 * s[j] + 1]; x[j] = sx[s[j]]; y[j] = sy[s[j]]; }
            ransac_homography(X, Y, x, y, H);
            sc = 0;
            for (int i = 0; i < n; ++i) sc += ransac_inlier(H, T, I, worlds[3 * i], worlds[3 * i + 1], su[i], sv[i], sok[i] != 0, thr2) ? 1 : 0;
        }
        if constexpr (STAGES) {
            const size_t o = (size_t)k * n_hyp + h;
            score_out[o] = sc;
            if (ok)
                for (int j = 0; j < 4; ++j) samples[4 * o + j] = s[j];
        }
        if (sc > best_s) { best_s = sc; best_h = h; }               // rounds ascend in h: a tie keeps the lower one
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int os = __shfl_xor(best_s, off), oh = __shfl_xor(best_h, off);
        if (os > best_s || (os == best_s && oh < best_h)) { best_s = os; best_h = oh; }
    }
    if (best_s < 0) { leave(TSCM_EXTRINSIC_NO_HYPOTHESIS, 0); return; }
    double Hb[9];
    ransac_sampled_homography(seed, k, best_h, n, worlds, sx, sy, Hb);
    if constexpr (STAGES) {
        if (lane == 0) {
            winner_out[k] = best_h;
            double f = 0.0;
            for (int i = 0; i < 9; ++i) f += Hb[i] * Hb[i];
            f = sqrt(f);
            for (int i = 0; i < 9; ++i) stage[kRansacHBest + i] = Hb[i] / f;     // unit Frobenius norm (the score does not depend on the scale)
        }
    }
    if (best_s < min_inliers) { leave(TSCM_EXTRINSIC_FEW_INLIERS, 0); return; }
    // ---- the winner's mask: lanes over corners from here on
    unsigned char *mask = inlier + (size_t)k * n;
    int m = 0;
    for (int i = lane; i < n; i += 64) {
        const bool in = ransac_inlier(Hb, T, I, worlds[3 * i], worlds[3 * i + 1], su[i], sv[i], sok[i] != 0, thr2);
        smask[i] = in; mask[i] = in; m += in;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
    __syncthreads();
    // ---- refit: the planar pose fit on the masked corners, every sum over the wave
    auto inlier_corner = [&](int i, double &x, double &y) {
        if (!smask[i]) return false;
        x = sx[i]; y = sy[i];
        return true;
    };
    double rv[3], t[3];
    const int code = tscm::fit_planar_pose(tscm::WaveLanes{}, inlier_corner, m, worlds, n, lane == 0 ? stage : nullptr, rv, t);
    if (code >= TSCM_EXTRINSIC_CONVERGED) {
        double R[9], dR[27];
        tscm::rotation_and_derivatives(rv, R, dR);
        if constexpr (STAGES) {
            // pixel RMS of the masked corners at the refit pose, through the full model
            double e2 = 0.0;
            for (int i = lane; i < n; i += 64) {
                if (!smask[i]) continue;
                const double wx = worlds[3 * i], wy = worlds[3 * i + 1];
                const double PX = R[0] * wx + R[1] * wy + t[0], PY = R[3] * wx + R[4] * wy + t[1], PZ = R[6] * wx + R[7] * wy + t[2];
                const double rx = T[0] * PX + T[3] * PY + T[6] * PZ, ry = T[1] * PX + T[4] * PY + T[7] * PZ, rz = T[2] * PX + T[5] * PY + T[8] * PZ;
                double qu, qv;
                tscm::project_point(I, rx, ry, rz, qu, qv);
                const double du = su[i] - qu, dv = sv[i] - qv;
                e2 += du * du + dv * dv;
            }
            e2 = tscm::WaveLanes::sum(e2);
            if (lane == 0) stage[kRansacRmsPx] = sqrt(e2 / m);
        }
        if (lane == 0) tscm::compose_rt(T, R, t, Rt_out + 9 * (size_t)k);
    }
    leave(code, m);
}

}  // namespace
