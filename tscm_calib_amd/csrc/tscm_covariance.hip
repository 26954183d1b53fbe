// tscm_covariance.hip -- parameter covariance of a calibration (tscm.h: tscm_covariance*): Ceres' convention
// Sigma = (J^T J)^-1 over the free columns, from the Schur-form normal equations in the host layout of
// tscm_eval_normal_equations_robust.  With B_i = board_gram[i], W_v = view_cross[v] on the free camera columns,
// Z_v = B_i^-1 W_v:
//   S = blockdiag(cam_gram) - sum_i sum_{v,v' of board i} W_v^T Z_v'     Sigma_cc = S^-1
//   Sigma_bb,i = B_i^-1 + sum_{v,v' of board i} Z_v Sigma_cc[m_v, m_v'] Z_v'^T
// All fp64, no floating-point atomics, every sum in an order fixed by the host plan (tscm_cov_plan.h), so two calls on
// the same input give the same bytes.
//
//   k_cov_boards        a workgroup per kCovBoardGroup free boards.  One thread per board factors the 6 x 6 block in
//                       registers (Cholesky, then B^-1 = L^-T L^-1, symmetric by construction) and leaves B^-1 in LDS and
//                       in global memory; then all threads form Z_v, one (view, column) per thread and step.  A pivot that
//                       is not > 0 puts the board's index into status[0] by an integer atomicMin (order-independent).
//   k_cov_schur         a workgroup per chunk of a camera-pair tile's (v, v') list.  Thread (i, j) of 15 x 15 adds
//                       W_v[:, i] . Z_v'[:, j] in list order, eight pairs staged in LDS at a time; the partial tile goes to
//                       scratch.
//   k_cov_schur_reduce  a workgroup per ordered camera pair: sums the tile's chunks in chunk order, subtracts from cam_gram
//                       (diagonal pairs), writes the 15-wide S; pairs (b, a), a < b, read the tile transposed.
//   k_cov_reduced       ONE workgroup: gathers the free columns' lower triangle, scales it to unit diagonal, factors it in
//                       place in global scratch (right-looking Cholesky, panels of 8: the diagonal block in LDS, a row per
//                       thread for the panel, 4 x 4 register tiles for the trailing update), inverts the factor a column per
//                       thread, forms L^-T L^-1 in 4 x 4 register tiles, undoes the scaling and scatters into the 15-wide
//                       matrix (zero elsewhere).  The first pivot that is not > 0 goes to status[1], the smallest pivot to
//                       *min_pivot.
//   k_cov_marginals     a one-wave workgroup per free board: for every (v, v') first T = Z_v Sigma_cc[m_v, m_v'] (6 x 15,
//                       through LDS), then T Z_v'^T; the sum is symmetrised and added to B^-1.
// Every index a kernel uses comes from the host plan; a singular block only produces NaN values, never another address.
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_cov_plan.h"
#include "tscm_host.h"
#include "tscm_layout.h"

#include <climits>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

using namespace tscm;

namespace {

constexpr int kPanel = 8;            // k_cov_reduced: panel width (16 spills: a panel row and the block's reads in registers)
constexpr int kReducedThreads = 1024;
constexpr int kStage = 8;            // k_cov_schur: pairs staged in LDS at a time

__global__ __launch_bounds__(256) void k_cov_boards(const double *__restrict__ board_gram, const double *__restrict__ view_cross,
                                                    const unsigned char *__restrict__ cam_free, const int *__restrict__ view_camera,
                                                    const int *__restrict__ free_boards, const int *__restrict__ board_start,
                                                    const int *__restrict__ board_views, const int *__restrict__ view_slot, int nfb,
                                                    double *__restrict__ binv, double *__restrict__ Z, int *__restrict__ status)
{
    __shared__ double sB[kCovBoardGroup][36];
    const int tid = threadIdx.x, s0 = blockIdx.x * kCovBoardGroup, s1 = min(nfb, s0 + kCovBoardGroup);
    if (tid < kCovBoardGroup && s0 + tid < s1) {
        const int board = free_boards[s0 + tid];
        const double *g = board_gram + 36 * (size_t)board;
        double L[6][6], M[6][6];
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) L[i][j] = g[6 * i + j];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            double d = L[k][k];
#pragma unroll
            for (int q = 0; q < k; ++q) d -= L[k][q] * L[k][q];
            bad = bad || !(d > 0.0);
            const double piv = sqrt(d);
            L[k][k] = piv;
#pragma unroll
            for (int i = k + 1; i < 6; ++i) {
                double x = L[i][k];
#pragma unroll
                for (int q = 0; q < k; ++q) x -= L[i][q] * L[k][q];
                L[i][k] = x / piv;
            }
        }
        // M = L^-1 (lower), column by column
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            M[j][j] = 1.0 / L[j][j];
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double x = 0.0;
#pragma unroll
                for (int q = j; q < i; ++q) x += L[i][q] * M[q][j];
                M[i][j] = -x / L[i][i];
            }
        }
        // B^-1 = M^T M
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double x = 0.0;
#pragma unroll
                for (int q = i; q < 6; ++q) x += M[q][i] * M[q][j];
                sB[tid][6 * i + j] = x;
                sB[tid][6 * j + i] = x;
            }
        if (bad) atomicMin(&status[0], board);
#pragma unroll
        for (int e = 0; e < 36; ++e) binv[36 * (size_t)(s0 + tid) + e] = sB[tid][e];
    }
    __syncthreads();
    const int lo = board_start[s0], n_items = (board_start[s1] - lo) * kCovCam;
    for (int item = tid; item < n_items; item += 256) {
        const int k = lo + item / kCovCam, j = item % kCovCam;
        const int v = board_views[k], s = view_slot[k] - s0;
        const bool is_free = cam_free[view_camera[v] * kCovCam + j] != 0;
        const double *w = view_cross + 90 * (size_t)v + j;
        double x[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) x[r] = is_free ? w[kCovCam * r] : 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double z = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) z += sB[s][6 * i + r] * x[r];
            Z[90 * (size_t)v + kCovCam * i + j] = z;
        }
    }
}

__global__ __launch_bounds__(256) void k_cov_schur(const double *__restrict__ view_cross, const double *__restrict__ Z,
                                                   const int *__restrict__ pair_v, const int *__restrict__ pair_w,
                                                   const int *__restrict__ chunk_begin, const int *__restrict__ chunk_end,
                                                   double *__restrict__ partial)
{
    __shared__ double sW[kStage][90], sZ[kStage][90];
    const int tid = threadIdx.x, i = tid / kCovCam, j = tid % kCovCam;
    const int e0 = chunk_begin[blockIdx.x], e1 = chunk_end[blockIdx.x];
    double acc = 0.0;
    for (int base = e0; base < e1; base += kStage) {
        const int n = min(kStage, e1 - base);
        for (int q = tid; q < n * 180; q += 256) {
            const int p = q / 180, r = q % 180;
            if (r < 90) sW[p][r] = view_cross[90 * (size_t)pair_v[base + p] + r];
            else sZ[p][r - 90] = Z[90 * (size_t)pair_w[base + p] + r - 90];
        }
        __syncthreads();
        if (tid < 225)
            for (int p = 0; p < n; ++p)
#pragma unroll
                for (int r = 0; r < 6; ++r) acc += sW[p][kCovCam * r + i] * sZ[p][kCovCam * r + j];
        __syncthreads();
    }
    if (tid < 225) partial[225 * (size_t)blockIdx.x + tid] = acc;
}

__global__ __launch_bounds__(256) void k_cov_schur_reduce(const double *__restrict__ cam_gram, const double *__restrict__ partial,
                                                          const int *__restrict__ tile_of, const int *__restrict__ tile_chunk, int C,
                                                          double *__restrict__ S)
{
    const int tid = threadIdx.x;
    if (tid >= 225) return;
    const int a = blockIdx.x / C, b = blockIdx.x % C, i = tid / kCovCam, j = tid % kCovCam;
    const int t = tile_of[min(a, b) * C + max(a, b)];
    double val = a == b ? cam_gram[225 * (size_t)a + tid] : 0.0;
    if (t >= 0) {
        const int e = a <= b ? tid : kCovCam * j + i;
        double s = 0.0;
        for (int c = tile_chunk[t]; c < tile_chunk[t + 1]; ++c) s += partial[225 * (size_t)c + e];
        val -= s;
    }
    S[(size_t)(kCovCam * a + i) * (kCovCam * C) + kCovCam * b + j] = val;
}

// A and Linv: n x n row-major scratch (Linv zeroed by the host), cov: (15 C)^2, zeroed by the host
__global__ __launch_bounds__(kReducedThreads) void k_cov_reduced(const double *__restrict__ S, const int *__restrict__ wide_of, int n, int n15,
                                                                 double *__restrict__ A, double *__restrict__ Linv, double *__restrict__ cov,
                                                                 int *__restrict__ status, double *__restrict__ min_pivot)
{
    __shared__ double sD[kPanel][kPanel + 1];
    __shared__ double sScale[kCovMaxCam * kCovCamFree];
    __shared__ int sBad;
    __shared__ double sMin;
    const int tid = threadIdx.x, NT = kReducedThreads;
    if (tid == 0) { sBad = INT_MAX; sMin = 1.0; }
    for (int p = tid; p < n; p += NT) {
        const double d = S[(size_t)wide_of[p] * n15 + wide_of[p]];
        sScale[p] = d > 0.0 ? 1.0 / sqrt(d) : __builtin_nan("");
    }
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += NT) {
        const int p = idx / n, q = idx % n;
        if (q < p) A[idx] = S[(size_t)wide_of[p] * n15 + wide_of[q]] * sScale[p] * sScale[q];
        else if (q == p) A[idx] = sScale[p] == sScale[p] ? 1.0 : __builtin_nan("");
    }
    // ---- A = L L^T in place, panels of kPanel columns
    const int dr = tid / kPanel, dc = tid % kPanel;
    for (int k0 = 0; k0 < n; k0 += kPanel) {
        const int w = min(kPanel, n - k0);
        __syncthreads();
        if (tid < kPanel * kPanel) sD[dr][dc] = dr < w && dc <= dr ? A[(size_t)(k0 + dr) * n + k0 + dc] : (dr == dc ? 1.0 : 0.0);
        __syncthreads();
        for (int kk = 0; kk < w; ++kk) {
            if (tid == 0) {
                const double piv = sD[kk][kk];
                if (sBad == INT_MAX) {
                    if (!(piv > 0.0)) { sBad = k0 + kk; sMin = piv; }
                    else if (piv < sMin) sMin = piv;
                }
                sD[kk][kk] = sqrt(piv);
            }
            __syncthreads();
            if (tid > kk && tid < w) sD[tid][kk] /= sD[kk][kk];
            __syncthreads();
            if (tid < kPanel * kPanel && dc > kk && dc <= dr && dr < w) sD[dr][dc] -= sD[dr][kk] * sD[dc][kk];
            __syncthreads();
        }
        if (tid < kPanel * kPanel && dr < w && dc <= dr) A[(size_t)(k0 + dr) * n + k0 + dc] = sD[dr][dc];
        // the panel below the diagonal block: row r times L_kk^-T (padding of sD: the identity)
        for (int r = k0 + w + tid; r < n; r += NT) {
            asm volatile("" ::: "memory");                   // sD is read per row: hoisted out of this loop it stays in registers
            double x[kPanel];
#pragma unroll
            for (int c = 0; c < kPanel; ++c) x[c] = c < w ? A[(size_t)r * n + k0 + c] : 0.0;
#pragma unroll
            for (int c = 0; c < kPanel; ++c) {
                double s = x[c];
#pragma unroll
                for (int k = 0; k < c; ++k) s -= x[k] * sD[c][k];
                x[c] = s / sD[c][c];
            }
#pragma unroll
            for (int c = 0; c < kPanel; ++c) if (c < w) A[(size_t)r * n + k0 + c] = x[c];
        }
        __syncthreads();
        // trailing update, lower triangle, 4 x 4 tiles
        const int base = k0 + w, mt = (n - base + 3) / 4;
        for (int idx = tid; idx < mt * mt; idx += NT) {
            const int tr = idx / mt, tc = idx % mt;
            if (tc > tr) continue;
            const int r0 = base + 4 * tr, c0 = base + 4 * tc;
            double acc[4][4] = {};
#pragma unroll
            for (int kk = 0; kk < kPanel; ++kk) {            // (a trailing matrix exists only behind a full panel: w == kPanel)
                double lr[4], lc[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    lr[a] = r0 + a < n ? A[(size_t)(r0 + a) * n + k0 + kk] : 0.0;
                    lc[a] = c0 + a < n ? A[(size_t)(c0 + a) * n + k0 + kk] : 0.0;
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[a][b] += lr[a] * lc[b];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (r0 + a < n && c0 + b <= r0 + a) A[(size_t)(r0 + a) * n + c0 + b] -= acc[a][b];
        }
    }
    __syncthreads();
    if (tid == 0) { status[1] = sBad; *min_pivot = sMin; }
    // ---- Linv = L^-1, column j on thread j; the rows above the wave's first column are zero
    if (tid < n) {
        const int j = tid, kstart = j & ~63;
        for (int r = kstart; r < n; ++r) {
            // four partial sums, eight loads in flight: one sum in one chain waits a memory round trip per term
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            const double *a = A + (size_t)r * n, *x = Linv + j;
            int k = kstart;
            for (; k + 4 <= r; k += 4) {
                s0 += a[k] * x[(size_t)k * n];
                s1 += a[k + 1] * x[(size_t)(k + 1) * n];
                s2 += a[k + 2] * x[(size_t)(k + 2) * n];
                s3 += a[k + 3] * x[(size_t)(k + 3) * n];
            }
            for (; k < r; ++k) s0 += a[k] * x[(size_t)k * n];
            const double s = (s0 + s1) + (s2 + s3);
            Linv[(size_t)r * n + j] = r < j ? 0.0 : ((r == j ? 1.0 : 0.0) - s) / A[(size_t)r * n + r];
        }
    }
    __syncthreads();
    // ---- Sigma = Linv^T Linv on the lower triangle, scaling undone, scattered to both triangles of the 15-wide matrix
    const int mt = (n + 3) / 4;
    for (int idx = tid; idx < mt * mt; idx += NT) {
        const int tr = idx / mt, tc = idx % mt;
        if (tc > tr) continue;
        const int p0 = 4 * tr, q0 = 4 * tc;
        double acc[4][4] = {};
#pragma unroll 4
        for (int r = p0; r < n; ++r) {
            double lp[4], lq[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                lp[a] = p0 + a < n ? Linv[(size_t)r * n + p0 + a] : 0.0;
                lq[a] = q0 + a < n ? Linv[(size_t)r * n + q0 + a] : 0.0;
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] += lp[a] * lq[b];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int p = p0 + a, q = q0 + b;
                if (p < n && q <= p) {
                    const double x = acc[a][b] * sScale[p] * sScale[q];
                    cov[(size_t)wide_of[p] * n15 + wide_of[q]] = x;
                    cov[(size_t)wide_of[q] * n15 + wide_of[p]] = x;
                }
            }
    }
}

__global__ __launch_bounds__(64) void k_cov_marginals(const double *__restrict__ binv, const double *__restrict__ Z, const double *__restrict__ cov,
                                                      const int *__restrict__ view_camera, const int *__restrict__ free_boards,
                                                      const int *__restrict__ board_start, const int *__restrict__ board_views, int n15,
                                                      double *__restrict__ board_cov)
{
    __shared__ double sZv[90], sZw[90], sT[90], sM[36];
    const int tid = threadIdx.x, s = blockIdx.x, i = tid / 6, j = tid % 6;
    const int lo = board_start[s], hi = board_start[s + 1];
    double acc = 0.0;
    for (int a = lo; a < hi; ++a) {
        const int v = board_views[a], mv = view_camera[v];
        for (int b = lo; b < hi; ++b) {
            const int w = board_views[b], mw = view_camera[w];
            for (int q = tid; q < 90; q += 64) { sZv[q] = Z[90 * (size_t)v + q]; sZw[q] = Z[90 * (size_t)w + q]; }
            __syncthreads();
            for (int q = tid; q < 90; q += 64) {
                const int ti = q / kCovCam, tc = q % kCovCam;
                const double *sc = cov + (size_t)(kCovCam * mv) * n15 + kCovCam * mw + tc;
                double t = 0.0;
#pragma unroll
                for (int c = 0; c < kCovCam; ++c) t += sZv[kCovCam * ti + c] * sc[(size_t)c * n15];
                sT[q] = t;
            }
            __syncthreads();
            if (tid < 36)
#pragma unroll
                for (int c = 0; c < kCovCam; ++c) acc += sT[kCovCam * i + c] * sZw[kCovCam * j + c];
            __syncthreads();
        }
    }
    if (tid < 36) sM[tid] = acc;
    __syncthreads();
    if (tid < 36) board_cov[36 * (size_t)free_boards[s] + tid] = binv[36 * (size_t)s + tid] + 0.5 * (sM[6 * i + j] + sM[6 * j + i]);
}

// ------------------------------------------------------------------------------------------------ host
void reset_info(tscm_covariance_info *info)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    info->status = 0; info->where = -1; info->n_free = 0; info->n_residuals = 0;
    info->cost = 0.0; info->sigma2 = nan; info->min_pivot_ratio = nan;
    for (double &s : info->seconds_kernel) s = 0.0;
}

int check_info(const tscm_covariance_info *info)
{
    if (!info) return tscm_set_error(TSCM_E_INVALID, "info is NULL");
    return check_struct_size(info, "tscm_covariance_info", "info");
}

// The four stages on planned blocks.  cam_cov [(15 C)^2] and board_cov [B * 36] are host arrays (not NULL here); a singular
// block leaves them NaN and sets info->status / where.
int covariance_run(const CovPlan &pl, const int *view_camera, const double *board_gram, const double *view_cross, const double *cam_gram,
                   const unsigned char *cam_free, int device, const char *who, double *cam_cov, double *board_cov, tscm_covariance_info *info)
{
    if (int rc = select_device(device, who)) return rc;
    const int C = pl.C, B = pl.B, V = pl.V, n = pl.n_cam_free, n15 = kCovCam * C;
    const int nfb = (int)pl.free_boards.size(), n_chunks = (int)pl.chunk_begin.size();
    DeviceMem mem;
    EventSpan span;
    const double *d_bg = nullptr, *d_vc = nullptr, *d_cg = nullptr;
    const unsigned char *d_free = nullptr;
    const int *d_cam = nullptr, *d_fb = nullptr, *d_bs = nullptr, *d_bv = nullptr, *d_slot = nullptr, *d_pv = nullptr, *d_pw = nullptr, *d_cb = nullptr,
              *d_ce = nullptr, *d_tile = nullptr, *d_tc = nullptr, *d_wide = nullptr;
    double *d_binv = nullptr, *d_Z = nullptr, *d_part = nullptr, *d_S = nullptr, *d_A = nullptr, *d_Linv = nullptr, *d_cov = nullptr, *d_bcov = nullptr,
           *d_minp = nullptr;
    int *d_status = nullptr;
    HIP_TRY(mem.upload(&d_bg, board_gram, (size_t)36 * B));
    HIP_TRY(mem.upload(&d_vc, view_cross, (size_t)90 * V));
    HIP_TRY(mem.upload(&d_cg, cam_gram, (size_t)225 * C));
    HIP_TRY(mem.upload(&d_free, cam_free, (size_t)n15));
    HIP_TRY(mem.upload(&d_cam, view_camera, (size_t)V));
    HIP_TRY(mem.upload(&d_fb, pl.free_boards));
    HIP_TRY(mem.upload(&d_bs, pl.board_start));
    HIP_TRY(mem.upload(&d_bv, pl.board_views));
    HIP_TRY(mem.upload(&d_slot, pl.view_slot));
    HIP_TRY(mem.upload(&d_pv, pl.pair_v));
    HIP_TRY(mem.upload(&d_pw, pl.pair_w));
    HIP_TRY(mem.upload(&d_cb, pl.chunk_begin));
    HIP_TRY(mem.upload(&d_ce, pl.chunk_end));
    HIP_TRY(mem.upload(&d_tile, pl.tile_of));
    HIP_TRY(mem.upload(&d_tc, pl.tile_chunk));
    HIP_TRY(mem.upload(&d_wide, pl.wide_of));
    HIP_TRY(mem.alloc(&d_binv, (size_t)36 * nfb));
    HIP_TRY(mem.alloc(&d_Z, (size_t)90 * V));
    HIP_TRY(mem.alloc(&d_part, (size_t)225 * n_chunks));
    HIP_TRY(mem.alloc(&d_S, (size_t)n15 * n15));
    HIP_TRY(mem.alloc(&d_A, (size_t)n * n));
    HIP_TRY(mem.alloc(&d_Linv, (size_t)n * n));
    HIP_TRY(mem.alloc(&d_cov, (size_t)n15 * n15));
    HIP_TRY(mem.alloc(&d_bcov, (size_t)36 * B));
    const int status0[2] = { INT_MAX, INT_MAX };
    const double minp0 = 1.0;                                // an empty reduced system: no pivot below its unit diagonal
    HIP_TRY(mem.upload(&d_status, status0, (size_t)2));
    HIP_TRY(mem.upload(&d_minp, &minp0, (size_t)1));
    HIP_TRY(hipMemset(d_Linv, 0, sizeof(double) * std::max<size_t>((size_t)n * n, 1)));
    HIP_TRY(hipMemset(d_cov, 0, sizeof(double) * (size_t)n15 * n15));
    HIP_TRY(hipMemset(d_bcov, 0, sizeof(double) * std::max<size_t>((size_t)36 * B, 1)));
    HIP_TRY(span.create(5));
    HIP_TRY(span.mark(0));
    if (nfb > 0)
        hipLaunchKernelGGL(k_cov_boards, dim3((nfb + kCovBoardGroup - 1) / kCovBoardGroup), dim3(256), 0, 0, d_bg, d_vc, d_free, d_cam, d_fb, d_bs, d_bv, d_slot, nfb,
                           d_binv, d_Z, d_status);
    HIP_TRY(span.mark(1));
    if (n_chunks > 0) hipLaunchKernelGGL(k_cov_schur, dim3(n_chunks), dim3(256), 0, 0, d_vc, d_Z, d_pv, d_pw, d_cb, d_ce, d_part);
    hipLaunchKernelGGL(k_cov_schur_reduce, dim3(C * C), dim3(256), 0, 0, d_cg, d_part, d_tile, d_tc, C, d_S);
    HIP_TRY(span.mark(2));
    if (n > 0) hipLaunchKernelGGL(k_cov_reduced, dim3(1), dim3(kReducedThreads), 0, 0, d_S, d_wide, n, n15, d_A, d_Linv, d_cov, d_status, d_minp);
    HIP_TRY(span.mark(3));
    if (nfb > 0) hipLaunchKernelGGL(k_cov_marginals, dim3(nfb), dim3(64), 0, 0, d_binv, d_Z, d_cov, d_cam, d_fb, d_bs, d_bv, n15, d_bcov);
    HIP_TRY(span.finish(4, info->seconds_kernel, nullptr));
    int status[2];
    HIP_TRY(hipMemcpy(status, d_status, sizeof(status), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&info->min_pivot_ratio, d_minp, sizeof(double), hipMemcpyDeviceToHost));
    info->n_free = pl.n_free;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (status[0] != INT_MAX || status[1] != INT_MAX) {
        info->status = status[0] != INT_MAX ? 1 : 2;
        info->where = status[0] != INT_MAX ? status[0] : pl.wide_of[status[1]];
        if (info->status == 1) info->min_pivot_ratio = nan;
        std::fill(cam_cov, cam_cov + (size_t)n15 * n15, nan);
        std::fill(board_cov, board_cov + (size_t)36 * B, nan);
        return 0;
    }
    HIP_TRY(hipMemcpy(cam_cov, d_cov, sizeof(double) * (size_t)n15 * n15, hipMemcpyDeviceToHost));
    if (B > 0) HIP_TRY(hipMemcpy(board_cov, d_bcov, sizeof(double) * (size_t)36 * B, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" int tscm_covariance_from_normal_equations(int n_cameras, int n_boards, int n_views, const int *view_camera, const int *view_board,
                                                     const double *board_gram, const double *view_cross, const double *cam_gram,
                                                     const unsigned char *cam_free, const unsigned char *board_free, int device, double *cam_cov,
                                                     double *board_cov, tscm_covariance_info *info)
{
    if (int rc = check_info(info)) return rc;
    reset_info(info);
    CovPlan pl;
    std::string err;
    if (int rc = plan_covariance(n_cameras, n_boards, n_views, view_camera, view_board, cam_free, board_free, pl, err)) return tscm_set_error(rc, err);
    if (n_boards > 0 && !board_gram) return tscm_set_error(TSCM_E_INVALID, "board_gram is NULL");
    if (n_views > 0 && !view_cross) return tscm_set_error(TSCM_E_INVALID, "view_cross is NULL");
    if (!cam_gram) return tscm_set_error(TSCM_E_INVALID, "cam_gram is NULL");
    const size_t n15 = (size_t)kCovCam * n_cameras;
    std::vector<double> own_cam, own_board;
    if (!cam_cov) { own_cam.resize(n15 * n15); cam_cov = own_cam.data(); }
    if (!board_cov) { own_board.resize((size_t)36 * n_boards + 1); board_cov = own_board.data(); }
    return covariance_run(pl, view_camera, board_gram, view_cross, cam_gram, cam_free, device, "tscm_covariance_from_normal_equations", cam_cov, board_cov, info);
}

// weights: the problem's corner weights (tscm_solver_set_corner_weights) or NULL -- the blocks are then those of the weighted
// normal equations and a corner with weight 0 is no residual
// priors: camera priors (tscm_solver_set_camera_priors) or NULL -- a prior on a free column is one more residual, in the blocks,
// the cost and n_residuals; on a column that is not free it is nothing
static int covariance_of_problem(const tscm_problem *p, int device, const unsigned short *fixed, const double *weights, int loss_kind, double loss_scale,
                                 const tscm_camera_priors *priors, double *cam_cov, double *board_cov, double *cam_rt_std, double *intr_std, double *board_rt_std, tscm_covariance_info *info)
{
    if (int rc = check_info(info)) return rc;
    reset_info(info);
    if (!p) return tscm_set_error(TSCM_E_INVALID, "problem is NULL");
    if (p->n_cameras < 1 || p->n_cameras > kCovMaxCam) return tscm_set_error(TSCM_E_INVALID, "problem: n_cameras " + std::to_string(p->n_cameras) + " outside 1..32");
    std::string err;
    if (int rc = validate(p, err)) return tscm_set_error(rc, "problem: " + err);
    const int C = p->n_cameras, B = p->n_boards, V = p->n_views;
    if (fixed)
        for (int m = 0; m < C; ++m)
            if (fixed[m] & ~TSCM_FIX_ALL) return tscm_set_error(TSCM_E_INVALID, "fixed[" + std::to_string(m) + "]: unknown bits in a fixed-intrinsics mask (bits 0-8 only)");
    if (loss_kind < TSCM_LOSS_NONE || loss_kind > TSCM_LOSS_CAUCHY) return tscm_set_error(TSCM_E_INVALID, "loss_kind " + std::to_string(loss_kind) + " is not a TSCM_LOSS_* kind");
    if (loss_kind != TSCM_LOSS_NONE && (!std::isfinite(loss_scale) || !(loss_scale > 0.0)))
        return tscm_set_error(TSCM_E_INVALID, "loss_scale must be finite and > 0");
    if (int rc = check_camera_priors(priors, C, err)) return tscm_set_error(rc, err);
    std::vector<unsigned char> cam_free, board_free;
    cov_masks(p, fixed, cam_free, board_free);
    // the priors of the free columns, in the caller's layout: what the evaluation below adds and n_residuals counts.  The
    // evaluation's solver has no mask and zeroes a weight only outside ITS free columns (effective_priors on plan_columns(fixed =
    // NULL)): what is kept here must lie inside those, or the P of n_residuals is not what the kernel adds.  cov_masks without a
    // mask states the same rule (pose not mono / constant, camera with corners, never b, c), so cam_free must be a subset of it
    {
        std::vector<unsigned char> unmasked, boards;
        cov_masks(p, nullptr, unmasked, boards);
        for (size_t i = 0; i < cam_free.size(); ++i)
            if (cam_free[i] && !unmasked[i]) return tscm_set_error(TSCM_E_UNSUPPORTED, "internal error: a held-intrinsics mask freed a camera column");
    }
    std::vector<double> pw_cam, pw_intr;
    tscm_camera_priors eff{ sizeof(tscm_camera_priors), nullptr, nullptr, nullptr, nullptr };
    long long n_prior = 0;
    if (priors) {
        eff = *priors;
        auto keep_free = [&](const double *w, int per, int first, std::vector<double> &out) {
            if (!w) return static_cast<const double *>(nullptr);
            out.assign(w, w + per * (size_t)C);
            for (int m = 0; m < C; ++m)
                for (int a = 0; a < per; ++a) {
                    double &x = out[per * (size_t)m + a];
                    if (!cam_free[(size_t)kCovCam * m + first + a]) x = 0.0;
                    n_prior += x > 0.0 ? 1 : 0;
                }
            return static_cast<const double *>(out.data());
        };
        eff.cam_rt_weight = keep_free(priors->cam_rt_weight, 6, 0, pw_cam);
        eff.intr_weight = keep_free(priors->intr_weight, 9, 6, pw_intr);
    }
    CovPlan pl;
    if (int rc = plan_covariance(C, B, V, p->view_camera, p->view_board, cam_free.data(), board_free.data(), pl, err)) return tscm_set_error(rc, "problem: " + err);
    long long N = 0;
    for (int v = 0; v < V; ++v) N += p->view_count[v];
    // the blocks, from the default fp64 Gram kernel through the public evaluation
    std::vector<double> bg((size_t)36 * B + 1), vc((size_t)90 * V + 1), cg((size_t)225 * C);
    double cost = 0.0;
    if (int rc = tscm_eval_normal_equations_spec(p, device, nullptr, spec_args(loss_kind, loss_scale, nullptr, weights, priors ? &eff : nullptr), bg.data(), nullptr, vc.data(), cg.data(), nullptr, &cost)) return rc;
    if (weights) {
        long long kept = 0;
        for (long long i = 0; i < N; ++i) kept += weights[i] > 0.0 ? 1 : 0;
        N = kept;
    }
    const size_t n15 = (size_t)kCovCam * C;
    std::vector<double> own_cam, own_board;
    if (!cam_cov) { own_cam.resize(n15 * n15); cam_cov = own_cam.data(); }
    if (!board_cov) { own_board.resize((size_t)36 * B + 1); board_cov = own_board.data(); }
    if (int rc = covariance_run(pl, p->view_camera, bg.data(), vc.data(), cg.data(), cam_free.data(), device, "tscm_covariance", cam_cov, board_cov, info)) return rc;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const long long dof = 2 * N + n_prior - pl.n_free;
    info->n_residuals = 2 * N + n_prior;
    info->cost = cost;
    info->sigma2 = dof > 0 ? 2.0 * cost / (double)dof : nan;
    // standard deviations: sqrt(sigma2 * diagonal), exactly 0 where the column is not free; NaN behind a singular block
    const bool singular = info->status != 0;
    auto sd = [&](bool is_free, double var) { return !is_free ? 0.0 : singular ? nan : std::sqrt(info->sigma2 * var); };
    for (int m = 0; m < C; ++m)
        for (int a = 0; a < kCovCam; ++a) {
            const size_t i = (size_t)kCovCam * m + a;
            const double s = sd(cam_free[i] != 0, cam_cov[i * n15 + i]);
            if (a < 6) { if (cam_rt_std) cam_rt_std[6 * m + a] = s; }
            else if (intr_std) intr_std[9 * m + a - 6] = s;
        }
    if (board_rt_std)
        for (int b = 0; b < B; ++b)
            for (int a = 0; a < 6; ++a) board_rt_std[6 * (size_t)b + a] = sd(board_free[b] != 0, board_cov[36 * (size_t)b + 7 * a]);
    if (singular) {                                           // "all outputs NaN": the not-free entries too
        if (cam_rt_std) std::fill(cam_rt_std, cam_rt_std + 6 * (size_t)C, nan);
        if (intr_std) std::fill(intr_std, intr_std + 9 * (size_t)C, nan);
        if (board_rt_std) std::fill(board_rt_std, board_rt_std + 6 * (size_t)B, nan);
    }
    return 0;
}

extern "C" int tscm_covariance(const tscm_problem *p, int device, const unsigned short *fixed, int loss_kind, double loss_scale, double *cam_cov,
                               double *board_cov, double *cam_rt_std, double *intr_std, double *board_rt_std, tscm_covariance_info *info)
{
    return covariance_of_problem(p, device, fixed, nullptr, loss_kind, loss_scale, nullptr, cam_cov, board_cov, cam_rt_std, intr_std, board_rt_std, info);
}

extern "C" int tscm_covariance_weighted(const tscm_problem *p, int device, const unsigned short *fixed, const double *weights, int loss_kind,
                                        double loss_scale, double *cam_cov, double *board_cov, double *cam_rt_std, double *intr_std,
                                        double *board_rt_std, tscm_covariance_info *info)
{
    return covariance_of_problem(p, device, fixed, weights, loss_kind, loss_scale, nullptr, cam_cov, board_cov, cam_rt_std, intr_std, board_rt_std, info);
}

extern "C" int tscm_covariance_prior(const tscm_problem *p, int device, const unsigned short *fixed, const double *weights, int loss_kind, double loss_scale,
                                     const tscm_camera_priors *priors, double *cam_cov, double *board_cov, double *cam_rt_std, double *intr_std,
                                     double *board_rt_std, tscm_covariance_info *info)
{
    return covariance_of_problem(p, device, fixed, weights, loss_kind, loss_scale, priors, cam_cov, board_cov, cam_rt_std, intr_std, board_rt_std, info);
}
