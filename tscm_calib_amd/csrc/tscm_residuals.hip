// tscm_residuals.hip -- residual report of a calibration (tscm.h: tscm_residual_report): every corner's residual at
// the problem's parameters, statistics per view and per camera, and per camera the residual field over an image grid and
// over bins of the incidence angle.  A stage of its own: no kernel of the LM iteration runs or is compiled here.
//
//   k_residual_views<WEIGHTED>  one wave per view.  Lanes 0 and 1 form the board's and the camera's pose constants
//                       (board_constants, camera_constants: what k_pose_prep leaves for load_view_const) in LDS, every lane
//                       takes the view's ViewConst from there; lanes run over the corners j = lane (mod 64) ascending.  The
//                       residual comes from corner_residual_jacobian, the function k_eval_functor evaluates (its Jacobian
//                       rows are dead code here), rho and rho' from robust_rho.  A corner's six outputs leave as three
//                       16-byte stores, consecutive lanes consecutive rows; its grid cell and angle bin leave as one 32-bit
//                       word for k_residual_field.  The view's sums: each lane in corner order, then one xor butterfly;
//                       the maximum carries its corner index, ties to the lower index.
//   k_residual_cameras  one workgroup per camera: thread t sums the camera's views t, t + 1024, ... in problem order, then a
//                       fixed binary tree in LDS; the maximum carries its view, ties to the lower view.
//   k_residual_field    one workgroup per chunk of a camera's views (tscm_residual_plan.h).  Integer tables in LDS, sized to
//                       the requested grid and bins (64 x 64 cells x 4 words x 8 B = 128 KiB of the 160 KiB, plus the bins):
//                       a corner adds llrint(x * 2^24) by 64-bit LDS integer atomics; the workgroup then adds its non-zero
//                       words to the camera's table in global memory by 64-bit integer atomics.  Exact, so neither the order
//                       nor the chunking matters.  A cell's count and n_clamped share one word (low and high half).
//   k_residual_field_means  one thread per cell or bin: the integer sums into the double outputs.
// No floating-point atomics and every floating-point sum in a fixed order: two calls give the same bytes.  Every index a
// kernel uses comes from arguments the host checked or from the host plan; the word of a corner holds a cell below
// grid_w * grid_h and a bin below n_angle_bins by construction.
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_host.h"
#include "tscm_math.h"
#include "tscm_fastmath.h"
#include "tscm_nd_plan.h"
#include "tscm_layout.h"
#include "tscm_exec_plan.h"
#include "tscm_columns.h"
#include "tscm_ctrl.h"
#include "tscm_spec.h"
#include "tscm_residual_plan.h"

namespace tscm {
// the shared device functions as they are: the buffer and tile helpers tscm_geometry.h is written against, then robust_rho
#include "tscm_dev.h"
#include "tscm_geometry.h"
}  // namespace tscm

#include <climits>
#include <cmath>
#include <string>
#include <vector>

using namespace tscm;

namespace {

constexpr int kRvWave = 64;
constexpr int kRcThreads = 1024;
constexpr int kRfThreads = 256;
constexpr int kViewRaw = 8;              // per-view raw sums for k_residual_cameras: n_used sum_w sum_ws sum_w|r| max cost worst 0
constexpr int kCamRaw = 4;               // per-camera raw sums for the host: sum_w sum_ws cost n_views_used
constexpr int kCellWords = 4;            // count | n_clamped << 32, sum r_u, sum r_v, sum s
constexpr int kBinWords = 5;             // count | n_clamped << 32, sum r_rad, sum r_tan, sum s, sum angle
constexpr unsigned kHalfOutside = 0xFFFFu, kHalfUnused = 0xFFFEu, kHalfClamped = 0x8000u;
constexpr double kQuantum = 16777216.0;  // 2^24
constexpr long long kMaxFieldCorners = 1ll << 26;

thread_local int g_chunk_target = 0;

struct ResidualArgs {
    const int *view_camera, *view_board, *view_offset, *view_count;
    const long long *view_first;
    const double *board_xy, *obs_u, *obs_v, *weights;
    const double *cam_rt, *intr, *board_rt;
    int mono;
    LossArg loss;
    int grid_w, grid_h, image_width, image_height, n_bins;
    double max_angle, clamp;
};

__device__ __forceinline__ unsigned long long quantise(double x) { return (unsigned long long)llrint(x * kQuantum); }

template <bool WEIGHTED>
__global__ __launch_bounds__(kRvWave) void k_residual_views(ResidualArgs A, double *__restrict__ corner, double *__restrict__ view_row,
                                                           int *__restrict__ view_worst, double *__restrict__ view_raw, unsigned *__restrict__ word)
{
    __shared__ double sc[kBoardConst + kCamConst];
    const int view = blockIdx.x, lane = threadIdx.x;
    const int cam = A.view_camera[view], board = A.view_board[view], count = A.view_count[view];
    if (lane == 0) board_constants(A.board_rt + 6 * (size_t)board, sc);
    if (lane == 1 && !A.mono) camera_constants(A.cam_rt + 6 * (size_t)cam, sc + kBoardConst);
    __syncthreads();
    ViewConst vc;
    const double *I = A.intr + 9 * (size_t)cam;
    if (A.mono) {
        mono_view_const(I, vc);
    } else {
        for (int k = 0; k < 9; ++k) vc.Rc[k] = sc[kBoardConst + k];
        for (int k = 0; k < 27; ++k) vc.dRc[k] = sc[kBoardConst + 9 + k];
        for (int k = 0; k < 3; ++k) vc.tc[k] = A.cam_rt[6 * (size_t)cam + 3 + k];
        vc.fx = I[0]; vc.fy = I[1]; vc.cx = I[2]; vc.cy = I[3]; vc.xi = I[4]; vc.lam = I[5]; vc.al = I[6];
    }
    for (int k = 0; k < 3; ++k) { vc.r1[k] = sc[k]; vc.r2[k] = sc[3 + k]; vc.tb[k] = A.board_rt[6 * (size_t)board + 3 + k]; }
    for (int k = 0; k < 3; ++k) for (int q = 0; q < 6; ++q) vc.db[k][q] = sc[6 + 6 * k + q];

    const long long first = A.view_first[view];
    const int obs0 = A.view_offset[view];
    int n = 0, worst = INT_MAX;
    double sw = 0.0, sws = 0.0, swe = 0.0, su = 0.0, sv = 0.0, srad = 0.0, cost = 0.0, mx = -1.0;
    for (int j = lane; j < count; j += kRvWave) {
        const double om = WEIGHTED ? A.weights[first + j] : 1.0;
        const bool used = om > 0.0;
        const double ou = used ? A.obs_u[obs0 + j] : 0.0, ov = used ? A.obs_v[obs0 + j] : 0.0;   // a masked observation may hold anything
        const double x = A.board_xy[2 * j], y = A.board_xy[2 * j + 1];
        double r[2], JE[2][kE], JF[2][kFA];
        corner_residual_jacobian(vc, x, y, ou, ov, r, JE, JF);
        // the camera-frame point, as corner_residual_jacobian forms it
        const double Pw0 = x * vc.r1[0] + y * vc.r2[0] + vc.tb[0];
        const double Pw1 = x * vc.r1[1] + y * vc.r2[1] + vc.tb[1];
        const double Pw2 = x * vc.r1[2] + y * vc.r2[2] + vc.tb[2];
        const double X = vc.Rc[0] * Pw0 + vc.Rc[1] * Pw1 + vc.Rc[2] * Pw2 + vc.tc[0];
        const double Y = vc.Rc[3] * Pw0 + vc.Rc[4] * Pw1 + vc.Rc[5] * Pw2 + vc.tc[1];
        const double Z = vc.Rc[6] * Pw0 + vc.Rc[7] * Pw1 + vc.Rc[8] * Pw2 + vc.tc[2];
        const double angle = atan2(sqrt(X * X + Y * Y), Z);
        const double s = r[0] * r[0] + r[1] * r[1];
        const double err = sqrt(s);
        // the direction from the principal point to the projected pixel p = observed - r
        const double px = (ou - r[0]) - vc.cx, py = (ov - r[1]) - vc.cy;
        const double pn = sqrt(px * px + py * py);
        const double ex = pn > 0.0 ? px / pn : 1.0, ey = pn > 0.0 ? py / pn : 0.0;
        const double r_rad = r[0] * ex + r[1] * ey, r_tan = ex * r[1] - ey * r[0];
        double rho, w;
        robust_rho<true>(A.loss, s, rho, w, 1.0);         // omega = 1: rho(s) and sqrt(rho'(s)), clamped
        const double rho1 = w * w;
        if (corner) {
            d2 *row = reinterpret_cast<d2 *>(corner + 6 * (size_t)(first + j));
            d2 a, b, c;
            a[0] = used ? r[0] : 0.0;  a[1] = used ? r[1] : 0.0;
            b[0] = used ? r_rad : 0.0; b[1] = used ? r_tan : 0.0;
            c[0] = used ? angle : 0.0; c[1] = used ? rho1 : 0.0;
            row[0] = a; row[1] = b; row[2] = c;
        }
        if (word) {
            unsigned lo = kHalfUnused, hi = kHalfUnused;
            if (used) {
                const unsigned clamped = fmax(fabs(r[0]), fabs(r[1])) > A.clamp ? kHalfClamped : 0u;
                if (A.grid_w > 0) {
                    const double fx_ = floor(ou * (double)A.grid_w / (double)A.image_width), fy_ = floor(ov * (double)A.grid_h / (double)A.image_height);
                    const bool in = fx_ >= 0.0 && fx_ < (double)A.grid_w && fy_ >= 0.0 && fy_ < (double)A.grid_h;     // false for NaN
                    lo = in ? ((unsigned)((int)fy_ * A.grid_w + (int)fx_) | clamped) : kHalfOutside;
                }
                if (A.n_bins > 0) {
                    const bool in = angle >= 0.0 && angle <= A.max_angle;
                    int bin = (int)floor(angle * (double)A.n_bins / A.max_angle);
                    bin = bin < 0 ? 0 : bin > A.n_bins - 1 ? A.n_bins - 1 : bin;
                    hi = in ? ((unsigned)bin | clamped) : kHalfOutside;
                }
            }
            word[first + j] = lo | (hi << 16);
        }
        if (used) {
            ++n;
            sw += om; sws += om * s; swe += om * err; su += om * r[0]; sv += om * r[1]; srad += om * r_rad; cost += om * rho;
            if (err > mx) { mx = err; worst = j; }
        }
    }
    for (int sft = 32; sft > 0; sft >>= 1) {
        n += __shfl_xor(n, sft);
        sw += __shfl_xor(sw, sft); sws += __shfl_xor(sws, sft); swe += __shfl_xor(swe, sft); su += __shfl_xor(su, sft);
        sv += __shfl_xor(sv, sft); srad += __shfl_xor(srad, sft); cost += __shfl_xor(cost, sft);
        const double omx = __shfl_xor(mx, sft);
        const int ow = __shfl_xor(worst, sft);
        if (omx > mx || (omx == mx && ow < worst)) { mx = omx; worst = ow; }
    }
    if (lane == 0) {
        const bool any = n > 0;
        double *o = view_row + 8 * (size_t)view;
        o[0] = (double)n; o[1] = sw;
        o[2] = any ? sqrt(sws / sw) : 0.0; o[3] = any ? swe / sw : 0.0; o[4] = any ? mx : 0.0;
        o[5] = any ? su / sw : 0.0; o[6] = any ? sv / sw : 0.0; o[7] = any ? srad / sw : 0.0;
        view_worst[view] = any ? worst : -1;
        double *q = view_raw + kViewRaw * (size_t)view;
        q[0] = (double)n; q[1] = sw; q[2] = sws; q[3] = swe; q[4] = any ? mx : -1.0; q[5] = cost; q[6] = 0.0; q[7] = 0.0;
    }
}

// camera [C][8], cam_raw [C][kCamRaw]
__global__ __launch_bounds__(kRcThreads) void k_residual_cameras(const int *__restrict__ cam_start, const int *__restrict__ cam_views,
                                                                const double *__restrict__ view_raw, double *__restrict__ camera,
                                                                double *__restrict__ cam_raw)
{
    __shared__ double sS[5][kRcThreads];          // n_used, sum_w, sum_ws, sum_w|r|, cost
    __shared__ double sM[kRcThreads];
    __shared__ int sV[kRcThreads], sN[kRcThreads];
    const int m = blockIdx.x, t = threadIdx.x;
    double a[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 }, mx = -1.0;
    int wv = INT_MAX, nv = 0;
    for (int k = cam_start[m] + t; k < cam_start[m + 1]; k += kRcThreads) {
        const int v = cam_views[k];
        const double *q = view_raw + kViewRaw * (size_t)v;
        if (!(q[0] > 0.0)) continue;
        a[0] += q[0]; a[1] += q[1]; a[2] += q[2]; a[3] += q[3]; a[4] += q[5];
        ++nv;
        if (q[4] > mx) { mx = q[4]; wv = v; }      // views ascend within a thread: the lower view stays on ties
    }
    for (int i = 0; i < 5; ++i) sS[i][t] = a[i];
    sM[t] = mx; sV[t] = wv; sN[t] = nv;
    __syncthreads();
    for (int h = kRcThreads / 2; h > 0; h >>= 1) {
        if (t < h) {
            for (int i = 0; i < 5; ++i) sS[i][t] += sS[i][t + h];
            sN[t] += sN[t + h];
            if (sM[t + h] > sM[t] || (sM[t + h] == sM[t] && sV[t + h] < sV[t])) { sM[t] = sM[t + h]; sV[t] = sV[t + h]; }
        }
        __syncthreads();
    }
    if (t == 0) {
        const bool any = sS[0][0] > 0.0;
        double *o = camera + 8 * (size_t)m;
        o[0] = sS[0][0]; o[1] = sS[1][0];
        o[2] = any ? sqrt(sS[2][0] / sS[1][0]) : 0.0; o[3] = any ? sS[3][0] / sS[1][0] : 0.0; o[4] = any ? sM[0] : 0.0;
        o[5] = any ? (double)sV[0] : -1.0; o[6] = (double)sN[0]; o[7] = 0.0;
        double *q = cam_raw + kCamRaw * (size_t)m;
        q[0] = sS[1][0]; q[1] = sS[2][0]; q[2] = sS[4][0]; q[3] = (double)sN[0];
    }
}

// table: per camera `stride` words: cells * kCellWords, bins * kBinWords, grid_outside, angle_outside
__global__ __launch_bounds__(kRfThreads) void k_residual_field(const int *__restrict__ chunk_camera, const int *__restrict__ chunk_begin,
                                                              const int *__restrict__ chunk_end, const int *__restrict__ field_views,
                                                              const long long *__restrict__ view_first, const int *__restrict__ view_count,
                                                              const double *__restrict__ corner, const unsigned *__restrict__ word, int cells, int bins,
                                                              unsigned long long *__restrict__ table)
{
    extern __shared__ unsigned long long tab[];
    const int stride = cells * kCellWords + bins * kBinWords + 2;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, chunk = blockIdx.x;
    for (int e = t; e < stride; e += kRfThreads) tab[e] = 0ull;
    __syncthreads();
    unsigned long long *bt = tab + cells * kCellWords, *outside = bt + bins * kBinWords;
    for (int k = chunk_begin[chunk] + wave; k < chunk_end[chunk]; k += kRfThreads / 64) {
        const int v = field_views[k];
        const long long first = view_first[v];
        for (int j = lane; j < view_count[v]; j += 64) {
            const unsigned wd = word[first + j], lo = wd & 0xFFFFu, hi = wd >> 16;
            if (lo == kHalfUnused && hi == kHalfUnused) continue;
            const double *row = corner + 6 * (size_t)(first + j);
            const double ru = row[0], rv = row[1];
            const unsigned long long qs = quantise(ru * ru + rv * rv);
            if (lo == kHalfOutside) atomicAdd(&outside[0], 1ull);
            else if (lo != kHalfUnused) {
                unsigned long long *c = tab + kCellWords * (lo & 0x7FFFu);
                if (lo & kHalfClamped) atomicAdd(&c[0], 1ull << 32);
                else { atomicAdd(&c[0], 1ull); atomicAdd(&c[1], quantise(ru)); atomicAdd(&c[2], quantise(rv)); atomicAdd(&c[3], qs); }
            }
            if (hi == kHalfOutside) atomicAdd(&outside[1], 1ull);
            else if (hi != kHalfUnused) {
                unsigned long long *b = bt + kBinWords * (hi & 0x7FFFu);
                if (hi & kHalfClamped) atomicAdd(&b[0], 1ull << 32);
                else {
                    atomicAdd(&b[0], 1ull); atomicAdd(&b[1], quantise(row[2])); atomicAdd(&b[2], quantise(row[3])); atomicAdd(&b[3], qs);
                    atomicAdd(&b[4], quantise(row[4]));
                }
            }
        }
    }
    __syncthreads();
    unsigned long long *g = table + (size_t)stride * chunk_camera[chunk];
    for (int e = t; e < stride; e += kRfThreads)
        if (tab[e] != 0ull) atomicAdd(&g[e], tab[e]);
}

__device__ __forceinline__ double field_mean(unsigned long long sum, long long count) { return (double)(long long)sum * (1.0 / kQuantum) / (double)count; }

// one thread per (camera, cell or bin)
__global__ __launch_bounds__(256) void k_residual_field_means(const unsigned long long *__restrict__ table, int n_cameras, int cells, int bins,
                                                             long long *__restrict__ grid_count, double *__restrict__ grid,
                                                             long long *__restrict__ angle_count, double *__restrict__ angle)
{
    const int per = cells + bins, stride = cells * kCellWords + bins * kBinWords + 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cameras * per) return;
    const int m = i / per, e = i % per;
    const unsigned long long *g = table + (size_t)stride * m;
    if (e < cells) {
        const unsigned long long *c = g + kCellWords * e;
        const long long count = (long long)(c[0] & 0xFFFFFFFFull), clamped = (long long)(c[0] >> 32);
        const size_t o = (size_t)m * cells + e;
        grid_count[2 * o] = count; grid_count[2 * o + 1] = clamped;
        grid[3 * o] = count ? field_mean(c[1], count) : 0.0;
        grid[3 * o + 1] = count ? field_mean(c[2], count) : 0.0;
        grid[3 * o + 2] = count ? sqrt(field_mean(c[3], count)) : 0.0;
    } else {
        const int k = e - cells;
        const unsigned long long *b = g + cells * kCellWords + kBinWords * k;
        const long long count = (long long)(b[0] & 0xFFFFFFFFull), clamped = (long long)(b[0] >> 32);
        const size_t o = (size_t)m * bins + k;
        angle_count[2 * o] = count; angle_count[2 * o + 1] = clamped;
        angle[4 * o] = count ? field_mean(b[1], count) : 0.0;
        angle[4 * o + 1] = count ? field_mean(b[2], count) : 0.0;
        angle[4 * o + 2] = count ? sqrt(field_mean(b[3], count)) : 0.0;
        angle[4 * o + 3] = count ? field_mean(b[4], count) : 0.0;
    }
}

int invalid(const std::string &msg) { return tscm_set_error(TSCM_E_INVALID, msg); }

void reset_info(tscm_residual_info *info)
{
    info->n_views_used = 0; info->n_used = 0; info->sum_w = 0.0; info->cost = 0.0; info->rmse = 0.0;
    for (long long &x : info->grid_outside) x = 0;
    for (long long &x : info->angle_outside) x = 0;
    for (double &s : info->seconds_kernel) s = 0.0;
}

// the argument checks, in the order tscm.h lists them; spec: the loss, completed
int check_args(const tscm_problem *p, const double *weights, const tscm_residual_params *q, const long long *grid_count, const double *grid,
               const long long *angle_count, const double *angle, const tscm_residual_info *info, SolveSpec &spec)
{
    if (!p) return invalid("problem is NULL");
    if (!q) return invalid("params is NULL");
    if (!info) return invalid("info is NULL");
    if (int rc = check_struct_size(q, "tscm_residual_params")) return rc;
    if (int rc = check_struct_size(info, "tscm_residual_info", "info")) return rc;
    if (q->loss_kind < TSCM_LOSS_NONE || q->loss_kind > TSCM_LOSS_CAUCHY) return invalid("params: loss_kind " + std::to_string(q->loss_kind) + " is not a TSCM_LOSS_* kind");
    if (q->loss_kind != TSCM_LOSS_NONE && (!std::isfinite(q->loss_scale) || !(q->loss_scale > 0.0))) return invalid("params: loss_scale must be finite and > 0");
    std::string err;
    if (int rc = make_spec(q->loss_kind, q->loss_scale, nullptr, 0, spec, err)) return tscm_set_error(rc, "params: " + err);
    if (q->grid_w < 0 || q->grid_w > 64 || q->grid_h < 0 || q->grid_h > 64 || (q->grid_w == 0) != (q->grid_h == 0))
        return invalid("params: grid_w x grid_h = " + std::to_string(q->grid_w) + " x " + std::to_string(q->grid_h) + " outside 1..64 each (0 x 0: no grid)");
    if (q->n_angle_bins < 0 || q->n_angle_bins > 64) return invalid("params: n_angle_bins " + std::to_string(q->n_angle_bins) + " outside 0..64");
    if (q->grid_w > 0 && (q->image_width <= 0 || q->image_height <= 0))
        return invalid("params: image_width x image_height = " + std::to_string(q->image_width) + " x " + std::to_string(q->image_height) + " is not positive, with a grid");
    if (q->n_angle_bins > 0 && (!std::isfinite(q->max_angle) || !(q->max_angle > 0.0) || q->max_angle > 3.14159265358979323846))
        return invalid("params: max_angle must lie in (0, pi]");
    if (!std::isfinite(q->clamp) || !(q->clamp > 0.0) || q->clamp > 64.0) return invalid("params: clamp must lie in (0, 64]");
    if (q->grid_w > 0 && !grid_count) return invalid("grid_count is NULL with a grid requested");
    if (q->grid_w > 0 && !grid) return invalid("grid is NULL with a grid requested");
    if (q->n_angle_bins > 0 && !angle_count) return invalid("angle_count is NULL with angle bins requested");
    if (q->n_angle_bins > 0 && !angle) return invalid("angle is NULL with angle bins requested");
    if (int rc = validate(p, err)) return tscm_set_error(rc, "problem: " + err);
    if (weights) {
        long long n = 0;
        for (int v = 0; v < p->n_views; ++v)
            for (int j = 0; j < p->view_count[v]; ++j, ++n)
                if (!std::isfinite(weights[n]) || weights[n] < 0.0)
                    return invalid("weights[" + std::to_string(n) + "] (view " + std::to_string(v) + ", corner " + std::to_string(j) + ") is negative, NaN or infinite");
    }
    return 0;
}

}  // namespace

extern "C" void tscm_residual_default_params(tscm_residual_params *q)
{
    if (!q) return;
    q->struct_size = (int)sizeof(tscm_residual_params);
    q->loss_kind = TSCM_LOSS_NONE; q->loss_scale = 1.0;
    q->grid_w = 0; q->grid_h = 0; q->image_width = 0; q->image_height = 0;
    q->n_angle_bins = 0; q->pad = 0;
    q->max_angle = 1.57079632679489661923;
    q->clamp = 64.0;
}

extern "C" void tscm_residual_debug_chunk_target(int corners) { g_chunk_target = corners > 0 ? corners : 0; }

extern "C" int tscm_residual_report(const tscm_problem *p, int device, const double *weights, const tscm_residual_params *params, double *corner, double *view,
                                    int *view_worst, double *camera, long long *grid_count, double *grid, long long *angle_count, double *angle,
                                    tscm_residual_info *info)
{
    SolveSpec spec{};
    if (int rc = check_args(p, weights, params, grid_count, grid, angle_count, angle, info, spec)) return rc;
    reset_info(info);
    const int C = p->n_cameras, V = p->n_views, B = p->n_boards;
    ResidualPlan pl;
    std::string err;
    if (int rc = plan_residuals(C, V, p->view_camera, p->view_count, g_chunk_target, pl, err)) return tscm_set_error(rc, "problem: " + err);
    const long long N = pl.N;
    const int cells = params->grid_w * params->grid_h, bins = params->n_angle_bins;
    const bool field = cells > 0 || bins > 0;
    if (field) {
        std::vector<long long> used((size_t)C, 0);
        for (int v = 0; v < V; ++v)
            for (int j = 0; j < p->view_count[v]; ++j)
                if (!weights || weights[pl.view_first[v] + j] > 0.0) used[p->view_camera[v]]++;
        for (int m = 0; m < C; ++m)
            if (used[m] > kMaxFieldCorners)
                return tscm_set_error(TSCM_E_UNSUPPORTED, "camera " + std::to_string(m) + " has more than 2^26 used corners: the field's 64-bit sums could overflow");
    }
    if (int rc = select_device(device, "tscm_residual_report")) return rc;
    size_t n_obs = 0;
    for (int v = 0; v < V; ++v) n_obs = std::max(n_obs, (size_t)p->view_offset[v] + (size_t)p->view_count[v]);

    DeviceMem mem;
    EventSpan span;
    ResidualArgs A{};
    HIP_TRY(mem.upload(&A.view_camera, p->view_camera, (size_t)V));
    HIP_TRY(mem.upload(&A.view_board, p->view_board, (size_t)V));
    HIP_TRY(mem.upload(&A.view_offset, p->view_offset, (size_t)V));
    HIP_TRY(mem.upload(&A.view_count, p->view_count, (size_t)V));
    HIP_TRY(mem.upload(&A.view_first, pl.view_first));
    HIP_TRY(mem.upload(&A.board_xy, p->board_xy, (size_t)2 * p->n_points));
    HIP_TRY(mem.upload(&A.obs_u, p->obs_u, n_obs));
    HIP_TRY(mem.upload(&A.obs_v, p->obs_v, n_obs));
    if (weights) HIP_TRY(mem.upload(&A.weights, weights, (size_t)N));
    if (!p->mono) HIP_TRY(mem.upload(&A.cam_rt, p->cam_rt, (size_t)6 * C));
    HIP_TRY(mem.upload(&A.intr, p->intr, (size_t)9 * C));
    HIP_TRY(mem.upload(&A.board_rt, p->board_rt, (size_t)6 * B));
    A.mono = p->mono ? 1 : 0;
    A.loss = spec.loss;
    A.grid_w = params->grid_w; A.grid_h = params->grid_h; A.image_width = params->image_width; A.image_height = params->image_height;
    A.n_bins = bins; A.max_angle = params->max_angle; A.clamp = params->clamp;

    double *d_corner = nullptr, *d_view = nullptr, *d_raw = nullptr, *d_camera = nullptr, *d_cam_raw = nullptr, *d_grid = nullptr, *d_angle = nullptr;
    int *d_worst = nullptr;
    unsigned *d_word = nullptr;
    unsigned long long *d_table = nullptr;
    long long *d_grid_count = nullptr, *d_angle_count = nullptr;
    const int *d_cam_start = nullptr, *d_cam_views = nullptr, *d_chunk_cam = nullptr, *d_chunk_begin = nullptr, *d_chunk_end = nullptr, *d_field_views = nullptr;
    if (corner || field) HIP_TRY(mem.alloc(&d_corner, (size_t)6 * N));
    HIP_TRY(mem.alloc(&d_view, (size_t)8 * V));
    HIP_TRY(mem.alloc(&d_worst, (size_t)V));
    HIP_TRY(mem.alloc(&d_raw, (size_t)kViewRaw * V));
    HIP_TRY(mem.alloc(&d_camera, (size_t)8 * C));
    HIP_TRY(mem.alloc(&d_cam_raw, (size_t)kCamRaw * C));
    HIP_TRY(mem.upload(&d_cam_start, pl.cam_start));
    HIP_TRY(mem.upload(&d_cam_views, pl.cam_views));
    const int stride = cells * kCellWords + bins * kBinWords + 2;
    const int n_chunks = (int)pl.chunk_begin.size();
    const size_t lds = sizeof(unsigned long long) * (size_t)stride;
    if (field) {
        HIP_TRY(mem.alloc(&d_word, (size_t)N));
        HIP_TRY(mem.alloc(&d_table, (size_t)stride * C));
        HIP_TRY(hipMemset(d_table, 0, sizeof(unsigned long long) * (size_t)stride * C));
        HIP_TRY(mem.upload(&d_chunk_cam, pl.chunk_camera));
        HIP_TRY(mem.upload(&d_chunk_begin, pl.chunk_begin));
        HIP_TRY(mem.upload(&d_chunk_end, pl.chunk_end));
        HIP_TRY(mem.upload(&d_field_views, pl.field_views));
        HIP_TRY(mem.alloc(&d_grid_count, (size_t)2 * C * cells));
        HIP_TRY(mem.alloc(&d_grid, (size_t)3 * C * cells));
        HIP_TRY(mem.alloc(&d_angle_count, (size_t)2 * C * bins));
        HIP_TRY(mem.alloc(&d_angle, (size_t)4 * C * bins));
        if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_residual_field), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    HIP_TRY(span.create(5));
    HIP_TRY(span.mark(0));
    if (V > 0) {
        if (weights) hipLaunchKernelGGL(k_residual_views<true>, dim3(V), dim3(kRvWave), 0, 0, A, d_corner, d_view, d_worst, d_raw, d_word);
        else hipLaunchKernelGGL(k_residual_views<false>, dim3(V), dim3(kRvWave), 0, 0, A, d_corner, d_view, d_worst, d_raw, d_word);
    }
    HIP_TRY(span.mark(1));
    hipLaunchKernelGGL(k_residual_cameras, dim3(C), dim3(kRcThreads), 0, 0, d_cam_start, d_cam_views, d_raw, d_camera, d_cam_raw);
    HIP_TRY(span.mark(2));
    if (field && n_chunks > 0)
        hipLaunchKernelGGL(k_residual_field, dim3(n_chunks), dim3(kRfThreads), lds, 0, d_chunk_cam, d_chunk_begin, d_chunk_end, d_field_views, A.view_first,
                           A.view_count, d_corner, d_word, cells, bins, d_table);
    HIP_TRY(span.mark(3));
    if (field)
        hipLaunchKernelGGL(k_residual_field_means, dim3((C * (cells + bins) + 255) / 256), dim3(256), 0, 0, d_table, C, cells, bins, d_grid_count, d_grid,
                           d_angle_count, d_angle);
    HIP_TRY(span.finish(4, info->seconds_kernel, nullptr));

    if (corner && N > 0) HIP_TRY(hipMemcpy(corner, d_corner, sizeof(double) * 6 * (size_t)N, hipMemcpyDeviceToHost));
    if (view && V > 0) HIP_TRY(hipMemcpy(view, d_view, sizeof(double) * 8 * (size_t)V, hipMemcpyDeviceToHost));
    if (view_worst && V > 0) HIP_TRY(hipMemcpy(view_worst, d_worst, sizeof(int) * (size_t)V, hipMemcpyDeviceToHost));
    std::vector<double> cam_rows((size_t)8 * C), cam_raw((size_t)kCamRaw * C);
    HIP_TRY(hipMemcpy(cam_rows.data(), d_camera, sizeof(double) * cam_rows.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cam_raw.data(), d_cam_raw, sizeof(double) * cam_raw.size(), hipMemcpyDeviceToHost));
    if (camera) std::copy(cam_rows.begin(), cam_rows.end(), camera);
    // the call's totals: over the cameras in order
    double sw = 0.0, sws = 0.0, cost = 0.0;
    for (int m = 0; m < C; ++m) {
        info->n_used += (long long)cam_rows[8 * (size_t)m];
        info->n_views_used += (int)cam_raw[kCamRaw * (size_t)m + 3];
        sw += cam_raw[kCamRaw * (size_t)m]; sws += cam_raw[kCamRaw * (size_t)m + 1]; cost += cam_raw[kCamRaw * (size_t)m + 2];
    }
    info->sum_w = sw;
    info->cost = 0.5 * cost;
    info->rmse = sw > 0.0 ? std::sqrt(sws / sw) : 0.0;
    if (field) {
        if (cells > 0) {
            HIP_TRY(hipMemcpy(grid_count, d_grid_count, sizeof(long long) * 2 * (size_t)C * cells, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(grid, d_grid, sizeof(double) * 3 * (size_t)C * cells, hipMemcpyDeviceToHost));
        }
        if (bins > 0) {
            HIP_TRY(hipMemcpy(angle_count, d_angle_count, sizeof(long long) * 2 * (size_t)C * bins, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(angle, d_angle, sizeof(double) * 4 * (size_t)C * bins, hipMemcpyDeviceToHost));
        }
        std::vector<unsigned long long> table((size_t)stride * C);
        HIP_TRY(hipMemcpy(table.data(), d_table, sizeof(unsigned long long) * table.size(), hipMemcpyDeviceToHost));
        for (int m = 0; m < C; ++m) {
            info->grid_outside[m] = (long long)table[(size_t)stride * m + stride - 2];
            info->angle_outside[m] = (long long)table[(size_t)stride * m + stride - 1];
        }
    }
    return 0;
}
