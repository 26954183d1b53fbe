// tscm_init.hip -- focal-length initialisation on the device (mono part):
// TripleSphereCamera::estimate_focal (TS.cpp:110-168).  One thread per (image, board row): the
// width x 4 circle-fit design matrix is reduced to its 4 x 4 triangular factor by Householder
// reflections in thread-private memory, and the null vector (cv::SVD::solveZ) comes from a
// one-sided Jacobi SVD of that factor held in registers.  The accepted samples are averaged on the
// host in the reference's (image, row) order.
// Below it the pose of every image (estimate_extrinsic, TS.cpp:170-203): the least-squares planar PnP, one thread per
// image, and the consensus search with a refit on the inliers, one wave per image (tscm_init_ransac.h).  Both run the one
// fit of tscm_planar_pose.h.
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_host.h"
#include "tscm_init_ransac.h"

#include <cmath>
#include <string>
#include <vector>

namespace {

constexpr int kMaxBoardW = 32;

// gamma of one board row, or a negative marker: -1 image without board, -2 rejected (TS.cpp:149, :153)
__global__ __launch_bounds__(64) void k_focal_rows(const double *__restrict__ pu, const double *__restrict__ pv, const int *__restrict__ count,
                                                   int n_views, int width, int height, double cx, double cy, double *__restrict__ gamma)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_views * height) return;
    const int k = t / height, i = t - k * height;
    if (count[k] == 0) { gamma[t] = -1.0; return; }
    double A[kMaxBoardW][4];
    const size_t base = ((size_t)k * height + i) * width;
    for (int j = 0; j < width; ++j) {
        const double x = pu[base + j] - cx, y = pv[base + j] - cy;
        A[j][0] = x; A[j][1] = y; A[j][2] = 0.5; A[j][3] = -0.5 * (x * x + y * y);
    }
    // Householder QR: A -> R (upper triangular, rows 0..3); Q is not needed for a null vector
    for (int c = 0; c < 4; ++c) {
        double s = 0.0;
        for (int r = c; r < width; ++r) s += A[r][c] * A[r][c];
        const double nrm = sqrt(s);
        if (nrm == 0.0) continue;
        const double alpha = A[c][c] > 0 ? -nrm : nrm;
        const double v0 = A[c][c] - alpha;
        const double vtv = s - A[c][c] * A[c][c] + v0 * v0;
        if (vtv == 0.0) continue;
        for (int cc = c + 1; cc < 4; ++cc) {
            double dot = v0 * A[c][cc];
            for (int r = c + 1; r < width; ++r) dot += A[r][c] * A[r][cc];
            const double f = 2.0 * dot / vtv;
            A[c][cc] -= f * v0;
            for (int r = c + 1; r < width; ++r) A[r][cc] -= f * A[r][c];
        }
        A[c][c] = alpha;                                     // the entries below (the reflector) are not read again
    }
    // one-sided Jacobi on the columns of R, V accumulates the right singular vectors
    double R[4][4], V[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { R[r][c] = c >= r ? A[r][c] : 0.0; V[r][c] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double a = 0, b = 0, g = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) { a += R[r][p] * R[r][p]; b += R[r][q] * R[r][q]; g += R[r][p] * R[r][q]; }
                if (g == 0.0 || fabs(g) <= 1e-17 * sqrt(a * b)) continue;
                rotated = true;
                const double zeta = (b - a) / (2.0 * g);
                const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double x = R[r][p], y = R[r][q];
                    R[r][p] = cs * x - sn * y; R[r][q] = sn * x + cs * y;
                    const double vx = V[r][p], vy = V[r][q];
                    V[r][p] = cs * vx - sn * vy; V[r][q] = sn * vx + cs * vy;
                }
            }
        if (!rotated) break;
    }
    double smin = INFINITY, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double s = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) s += R[r][j] * R[r][j];
        if (s < smin) { smin = s; c1 = V[0][j]; c2 = V[1][j]; c3 = V[2][j]; c4 = V[3][j]; }
    }
    const double tq = c1 * c1 + c2 * c2 + c3 * c4;                 // TS.cpp:148-156
    if (tq < 0) { gamma[t] = -2.0; return; }
    const double d = sqrt(1 / tq);
    const double nx = c1 * d, ny = c2 * d;
    if (nx * nx + ny * ny > 0.95) { gamma[t] = -2.0; return; }
    const double nz = sqrt(1 - nx * nx - ny * ny);
    gamma[t] = fabs(c3 * d / nz);
}

// STAGES = false: Rt_out [n_views][9], ok_out[k] = 1 where a pose was written (tscm_estimate_extrinsic).
// STAGES = true: Rt_out [n_views][kStageRec] = Rt | T | H | rv0 t0 | rv t | GN steps, ok_out[k] = the
// TSCM_EXTRINSIC_* exit code (tscm_estimate_extrinsic_stages); stage fields not reached keep their values.
constexpr int kStageRec = 40, kStageT = 9;

// estimate_extrinsic (TS.cpp:170-203), one thread per image: tscm_planar_pose.h's fit over all corners, serial sums.
template <bool STAGES>
__global__ __launch_bounds__(64) void k_estimate_extrinsic(const double *__restrict__ intr, const double *__restrict__ pu, const double *__restrict__ pv,
                                                           const int *__restrict__ count, int n_views, const double *__restrict__ worlds, int n, int board_w,
                                                           double *__restrict__ Rt_out, unsigned char *__restrict__ ok_out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_views) return;
    double *stage = STAGES ? Rt_out + (size_t)kStageRec * k : nullptr;
    if (count[k] == 0) {
        ok_out[k] = STAGES ? TSCM_EXTRINSIC_NO_BOARD : 0;
        return;
    }
    double I[9];
    for (int i = 0; i < 9; ++i) I[i] = intr[i];
    const double *u = pu + (size_t)k * n, *v = pv + (size_t)k * n;
    const int ref = n / 2 - board_w / 2 - 1;
    double T[9];
    tscm::look_at_turn(I, u[ref], v[ref], T);
    if constexpr (STAGES)
        for (int i = 0; i < 9; ++i) stage[kStageT + i] = T[i];
    auto normalised = [&](int i, double &x, double &y) {                  // every corner takes part
        double Z;
        tscm::turned_corner(I, T, u[i], v[i], x, y, Z);
        return true;
    };
    double rv[3], t[3], R[9], dR[27];
    const int code = tscm::fit_planar_pose(tscm::SerialLanes{}, normalised, n, worlds, n, stage, rv, t);
    if (code >= TSCM_EXTRINSIC_CONVERGED) {
        tscm::rotation_and_derivatives(rv, R, dR);
        tscm::compose_rt(T, R, t, STAGES ? stage : Rt_out + 9 * (size_t)k);
    }
    ok_out[k] = STAGES ? code : code >= TSCM_EXTRINSIC_CONVERGED;
}

}  // namespace

// k_focal_rows over every (image, row): g[k * board_h + i] = the kernel's value.  Both focal entry points call this.
static int focal_rows(const double *pix_u, const double *pix_v, const int *count, int n_views, int board_w, int board_h,
                      double cx, double cy, int device, std::vector<double> &g)
{
    if (board_w < 4 || board_h < 1) return tscm_set_error(TSCM_E_UNSUPPORTED, "estimate_focal needs boards at least 4 corners wide");
    if (board_w > kMaxBoardW) return tscm_set_error(TSCM_E_UNSUPPORTED, "boards wider than 32 corners");
    if (int rc = tscm::select_device(device, "tscm_estimate_focal")) return rc;
    const size_t rows = (size_t)n_views * board_h, npix = rows * board_w;
    g.assign(rows, 0.0);
    if (rows == 0) return 0;
    tscm::DeviceMem mem;
    const double *d_u = nullptr, *d_v = nullptr;
    const int *d_c = nullptr;
    double *d_g = nullptr;
    HIP_TRY(mem.upload(&d_u, pix_u, npix));
    HIP_TRY(mem.upload(&d_v, pix_v, npix));
    HIP_TRY(mem.upload(&d_c, count, (size_t)n_views));
    HIP_TRY(mem.alloc(&d_g, rows));
    hipLaunchKernelGGL(k_focal_rows, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, 0, d_u, d_v, d_c, n_views, board_w, board_h, cx, cy, d_g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(g.data(), d_g, rows * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tscm_estimate_focal(const double *pix_u, const double *pix_v, const int *count, int n_views, int board_w, int board_h,
                                   double cx, double cy, int device, double *focal, int *n_used)
{
    if (!focal || !n_used || n_views < 0 || (n_views > 0 && (!pix_u || !pix_v || !count))) return tscm_set_error(TSCM_E_INVALID, "NULL argument");
    std::vector<double> g;
    const int rc = focal_rows(pix_u, pix_v, count, n_views, board_w, board_h, cx, cy, device, g);
    if (rc) return rc;
    double f = 0.0;
    int total = 0;
    for (const double x : g) {                              // focal_ += gamma in (image, row) order (:155-156)
        if (x < 0.0) continue;                              // markers; NaN samples are summed like the reference does
        f += x; ++total;
    }
    if (total > 0) f /= total;
    *focal = f; *n_used = total;
    return 0;
}

extern "C" int tscm_estimate_focal_rows(const double *pix_u, const double *pix_v, const int *count, int n_views, int board_w, int board_h,
                                        double cx, double cy, int device, double *gamma)
{
    if (n_views < 0 || (n_views > 0 && (!pix_u || !pix_v || !count || !gamma))) return tscm_set_error(TSCM_E_INVALID, "NULL argument");
    std::vector<double> g;
    const int rc = focal_rows(pix_u, pix_v, count, n_views, board_w, board_h, cx, cy, device, g);
    if (rc) return rc;
    for (size_t r = 0; r < g.size(); ++r) gamma[r] = g[r];
    return 0;
}

// What both pose kernels read, on the device: the inputs, and in `rec` the caller's nrec doubles (Rt, or the stage
// records of k_estimate_extrinsic<true>), uploaded so that views without a pose keep the caller's values.
struct PoseInputs {
    const double *intr = nullptr, *u = nullptr, *v = nullptr, *worlds = nullptr;
    const int *count = nullptr;
    double *rec = nullptr;

    int upload(tscm::DeviceMem &mem, const double *intr9, const double *pix_u, const double *pix_v, const int *cnt, size_t n_views,
               const double *w, int n_points, const double *caller_rec, size_t nrec)
    {
        HIP_TRY(mem.upload(&intr, intr9, 9));
        HIP_TRY(mem.upload(&u, pix_u, n_views * n_points));
        HIP_TRY(mem.upload(&v, pix_v, n_views * n_points));
        HIP_TRY(mem.upload(&worlds, w, 3 * (size_t)n_points));
        HIP_TRY(mem.upload(&rec, caller_rec, nrec));
        HIP_TRY(mem.upload(&count, cnt, n_views));
        return 0;
    }
};

// H, pose0, pose and the Gauss-Newton steps of view k from the fit's part r of its stage record (either kernel's).  A stage
// the view did not reach is NaN, its steps -1.
static void unpack_fit_stages(const double *r, size_t k, double *H, double *pose0, double *pose, int *steps)
{
    for (int i = 0; i < 9; ++i) H[9 * k + i] = r[tscm::kStageH + i];
    for (int i = 0; i < 6; ++i) { pose0[6 * k + i] = r[tscm::kStagePose0 + i]; pose[6 * k + i] = r[tscm::kStagePose + i]; }
    steps[k] = std::isnan(r[tscm::kStageSteps]) ? -1 : (int)r[tscm::kStageSteps];
}

// One launch of k_estimate_extrinsic<STAGES> over every image.  rec: [n_views][STAGES ? kStageRec : 9] host records,
// uploaded and read back whole (so the fields a view does not reach keep the caller's values); ok: [n_views].
template <bool STAGES>
static int extrinsic_views(const double *intr9, const double *pix_u, const double *pix_v, const int *count, int n_views,
                           const double *worlds, int n_points, int board_w, int device, double *rec, unsigned char *ok)
{
    if (board_w < 1 || n_points / 2 - board_w / 2 - 1 < 0) return tscm_set_error(TSCM_E_INVALID, "board width does not fit the corner count");
    if (int rc = tscm::select_device(device, "tscm_estimate_extrinsic")) return rc;
    if (n_views == 0) return 0;
    const size_t nrec = (size_t)n_views * (STAGES ? kStageRec : 9);
    tscm::DeviceMem mem;
    PoseInputs d;
    unsigned char *d_ok = nullptr;
    if (int rc = d.upload(mem, intr9, pix_u, pix_v, count, (size_t)n_views, worlds, n_points, rec, nrec)) return rc;
    HIP_TRY(mem.alloc(&d_ok, (size_t)n_views));
    hipLaunchKernelGGL(k_estimate_extrinsic<STAGES>, dim3((unsigned)((n_views + 63) / 64)), dim3(64), 0, 0, d.intr, d.u, d.v, d.count, n_views, d.worlds, n_points, board_w, d.rec, d_ok);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(rec, d.rec, nrec * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ok, d_ok, (size_t)n_views, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tscm_estimate_extrinsic(const double *intr9, const double *pix_u, const double *pix_v, const int *count, int n_views,
                                       const double *worlds, int n_points, int board_w, int device, double *Rt, int *n_estimated)
{
    if (!intr9 || !worlds || n_views < 0 || n_points < 4 || (n_views > 0 && (!pix_u || !pix_v || !count || !Rt))) return tscm_set_error(TSCM_E_INVALID, "NULL or inconsistent argument");
    if (n_estimated) *n_estimated = 0;
    std::vector<unsigned char> ok(n_views);
    const int rc = extrinsic_views<false>(intr9, pix_u, pix_v, count, n_views, worlds, n_points, board_w, device, Rt, ok.data());
    if (rc) return rc;
    int done = 0;
    for (unsigned char f : ok) done += f;
    if (n_estimated) *n_estimated = done;
    return 0;
}

extern "C" int tscm_estimate_extrinsic_stages(const double *intr9, const double *pix_u, const double *pix_v, const int *count, int n_views,
                                              const double *worlds, int n_points, int board_w, int device, double *Rt, int *n_estimated,
                                              double *T, double *H, double *pose0, double *pose, int *steps, int *exit_code)
{
    if (!intr9 || !worlds || n_views < 0 || n_points < 4 ||
        (n_views > 0 && (!pix_u || !pix_v || !count || !Rt || !T || !H || !pose0 || !pose || !steps || !exit_code)))
        return tscm_set_error(TSCM_E_INVALID, "NULL or inconsistent argument");
    if (n_estimated) *n_estimated = 0;
    std::vector<double> rec((size_t)n_views * kStageRec, NAN);
    for (int k = 0; k < n_views; ++k)
        for (int i = 0; i < 9; ++i) rec[(size_t)kStageRec * k + i] = Rt[9 * (size_t)k + i];
    std::vector<unsigned char> code(n_views);
    const int rc = extrinsic_views<true>(intr9, pix_u, pix_v, count, n_views, worlds, n_points, board_w, device, rec.data(), code.data());
    if (rc) return rc;
    int done = 0;
    for (int k = 0; k < n_views; ++k) {
        const double *r = rec.data() + (size_t)kStageRec * k;
        for (int i = 0; i < 9; ++i) { Rt[9 * (size_t)k + i] = r[i]; T[9 * (size_t)k + i] = r[kStageT + i]; }
        unpack_fit_stages(r, k, H, pose0, pose, steps);
        exit_code[k] = code[k];
        done += code[k] >= TSCM_EXTRINSIC_CONVERGED;
    }
    if (n_estimated) *n_estimated = done;
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// tscm_estimate_extrinsic_ransac: argument checks, one launch of k_estimate_extrinsic_ransac<STAGES>, read-back.
// ---------------------------------------------------------------------------------------------------
extern "C" void tscm_ransac_default_params(tscm_ransac_params *p)
{
    if (!p) return;
    p->struct_size = (int)sizeof(tscm_ransac_params);
    p->threshold_px = 8.0;
    p->n_hypotheses = 256;
    p->min_inliers = 0;
    p->seed = 0;
}

namespace {

struct RansacStages {                       // host pointers of the stages entry, all non-NULL there
    int *samples, *score, *winner;
    double *T, *H_best, *H_refit, *pose0, *pose;
    int *steps;
    double *rms_px;
};

template <bool STAGES>
int ransac_views(const double *intr9, const double *pix_u, const double *pix_v, const int *count, int n_views, const double *worlds,
                 int n_points, int board_w, const tscm_ransac_params *params, int device_index, double *Rt, unsigned char *inlier,
                 int *n_inliers, int *exit_code, int *n_estimated, double *seconds_kernel, const RansacStages &st)
{
    const char *who = STAGES ? "tscm_estimate_extrinsic_ransac_stages" : "tscm_estimate_extrinsic_ransac";
    if (!intr9) return tscm_set_error(TSCM_E_INVALID, "intr9 is NULL");
    if (!worlds) return tscm_set_error(TSCM_E_INVALID, "worlds is NULL");
    if (!params) return tscm_set_error(TSCM_E_INVALID, "params is NULL");
    if (!n_estimated) return tscm_set_error(TSCM_E_INVALID, "n_estimated is NULL");
    if (n_views < 0) return tscm_set_error(TSCM_E_INVALID, "n_views is negative");
    if (n_points < 4) return tscm_set_error(TSCM_E_INVALID, "n_points " + std::to_string(n_points) + " < 4");
    if (n_views > 0) {
        if (!pix_u) return tscm_set_error(TSCM_E_INVALID, "pix_u is NULL");
        if (!pix_v) return tscm_set_error(TSCM_E_INVALID, "pix_v is NULL");
        if (!count) return tscm_set_error(TSCM_E_INVALID, "count is NULL");
        if (!Rt) return tscm_set_error(TSCM_E_INVALID, "Rt is NULL");
        if (!inlier) return tscm_set_error(TSCM_E_INVALID, "inlier is NULL");
        if constexpr (STAGES) {
            const void *ptr[] = { st.samples, st.score, st.winner, st.T, st.H_best, st.H_refit, st.pose0, st.pose, st.steps, st.rms_px };
            const char *name[] = { "samples", "score", "winner", "T", "H_best", "H_refit", "pose0", "pose", "steps", "rms_px" };
            for (int i = 0; i < 10; ++i)
                if (!ptr[i]) return tscm_set_error(TSCM_E_INVALID, std::string(name[i]) + " is NULL");
        }
    }
    if (int rc = tscm::check_struct_size(params, "tscm_ransac_params")) return rc;
    if (!(params->threshold_px > 0.0)) return tscm_set_error(TSCM_E_INVALID, "params: threshold_px " + std::to_string(params->threshold_px) + " is not > 0");
    if (params->n_hypotheses < 1 || params->n_hypotheses > kRansacMaxHypotheses)
        return tscm_set_error(TSCM_E_INVALID, "params: n_hypotheses " + std::to_string(params->n_hypotheses) + " outside 1..4096");
    if (params->min_inliers < 0 || params->min_inliers > n_points || (params->min_inliers >= 1 && params->min_inliers <= 3))
        return tscm_set_error(TSCM_E_INVALID, "params: min_inliers " + std::to_string(params->min_inliers) + " is neither 0 nor in 4..n_points");
    if (board_w < 1 || n_points / 2 - board_w / 2 - 1 < 0) return tscm_set_error(TSCM_E_INVALID, "board_w: board width does not fit the corner count");
    if (n_points > kRansacMaxPoints) return tscm_set_error(TSCM_E_UNSUPPORTED, "n_points: more than 1024 corners per view");
    *n_estimated = 0;
    if (seconds_kernel) *seconds_kernel = 0.0;
    if (n_views == 0) return 0;
    if (int rc = tscm::select_device(device_index, who)) return rc;
    const int min_inliers = params->min_inliers ? params->min_inliers : std::max(4, (n_points + 1) / 2);
    const int H = params->n_hypotheses;
    const size_t V = (size_t)n_views, npix = V * n_points;
    tscm::DeviceMem mem;
    PoseInputs d;
    double *d_stage = nullptr;
    unsigned char *d_in = nullptr;
    int *d_ninl = nullptr, *d_code = nullptr, *d_samples = nullptr, *d_score = nullptr, *d_winner = nullptr;
    if (int rc = d.upload(mem, intr9, pix_u, pix_v, count, V, worlds, n_points, Rt, 9 * V)) return rc;
    HIP_TRY(mem.alloc(&d_in, npix));
    HIP_TRY(hipMemset(d_in, 0, npix));
    HIP_TRY(mem.alloc(&d_ninl, V));
    HIP_TRY(mem.alloc(&d_code, V));
    std::vector<double> rec;
    if constexpr (STAGES) {
        HIP_TRY(mem.alloc(&d_samples, 4 * V * H));
        HIP_TRY(mem.alloc(&d_score, V * H));
        HIP_TRY(hipMemset(d_samples, 0xff, 4 * V * H * sizeof(int)));       // -1
        HIP_TRY(hipMemset(d_score, 0xff, V * H * sizeof(int)));
        HIP_TRY(mem.alloc(&d_winner, V));
        rec.assign(V * kRansacRec, NAN);
        HIP_TRY(mem.upload(&d_stage, rec));
    }
    const size_t lds = ((size_t)34 * n_points + 7) / 8 * 8;
    const double thr2 = params->threshold_px * params->threshold_px;
    tscm::EventSpan span;
    HIP_TRY(span.create(2));
    HIP_TRY(span.mark(0));
    hipLaunchKernelGGL(k_estimate_extrinsic_ransac<STAGES>, dim3((unsigned)n_views), dim3(64), lds, 0, d.intr, d.u, d.v, d.count, d.worlds, n_points, board_w, thr2, H,
                       min_inliers, params->seed, d.rec, d_in, d_ninl, d_code, d_samples, d_score, d_winner, d_stage);
    HIP_TRY(span.finish(1, nullptr, seconds_kernel));
    std::vector<int> code(V), ninl(V);
    HIP_TRY(hipMemcpy(Rt, d.rec, 9 * V * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(inlier, d_in, npix, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(code.data(), d_code, V * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ninl.data(), d_ninl, V * sizeof(int), hipMemcpyDeviceToHost));
    if constexpr (STAGES) {
        HIP_TRY(hipMemcpy(st.samples, d_samples, 4 * V * H * sizeof(int), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(st.score, d_score, V * H * sizeof(int), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(st.winner, d_winner, V * sizeof(int), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(rec.data(), d_stage, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < V; ++k) {
            const double *r = rec.data() + kRansacRec * k;
            for (int i = 0; i < 9; ++i) { st.T[9 * k + i] = r[kRansacT + i]; st.H_best[9 * k + i] = r[kRansacHBest + i]; }
            unpack_fit_stages(r, k, st.H_refit, st.pose0, st.pose, st.steps);
            st.rms_px[k] = r[kRansacRmsPx];
        }
    }
    int done = 0;
    for (size_t k = 0; k < V; ++k) {
        if (exit_code) exit_code[k] = code[k];
        if (n_inliers) n_inliers[k] = ninl[k];
        done += code[k] >= TSCM_EXTRINSIC_CONVERGED && code[k] <= TSCM_EXTRINSIC_GN_CHOLESKY;
    }
    *n_estimated = done;
    return 0;
}

}  // namespace

extern "C" int tscm_estimate_extrinsic_ransac(const double *intr9, const double *pix_u, const double *pix_v, const int *count, int n_views,
                                              const double *worlds, int n_points, int board_w, const tscm_ransac_params *params, int device_index,
                                              double *Rt, unsigned char *inlier, int *n_inliers, int *exit_code, int *n_estimated, double *seconds_kernel)
{
    return ransac_views<false>(intr9, pix_u, pix_v, count, n_views, worlds, n_points, board_w, params, device_index, Rt, inlier, n_inliers, exit_code,
                               n_estimated, seconds_kernel, RansacStages{});
}

extern "C" int tscm_estimate_extrinsic_ransac_stages(const double *intr9, const double *pix_u, const double *pix_v, const int *count, int n_views,
                                                     const double *worlds, int n_points, int board_w, const tscm_ransac_params *params, int device_index,
                                                     double *Rt, unsigned char *inlier, int *n_inliers, int *exit_code, int *n_estimated,
                                                     double *seconds_kernel, int *samples, int *score, int *winner, double *T, double *H_best,
                                                     double *H_refit, double *pose0, double *pose, int *steps, double *rms_px)
{
    const RansacStages st{ samples, score, winner, T, H_best, H_refit, pose0, pose, steps, rms_px };
    return ransac_views<true>(intr9, pix_u, pix_v, count, n_views, worlds, n_points, board_w, params, device_index, Rt, inlier, n_inliers, exit_code,
                              n_estimated, seconds_kernel, st);
}
