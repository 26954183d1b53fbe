// tscm_uncertainty.hip -- projection uncertainty maps (tscm.h: tscm_projection_uncertainty): the 2 x 2 covariance
// of a pixel of camera a transferred to camera b at a given inverse distance (or observed in its own camera), under the
// joint parameter covariance of tscm_covariance:  Cov(q_b) = sigma2 J Sigma_theta J^T, J = d q_b / d theta (2 x 26 or 2 x 13).
//
//   k_uncertainty   grid (pixel blocks, requests), one thread per grid pixel.  What is uniform over a request reaches the
//                   lanes through LDS: the lower triangle of Sigma_theta (351 or 91 doubles, gathered by the host from the
//                   15-wide cam_cov), R and dR/dw of both cameras (one lane each calls rotation_and_derivatives), their
//                   translations and intrinsics.  A lane unprojects its pixel, transfers and projects it, builds the two
//                   rows of J in registers and accumulates J Sigma J^T row of Sigma by row of Sigma (all LDS reads are
//                   broadcasts at compile-time offsets); no 26 x 26 product is held.  The request's summary -- pixels that
//                   project, and the largest sd_worst as the integer maximum of its bit pattern -- goes through LDS integer
//                   atomics to one pair of global integer atomics per workgroup: order-independent.
// All fp64, no floating-point atomics, every sum in a fixed order: two calls give the same bytes.  Every index comes from
// arguments the host checked; a NaN input only produces NaN values, never another address.
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_host.h"
#include "tscm_math.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace tscm;

namespace {

constexpr int kUncThreads = 256;
constexpr int kUncTheta = kFA;                                   // 13 columns of a camera: pose 6, intrinsics 7
constexpr int kUncTri = (2 * kUncTheta) * (2 * kUncTheta + 1) / 2;   // 351: the triangle of a transfer request
constexpr int kUncPlanes = 7;
constexpr int kUncCam = 15;                                      // a camera's width in cam_cov

thread_local double g_last_kernel_seconds = 0.0;

struct UncRequest { int a, b; double iota; };

// The functor's projection of (X, Y, Z) with I = (fx fy cx cy xi lambda alpha) and its derivatives, operation by operation
// as corner_residual_jacobian has them (tscm_math.h): a = d(u, v) / dp row-major, the intrinsic columns are
// (mx 0), (0 my), (1 0), (0 1), (gu[0] gv[0]) xi, (gu[1] gv[1]) lambda, (gu[2] gv[2]) alpha.
struct ProjJ {
    double u, v, k, mx, my;
    double a[6];
    double gu[3], gv[3];
};

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

// the three square-root arguments of unproject_pixel (tscm_math.h) with b = c = 0, in its operations: all > 0?
__device__ __forceinline__ bool unprojects(const double *I, double px, double py)
{
    const double fx = I[0], fy = I[1], cx = I[2], cy = I[3], xi = I[4], lam = I[5], al = I[6];
    const double x = px - cx, y = py - cy;
    const double det = fx * fy;
    const double mx = (fy * x) / det;
    const double my = (fx * y) / det;
    const double ksai = al / (1.0 - al);
    const double r2 = mx * mx + my * my;
    const double a1 = 1.0 + (1.0 - ksai * ksai) * r2;
    const double gamma = (ksai + sqrt(a1)) / (r2 + 1.0);
    const double gk = gamma - ksai;
    const double a2 = (gk * gk - 1.0) * lam * lam + 1.0;
    const double yita = lam * gk + sqrt(a2);
    const double ml = yita * gk - lam;
    const double a3 = xi * xi * (ml * ml - 1.0) + 1.0;
    return a1 > 0.0 && a2 > 0.0 && a3 > 0.0;
}

// J Sigma J^T from the packed lower triangle (row i at i (i + 1) / 2), row by row, in the order tscm.h states
template <int N>
__device__ __forceinline__ void quadratic_form(const double *__restrict__ sT, const double (&Ju)[N], const double (&Jv)[N], double &cuu, double &cuv,
                                               double &cvv)
{
    cuu = 0.0; cuv = 0.0; cvv = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double su = 0.0, sv = 0.0;
#pragma unroll
        for (int j = 0; j < i; ++j) {
            const double s = sT[i * (i + 1) / 2 + j];
            su += s * Ju[j];
            sv += s * Jv[j];
        }
        const double d = sT[i * (i + 1) / 2 + i];
        cuu += Ju[i] * (d * Ju[i] + 2.0 * su);
        cvv += Jv[i] * (d * Jv[i] + 2.0 * sv);
        cuv += Ju[i] * (d * Jv[i] + sv) + Jv[i] * su;
    }
}

// One pixel.  sR[c]: R (9, row-major) and dR/dw_k (27) of camera c = a (0), b (1); sP[c]: t (3), I (7).  out[7]; returns the flags.
template <bool kTransfer>
__device__ __forceinline__ unsigned char pixel_uncertainty(const double *__restrict__ sT, const double (*sR)[36], const double (*sP)[10], double iota,
                                                           double sigma2, double px, double py, int width_b, int height_b, double out[kUncPlanes])
{
    constexpr int N = kTransfer ? 2 * kUncTheta : kUncTheta, OB = kTransfer ? kUncTheta : 0;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int i = 0; i < kUncPlanes; ++i) out[i] = nan;
    const double *Ra = sR[0], *Rb = sR[1], *ta = sP[0], *tb = sP[1], *Ia = sP[0] + 3, *Ib = sP[1] + 3;
    if (!unprojects(Ia, px, py)) return 0;
    const double I9[9] = { Ia[0], Ia[1], Ia[2], Ia[3], Ia[4], Ia[5], Ia[6], 0.0, 0.0 };
    double r[3];
    unproject_pixel(I9, px, py, r);
    const double s0 = r[0] - iota * ta[0], s1 = r[1] - iota * ta[1], s2 = r[2] - iota * ta[2];
    const double D0 = Ra[0] * s0 + Ra[3] * s1 + Ra[6] * s2;
    const double D1 = Ra[1] * s0 + Ra[4] * s1 + Ra[7] * s2;
    const double D2 = Ra[2] * s0 + Ra[5] * s1 + Ra[8] * s2;
    const double X = Rb[0] * D0 + Rb[1] * D1 + Rb[2] * D2 + iota * tb[0];
    const double Y = Rb[3] * D0 + Rb[4] * D1 + Rb[5] * D2 + iota * tb[1];
    const double Z = Rb[6] * D0 + Rb[7] * D1 + Rb[8] * D2 + iota * tb[2];
    ProjJ pb;
    project_jacobian(Ib, X, Y, Z, pb);
    if (!(pb.k > 0.0)) return 1;
    unsigned char fl = 3;
    if (width_b > 0 && height_b > 0 && pb.u >= 0.0 && pb.u <= (double)(width_b - 1) && pb.v >= 0.0 && pb.v <= (double)(height_b - 1)) fl |= 4;

    double Ju[N], Jv[N];
    // camera b: rotation, translation, intrinsics
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double *Dk = Rb + 9 + 9 * k;
        const double g0 = Dk[0] * D0 + Dk[1] * D1 + Dk[2] * D2;
        const double g1 = Dk[3] * D0 + Dk[4] * D1 + Dk[5] * D2;
        const double g2 = Dk[6] * D0 + Dk[7] * D1 + Dk[8] * D2;
        Ju[OB + k] = pb.a[0] * g0 + pb.a[1] * g1 + pb.a[2] * g2;
        Jv[OB + k] = pb.a[3] * g0 + pb.a[4] * g1 + pb.a[5] * g2;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { Ju[OB + 3 + c] = iota * pb.a[c]; Jv[OB + 3 + c] = iota * pb.a[3 + c]; }
    Ju[OB + 6] = pb.mx; Jv[OB + 6] = 0.0;
    Ju[OB + 7] = 0.0;   Jv[OB + 7] = pb.my;
    Ju[OB + 8] = 1.0;   Jv[OB + 8] = 0.0;
    Ju[OB + 9] = 0.0;   Jv[OB + 9] = 1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) { Ju[OB + 10 + c] = pb.gu[c]; Jv[OB + 10 + c] = pb.gv[c]; }

    double eu = 0.0, ev = 0.0;
    if (kTransfer) {
        // AR = A_b R_b, M = AR R_a^T
        double AR[6], M[6];
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) AR[3 * e + c] = pb.a[3 * e] * Rb[c] + pb.a[3 * e + 1] * Rb[3 + c] + pb.a[3 * e + 2] * Rb[6 + c];
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) M[3 * e + c] = AR[3 * e] * Ra[3 * c] + AR[3 * e + 1] * Ra[3 * c + 1] + AR[3 * e + 2] * Ra[3 * c + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {                            // (dR_a,k)^T s
            const double *Dk = Ra + 9 + 9 * k;
            const double h0 = Dk[0] * s0 + Dk[3] * s1 + Dk[6] * s2;
            const double h1 = Dk[1] * s0 + Dk[4] * s1 + Dk[7] * s2;
            const double h2 = Dk[2] * s0 + Dk[5] * s1 + Dk[8] * s2;
            Ju[k] = AR[0] * h0 + AR[1] * h1 + AR[2] * h2;
            Jv[k] = AR[3] * h0 + AR[4] * h1 + AR[5] * h2;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { Ju[3 + c] = -(iota * M[c]); Jv[3 + c] = -(iota * M[3 + c]); }
        // the ray's dependence on I_a: dr = -A_a^T (A_a A_a^T)^-1 G_a dI_a
        ProjJ pa;
        project_jacobian(Ia, r[0], r[1], r[2], pa);
        const double w00 = pa.a[0] * pa.a[0] + pa.a[1] * pa.a[1] + pa.a[2] * pa.a[2];
        const double w01 = pa.a[0] * pa.a[3] + pa.a[1] * pa.a[4] + pa.a[2] * pa.a[5];
        const double w11 = pa.a[3] * pa.a[3] + pa.a[4] * pa.a[4] + pa.a[5] * pa.a[5];
        const double idet = 1.0 / (w00 * w11 - w01 * w01);
        const double ma00 = M[0] * pa.a[0] + M[1] * pa.a[1] + M[2] * pa.a[2], ma01 = M[0] * pa.a[3] + M[1] * pa.a[4] + M[2] * pa.a[5];
        const double ma10 = M[3] * pa.a[0] + M[4] * pa.a[1] + M[5] * pa.a[2], ma11 = M[3] * pa.a[3] + M[4] * pa.a[4] + M[5] * pa.a[5];
        const double n00 = (ma00 * w11 - ma01 * w01) * idet, n01 = (ma01 * w00 - ma00 * w01) * idet;
        const double n10 = (ma10 * w11 - ma11 * w01) * idet, n11 = (ma11 * w00 - ma10 * w01) * idet;
        Ju[6] = -(n00 * pa.mx); Jv[6] = -(n10 * pa.mx);
        Ju[7] = -(n01 * pa.my); Jv[7] = -(n11 * pa.my);
        Ju[8] = -n00;           Jv[8] = -n10;
        Ju[9] = -n01;           Jv[9] = -n11;
#pragma unroll
        for (int c = 0; c < 3; ++c) { Ju[10 + c] = -(n00 * pa.gu[c] + n01 * pa.gv[c]); Jv[10 + c] = -(n10 * pa.gu[c] + n11 * pa.gv[c]); }
        // e = d q_b / d iota = A_b t_b - M t_a
        eu = (pb.a[0] * tb[0] + pb.a[1] * tb[1] + pb.a[2] * tb[2]) - (M[0] * ta[0] + M[1] * ta[1] + M[2] * ta[2]);
        ev = (pb.a[3] * tb[0] + pb.a[4] * tb[1] + pb.a[5] * tb[2]) - (M[3] * ta[0] + M[4] * ta[1] + M[5] * ta[2]);
    }
    double cuu, cuv, cvv;
    quadratic_form<N>(sT, Ju, Jv, cuu, cuv, cvv);
    cuu *= sigma2; cuv *= sigma2; cvv *= sigma2;
    out[0] = pb.u; out[1] = pb.v; out[2] = cuu; out[3] = cuv; out[4] = cvv;
    const double dd = cuu - cvv;
    out[5] = sqrt(0.5 * (cuu + cvv + sqrt(dd * dd + 4.0 * cuv * cuv)));
    if (kTransfer) {
        const double e2 = eu * eu + ev * ev;
        if (e2 > 0.0) out[6] = sqrt((ev * ev * cuu - 2.0 * eu * ev * cuv + eu * eu * cvv) / e2);
    }
    return fl;
}

// tri [R][kUncTri], summary [R][2]: bit pattern of the largest sd_worst, number of valid pixels (zeroed by the host)
__global__ __launch_bounds__(kUncThreads) void k_uncertainty(const double *__restrict__ cam_rt, const double *__restrict__ intr,
                                                             const double *__restrict__ tri, const UncRequest *__restrict__ req, int nx, int npix,
                                                             int width_b, int height_b, double x0, double y0, double dx, double dy, double sigma2,
                                                             double *__restrict__ planes, unsigned char *__restrict__ flags,
                                                             unsigned long long *__restrict__ summary)
{
    __shared__ double sT[kUncTri];
    __shared__ double sR[2][36];
    __shared__ double sP[2][10];
    __shared__ unsigned long long sMax;
    __shared__ unsigned int sCnt;
    const int tid = threadIdx.x, rq = blockIdx.y;
    const int a = req[rq].a, b = req[rq].b;
    const double iota = req[rq].iota;
    const bool transfer = a != b;
    const int ntri = transfer ? kUncTri : kUncTheta * (kUncTheta + 1) / 2;
    for (int q = tid; q < ntri; q += kUncThreads) sT[q] = tri[(size_t)kUncTri * rq + q];
    if (tid == 0) { sMax = 0ull; sCnt = 0u; }
    if (tid == 0 || tid == 64) {                                 // a lane of two different waves: one camera each
        const int c = tid == 0 ? 0 : 1, cam = c == 0 ? a : b;
        const double w[3] = { cam_rt[6 * cam], cam_rt[6 * cam + 1], cam_rt[6 * cam + 2] };
        rotation_and_derivatives(w, sR[c], sR[c] + 9);
    }
    if (tid >= 128 && tid < 148) {
        const int c = (tid - 128) / 10, j = (tid - 128) % 10, cam = c == 0 ? a : b;
        sP[c][j] = j < 3 ? cam_rt[6 * cam + 3 + j] : intr[9 * cam + j - 3];
    }
    __syncthreads();
    const int p = blockIdx.x * kUncThreads + tid;
    if (p < npix) {
        const int col = p % nx, row = p / nx;
        const double px = x0 + col * dx, py = y0 + row * dy;
        double out[kUncPlanes];
        unsigned char fl;
        if (transfer) fl = pixel_uncertainty<true>(sT, sR, sP, iota, sigma2, px, py, width_b, height_b, out);
        else fl = pixel_uncertainty<false>(sT, sR, sP, iota, sigma2, px, py, width_b, height_b, out);
#pragma unroll
        for (int k = 0; k < kUncPlanes; ++k) planes[((size_t)rq * kUncPlanes + k) * npix + p] = out[k];
        flags[(size_t)rq * npix + p] = fl;
        if ((fl & 3) == 3) {
            atomicAdd(&sCnt, 1u);
            if (out[5] > 0.0) atomicMax(&sMax, (unsigned long long)__double_as_longlong(out[5]));
        }
    }
    __syncthreads();
    if (tid == 0 && sCnt > 0u) {
        atomicMax(&summary[2 * rq], sMax);
        atomicAdd(&summary[2 * rq + 1], (unsigned long long)sCnt);
    }
}

int invalid(const std::string &msg) { return tscm_set_error(TSCM_E_INVALID, msg); }

}  // namespace

extern "C" int tscm_projection_uncertainty(int n_cameras, const double *cam_rt, const double *intr, const double *cam_cov, double sigma2,
                                           const tscm_uncertainty_grid *grid, const tscm_uncertainty_request *requests, int n_requests, int device,
                                           double *planes, unsigned char *flags, double *max_sd, long long *n_valid)
{
    g_last_kernel_seconds = 0.0;
    if (n_cameras < 1 || n_cameras > 32) return invalid("n_cameras " + std::to_string(n_cameras) + " outside 1..32");
    if (!cam_rt) return invalid("cam_rt is NULL");
    if (!intr) return invalid("intr is NULL");
    if (!cam_cov) return invalid("cam_cov is NULL");
    if (!(sigma2 >= 0.0)) return invalid("sigma2 must be >= 0 and not NaN");
    if (!grid) return invalid("grid is NULL");
    if (int rc = check_struct_size(grid, "tscm_uncertainty_grid", "grid")) return rc;
    if (grid->nx <= 0) return invalid("grid: nx " + std::to_string(grid->nx) + " <= 0");
    if (grid->ny <= 0) return invalid("grid: ny " + std::to_string(grid->ny) + " <= 0");
    if ((long long)grid->nx * grid->ny > (1ll << 30)) return invalid("grid: nx * ny above 2^30");
    if (!std::isfinite(grid->x0) || !std::isfinite(grid->y0)) return invalid("grid: x0 or y0 is not finite");
    if (!std::isfinite(grid->dx)) return invalid("grid: dx is not finite");
    if (!std::isfinite(grid->dy)) return invalid("grid: dy is not finite");
    if (!requests) return invalid("requests is NULL");
    if (n_requests <= 0) return invalid("n_requests " + std::to_string(n_requests) + " <= 0");
    if (n_requests > 65535) return invalid("n_requests " + std::to_string(n_requests) + " above 65535");
    for (int r = 0; r < n_requests; ++r) {
        const tscm_uncertainty_request &q = requests[r];
        const std::string at = "requests[" + std::to_string(r) + "]: ";
        if (q.camera_a < 0 || q.camera_a >= n_cameras) return invalid(at + "camera_a " + std::to_string(q.camera_a) + " out of range");
        if (q.camera_b < 0 || q.camera_b >= n_cameras) return invalid(at + "camera_b " + std::to_string(q.camera_b) + " out of range");
        if (!std::isfinite(q.inv_distance) || q.inv_distance < 0.0) return invalid(at + "inv_distance must be finite and >= 0");
    }
    if (!planes) return invalid("planes is NULL");
    if (!flags) return invalid("flags is NULL");
    if (int rc = select_device(device, "tscm_projection_uncertainty")) return rc;

    // Sigma_theta of every request: the lower triangle over theta's columns, b and c of the 15-wide layout skipped
    const int C = n_cameras, R = n_requests, npix = grid->nx * grid->ny;
    const size_t n15 = (size_t)kUncCam * C;
    std::vector<double> tri((size_t)kUncTri * R, 0.0);
    std::vector<UncRequest> req(R);
    for (int r = 0; r < R; ++r) {
        const int a = requests[r].camera_a, b = requests[r].camera_b, n = a != b ? 2 * kUncTheta : kUncTheta;
        req[r] = UncRequest{ a, b, requests[r].inv_distance };
        double *t = tri.data() + (size_t)kUncTri * r;
        for (int i = 0; i < n; ++i) {
            const size_t wi = (size_t)kUncCam * (i < kUncTheta ? a : b) + i % kUncTheta;
            for (int j = 0; j <= i; ++j) {
                const size_t wj = (size_t)kUncCam * (j < kUncTheta ? a : b) + j % kUncTheta;
                t[i * (i + 1) / 2 + j] = cam_cov[wi * n15 + wj];
            }
        }
    }
    DeviceMem mem;
    EventSpan span;
    const double *d_rt = nullptr, *d_intr = nullptr, *d_tri = nullptr;
    const UncRequest *d_req = nullptr;
    double *d_planes = nullptr;
    unsigned char *d_flags = nullptr;
    unsigned long long *d_sum = nullptr;
    HIP_TRY(mem.upload(&d_rt, cam_rt, (size_t)6 * C));
    HIP_TRY(mem.upload(&d_intr, intr, (size_t)9 * C));
    HIP_TRY(mem.upload(&d_tri, tri));
    HIP_TRY(mem.upload(&d_req, req));
    HIP_TRY(mem.alloc(&d_planes, (size_t)R * kUncPlanes * npix));
    HIP_TRY(mem.alloc(&d_flags, (size_t)R * npix));
    HIP_TRY(mem.alloc(&d_sum, (size_t)2 * R));
    HIP_TRY(hipMemset(d_sum, 0, sizeof(unsigned long long) * 2 * (size_t)R));
    HIP_TRY(span.create(2));
    HIP_TRY(span.mark(0));
    hipLaunchKernelGGL(k_uncertainty, dim3((npix + kUncThreads - 1) / kUncThreads, R), dim3(kUncThreads), 0, 0, d_rt, d_intr, d_tri, d_req, grid->nx, npix,
                       grid->width_b, grid->height_b, grid->x0, grid->y0, grid->dx, grid->dy, sigma2, d_planes, d_flags, d_sum);
    double seconds = 0.0;
    HIP_TRY(span.finish(1, &seconds, nullptr));
    g_last_kernel_seconds = seconds;
    HIP_TRY(hipMemcpy(planes, d_planes, sizeof(double) * (size_t)R * kUncPlanes * npix, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(flags, d_flags, (size_t)R * npix, hipMemcpyDeviceToHost));
    if (max_sd || n_valid) {
        std::vector<unsigned long long> sum((size_t)2 * R);
        HIP_TRY(hipMemcpy(sum.data(), d_sum, sizeof(unsigned long long) * sum.size(), hipMemcpyDeviceToHost));
        for (int r = 0; r < R; ++r) {
            if (max_sd) std::memcpy(&max_sd[r], &sum[2 * (size_t)r], sizeof(double));
            if (n_valid) n_valid[r] = (long long)sum[2 * (size_t)r + 1];
        }
    }
    return 0;
}

extern "C" double tscm_projection_uncertainty_seconds(void) { return g_last_kernel_seconds; }
