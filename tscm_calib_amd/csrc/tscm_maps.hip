// tscm_maps.hip -- remap-table generation: TripleSphereCamera::undistort
// (TS.cpp:284-306), the table of undistort_chessboard (TS.cpp:308-330) and the rectification tables
// of EpipolarRectify/rectify.cpp:86-199, all instances of one per-pixel loop (see tscm.h).
// One thread per 4 consecutive output pixels of a row, float4 stores where the row allows it;
// the map descriptor is wave-uniform (blockIdx.y) and read through the scalar path.
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_fastmath.h"
#include "tscm_host.h"
#include "tscm_math.h"

#include <cmath>
#include <string>
#include <vector>

using namespace tscm;

namespace {

// the reference's arithmetic, operation by operation (x86-64 gcc without FMA contraction)
__device__ __forceinline__ void map_pixel_exact(const tscm_map_desc &m, double beta, int i, int j, float &mx, float &my)
{
    const double x0 = __ddiv_rn(__dsub_rn((double)j, m.cx), m.fx);
    const double y0 = __ddiv_rn(__dsub_rn((double)i, m.cy), m.fy);
    // cv::Mat product R * p: sum over k in order, starting from the first product
    const double X = __dadd_rn(__dadd_rn(__dmul_rn(m.R[0], x0), __dmul_rn(m.R[1], y0)), m.R[2]);
    const double Y = __dadd_rn(__dadd_rn(__dmul_rn(m.R[3], x0), __dmul_rn(m.R[4], y0)), m.R[5]);
    const double Z = __dadd_rn(__dadd_rn(__dmul_rn(m.R[6], x0), __dmul_rn(m.R[7], y0)), m.R[8]);
    const double rho2 = __dadd_rn(__dmul_rn(X, X), __dmul_rn(Y, Y));
    const double d1 = __dsqrt_rn(__dadd_rn(rho2, __dmul_rn(Z, Z)));
    const double z1 = __dadd_rn(Z, __dmul_rn(m.intr[4], d1));
    const double d2 = __dsqrt_rn(__dadd_rn(rho2, __dmul_rn(z1, z1)));
    const double z2 = __dadd_rn(z1, __dmul_rn(m.intr[5], d2));
    const double d3 = __dsqrt_rn(__dadd_rn(rho2, __dmul_rn(z2, z2)));
    const double ksai = __dadd_rn(z2, __dmul_rn(beta, d3));
    double u = __dadd_rn(__dadd_rn(__ddiv_rn(__dmul_rn(m.intr[0], X), ksai), __ddiv_rn(__dmul_rn(m.intr[7], Y), ksai)), m.intr[2]);
    double v = __dadd_rn(__dadd_rn(__ddiv_rn(__dmul_rn(m.intr[8], X), ksai), __ddiv_rn(__dmul_rn(m.intr[1], Y), ksai)), m.intr[3]);
    if (m.check_w2 && Z <= __dmul_rn(-m.w2, d1)) { u = -1.0; v = -1.0; }
    mx = (float)__dadd_rn(u, m.offset_x);
    my = (float)__dadd_rn(v, m.offset_y);
}

__device__ __forceinline__ void map_pixel_fast(const tscm_map_desc &m, double beta, double ifx, double ify, int i, int j, float &mx, float &my)
{
    const double x0 = ((double)j - m.cx) * ifx, y0 = ((double)i - m.cy) * ify;
    const double X = __builtin_fma(m.R[0], x0, __builtin_fma(m.R[1], y0, m.R[2]));
    const double Y = __builtin_fma(m.R[3], x0, __builtin_fma(m.R[4], y0, m.R[5]));
    const double Z = __builtin_fma(m.R[6], x0, __builtin_fma(m.R[7], y0, m.R[8]));
    const double rho2 = __builtin_fma(Y, Y, X * X);
    const double s1 = __builtin_fma(Z, Z, rho2);
    const double d1 = s1 * fast_rsqrt(s1);
    const double z1 = __builtin_fma(m.intr[4], d1, Z);
    const double s2 = __builtin_fma(z1, z1, rho2);
    const double d2 = s2 * fast_rsqrt(s2);
    const double z2 = __builtin_fma(m.intr[5], d2, z1);
    const double s3 = __builtin_fma(z2, z2, rho2);
    const double d3 = s3 * fast_rsqrt(s3);
    const double ik = fast_rcp(__builtin_fma(beta, d3, z2));
    const double xn = X * ik, yn = Y * ik;
    double u = __builtin_fma(m.intr[0], xn, __builtin_fma(m.intr[7], yn, m.intr[2]));
    double v = __builtin_fma(m.intr[8], xn, __builtin_fma(m.intr[1], yn, m.intr[3]));
    if (m.check_w2 && Z <= -m.w2 * d1) { u = -1.0; v = -1.0; }
    mx = (float)(u + m.offset_x);
    my = (float)(v + m.offset_y);
}

// grid (ceil(max quads per map / 256), n_maps) x 256.  A quad = 4 consecutive output ELEMENTS:
// for a contiguous table (out_stride == width) quads run over the flat element index, crossing row
// ends, so that every store is one aligned float4 when out_offset is a multiple of 4; tables with
// row padding use quads inside a row.
template <bool EXACT>
__global__ __launch_bounds__(256) void k_build_maps(const tscm_map_desc *__restrict__ maps, float *__restrict__ mapx, float *__restrict__ mapy)
{
    const tscm_map_desc m = maps[blockIdx.y];
    const bool flat = m.out_stride == m.width;
    const int qpr = (m.width + 3) >> 2;                       // quads per row (padded tables)
    const long long total = (long long)m.width * m.height;
    const long long nquads = flat ? (total + 3) >> 2 : (long long)qpr * m.height;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nquads) return;
    // row / column of the quad's first element without an integer division: fp64 quotient + one correction
    const int den = flat ? m.width : qpr;
    const long long num = flat ? 4 * q : q;
    int i = (int)((double)num * fast_rcp((double)den));
    int r = (int)(num - (long long)i * den);
    if (r < 0) { --i; r += den; }
    if (r >= den) { ++i; r -= den; }
    int j = flat ? r : r * 4;
    const double beta = EXACT ? __ddiv_rn(m.intr[6], __dsub_rn(1.0, m.intr[6])) : m.intr[6] * fast_rcp(1.0 - m.intr[6]);
    const double ifx = EXACT ? 0.0 : fast_rcp(m.fx), ify = EXACT ? 0.0 : fast_rcp(m.fy);
    const long long base = m.out_offset + (flat ? 4 * q : (long long)i * m.out_stride + j);
    const int n = flat ? (int)min(4LL, total - 4 * q) : min(4, m.width - j);
    float ox[4], oy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (EXACT) map_pixel_exact(m, beta, i, j, ox[k], oy[k]);
        else map_pixel_fast(m, beta, ifx, ify, i, j, ox[k], oy[k]);
        if (++j == m.width) { j = 0; ++i; }                  // flat quads continue on the next row
    }
    if (n == 4 && (base & 3) == 0) {
        *reinterpret_cast<float4 *>(mapx + base) = make_float4(ox[0], ox[1], ox[2], ox[3]);
        *reinterpret_cast<float4 *>(mapy + base) = make_float4(oy[0], oy[1], oy[2], oy[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) { mapx[base + k] = ox[k]; mapy[base + k] = oy[k]; }
    }
}

// ------------------------------------------------------------------------------------------------
// Output images that are not pinholes (tscm.h: TSCM_PROJ_*).  Only the ray of an output element changes; from the ray
// on -- R, TripleSphereCamera::project, the w2 rule, the offsets -- the arithmetic is that of map_pixel_*, with the
// third ray component no longer the constant 1.
__device__ __forceinline__ void map_ray_exact(const tscm_map_desc &m, double beta, double x, double y, double z, float &mx, float &my)
{
    const double X = __dadd_rn(__dadd_rn(__dmul_rn(m.R[0], x), __dmul_rn(m.R[1], y)), __dmul_rn(m.R[2], z));
    const double Y = __dadd_rn(__dadd_rn(__dmul_rn(m.R[3], x), __dmul_rn(m.R[4], y)), __dmul_rn(m.R[5], z));
    const double Z = __dadd_rn(__dadd_rn(__dmul_rn(m.R[6], x), __dmul_rn(m.R[7], y)), __dmul_rn(m.R[8], z));
    const double rho2 = __dadd_rn(__dmul_rn(X, X), __dmul_rn(Y, Y));
    const double d1 = __dsqrt_rn(__dadd_rn(rho2, __dmul_rn(Z, Z)));
    const double z1 = __dadd_rn(Z, __dmul_rn(m.intr[4], d1));
    const double d2 = __dsqrt_rn(__dadd_rn(rho2, __dmul_rn(z1, z1)));
    const double z2 = __dadd_rn(z1, __dmul_rn(m.intr[5], d2));
    const double d3 = __dsqrt_rn(__dadd_rn(rho2, __dmul_rn(z2, z2)));
    const double ksai = __dadd_rn(z2, __dmul_rn(beta, d3));
    double u = __dadd_rn(__dadd_rn(__ddiv_rn(__dmul_rn(m.intr[0], X), ksai), __ddiv_rn(__dmul_rn(m.intr[7], Y), ksai)), m.intr[2]);
    double v = __dadd_rn(__dadd_rn(__ddiv_rn(__dmul_rn(m.intr[8], X), ksai), __ddiv_rn(__dmul_rn(m.intr[1], Y), ksai)), m.intr[3]);
    if (m.check_w2 && Z <= __dmul_rn(-m.w2, d1)) { u = -1.0; v = -1.0; }
    mx = (float)__dadd_rn(u, m.offset_x);
    my = (float)__dadd_rn(v, m.offset_y);
}

__device__ __forceinline__ void map_ray_fast(const tscm_map_desc &m, double beta, double x, double y, double z, float &mx, float &my)
{
    const double X = __builtin_fma(m.R[0], x, __builtin_fma(m.R[1], y, m.R[2] * z));
    const double Y = __builtin_fma(m.R[3], x, __builtin_fma(m.R[4], y, m.R[5] * z));
    const double Z = __builtin_fma(m.R[6], x, __builtin_fma(m.R[7], y, m.R[8] * z));
    const double rho2 = __builtin_fma(Y, Y, X * X);
    const double s1 = __builtin_fma(Z, Z, rho2);
    const double d1 = s1 * fast_rsqrt(s1);
    const double z1 = __builtin_fma(m.intr[4], d1, Z);
    const double s2 = __builtin_fma(z1, z1, rho2);
    const double d2 = s2 * fast_rsqrt(s2);
    const double z2 = __builtin_fma(m.intr[5], d2, z1);
    const double s3 = __builtin_fma(z2, z2, rho2);
    const double d3 = s3 * fast_rsqrt(s3);
    const double ik = fast_rcp(__builtin_fma(beta, d3, z2));
    const double xn = X * ik, yn = Y * ik;
    double u = __builtin_fma(m.intr[0], xn, __builtin_fma(m.intr[7], yn, m.intr[2]));
    double v = __builtin_fma(m.intr[8], xn, __builtin_fma(m.intr[1], yn, m.intr[3]));
    if (m.check_w2 && Z <= -m.w2 * d1) { u = -1.0; v = -1.0; }
    mx = (float)(u + m.offset_x);
    my = (float)(v + m.offset_y);
}

// The part of the ray that depends on the output row alone: b = (i - cy)/fy for CYLINDRICAL and STEREOGRAPHIC,
// (sin b, cos b) for LONGLAT and EQUIRECT.  One per quad (and one more where a flat quad runs over a row end).
template <bool EXACT>
__device__ __forceinline__ void row_term(const tscm_map_desc &m, int kind, double ify, int i, double &p, double &q)
{
    const double b = EXACT ? __ddiv_rn(__dsub_rn((double)i, m.cy), m.fy) : ((double)i - m.cy) * ify;
    p = b; q = 0.0;
    if (kind == TSCM_PROJ_LONGLAT || kind == TSCM_PROJ_EQUIRECT) sincos(b, &p, &q);
}

// k_build_maps for batches with a projection kind other than PERSPECTIVE among them: same grid, same quads, same stores;
// the kind of a map comes from a second wave-uniform array, so the branch on it is uniform.  PERSPECTIVE maps of the batch
// go through map_pixel_exact / map_pixel_fast and keep their bits.
template <bool EXACT>
__global__ __launch_bounds__(256) void k_build_maps_proj(const tscm_map_desc *__restrict__ maps, const int *__restrict__ kinds, float *__restrict__ mapx,
                                                         float *__restrict__ mapy)
{
    const tscm_map_desc m = maps[blockIdx.y];
    const int kind = kinds[blockIdx.y];
    const bool flat = m.out_stride == m.width;
    const int qpr = (m.width + 3) >> 2;
    const long long total = (long long)m.width * m.height;
    const long long nquads = flat ? (total + 3) >> 2 : (long long)qpr * m.height;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nquads) return;
    const int den = flat ? m.width : qpr;
    const long long num = flat ? 4 * q : q;
    int i = (int)((double)num * fast_rcp((double)den));
    int r = (int)(num - (long long)i * den);
    if (r < 0) { --i; r += den; }
    if (r >= den) { ++i; r -= den; }
    int j = flat ? r : r * 4;
    const double beta = EXACT ? __ddiv_rn(m.intr[6], __dsub_rn(1.0, m.intr[6])) : m.intr[6] * fast_rcp(1.0 - m.intr[6]);
    const double ifx = EXACT ? 0.0 : fast_rcp(m.fx), ify = EXACT ? 0.0 : fast_rcp(m.fy);
    const long long base = m.out_offset + (flat ? 4 * q : (long long)i * m.out_stride + j);
    const int n = flat ? (int)min(4LL, total - 4 * q) : min(4, m.width - j);
    float ox[4], oy[4];
    if (kind == TSCM_PROJ_PERSPECTIVE) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (EXACT) map_pixel_exact(m, beta, i, j, ox[k], oy[k]);
            else map_pixel_fast(m, beta, ifx, ify, i, j, ox[k], oy[k]);
            if (++j == m.width) { j = 0; ++i; }
        }
    } else {
        double rp, rq;
        row_term<EXACT>(m, kind, ify, i, rp, rq);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double a = EXACT ? __ddiv_rn(__dsub_rn((double)j, m.cx), m.fx) : ((double)j - m.cx) * ifx;
            double x, y, z;
            if (kind == TSCM_PROJ_STEREOGRAPHIC) {
                const double h = 0.25 * __builtin_fma(a, a, rp * rp);
                const double inv = EXACT ? __ddiv_rn(1.0, 1.0 + h) : fast_rcp(1.0 + h);
                x = a * inv; y = rp * inv; z = (1.0 - h) * inv;
            } else {
                double sa, ca;
                sincos(a, &sa, &ca);
                if (kind == TSCM_PROJ_LONGLAT) { x = sa; y = ca * rp; z = ca * rq; }
                else if (kind == TSCM_PROJ_CYLINDRICAL) { x = sa; y = rp; z = ca; }
                else { x = rq * sa; y = rp; z = rq * ca; }                      // EQUIRECT
            }
            if (EXACT) map_ray_exact(m, beta, x, y, z, ox[k], oy[k]);
            else map_ray_fast(m, beta, x, y, z, ox[k], oy[k]);
            if (++j == m.width) { j = 0; ++i; if (k < 3) row_term<EXACT>(m, kind, ify, i, rp, rq); }
        }
    }
    if (n == 4 && (base & 3) == 0) {
        *reinterpret_cast<float4 *>(mapx + base) = make_float4(ox[0], ox[1], ox[2], ox[3]);
        *reinterpret_cast<float4 *>(mapy + base) = make_float4(oy[0], oy[1], oy[2], oy[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) { mapx[base + k] = ox[k]; mapy[base + k] = oy[k]; }
    }
}

// tscm_build_sweep_maps: the sibling of k_build_maps_proj for the sphere sweep.  Table (k, z) = blockIdx.y of [n][D] looks
// from camera k at the point dir / inv_distance[z]: the ray in front of R is dir - inv_distance[z] * centers[k] (the point
// seen from the camera centre, scaled by inv, which the projection ignores; inv = 0 leaves dir itself, bit for bit).  Same
// quads, same stores; the output is dense, plane (k, z) at element (k * D + z) * width * height.
template <bool EXACT>
__global__ __launch_bounds__(256) void k_build_maps_sweep(const tscm_map_desc *__restrict__ maps, const int *__restrict__ kinds, const double *__restrict__ centers,
                                                          const double *__restrict__ inv_distance, int D, float *__restrict__ mapx, float *__restrict__ mapy)
{
    const int cam = blockIdx.y / D, hyp = blockIdx.y - cam * D;
    const tscm_map_desc m = maps[cam];
    const int kind = kinds[cam];
    const double inv = inv_distance[hyp], tx = centers[3 * cam], ty = centers[3 * cam + 1], tz = centers[3 * cam + 2];
    const long long total = (long long)m.width * m.height;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (total + 3) >> 2) return;
    const long long num = 4 * q;
    int i = (int)((double)num * fast_rcp((double)m.width));
    int j = (int)(num - (long long)i * m.width);
    if (j < 0) { --i; j += m.width; }
    if (j >= m.width) { ++i; j -= m.width; }
    const double beta = EXACT ? __ddiv_rn(m.intr[6], __dsub_rn(1.0, m.intr[6])) : m.intr[6] * fast_rcp(1.0 - m.intr[6]);
    const double ifx = EXACT ? 0.0 : fast_rcp(m.fx), ify = EXACT ? 0.0 : fast_rcp(m.fy);
    const long long base = (long long)blockIdx.y * total + 4 * q;
    const int n = (int)min(4LL, total - 4 * q);
    float ox[4], oy[4];
    double rp, rq;
    row_term<EXACT>(m, kind, ify, i, rp, rq);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double a = EXACT ? __ddiv_rn(__dsub_rn((double)j, m.cx), m.fx) : ((double)j - m.cx) * ifx;
        double x, y, z;
        if (kind == TSCM_PROJ_STEREOGRAPHIC) {
            const double h = 0.25 * __builtin_fma(a, a, rp * rp);
            const double ih = EXACT ? __ddiv_rn(1.0, 1.0 + h) : fast_rcp(1.0 + h);
            x = a * ih; y = rp * ih; z = (1.0 - h) * ih;
        } else {
            double sa, ca;
            sincos(a, &sa, &ca);
            if (kind == TSCM_PROJ_LONGLAT) { x = sa; y = ca * rp; z = ca * rq; }
            else if (kind == TSCM_PROJ_CYLINDRICAL) { x = sa; y = rp; z = ca; }
            else { x = rq * sa; y = rp; z = rq * ca; }                      // EQUIRECT
        }
        if (EXACT) {
            x = __dsub_rn(x, __dmul_rn(inv, tx)); y = __dsub_rn(y, __dmul_rn(inv, ty)); z = __dsub_rn(z, __dmul_rn(inv, tz));
            map_ray_exact(m, beta, x, y, z, ox[k], oy[k]);
        } else {
            x = __builtin_fma(-inv, tx, x); y = __builtin_fma(-inv, ty, y); z = __builtin_fma(-inv, tz, z);
            map_ray_fast(m, beta, x, y, z, ox[k], oy[k]);
        }
        if (++j == m.width) { j = 0; ++i; if (k < 3) row_term<EXACT>(m, kind, ify, i, rp, rq); }
    }
    if (n == 4 && (base & 3) == 0) {
        *reinterpret_cast<float4 *>(mapx + base) = make_float4(ox[0], ox[1], ox[2], ox[3]);
        *reinterpret_cast<float4 *>(mapy + base) = make_float4(oy[0], oy[1], oy[2], oy[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) { mapx[base + k] = ox[k]; mapy[base + k] = oy[k]; }
    }
}

// tscm_rectify_points: one thread per pixel of the sampled camera -> its place in the output image of `m`
__global__ __launch_bounds__(256) void k_rectify_points(const tscm_map_desc *__restrict__ map, int kind, const double *__restrict__ pixels, int n,
                                                        double *__restrict__ out, unsigned char *__restrict__ valid)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const tscm_map_desc m = map[0];
    double c[3];
    unproject_pixel(m.intr, pixels[2 * t], pixels[2 * t + 1], c);
    bool ok = c[0] == c[0] && c[1] == c[1] && c[2] == c[2];
    if (m.check_w2 && c[2] <= -m.w2 * sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])) ok = false;
    const double x = m.R[0] * c[0] + m.R[3] * c[1] + m.R[6] * c[2];              // R^T
    const double y = m.R[1] * c[0] + m.R[4] * c[1] + m.R[7] * c[2];
    const double z = m.R[2] * c[0] + m.R[5] * c[1] + m.R[8] * c[2];
    double a = 0.0, b = 0.0;
    if (kind == TSCM_PROJ_PERSPECTIVE) {
        if (z <= 0.0) ok = false;
        a = x / z; b = y / z;
    } else if (kind == TSCM_PROJ_LONGLAT) {
        a = atan2(x, hypot(y, z)); b = atan2(y, z);
    } else if (kind == TSCM_PROJ_CYLINDRICAL) {
        const double h = hypot(x, z);
        if (h == 0.0) ok = false;
        a = atan2(x, z); b = y / h;
    } else if (kind == TSCM_PROJ_STEREOGRAPHIC) {
        const double nrm = sqrt(x * x + y * y + z * z), d = nrm + z;
        if (!(d > 0.0)) ok = false;
        a = 2.0 * x / d; b = 2.0 * y / d;
    } else {
        a = atan2(x, z); b = atan2(y, hypot(x, z));
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    out[2 * t] = ok ? a * m.fx + m.cx : nan;
    out[2 * t + 1] = ok ? b * m.fy + m.cy : nan;
    valid[t] = ok ? 1 : 0;
}

}  // namespace

// kinds == NULL: every map is a pinhole, k_build_maps; otherwise [n_maps] valid kinds, k_build_maps_proj
static int build_maps_host(const tscm_map_desc *maps, const int *kinds, int n_maps, int device, int exact, float *mapx, float *mapy, size_t n_elems,
                           double *seconds_kernel)
{
    if (n_maps < 0 || (n_maps > 0 && (!maps || !mapx || !mapy))) return tscm_set_error(TSCM_E_INVALID, "NULL argument");
    if (n_maps > 65535) return tscm_set_error(TSCM_E_UNSUPPORTED, "more than 65535 maps in one call");
    long long max_quads = 0;
    unsigned long long covered = 0;
    for (int m = 0; m < n_maps; ++m) {
        const tscm_map_desc &d = maps[m];
        if (d.width < 0 || d.height < 0 || d.out_stride < d.width || d.out_offset < 0) return tscm_set_error(TSCM_E_INVALID, "map " + std::to_string(m) + ": bad geometry");
        if (d.width == 0 || d.height == 0) continue;
        const unsigned long long last = (unsigned long long)d.out_offset + (unsigned long long)(d.height - 1) * d.out_stride + d.width;
        if (last > n_elems) return tscm_set_error(TSCM_E_INVALID, "map " + std::to_string(m) + " does not fit the output arrays");
        max_quads = std::max(max_quads, d.out_stride == d.width ? ((long long)d.width * d.height + 3) / 4 : (long long)((d.width + 3) / 4) * d.height);
        covered += (unsigned long long)d.width * d.height;
    }
    if (int rc = select_device(device, "tscm_build_maps")) return rc;
    if (seconds_kernel) *seconds_kernel = 0.0;
    if (n_maps == 0 || max_quads == 0) return 0;
    DeviceMem mem;
    const tscm_map_desc *d_maps = nullptr;
    const int *d_kinds = nullptr;
    float *d_x = nullptr, *d_y = nullptr;
    HIP_TRY(mem.upload(&d_maps, maps, (size_t)n_maps));
    if (kinds) HIP_TRY(mem.upload(&d_kinds, kinds, (size_t)n_maps));
    // elements no map covers (row padding, gaps) keep the caller's values
    if (covered < n_elems) {
        HIP_TRY(mem.upload(&d_x, mapx, n_elems)); HIP_TRY(mem.upload(&d_y, mapy, n_elems));
    } else {
        HIP_TRY(mem.alloc(&d_x, n_elems)); HIP_TRY(mem.alloc(&d_y, n_elems));
    }
    EventSpan span;
    HIP_TRY(span.create(2));
    HIP_TRY(span.mark(0));
    const dim3 grid((unsigned)((max_quads + 255) / 256), (unsigned)n_maps);
    if (!kinds) {
        if (exact) hipLaunchKernelGGL(k_build_maps<true>, grid, dim3(256), 0, 0, d_maps, d_x, d_y);
        else hipLaunchKernelGGL(k_build_maps<false>, grid, dim3(256), 0, 0, d_maps, d_x, d_y);
    } else {
        if (exact) hipLaunchKernelGGL(k_build_maps_proj<true>, grid, dim3(256), 0, 0, d_maps, d_kinds, d_x, d_y);
        else hipLaunchKernelGGL(k_build_maps_proj<false>, grid, dim3(256), 0, 0, d_maps, d_kinds, d_x, d_y);
    }
    HIP_TRY(span.finish(1, nullptr, seconds_kernel));
    HIP_TRY(hipMemcpy(mapx, d_x, sizeof(float) * n_elems, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mapy, d_y, sizeof(float) * n_elems, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tscm_build_maps(const tscm_map_desc *maps, int n_maps, int device, int exact, float *mapx, float *mapy, size_t n_elems,
                               double *seconds_kernel)
{
    return build_maps_host(maps, nullptr, n_maps, device, exact, mapx, mapy, n_elems, seconds_kernel);
}

static bool known_projection(int kind) { return kind >= TSCM_PROJ_PERSPECTIVE && kind <= TSCM_PROJ_EQUIRECT; }

extern "C" int tscm_build_maps_ex(const tscm_map_desc *maps, const int *projection, int n_maps, int device, int exact, float *mapx, float *mapy,
                                  size_t n_elems, double *seconds_kernel)
{
    bool pinholes = true;
    for (int m = 0; projection && m < n_maps; ++m) {
        if (!known_projection(projection[m]))
            return tscm_set_error(TSCM_E_INVALID, "map " + std::to_string(m) + ": unknown projection kind " + std::to_string(projection[m]));
        pinholes = pinholes && projection[m] == TSCM_PROJ_PERSPECTIVE;
    }
    return build_maps_host(maps, pinholes ? nullptr : projection, n_maps, device, exact, mapx, mapy, n_elems, seconds_kernel);
}

extern "C" int tscm_build_sweep_maps(const tscm_map_desc *maps, const int *projection, int n_cameras, const double *centers, const double *inv_distance, int D,
                                     int device, int exact, float *mapx, float *mapy, size_t n_elems, double *seconds_kernel)
{
    if (!maps) return tscm_set_error(TSCM_E_INVALID, "maps is NULL");
    if (!projection) return tscm_set_error(TSCM_E_INVALID, "projection is NULL");
    if (!centers) return tscm_set_error(TSCM_E_INVALID, "centers is NULL");
    if (!inv_distance) return tscm_set_error(TSCM_E_INVALID, "inv_distance is NULL");
    if (!mapx) return tscm_set_error(TSCM_E_INVALID, "mapx is NULL");
    if (!mapy) return tscm_set_error(TSCM_E_INVALID, "mapy is NULL");
    if (n_cameras < 1) return tscm_set_error(TSCM_E_INVALID, "n_cameras " + std::to_string(n_cameras) + " below 1");
    if (D < 1) return tscm_set_error(TSCM_E_INVALID, "D " + std::to_string(D) + " below 1");
    for (int k = 0; k < n_cameras; ++k) {
        const tscm_map_desc &d = maps[k];
        if (d.width < 0 || d.height < 0) return tscm_set_error(TSCM_E_INVALID, "maps[" + std::to_string(k) + "]: negative width or height");
        if (d.width != maps[0].width || d.height != maps[0].height)
            return tscm_set_error(TSCM_E_INVALID, "maps[" + std::to_string(k) + "]: width / height differ from maps[0]; the tables of a sweep share one output grid");
        if (d.out_stride != d.width) return tscm_set_error(TSCM_E_INVALID, "maps[" + std::to_string(k) + "]: out_stride " + std::to_string(d.out_stride) + " is not width; the output is dense");
        if (d.out_offset != 0) return tscm_set_error(TSCM_E_INVALID, "maps[" + std::to_string(k) + "]: out_offset is not 0; the output is dense");
        if (!known_projection(projection[k])) return tscm_set_error(TSCM_E_INVALID, "projection[" + std::to_string(k) + "]: unknown projection kind " + std::to_string(projection[k]));
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(centers[3 * k + c])) return tscm_set_error(TSCM_E_INVALID, "centers[" + std::to_string(k) + "] is not finite");
    }
    for (int z = 0; z < D; ++z) {
        if (!std::isfinite(inv_distance[z]) || inv_distance[z] < 0.0)
            return tscm_set_error(TSCM_E_INVALID, "inv_distance[" + std::to_string(z) + "] is negative or not finite");
        if (z > 0 && !(inv_distance[z] > inv_distance[z - 1])) return tscm_set_error(TSCM_E_INVALID, "inv_distance[" + std::to_string(z) + "] is not above its predecessor");
    }
    const unsigned long long total = (unsigned long long)maps[0].width * (unsigned long long)maps[0].height;
    const unsigned long long planes = (unsigned long long)n_cameras * (unsigned long long)D;
    if (total && planes > (unsigned long long)n_elems / total)
        return tscm_set_error(TSCM_E_INVALID, "n_elems " + std::to_string(n_elems) + " below n_cameras * D * height * width");
    for (int k = 0; k < n_cameras; ++k)
        if (projection[k] == TSCM_PROJ_PERSPECTIVE) return tscm_set_error(TSCM_E_UNSUPPORTED, "projection[" + std::to_string(k) + "]: PERSPECTIVE (plane sweep) is not built");
    if (planes > 65535) return tscm_set_error(TSCM_E_UNSUPPORTED, "more than 65535 tables in one call");
    if (int rc = select_device(device, "tscm_build_sweep_maps")) return rc;
    if (seconds_kernel) *seconds_kernel = 0.0;
    if (total == 0) return 0;
    const size_t n_out = (size_t)(planes * total);
    DeviceMem mem;
    const tscm_map_desc *d_maps = nullptr;
    const int *d_kinds = nullptr;
    const double *d_centers = nullptr, *d_inv = nullptr;
    float *d_x = nullptr, *d_y = nullptr;
    HIP_TRY(mem.upload(&d_maps, maps, (size_t)n_cameras));
    HIP_TRY(mem.upload(&d_kinds, projection, (size_t)n_cameras));
    HIP_TRY(mem.upload(&d_centers, centers, 3 * (size_t)n_cameras));
    HIP_TRY(mem.upload(&d_inv, inv_distance, (size_t)D));
    HIP_TRY(mem.alloc(&d_x, n_out)); HIP_TRY(mem.alloc(&d_y, n_out));
    EventSpan span;
    HIP_TRY(span.create(2));
    HIP_TRY(span.mark(0));
    const dim3 grid((unsigned)(((total + 3) / 4 + 255) / 256), (unsigned)planes);
    if (exact) hipLaunchKernelGGL(k_build_maps_sweep<true>, grid, dim3(256), 0, 0, d_maps, d_kinds, d_centers, d_inv, D, d_x, d_y);
    else hipLaunchKernelGGL(k_build_maps_sweep<false>, grid, dim3(256), 0, 0, d_maps, d_kinds, d_centers, d_inv, D, d_x, d_y);
    HIP_TRY(span.finish(1, nullptr, seconds_kernel));
    HIP_TRY(hipMemcpy(mapx, d_x, sizeof(float) * n_out, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mapy, d_y, sizeof(float) * n_out, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tscm_rectify_points(const tscm_map_desc *map, int projection, const double *pixels, int n, int device, double *out, unsigned char *valid)
{
    if (!map || n < 0 || (n > 0 && (!pixels || !out || !valid))) return tscm_set_error(TSCM_E_INVALID, n < 0 ? "negative point count" : "NULL argument");
    if (!known_projection(projection)) return tscm_set_error(TSCM_E_INVALID, "map 0: unknown projection kind " + std::to_string(projection));
    if (n == 0) return 0;
    if (int rc = select_device(device, "tscm_rectify_points")) return rc;
    DeviceMem mem;
    const tscm_map_desc *d_map = nullptr;
    const double *d_p = nullptr;
    double *d_o = nullptr;
    unsigned char *d_v = nullptr;
    HIP_TRY(mem.upload(&d_map, map, 1)); HIP_TRY(mem.upload(&d_p, pixels, 2 * (size_t)n));
    HIP_TRY(mem.alloc(&d_o, 2 * (size_t)n)); HIP_TRY(mem.alloc(&d_v, (size_t)n));
    hipLaunchKernelGGL(k_rectify_points, dim3((n + 255) / 256), dim3(256), 0, 0, d_map, projection, d_p, n, d_o, d_v);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_o, 2 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(valid, d_v, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// cv::remap(src, dst, mapx, mapy, INTER_LINEAR) for 8-bit images (TS.cpp:304, :329), border constant 0, optionally
// followed by BGR2GRAY (findCorner.cpp:9-10).  OpenCV's fixed-point scheme (see oracle/tscm_oracle_remap.c): map
// coordinates rounded to 1/32 pixel, 15-bit weights, (sum + 2^14) >> 15.  Integer arithmetic: bit-identical to the oracle.
namespace {

template <int CH>
__global__ __launch_bounds__(256) void k_remap(const unsigned char *src, int w, int h, int stride, const float *mapx, const float *mapy, int map_w, int map_h,
                                               int to_gray, unsigned char *dst, int dst_stride)
{
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= map_w) return;
    const int sx = __float2int_rn(mapx[(size_t)i * map_w + j] * 32.0f), sy = __float2int_rn(mapy[(size_t)i * map_w + j] * 32.0f);
    const int ix = max(-32768, min(32767, sx >> 5)), iy = max(-32768, min(32767, sy >> 5));
    const int fx = sx & 31, fy = sy & 31;
    int wgt[4] = { 32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy), 32 * (32 - fx) * fy, 32 * fx * fy };
    if (wgt[0] == 32768) { wgt[0] = 32767; wgt[3] = 1; }
    int px[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = ix + (k & 1), y = iy + (k >> 1);
            const int p = (x >= 0 && x < w && y >= 0 && y < h) ? src[(size_t)y * stride + (size_t)x * CH + c] : 0;
            acc += wgt[k] * p;
        }
        px[c] = max(0, min(255, (acc + (1 << 14)) >> 15));
    }
    if (CH == 3 && to_gray) dst[(size_t)i * dst_stride + j] = (unsigned char)((px[0] * 1868 + px[CH > 1 ? 1 : 0] * 9617 + px[CH > 2 ? 2 : 0] * 4899 + (1 << 13)) >> 14);
    else {
#pragma unroll
        for (int c = 0; c < CH; ++c) dst[(size_t)i * dst_stride + (size_t)j * CH + c] = (unsigned char)px[c];
    }
}

}  // namespace

extern "C" int tscm_remap(const unsigned char *src, int width, int height, int stride, int channels, const float *mapx, const float *mapy, int map_width,
                          int map_height, int map_stride, int to_gray, int device, unsigned char *dst, int dst_stride)
{
    if (!src || !mapx || !mapy || !dst) return tscm_set_error(TSCM_E_INVALID, "NULL argument");
    if (channels != 1 && channels != 3) return tscm_set_error(TSCM_E_UNSUPPORTED, "remap: 1 or 3 channels");
    const int out_ch = (to_gray || channels == 1) ? 1 : channels;
    if (width < 1 || height < 1 || stride < width * channels || map_width < 0 || map_height < 0 || map_stride < map_width || dst_stride < map_width * out_ch)
        return tscm_set_error(TSCM_E_INVALID, "bad image / map description");
    if (width > 32767 || height > 32767) return tscm_set_error(TSCM_E_UNSUPPORTED, "images beyond 32767 pixels per side");
    if (map_width == 0 || map_height == 0) return 0;
    if (int rc = select_device(device, "tscm_remap")) return rc;
    DeviceMem mem;
    const unsigned char *d_src = nullptr;
    unsigned char *d_dst = nullptr;
    float *d_mx = nullptr, *d_my = nullptr;
    const size_t nmap = (size_t)map_width * map_height, dst_row = (size_t)map_width * out_ch;
    HIP_TRY(mem.upload(&d_src, src, (size_t)stride * height));
    HIP_TRY(mem.alloc(&d_mx, nmap)); HIP_TRY(mem.alloc(&d_my, nmap));
    HIP_TRY(mem.alloc(&d_dst, dst_row * map_height));
    HIP_TRY(copy_rows(d_mx, map_width, mapx, map_stride, map_width, map_height, hipMemcpyHostToDevice));
    HIP_TRY(copy_rows(d_my, map_width, mapy, map_stride, map_width, map_height, hipMemcpyHostToDevice));
    const dim3 grid((map_width + 255) / 256, map_height);
    if (channels == 1)
        hipLaunchKernelGGL(k_remap<1>, grid, dim3(256), 0, nullptr, d_src, width, height, stride, d_mx, d_my, map_width, map_height, 0, d_dst, (int)dst_row);
    else
        hipLaunchKernelGGL(k_remap<3>, grid, dim3(256), 0, nullptr, d_src, width, height, stride, d_mx, d_my, map_width, map_height, to_gray ? 1 : 0, d_dst, (int)dst_row);
    HIP_TRY(hipGetLastError());
    HIP_TRY(copy_rows(dst, dst_stride, d_dst, dst_row, dst_row, map_height, hipMemcpyDeviceToHost));
    return 0;
}
