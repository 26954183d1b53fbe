// tscm_stereo.hip -- stereo matching on a rectified pair (tscm.h: tscm_stereo_*): 9 x 7 census, Hamming cost,
// semi-global aggregation along 4 or 8 directions, winner / uniqueness / left-right check / sub-pixel, and the 3-D points
// of a disparity map.  Everything up to the disparity map is integer arithmetic, defined in tscm.h so that a host
// restatement (tests/stereo_ref.py) gives the same bits.
//
// Layout: census [h][w] uint64, cost C [h][w][D] uint8, aggregated S [h][w][D] uint16 (D = num_disparities).
//   k_census        64 x 16 tile + 4/3 halo in LDS, one uint64 per pixel
//   k_cost          256 pixels of a row per block, their 256 + D - 1 right-hand codes in LDS, 4 costs per 32-bit store
//   k_aggregate     one wave per scanline, the D disparities of a step across the lanes (NPL = ceil(D / 64) per lane); the
//                   k +- 1 neighbours and the minimum over k travel by DPP, the loads of U steps are issued ahead of the chain
//   k_right_winner  kR of the left-right check: a row segment's S read once, coalesced, minima by LDS atomics
//   k_winner        one wave per pixel: k*, uniqueness, left-right check, sub-pixel
// k_aggregate and k_winner live in tscm_stereo_kernels.h, which the sphere sweep (tscm_sweep.hip) includes too.
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_host.h"
#include "tscm_stereo_kernels.h"

#include <cstdint>
#include <string>

using namespace tscm;

namespace {

constexpr int kCensusTileW = 64, kCensusTileH = 16;
constexpr int kCostSegment = 256;     // pixels of a row per k_cost / k_right_winner block

// ------------------------------------------------------------------------------------------------ census
// grid (ceil(w / 64), ceil(h / 16)) x 256: thread (tx, ty) of 64 x 4 computes pixels (tx, ty + 4 i), i < 4
__global__ __launch_bounds__(256) void k_census(const unsigned char *__restrict__ img, int w, int h, int stride, unsigned long long *__restrict__ out)
{
    constexpr int LW = kCensusTileW + 8, LH = kCensusTileH + 6;
    __shared__ unsigned char tile[LH][LW];
    const int x0 = blockIdx.x * kCensusTileW, y0 = blockIdx.y * kCensusTileH;
    for (int e = threadIdx.x; e < LW * LH; e += 256) {
        const int ty = e / LW, tx = e - ty * LW;
        const int gx = min(max(x0 + tx - 4, 0), w - 1), gy = min(max(y0 + ty - 3, 0), h - 1);      // replicated border
        tile[ty][tx] = img[(size_t)gy * stride + gx];
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ly = ty + 4 * i, x = x0 + tx, y = y0 + ly;
        if (x >= w || y >= h) continue;
        const int c = tile[ly + 3][tx + 4];
        unsigned long long code = 0;
#pragma unroll
        for (int dy = 0; dy < 7; ++dy)
#pragma unroll
            for (int dx = 0; dx < 9; ++dx) {
                if (dy == 3 && dx == 4) continue;
                code = (code << 1) | (unsigned long long)(tile[ly + dy][tx + dx] < c);
            }
        out[(size_t)y * w + x] = code;
    }
}

// ------------------------------------------------------------------------------------------------ cost
// grid (ceil(w / 256) * h) x 256: row y, pixels [s, s + 256); item e = pixel * (D / 4) + quad, one 32-bit store of 4 costs
__global__ __launch_bounds__(256) void k_cost(const unsigned long long *__restrict__ cl, const unsigned long long *__restrict__ cr, int w, int h, int D, int dmin,
                                              unsigned char *__restrict__ cost)
{
    __shared__ unsigned long long right[kCostSegment + 256];
    const int nseg = (w + kCostSegment - 1) / kCostSegment;
    const int y = blockIdx.x / nseg, s = (blockIdx.x - y * nseg) * kCostSegment;
    const int n = min(kCostSegment, w - s);
    const int r0 = s - (dmin + D - 1);                      // right[q] = code at column r0 + q, q < n + D - 1
    for (int q = threadIdx.x; q < n + D - 1; q += 256) {
        const int xr = r0 + q;
        right[q] = (xr >= 0 && xr < w) ? cr[(size_t)y * w + xr] : 0ULL;
    }
    __syncthreads();
    const int qpp = D >> 2;                                 // quads per pixel
    for (int e = threadIdx.x; e < n * qpp; e += 256) {
        const int px = e / qpp, quad = e - px * qpp;
        const int x = s + px;
        const unsigned long long code = cl[(size_t)y * w + x];
        unsigned packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 4 * quad + j, xr = x - (dmin + k);
            const unsigned c = (xr >= 0 && xr < w) ? (unsigned)__builtin_popcountll(code ^ right[xr - r0]) : 64u;
            packed |= c << (8 * j);
        }
        *reinterpret_cast<unsigned *>(cost + ((size_t)y * w + x) * D + 4 * quad) = packed;
    }
}

// ------------------------------------------------------------------------------------------------ winner
// kR(y, x2) = the lowest k that minimises S(y, x2 + dmin + k, k) over the k whose column is inside the image, -1 if none.
// grid (ceil(w / 256) * h) x 256: the block owns x2 in [s0, s0 + 256) of row y; its waves walk the columns that feed them.
template <int NPL>
__global__ __launch_bounds__(256) void k_right_winner(const unsigned short *__restrict__ sum, int w, int h, int D, int dmin, short *__restrict__ kr)
{
    __shared__ unsigned best[kCostSegment];
    const int nseg = (w + kCostSegment - 1) / kCostSegment;
    const int y = blockIdx.x / nseg, s0 = (blockIdx.x - y * nseg) * kCostSegment;
    best[threadIdx.x] = 0xffffffffu;
    __syncthreads();
    const int lane = threadIdx.x & 63, k0 = lane * NPL;
    const int lo = max(0, s0 + dmin), hi = min(w - 1, s0 + kCostSegment - 1 + dmin + D - 1);
    for (int xp = lo + (int)(threadIdx.x >> 6); xp <= hi; xp += 4) {
        int s[NPL];
#pragma unroll
        for (int j = 0; j < NPL; ++j) s[j] = 0;
        load_sum<NPL>(sum + ((size_t)y * w + xp) * D + k0, k0, D, s);
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int k = k0 + j, q = xp - dmin - k - s0;
            if (k < D && q >= 0 && q < kCostSegment) atomicMin(&best[q], ((unsigned)s[j] << 16) | (unsigned)k);
        }
    }
    __syncthreads();
    const int x2 = s0 + threadIdx.x;
    if (x2 < w) kr[(size_t)y * w + x2] = best[threadIdx.x] == 0xffffffffu ? (short)-1 : (short)(best[threadIdx.x] & 0xffffu);
}

// ------------------------------------------------------------------------------------------------ points
__global__ __launch_bounds__(256) void k_stereo_points(const short *__restrict__ disp, int w, int h, int invalid, int kind, double fx, double fy, double cx, double cy,
                                                       double baseline, double *__restrict__ points, unsigned char *__restrict__ valid)
{
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (size_t)w * h) return;
    const int y = (int)(pix / (size_t)w), x = (int)(pix - (size_t)y * w);
    const int raw = disp[pix];
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double X = nan, Y = nan, Z = nan;
    const bool ok = raw != invalid && raw > 0;
    if (ok) {
        const double d = (double)raw / 16.0;
        if (kind == TSCM_PROJ_PERSPECTIVE) {
            Z = fx * baseline / d;
            X = ((double)x - cx) / fx * Z;
            Y = ((double)y - cy) / fy * Z;
        } else {                                             // LONGLAT: law of sines in the epipolar plane
            const double aL = ((double)x - cx) / fx, da = d / fx, b = ((double)y - cy) / fy;
            const double r = baseline * cos(aL - da) / sin(da);
            double sa, ca, sb, cb;
            sincos(aL, &sa, &ca);
            sincos(b, &sb, &cb);
            X = r * sa; Y = r * ca * sb; Z = r * ca * cb;
        }
    }
    points[3 * pix] = X; points[3 * pix + 1] = Y; points[3 * pix + 2] = Z;
    valid[pix] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ host
int check_params(const tscm_stereo_params *p)
{
    if (!p) return tscm_set_error(TSCM_E_INVALID, "params is NULL");
    if (int rc = check_struct_size(p, "tscm_stereo_params")) return rc;
    if (p->num_disparities < 16 || p->num_disparities > 256 || p->num_disparities % 16)
        return tscm_set_error(TSCM_E_INVALID, "params: num_disparities " + std::to_string(p->num_disparities) + " is not a multiple of 16 in 16..256");
    if (p->min_disparity < -2047 || p->min_disparity + p->num_disparities > 2047)
        return tscm_set_error(TSCM_E_INVALID, "params: min_disparity " + std::to_string(p->min_disparity) + ": 16 * disparity does not fit the 16-bit output");
    if (p->paths != 4 && p->paths != 8) return tscm_set_error(TSCM_E_INVALID, "params: paths " + std::to_string(p->paths) + " is not 4 or 8");
    if (p->p1 < 0 || p->p1 > p->p2 || p->p2 > 255)
        return tscm_set_error(TSCM_E_INVALID, "params: p1 " + std::to_string(p->p1) + ", p2 " + std::to_string(p->p2) + " do not satisfy 0 <= p1 <= p2 <= 255");
    if (p->uniqueness_ratio < 0 || p->uniqueness_ratio > 99) return tscm_set_error(TSCM_E_INVALID, "params: uniqueness_ratio " + std::to_string(p->uniqueness_ratio) + " outside 0..99");
    return 0;
}

int check_images(const unsigned char *left, const unsigned char *right, int width, int height, int stride)
{
    if (!left) return tscm_set_error(TSCM_E_INVALID, "left is NULL");
    if (!right) return tscm_set_error(TSCM_E_INVALID, "right is NULL");
    if (width < 0 || height < 0) return tscm_set_error(TSCM_E_INVALID, "negative width or height");
    if (stride < width) return tscm_set_error(TSCM_E_INVALID, "stride " + std::to_string(stride) + " < width " + std::to_string(width));
    if (width > 32767 || height > 32767) return tscm_set_error(TSCM_E_UNSUPPORTED, "images beyond 32767 pixels per side");
    return 0;
}

thread_local double g_stage_seconds[5];

// The kernels of one pair.  Outputs are host pointers, any of them NULL; the winner stages run only for `disparity`.
int stereo_run(const unsigned char *left, const unsigned char *right, int w, int h, int stride, const tscm_stereo_params &p, int device, const char *who,
               unsigned long long *census_left, unsigned long long *census_right, unsigned char *cost, unsigned short *aggregated, short *disparity,
               int disp_stride, double *seconds_kernel)
{
    if (int rc = select_device(device, who)) return rc;
    const int D = p.num_disparities, dmin = p.min_disparity;
    const size_t npix = (size_t)w * h, nvol = npix * D;
    DeviceMem mem;
    StageOutputs stages(mem);
    EventSpan span;
    unsigned char *d_img[2] = { nullptr, nullptr }, *d_cost = nullptr;
    unsigned long long *d_census[2] = { nullptr, nullptr };
    unsigned short *d_sum = nullptr;
    short *d_kr = nullptr, *d_disp = nullptr;
    const unsigned char *host_img[2] = { left, right };
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(mem.alloc(&d_img[k], npix));
        HIP_TRY(copy_rows(d_img[k], w, host_img[k], stride, w, h, hipMemcpyHostToDevice));
        HIP_TRY(mem.alloc(&d_census[k], npix));
    }
    HIP_TRY(mem.alloc(&d_cost, nvol));
    HIP_TRY(mem.alloc(&d_sum, nvol));
    if (disparity) { HIP_TRY(mem.alloc(&d_kr, npix)); HIP_TRY(mem.alloc(&d_disp, npix)); }
    stages.from(census_left, d_census[0], npix);
    stages.from(census_right, d_census[1], npix);
    stages.from(cost, d_cost, nvol);
    stages.from(aggregated, d_sum, nvol);
    HIP_TRY(span.create(6));
    const int nseg = (w + kCostSegment - 1) / kCostSegment;
    HIP_TRY(span.mark(0));
    const dim3 cgrid((w + kCensusTileW - 1) / kCensusTileW, (h + kCensusTileH - 1) / kCensusTileH);
    for (int k = 0; k < 2; ++k) hipLaunchKernelGGL(k_census, cgrid, dim3(256), 0, 0, d_img[k], w, h, w, d_census[k]);
    HIP_TRY(span.mark(1));
    hipLaunchKernelGGL(k_cost, dim3((unsigned)(nseg * h)), dim3(256), 0, 0, d_census[0], d_census[1], w, h, D, dmin, d_cost);
    HIP_TRY(span.mark(2));
    launch_aggregate(d_cost, d_sum, w, h, D, p.p1, p.p2, p.paths);
    HIP_TRY(span.mark(3));
    if (disparity && p.disp12_max_diff >= 0)
        with_planes(D, [&](auto npl) {
            hipLaunchKernelGGL(k_right_winner<decltype(npl)::value>, dim3((unsigned)(nseg * h)), dim3(256), 0, 0, d_sum, w, h, D, dmin, d_kr);
        });
    HIP_TRY(span.mark(4));
    if (disparity)
        with_planes(D, [&](auto npl) {
            hipLaunchKernelGGL(k_winner<decltype(npl)::value>, dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, 0, d_sum, d_kr, w, h, D, dmin, p.uniqueness_ratio,
                               p.disp12_max_diff, d_disp);
        });
    HIP_TRY(span.finish(5, g_stage_seconds, seconds_kernel));
    HIP_TRY(stages.fetch());
    if (disparity) HIP_TRY(copy_rows(disparity, disp_stride, d_disp, w, w, h, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" void tscm_stereo_default_params(tscm_stereo_params *p)
{
    if (!p) return;
    p->struct_size = (int)sizeof(tscm_stereo_params);
    p->min_disparity = 0; p->num_disparities = 128;
    p->p1 = 8; p->p2 = 32; p->paths = 8;
    p->uniqueness_ratio = 10; p->disp12_max_diff = 1;
}

extern "C" int tscm_stereo_match(const unsigned char *left, const unsigned char *right, int width, int height, int stride, const tscm_stereo_params *params,
                                 int device, short *disparity, int disp_stride, double *seconds_kernel)
{
    if (int rc = check_images(left, right, width, height, stride)) return rc;
    if (int rc = check_params(params)) return rc;
    if (!disparity) return tscm_set_error(TSCM_E_INVALID, "disparity is NULL");
    if (disp_stride < width) return tscm_set_error(TSCM_E_INVALID, "disp_stride " + std::to_string(disp_stride) + " < width " + std::to_string(width));
    if (seconds_kernel) *seconds_kernel = 0.0;
    if (width == 0 || height == 0) return 0;
    return stereo_run(left, right, width, height, stride, *params, device, "tscm_stereo_match", nullptr, nullptr, nullptr, nullptr, disparity, disp_stride,
                      seconds_kernel);
}

extern "C" int tscm_stereo_stages(const unsigned char *left, const unsigned char *right, int width, int height, int stride, const tscm_stereo_params *params,
                                  int device, unsigned long long *census_left, unsigned long long *census_right, unsigned char *cost, unsigned short *aggregated)
{
    if (int rc = check_images(left, right, width, height, stride)) return rc;
    if (int rc = check_params(params)) return rc;
    if (width == 0 || height == 0) return 0;
    return stereo_run(left, right, width, height, stride, *params, device, "tscm_stereo_stages", census_left, census_right, cost, aggregated, nullptr, 0, nullptr);
}

extern "C" int tscm_stereo_stage_times(double *seconds)
{
    if (!seconds) return tscm_set_error(TSCM_E_INVALID, "seconds is NULL");
    for (int k = 0; k < 5; ++k) seconds[k] = g_stage_seconds[k];
    return 0;
}

extern "C" int tscm_stereo_points(const short *disparity, int width, int height, int disp_stride, int min_disparity, const tscm_map_desc *left_map,
                                  int projection, double baseline, int device, double *points, unsigned char *valid)
{
    if (!disparity) return tscm_set_error(TSCM_E_INVALID, "disparity is NULL");
    if (!left_map) return tscm_set_error(TSCM_E_INVALID, "left_map is NULL");
    if (!points) return tscm_set_error(TSCM_E_INVALID, "points is NULL");
    if (!valid) return tscm_set_error(TSCM_E_INVALID, "valid is NULL");
    if (width < 0 || height < 0) return tscm_set_error(TSCM_E_INVALID, "negative width or height");
    if (disp_stride < width) return tscm_set_error(TSCM_E_INVALID, "disp_stride " + std::to_string(disp_stride) + " < width " + std::to_string(width));
    if (projection != TSCM_PROJ_PERSPECTIVE && projection != TSCM_PROJ_LONGLAT)
        return tscm_set_error(TSCM_E_INVALID, "projection " + std::to_string(projection) + ": points come from PERSPECTIVE or LONGLAT pairs");
    if (min_disparity < -2047 || min_disparity > 2047) return tscm_set_error(TSCM_E_INVALID, "min_disparity " + std::to_string(min_disparity) + " outside the 16-bit output");
    if (width > 32767 || height > 32767) return tscm_set_error(TSCM_E_UNSUPPORTED, "images beyond 32767 pixels per side");
    if (width == 0 || height == 0) return 0;
    if (int rc = select_device(device, "tscm_stereo_points")) return rc;
    const size_t npix = (size_t)width * height;
    DeviceMem mem;
    short *d_disp = nullptr;
    double *d_pts = nullptr;
    unsigned char *d_valid = nullptr;
    HIP_TRY(mem.alloc(&d_disp, npix)); HIP_TRY(mem.alloc(&d_pts, 3 * npix)); HIP_TRY(mem.alloc(&d_valid, npix));
    HIP_TRY(copy_rows(d_disp, width, disparity, disp_stride, width, height, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_stereo_points, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, 0, d_disp, width, height, 16 * (min_disparity - 1), projection,
                       left_map->fx, left_map->fy, left_map->cx, left_map->cy, baseline, d_pts, d_valid);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(points, d_pts, 3 * npix * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(valid, d_valid, npix, hipMemcpyDeviceToHost));
    return 0;
}
