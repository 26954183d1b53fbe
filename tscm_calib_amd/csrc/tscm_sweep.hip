// tscm_sweep.hip -- sphere-sweep depth of a calibrated rig (tscm.h: tscm_sweep_*): for every pixel of the rig-frame panorama
// and every inverse-distance hypothesis the cameras that see the point are sampled through the sweep tables
// (tscm_build_sweep_maps), their 9 x 7 census codes are compared pair by pair, and the cost volume goes through the
// matcher's path aggregation and winner.  Integer arithmetic up to the index map, defined in tscm.h so that a host
// restatement (tests/sweep_ref.py) gives the same bits.
//
// Constant per rig, built once by tscm_sweep_create and kept on the device:
//   pack   [n][D][npix] uint2: the panorama's record, x = ix | iy << 16, y = fx | fy << 5 | a << 16
// Per frame:
//   k_sweep_cost     a block owns a 64 x 16 panorama tile and 4 consecutive hypotheses.  Per hypothesis it samples the tile
//                    with its 4/3 halo (72 x 22) of every camera from the records into LDS, forms the census codes of its
//                    pixels from LDS (a thread owns 4 rows of one column, so their windows share 10 rows of 9 bytes), sums
//                    the Hamming distances over the pairs of covering cameras and divides by their number; 4 cost bytes
//                    per 32-bit store.  Neither the warped planes nor their codes reach memory (except for the stages call).
//   k_aggregate      tscm_stereo_kernels.h, on the new volume
//   k_sweep_winner   winner_value of tscm_stereo_kernels.h with the rule C(k*) == 64 -> invalid
//   k_sweep_points   one thread per pixel, fp64
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_host.h"
#include "tscm_remap_sample.h"
#include "tscm_stereo_kernels.h"

#include <cmath>
#include <cstdint>
#include <memory>
#include <string>

using namespace tscm;

namespace {

constexpr int kMaxCameras = 8;
constexpr int kTileW = 64, kTileH = 16;                   // panorama pixels per block
constexpr int kLW = kTileW + 8, kLH = kTileH + 6;         // with the census halo: 4 columns, 3 rows on each side
constexpr int kHaloIters = (kLW * kLH + 255) / 256;       // halo elements per thread
constexpr int kZGroup = 4;                                // hypotheses per block: the 4 cost bytes of one store

// ------------------------------------------------------------------------------------------------ prepare
// grid (ceil(npix / 256), n * D) x 256: the packed record of table blockIdx.y = k * D + z; weight_mask bit k: camera k has
// a weight image (at wimg + k * w * h), otherwise a constant 255 inside the image
__global__ __launch_bounds__(256) void k_sweep_prepare(const float *__restrict__ mapx, const float *__restrict__ mapy, const unsigned char *__restrict__ wimg,
                                                       unsigned weight_mask, int w, int h, int D, size_t npix, uint2 *__restrict__ pack)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= npix) return;
    const int k = blockIdx.y / D;
    const size_t at = (size_t)blockIdx.y * npix + t;
    const int sx = __float2int_rn(mapx[at] * 32.0f), sy = __float2int_rn(mapy[at] * 32.0f);
    const int ix = max(-32768, min(32767, sx >> 5)), iy = max(-32768, min(32767, sy >> 5));
    const unsigned frac = (unsigned)(sx & 31) | ((unsigned)(sy & 31) << 5);
    int wgt[4];
    tap_weights(frac, wgt);
    const bool has = (weight_mask >> k) & 1u;
    const unsigned char *wk = wimg + (size_t)k * w * h;
    int acc = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int x = ix + (q & 1), y = iy + (q >> 1);
        if (x >= 0 && x < w && y >= 0 && y < h) acc += wgt[q] * (has ? (int)wk[(size_t)y * w + x] : 255);
    }
    const int a = max(0, min(255, (acc + (1 << 14)) >> 15));
    pack[at] = make_uint2(((unsigned)ix & 0xffffu) | ((unsigned)iy << 16), frac | ((unsigned)a << 16));
}

// ------------------------------------------------------------------------------------------------ cost
// (sum + (P >> 1)) / P for P = cnt (cnt - 1) / 2 pairs of cnt = 2..8 cameras by a multiply and a shift: with
// M = ceil(2^16 / P), (x M) >> 16 == x / P for every x <= 62 P + (P >> 1), which pairs_divide_exact() walks through.
constexpr unsigned pair_reciprocal(int cnt) { return (65536u + (unsigned)(cnt * (cnt - 1) / 2) - 1u) / (unsigned)(cnt * (cnt - 1) / 2); }
constexpr bool pairs_divide_exact()
{
    for (int cnt = 2; cnt <= kMaxCameras; ++cnt) {
        const unsigned P = (unsigned)(cnt * (cnt - 1) / 2), M = pair_reciprocal(cnt);
        for (unsigned x = 0; x <= 62u * P + (P >> 1); ++x)
            if (((x * M) >> 16) != x / P) return false;
    }
    return true;
}
static_assert(pairs_divide_exact(), "the multiply-shift division of the pair sums is not exact");

__device__ __forceinline__ int mean_pair_cost(int sum, int cnt)
{
    unsigned M = pair_reciprocal(2);
    if (cnt == 3) M = pair_reciprocal(3);
    else if (cnt == 4) M = pair_reciprocal(4);
    else if (cnt == 5) M = pair_reciprocal(5);
    else if (cnt == 6) M = pair_reciprocal(6);
    else if (cnt == 7) M = pair_reciprocal(7);
    else if (cnt == 8) M = pair_reciprocal(8);
    const unsigned P = (unsigned)(cnt * (cnt - 1)) >> 1;
    return (int)((((unsigned)sum + (P >> 1)) * M) >> 16);
}

// grid (ceil(pw / 64), ceil(ph / 16), D / 4) x 256.  Thread (tx, ty) of 64 x 4 owns the pixels (x0 + tx, y0 + 4 ty + i), i < 4.
// sampled / alpha / census (each [N][D][ph][pw], any of them NULL): the stage outputs.
template <int N>
__global__ __launch_bounds__(256) void k_sweep_cost(const uint2 *__restrict__ pack, const unsigned char *__restrict__ img, int w, int h, int pw, int ph, int D, int wrap,
                                                    unsigned char *__restrict__ cost, unsigned char *__restrict__ sampled, unsigned char *__restrict__ alpha,
                                                    unsigned long long *__restrict__ census)
{
    __shared__ unsigned char tile[N][kLH * kLW], cover[N][kLH * kLW];
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH, z0 = blockIdx.z * kZGroup;
    const size_t npix = (size_t)pw * ph, simg = (size_t)w * h;
    // where the halo elements of this thread lie in the panorama: rows clamped, columns wrapped or clamped; always inside
    unsigned src[kHaloIters];
#pragma unroll
    for (int it = 0; it < kHaloIters; ++it) {
        const int e = min(threadIdx.x + 256 * it, kLW * kLH - 1);
        const int ly = e / kLW, lx = e - ly * kLW;
        const int gy = min(max(y0 + ly - 3, 0), ph - 1);
        int gx = x0 + lx - 4;
        if (wrap) {
            if (gx < 0) gx += pw;
            else if (gx >= pw) gx -= pw;
            if (gx < 0 || gx >= pw) gx = ((gx % pw) + pw) % pw;                // panoramas narrower than the halo
        } else gx = min(max(gx, 0), pw - 1);
        src[it] = (unsigned)gy * (unsigned)pw + (unsigned)gx;
    }
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x = x0 + tx, yb = y0 + 4 * ty;
    unsigned packed[4] = { 0, 0, 0, 0 };
    for (int zz = 0; zz < kZGroup; ++zz) {
        const int z = z0 + zz;
        if (zz) __syncthreads();                                               // the previous hypothesis has been read
#pragma unroll 1
        for (int k = 0; k < N; ++k) {                                          // rolled: one camera's gathers in flight at a time
            const uint2 *pk = pack + ((size_t)k * D + z) * npix;
#pragma unroll
            for (int it = 0; it < kHaloIters; ++it) {
                const int e = threadIdx.x + 256 * it;
                if (e < kLW * kLH) {
                    const uint2 rec = pk[src[it]];
                    int px[1];
                    sample_px<1>(img + k * simg, w, h, rec, px);               // every tap bounds-checked
                    tile[k][e] = (unsigned char)px[0];
                    cover[k][e] = (unsigned char)(rec.y >> 16);
                }
            }
        }
        __syncthreads();
        if (x >= pw || yb >= ph) continue;                                     // no barrier below
        unsigned hi[N][4], lo[N][4];                                           // code = hi << 32 | lo: the first 30 bits, the last 32
        unsigned seen[4] = { 0, 0, 0, 0 };
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const unsigned char *T = tile[k] + (4 * ty) * kLW + tx;            // the window's corner of pixel i = 0
            int centre[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int at = (4 * ty + i + 3) * kLW + tx + 4;
                centre[i] = tile[k][at];
                hi[k][i] = 0; lo[k][i] = 0;
                if (cover[k][at] > 0) seen[i] |= 1u << k;
            }
#pragma unroll
            for (int r = 0; r < 10; ++r) {                                     // the 10 rows the 4 windows span
                int b[9];
#pragma unroll
                for (int dx = 0; dx < 9; ++dx) b[dx] = T[r * kLW + dx];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (r - i < 0 || r - i > 6) continue;
#pragma unroll
                    for (int dx = 0; dx < 9; ++dx) {
                        if (r - i == 3 && dx == 4) continue;
                        // word << 1 | (neighbour < centre): the sign of the difference of two bytes, shifted in by one v_alignbit
                        const unsigned diff = (unsigned)(b[dx] - centre[i]);
                        if ((r - i) * 9 + dx < 30) hi[k][i] = __builtin_amdgcn_alignbit(hi[k][i], diff, 31);
                        else lo[k][i] = __builtin_amdgcn_alignbit(lo[k][i], diff, 31);
                    }
                }
            }
            if (sampled || alpha || census) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (yb + i >= ph) continue;
                    const size_t o = ((size_t)k * D + z) * npix + (size_t)(yb + i) * pw + x;
                    const int at = (4 * ty + i + 3) * kLW + tx + 4;
                    if (sampled) sampled[o] = (unsigned char)centre[i];
                    if (alpha) alpha[o] = cover[k][at];
                    if (census) census[o] = ((unsigned long long)hi[k][i] << 32) | lo[k][i];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cnt = __builtin_popcount(seen[i]);
            int c = 64;
            if (cnt >= 2) {
                int sum = 0;
#pragma unroll
                for (int a = 0; a < N; ++a)
#pragma unroll
                    for (int b = a + 1; b < N; ++b)
                        if (((seen[i] >> a) & (seen[i] >> b)) & 1u) sum += __builtin_popcount(hi[a][i] ^ hi[b][i]) + __builtin_popcount(lo[a][i] ^ lo[b][i]);
                c = mean_pair_cost(sum, cnt);
            }
            packed[i] |= (unsigned)c << (8 * zz);
        }
    }
    if (x >= pw) return;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (yb + i < ph) *reinterpret_cast<unsigned *>(cost + ((size_t)(yb + i) * pw + x) * D + z0) = packed[i];
}

// ------------------------------------------------------------------------------------------------ winner
// one wave per pixel, 4 pixels per block: k_winner without the left-right check, with the rule of the uncovered winner
template <int NPL>
__global__ __launch_bounds__(256) void k_sweep_winner(const unsigned short *__restrict__ sum, const unsigned char *__restrict__ cost, int w, int h, int D, int uniqueness,
                                                      short *__restrict__ index16)
{
    const size_t pix = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= (size_t)w * h) return;                        // whole waves
    const int lane = threadIdx.x & 63;
    const int y = (int)(pix / (size_t)w), x = (int)(pix - (size_t)y * w);
    const int out = winner_value<NPL>(sum + pix * D, nullptr, cost + pix * D, lane, w, x, y, D, 0, uniqueness, -1);
    if (lane == 0) index16[pix] = (short)out;
}

// ------------------------------------------------------------------------------------------------ points
__global__ __launch_bounds__(256) void k_sweep_points(const short *__restrict__ index16, int w, int h, int kind, double fx, double fy, double cx, double cy,
                                                      const double *__restrict__ inv_distance, int D, double *__restrict__ points, unsigned char *__restrict__ valid)
{
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (size_t)w * h) return;
    const int i = (int)(pix / (size_t)w), j = (int)(pix - (size_t)i * w);
    const int raw = index16[pix];
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double X = nan, Y = nan, Z = nan;
    bool ok = raw >= 0;
    if (ok) {
        const double s = (double)raw / 16.0;
        const int k0 = min(raw >> 4, D - 2);
        const double inv = inv_distance[k0] + (s - (double)k0) * (inv_distance[k0 + 1] - inv_distance[k0]);
        ok = inv > 0.0;
        if (ok) {
            const double a = ((double)j - cx) / fx, b = ((double)i - cy) / fy;
            double x, y, z;
            if (kind == TSCM_PROJ_STEREOGRAPHIC) {
                const double q = 0.25 * (a * a + b * b);
                x = a / (1.0 + q); y = b / (1.0 + q); z = (1.0 - q) / (1.0 + q);
            } else {
                double sa, ca, sb, cb;
                sincos(a, &sa, &ca);
                sincos(b, &sb, &cb);
                if (kind == TSCM_PROJ_LONGLAT) { x = sa; y = ca * sb; z = ca * cb; }
                else if (kind == TSCM_PROJ_CYLINDRICAL) { x = sa; y = b; z = ca; }
                else { x = cb * sa; y = sb; z = cb * ca; }                       // EQUIRECT
            }
            X = x / inv; Y = y / inv; Z = z / inv;
        }
    }
    points[3 * pix] = X; points[3 * pix + 1] = Y; points[3 * pix + 2] = Z;
    valid[pix] = ok ? 1 : 0;
}

thread_local double g_stage_seconds[3];

}  // namespace

// ------------------------------------------------------------------------------------------------ host
struct tscm_sweep {
    int n = 0, w = 0, h = 0, pw = 0, ph = 0, D = 0, p1 = 0, p2 = 0, paths = 0, uniqueness = 0, wrap = 0, device = 0;
    size_t npix = 0;
    DeviceMem mem;
    uint2 *pack = nullptr;
    unsigned char *img = nullptr, *cost = nullptr;
    unsigned short *sum = nullptr;
    short *index16 = nullptr;
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
    ~tscm_sweep() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
};

namespace {

int check_params(const tscm_sweep_params *p)
{
    if (!p) return tscm_set_error(TSCM_E_INVALID, "params is NULL");
    if (p->struct_size != (int)sizeof(tscm_sweep_params))
        return tscm_set_error(TSCM_E_INVALID, "params: struct_size " + std::to_string(p->struct_size) + " is not sizeof(tscm_sweep_params) = " + std::to_string(sizeof(tscm_sweep_params)));
    if (p->num_hypotheses < 16 || p->num_hypotheses > 256 || p->num_hypotheses % 16)
        return tscm_set_error(TSCM_E_INVALID, "params: num_hypotheses " + std::to_string(p->num_hypotheses) + " is not a multiple of 16 in 16..256");
    if (p->paths != 4 && p->paths != 8) return tscm_set_error(TSCM_E_INVALID, "params: paths " + std::to_string(p->paths) + " is not 4 or 8");
    if (p->p1 < 0 || p->p1 > p->p2 || p->p2 > 255)
        return tscm_set_error(TSCM_E_INVALID, "params: p1 " + std::to_string(p->p1) + ", p2 " + std::to_string(p->p2) + " do not satisfy 0 <= p1 <= p2 <= 255");
    if (p->uniqueness_ratio < 0 || p->uniqueness_ratio > 99) return tscm_set_error(TSCM_E_INVALID, "params: uniqueness_ratio " + std::to_string(p->uniqueness_ratio) + " outside 0..99");
    return 0;
}

int check_frame(const tscm_sweep *s, const unsigned char *const *images, int stride)
{
    if (!s) return tscm_set_error(TSCM_E_INVALID, "s is NULL");
    if (!images) return tscm_set_error(TSCM_E_INVALID, "images is NULL");
    for (int k = 0; k < s->n; ++k)
        if (!images[k]) return tscm_set_error(TSCM_E_INVALID, "images[" + std::to_string(k) + "] is NULL");
    if (stride < s->w) return tscm_set_error(TSCM_E_INVALID, "stride " + std::to_string(stride) + " < width " + std::to_string(s->w));
    return 0;
}

using CostKernel = void (*)(const uint2 *, const unsigned char *, int, int, int, int, int, int, unsigned char *, unsigned char *, unsigned char *, unsigned long long *);

CostKernel cost_kernel(int n)
{
    switch (n) {
    case 2: return k_sweep_cost<2>;
    case 3: return k_sweep_cost<3>;
    case 4: return k_sweep_cost<4>;
    case 5: return k_sweep_cost<5>;
    case 6: return k_sweep_cost<6>;
    case 7: return k_sweep_cost<7>;
    default: return k_sweep_cost<8>;
    }
}

// The kernels of one frame.  sampled / alpha / census are device pointers (or NULL); the winner runs only `with_winner`.
int run_frame(tscm_sweep *s, const unsigned char *const *images, int stride, unsigned char *d_sampled, unsigned char *d_alpha, unsigned long long *d_census,
              bool with_winner, double *seconds_kernel)
{
    HIP_TRY(hipSetDevice(s->device));
    const size_t simg = (size_t)s->w * s->h;
    for (int k = 0; k < s->n; ++k) HIP_TRY(hipMemcpy2D(s->img + k * simg, (size_t)s->w, images[k], (size_t)stride, (size_t)s->w, (size_t)s->h, hipMemcpyHostToDevice));
    HIP_TRY(hipEventRecord(s->ev[0], 0));
    const dim3 grid((unsigned)((s->pw + kTileW - 1) / kTileW), (unsigned)((s->ph + kTileH - 1) / kTileH), (unsigned)(s->D / kZGroup));
    hipLaunchKernelGGL(cost_kernel(s->n), grid, dim3(256), 0, 0, s->pack, s->img, s->w, s->h, s->pw, s->ph, s->D, s->wrap, s->cost, d_sampled, d_alpha, d_census);
    HIP_TRY(hipEventRecord(s->ev[1], 0));
    launch_aggregate(s->cost, s->sum, s->pw, s->ph, s->D, s->p1, s->p2, s->paths);
    HIP_TRY(hipEventRecord(s->ev[2], 0));
    if (with_winner) {
        const dim3 g((unsigned)((s->npix + 3) / 4));
        const int npl = (s->D + 63) / 64;
        if (npl == 1) hipLaunchKernelGGL(k_sweep_winner<1>, g, dim3(256), 0, 0, s->sum, s->cost, s->pw, s->ph, s->D, s->uniqueness, s->index16);
        else if (npl == 2) hipLaunchKernelGGL(k_sweep_winner<2>, g, dim3(256), 0, 0, s->sum, s->cost, s->pw, s->ph, s->D, s->uniqueness, s->index16);
        else if (npl == 3) hipLaunchKernelGGL(k_sweep_winner<3>, g, dim3(256), 0, 0, s->sum, s->cost, s->pw, s->ph, s->D, s->uniqueness, s->index16);
        else hipLaunchKernelGGL(k_sweep_winner<4>, g, dim3(256), 0, 0, s->sum, s->cost, s->pw, s->ph, s->D, s->uniqueness, s->index16);
    }
    HIP_TRY(hipEventRecord(s->ev[3], 0));
    HIP_TRY(hipEventSynchronize(s->ev[3]));
    HIP_TRY(hipGetLastError());
    double total = 0.0;
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev[k], s->ev[k + 1]));
        g_stage_seconds[k] = 1e-3 * ms;
        total += 1e-3 * ms;
    }
    if (seconds_kernel) *seconds_kernel = total;
    return 0;
}

int create_on_device(tscm_sweep *s, const unsigned char *const *weights, const float *mapx, const float *mapy)
{
    const int n = s->n;
    const size_t simg = (size_t)s->w * s->h, ntab = (size_t)n * s->D * s->npix, nvol = s->npix * s->D;
    for (auto &e : s->ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(s->mem.alloc(&s->pack, ntab));
    HIP_TRY(s->mem.alloc(&s->img, n * simg));
    HIP_TRY(s->mem.alloc(&s->cost, nvol));
    HIP_TRY(s->mem.alloc(&s->sum, nvol));
    HIP_TRY(s->mem.alloc(&s->index16, s->npix));
    // the float tables and the weight images are needed only here
    float *d_mx = nullptr, *d_my = nullptr;
    unsigned char *d_w = nullptr;
    unsigned weight_mask = 0;
    HIP_TRY(s->mem.upload(&d_mx, mapx, ntab)); HIP_TRY(s->mem.upload(&d_my, mapy, ntab));
    HIP_TRY(s->mem.alloc(&d_w, n * simg));
    for (int k = 0; weights && k < n; ++k)
        if (weights[k]) {
            weight_mask |= 1u << k;
            HIP_TRY(hipMemcpy(d_w + k * simg, weights[k], simg, hipMemcpyHostToDevice));
        }
    hipLaunchKernelGGL(k_sweep_prepare, dim3((unsigned)((s->npix + 255) / 256), (unsigned)(n * s->D)), dim3(256), 0, 0, d_mx, d_my, d_w, weight_mask, s->w, s->h, s->D,
                       s->npix, s->pack);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    s->mem.release(d_mx); s->mem.release(d_my); s->mem.release(d_w);
    return 0;
}

}  // namespace

extern "C" void tscm_sweep_default_params(tscm_sweep_params *p)
{
    if (!p) return;
    p->struct_size = (int)sizeof(tscm_sweep_params);
    p->num_hypotheses = 64;
    p->p1 = 8; p->p2 = 32; p->paths = 8;
    p->uniqueness_ratio = 10; p->wrap_x = 1;
}

extern "C" int tscm_sweep_create(int n_cameras, int width, int height, const unsigned char *const *weights, const float *mapx, const float *mapy, int pano_w, int pano_h,
                                 const tscm_sweep_params *params, int device_index, tscm_sweep **out)
{
    if (!out) return tscm_set_error(TSCM_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!mapx) return tscm_set_error(TSCM_E_INVALID, "mapx is NULL");
    if (!mapy) return tscm_set_error(TSCM_E_INVALID, "mapy is NULL");
    if (int rc = check_params(params)) return rc;
    if (n_cameras < 2 || n_cameras > kMaxCameras) return tscm_set_error(TSCM_E_INVALID, "n_cameras " + std::to_string(n_cameras) + " outside 2..8");
    if (width < 1 || height < 1 || width > 32767 || height > 32767)
        return tscm_set_error(TSCM_E_INVALID, "width " + std::to_string(width) + ", height " + std::to_string(height) + ": a source image has 1..32767 pixels per side");
    if (pano_w < 1 || pano_h < 1) return tscm_set_error(TSCM_E_INVALID, "pano_w " + std::to_string(pano_w) + ", pano_h " + std::to_string(pano_h) + ": below 1");
    if ((unsigned long long)pano_w * (unsigned long long)pano_h > 0x7fffffffULL)
        return tscm_set_error(TSCM_E_UNSUPPORTED, "pano_w * pano_h beyond 2^31 - 1 pixels");
    if (int rc = select_device(device_index, "tscm_sweep_create")) return rc;
    std::unique_ptr<tscm_sweep> s(new tscm_sweep);
    s->n = n_cameras; s->w = width; s->h = height; s->pw = pano_w; s->ph = pano_h;
    s->D = params->num_hypotheses; s->p1 = params->p1; s->p2 = params->p2; s->paths = params->paths;
    s->uniqueness = params->uniqueness_ratio; s->wrap = params->wrap_x ? 1 : 0; s->device = device_index;
    s->npix = (size_t)pano_w * pano_h;
    if (int rc = create_on_device(s.get(), weights, mapx, mapy)) return rc;
    *out = s.release();
    return 0;
}

extern "C" int tscm_sweep_depth(tscm_sweep *s, const unsigned char *const *images, int stride, short *index16, int out_stride, double *seconds_kernel)
{
    if (int rc = check_frame(s, images, stride)) return rc;
    if (!index16) return tscm_set_error(TSCM_E_INVALID, "index16 is NULL");
    if (out_stride < s->pw) return tscm_set_error(TSCM_E_INVALID, "out_stride " + std::to_string(out_stride) + " < pano_w " + std::to_string(s->pw));
    if (seconds_kernel) *seconds_kernel = 0.0;
    if (int rc = run_frame(s, images, stride, nullptr, nullptr, nullptr, true, seconds_kernel)) return rc;
    // row padding of the caller's array keeps its values
    HIP_TRY(hipMemcpy2D(index16, (size_t)out_stride * sizeof(short), s->index16, (size_t)s->pw * sizeof(short), (size_t)s->pw * sizeof(short), (size_t)s->ph,
                        hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tscm_sweep_stages(tscm_sweep *s, const unsigned char *const *images, int stride, unsigned char *sampled, unsigned char *alpha, unsigned long long *census,
                                 unsigned char *cost, unsigned short *aggregated)
{
    if (int rc = check_frame(s, images, stride)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t ntab = (size_t)s->n * s->D * s->npix, nvol = s->npix * s->D;
    DeviceMem tmp;
    unsigned char *d_sampled = nullptr, *d_alpha = nullptr;
    unsigned long long *d_census = nullptr;
    if (sampled) HIP_TRY(tmp.alloc(&d_sampled, ntab));
    if (alpha) HIP_TRY(tmp.alloc(&d_alpha, ntab));
    if (census) HIP_TRY(tmp.alloc(&d_census, ntab));
    if (int rc = run_frame(s, images, stride, d_sampled, d_alpha, d_census, false, nullptr)) return rc;
    if (sampled) HIP_TRY(hipMemcpy(sampled, d_sampled, ntab, hipMemcpyDeviceToHost));
    if (alpha) HIP_TRY(hipMemcpy(alpha, d_alpha, ntab, hipMemcpyDeviceToHost));
    if (census) HIP_TRY(hipMemcpy(census, d_census, ntab * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (cost) HIP_TRY(hipMemcpy(cost, s->cost, nvol, hipMemcpyDeviceToHost));
    if (aggregated) HIP_TRY(hipMemcpy(aggregated, s->sum, nvol * sizeof(unsigned short), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tscm_sweep_stage_times(double *seconds)
{
    if (!seconds) return tscm_set_error(TSCM_E_INVALID, "seconds is NULL");
    for (int k = 0; k < 3; ++k) seconds[k] = g_stage_seconds[k];
    return 0;
}

extern "C" int tscm_sweep_points(const short *index16, int pano_w, int pano_h, int stride, const tscm_map_desc *pano_map, int projection, const double *inv_distance, int D,
                                 int device_index, double *points, unsigned char *valid)
{
    if (!index16) return tscm_set_error(TSCM_E_INVALID, "index16 is NULL");
    if (!pano_map) return tscm_set_error(TSCM_E_INVALID, "pano_map is NULL");
    if (!inv_distance) return tscm_set_error(TSCM_E_INVALID, "inv_distance is NULL");
    if (!points) return tscm_set_error(TSCM_E_INVALID, "points is NULL");
    if (!valid) return tscm_set_error(TSCM_E_INVALID, "valid is NULL");
    if (pano_w < 0 || pano_h < 0) return tscm_set_error(TSCM_E_INVALID, "negative pano_w or pano_h");
    if (stride < pano_w) return tscm_set_error(TSCM_E_INVALID, "stride " + std::to_string(stride) + " < pano_w " + std::to_string(pano_w));
    if (D < 2 || D > 2048) return tscm_set_error(TSCM_E_INVALID, "D " + std::to_string(D) + " outside 2..2048 (the interpolation needs two hypotheses, the index 16 bits)");
    for (int z = 0; z < D; ++z)
        if (!std::isfinite(inv_distance[z])) return tscm_set_error(TSCM_E_INVALID, "inv_distance[" + std::to_string(z) + "] is not finite");
    if (projection == TSCM_PROJ_PERSPECTIVE) return tscm_set_error(TSCM_E_UNSUPPORTED, "projection PERSPECTIVE: plane sweep is not built");
    if (projection < TSCM_PROJ_PERSPECTIVE || projection > TSCM_PROJ_EQUIRECT) return tscm_set_error(TSCM_E_INVALID, "unknown projection kind " + std::to_string(projection));
    if (pano_w == 0 || pano_h == 0) return 0;
    if (int rc = select_device(device_index, "tscm_sweep_points")) return rc;
    const size_t npix = (size_t)pano_w * pano_h;
    DeviceMem mem;
    short *d_idx = nullptr;
    const double *d_inv = nullptr;
    double *d_pts = nullptr;
    unsigned char *d_valid = nullptr;
    HIP_TRY(mem.alloc(&d_idx, npix)); HIP_TRY(mem.alloc(&d_pts, 3 * npix)); HIP_TRY(mem.alloc(&d_valid, npix));
    HIP_TRY(mem.upload(&d_inv, inv_distance, (size_t)D));
    HIP_TRY(hipMemcpy2D(d_idx, (size_t)pano_w * sizeof(short), index16, (size_t)stride * sizeof(short), (size_t)pano_w * sizeof(short), (size_t)pano_h, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_sweep_points, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, 0, d_idx, pano_w, pano_h, projection, pano_map->fx, pano_map->fy, pano_map->cx,
                       pano_map->cy, d_inv, D, d_pts, d_valid);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(points, d_pts, 3 * npix * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(valid, d_valid, npix, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" void tscm_sweep_destroy(tscm_sweep *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}
