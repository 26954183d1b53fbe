// tscm_stereo_refine.hip -- edge-aware weighted median of a disparity or sweep index map (tscm.h: tscm_stereo_refine*): each
// pixel takes the lower weighted median of the valid pixels of its (2 radius + 1)^2 window, a neighbour weighted by a table
// of the grey difference between it and the centre in a guide image.  Integers only and no atomics; equal values
// accumulate, so nothing depends on an order and a host restatement (tests/stereo_refine_ref.py) gives the same bits.
//
// No loop's trip count depends on the map: the median is found by bisection on the 16 bits of the order-preserving key
// d + 32768, and each of the 16 steps sweeps the whole window, (2 radius + 1)^2 * 16 compare-adds per pixel whatever the
// map holds.
//
//   k_refine<R>   one launch per pass, one workgroup per 32 x 8 tile, one thread per pixel.  The tile and its halo of R go
//                 into LDS as one word per pixel, key << 16 | valid << 8 | grey; rows outside the map, columns outside it
//                 (or taken modulo the width with wrap_x) and invalid pixels are resolved there, so the window loops test
//                 no bounds.  A thread reads its window once and keeps key << 16 | weight per neighbour in registers (the
//                 table, 256 bytes in LDS, is looked up once per pair, non-participants get weight 0); the sum of the
//                 weights at or below a threshold t is then one compare, one select and one add per neighbour:
//                 key <= t  <=>  packed < (t + 1) << 16, and the low half of the sum of the selected words is the sum of
//                 their weights.
// Passes ping-pong between two device maps; launch boundaries are the only ordering between workgroups.
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_host.h"

#include <climits>
#include <cmath>
#include <string>

using namespace tscm;

namespace {

constexpr int kTileW = 32, kTileH = 8;        // 256 threads; a wave holds two tile rows

template <int R>
__global__ __launch_bounds__(256) void k_refine(const short *__restrict__ d, const unsigned char *__restrict__ g, const unsigned char *__restrict__ lut, int w, int h,
                                                int invalid, int fill_invalid, int wrap, unsigned tiles_x, short *__restrict__ out, int *__restrict__ weight_sum,
                                                unsigned char *__restrict__ count)
{
    constexpr int SW = kTileW + 2 * R, SH = kTileH + 2 * R, N = (2 * R + 1) * (2 * R + 1);
    __shared__ unsigned tile[SH * SW];
    __shared__ unsigned char table[256];
    const int tid = threadIdx.x;
    const int tx0 = (int)(blockIdx.x % tiles_x) * kTileW, ty0 = (int)(blockIdx.x / tiles_x) * kTileH;
    table[tid] = lut[tid];
    for (int i = tid; i < SH * SW; i += 256) {
        const int sy = i / SW, sx = i - sy * SW, y = ty0 + sy - R;
        long long x = (long long)tx0 + sx - R;
        if (wrap) {
            x %= w;
            if (x < 0) x += w;
        }
        unsigned e = 0;                                      // key 0, not valid: weight 0 below
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const size_t at = (size_t)y * w + (size_t)x;
            const int v = d[at];
            e = ((unsigned)(v + 32768) << 16) | (v != invalid ? 0x100u : 0u) | g[at];
        }
        tile[i] = e;
    }
    __syncthreads();
    const int lx = tid & (kTileW - 1), ly = tid >> 5;
    const long long x = (long long)tx0 + lx;
    const int y = ty0 + ly;
    if (x >= w || y >= h) return;                            // after the only barrier
    const unsigned centre = tile[(ly + R) * SW + lx + R];
    const int gp = (int)(centre & 0xffu), dp = (int)(centre >> 16) - 32768;
    unsigned pk[N], W = 0, cnt = 0;
#pragma unroll
    for (int dy = 0; dy <= 2 * R; ++dy) {
#pragma unroll
        for (int dx = 0; dx <= 2 * R; ++dx) {
            const unsigned e = tile[(ly + dy) * SW + lx + dx], valid = (e >> 8) & 1u;
            const int diff = gp - (int)(e & 0xffu);
            const unsigned wq = (unsigned)table[diff < 0 ? -diff : diff] & (0u - valid);      // looked up always: no branch per neighbour
            pk[dy * (2 * R + 1) + dx] = (e & 0xffff0000u) | wq;
            W += wq;
            cnt += valid;
        }
        // One window row at a time, its packed words and the two sums pinned in registers here: left alone, the compiler
        // sinks the packing and the count behind the last row and keeps every row's words, greys, table entries and valid
        // bits live until then, three registers per neighbour instead of one.
#pragma unroll
        for (int dx = 0; dx <= 2 * R; ++dx) asm volatile("" : "+v"(pk[dy * (2 * R + 1) + dx]));
        asm volatile("" : "+v"(W), "+v"(cnt));
    }
    const size_t at = (size_t)y * w + (size_t)x;
    if (weight_sum) weight_sum[at] = (int)W;
    if (count) count[at] = (unsigned char)cnt;
    // the smallest key t with 2 S(t) >= W, S(t) the weight of the keys <= t, from its top bit down: with the higher bits
    // settled, bit b is set iff the keys strictly below (settled | bit) do not reach half of W.  S only steps at a
    // participant's key, so t is one of them whenever W > 0.
    unsigned t = 0;
#pragma unroll 1
    for (int b = 15; b >= 0; --b) {
        const unsigned trial = t | (1u << b), limit = trial << 16;
        unsigned s = 0;                                      // the whole words are added: the weights sum to at most 225 * 255
#pragma unroll                                               // < 2^16 and carries only travel upwards, so bits 0..15 of s
        for (int k = 0; k < N; ++k) s += pk[k] < limit ? pk[k] : 0u;      // are the sum of the weights
        if (2u * (s & 0xffffu) < W) t = trial;
    }
    int res = (int)t - 32768;
    if (W == 0) res = dp;
    if (dp == invalid && !fill_invalid) res = invalid;
    out[at] = (short)res;
}

typedef void (*refine_kernel)(const short *, const unsigned char *, const unsigned char *, int, int, int, int, int, unsigned, short *, int *, unsigned char *);
const refine_kernel kKernels[7] = { k_refine<1>, k_refine<2>, k_refine<3>, k_refine<4>, k_refine<5>, k_refine<6>, k_refine<7> };

// ------------------------------------------------------------------------------------------------ host
int check_refine_args(const short *disparity, int width, int height, int disp_stride, const unsigned char *guide, int guide_stride, const tscm_stereo_refine_params *p)
{
    if (int rc = check_map_args(disparity, width, height, disp_stride, p, "tscm_stereo_refine_params", &guide, guide_stride)) return rc;
    if (p->radius < 1 || p->radius > 7) return tscm_set_error(TSCM_E_INVALID, "params: radius " + std::to_string(p->radius) + " outside 1..7");
    if (p->iterations < 1 || p->iterations > 8) return tscm_set_error(TSCM_E_INVALID, "params: iterations " + std::to_string(p->iterations) + " outside 1..8");
    if (p->fill_invalid != 0 && p->fill_invalid != 1) return tscm_set_error(TSCM_E_INVALID, "params: fill_invalid " + std::to_string(p->fill_invalid) + " is not 0 or 1");
    if (p->wrap_x != 0 && p->wrap_x != 1) return tscm_set_error(TSCM_E_INVALID, "params: wrap_x " + std::to_string(p->wrap_x) + " is not 0 or 1");
    if (int rc = check_map_min_disparity(p->min_disparity)) return rc;
    if ((long long)width * height > INT_MAX)
        return tscm_set_error(TSCM_E_INVALID, "width " + std::to_string(width) + " x height " + std::to_string(height) + " above INT_MAX pixels");
    return 0;
}

// `passes` launches on one map.  Outputs are host pointers; out [h][out_stride] is the map after the last pass, weight_sum
// and count (either may be NULL) are those of the first.
int refine_run(const short *disparity, int w, int h, int disp_stride, const unsigned char *guide, int guide_stride, const unsigned char *range_weight,
               const tscm_stereo_refine_params &p, int passes, int device, const char *who, short *out, int out_stride, int *weight_sum, unsigned char *count,
               double *seconds_kernel)
{
    if (int rc = select_device(device, who)) return rc;
    const size_t n = (size_t)w * h;
    const int invalid = 16 * (p.min_disparity - 1);
    unsigned char table[256];
    for (int k = 0; k < 256; ++k) table[k] = range_weight ? range_weight[k] : 255;
    DeviceMem mem;
    StageOutputs stages(mem);
    EventSpan span;
    short *d_map[2] = { nullptr, nullptr };
    unsigned char *d_guide = nullptr, *d_table = nullptr, *d_count = nullptr;
    int *d_sum = nullptr;
    HIP_TRY(mem.alloc(&d_map[0], n));
    HIP_TRY(mem.alloc(&d_map[1], n));
    HIP_TRY(mem.alloc(&d_guide, n));
    HIP_TRY(mem.upload(&d_table, table, (size_t)256));
    HIP_TRY(stages.scratch(&d_sum, weight_sum, n));
    HIP_TRY(stages.scratch(&d_count, count, n));
    HIP_TRY(copy_rows(d_map[0], w, disparity, disp_stride, w, h, hipMemcpyHostToDevice));
    HIP_TRY(copy_rows(d_guide, w, guide, guide_stride, w, h, hipMemcpyHostToDevice));
    const unsigned tiles_x = (unsigned)(((long long)w + kTileW - 1) / kTileW), tiles_y = (unsigned)((h + kTileH - 1) / kTileH);
    HIP_TRY(span.create(2));
    HIP_TRY(span.mark(0));
    for (int i = 0; i < passes; ++i)                         // Jacobi: pass i + 1 reads the whole output of pass i
        hipLaunchKernelGGL(kKernels[p.radius - 1], dim3(tiles_x * tiles_y), dim3(256), 0, 0, d_map[i & 1], d_guide, d_table, w, h, invalid, p.fill_invalid, p.wrap_x,
                           tiles_x, d_map[(i + 1) & 1], i == 0 ? d_sum : nullptr, i == 0 ? d_count : nullptr);
    HIP_TRY(span.finish(1, nullptr, seconds_kernel));
    if (out) HIP_TRY(copy_rows(out, out_stride, d_map[passes & 1], w, w, h, hipMemcpyDeviceToHost));
    HIP_TRY(stages.fetch());
    return 0;
}

}  // namespace

extern "C" void tscm_stereo_refine_default_params(tscm_stereo_refine_params *p)
{
    if (!p) return;
    p->struct_size = (int)sizeof(tscm_stereo_refine_params);
    p->min_disparity = 0;
    p->radius = 3;
    p->iterations = 1;
    p->fill_invalid = 0;
    p->wrap_x = 0;
}

extern "C" void tscm_stereo_refine_weights(double sigma, unsigned char *range_weight)
{
    if (!range_weight) return;
    for (int k = 0; k < 256; ++k)
        range_weight[k] = sigma > 0.0 ? (unsigned char)std::floor(255.0 * std::exp(-(double)k / sigma) + 0.5) : (k == 0 ? 255 : 0);     // NaN is not > 0
}

extern "C" int tscm_stereo_refine(const short *disparity, int width, int height, int disp_stride, const unsigned char *guide, int guide_stride,
                                  const unsigned char *range_weight, const tscm_stereo_refine_params *params, int device, short *out, int out_stride,
                                  double *seconds_kernel)
{
    if (int rc = check_refine_args(disparity, width, height, disp_stride, guide, guide_stride, params)) return rc;
    if (int rc = check_map_out(out, out_stride, width)) return rc;
    if (seconds_kernel) *seconds_kernel = 0.0;
    if (width == 0 || height == 0) return 0;
    return refine_run(disparity, width, height, disp_stride, guide, guide_stride, range_weight, *params, params->iterations, device, "tscm_stereo_refine", out, out_stride,
                      nullptr, nullptr, seconds_kernel);
}

extern "C" int tscm_stereo_refine_stages(const short *disparity, int width, int height, int disp_stride, const unsigned char *guide, int guide_stride,
                                         const unsigned char *range_weight, const tscm_stereo_refine_params *params, int device, int *weight_sum,
                                         unsigned char *count, short *first_pass)
{
    if (int rc = check_refine_args(disparity, width, height, disp_stride, guide, guide_stride, params)) return rc;
    if (width == 0 || height == 0) return 0;
    return refine_run(disparity, width, height, disp_stride, guide, guide_stride, range_weight, *params, 1, device, "tscm_stereo_refine_stages", first_pass, width,
                      weight_sum, count, nullptr);
}
