// tscm_remap_sample.h -- the bilinear sample of the packed records (x = ix | iy << 16, y = fx | fy << 5 | alpha << 16) that
// the panorama composer (tscm_panorama.hip) and the sphere sweep (tscm_sweep.hip) keep per output pixel: the fixed-point
// arithmetic of k_remap.  Device code only, in an anonymous namespace like the other kernel headers.
#pragma once

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ void tap_weights(unsigned py, int (&wgt)[4])
{
    const int fx = py & 31, fy = (py >> 5) & 31;
    wgt[0] = 32 * (32 - fx) * (32 - fy); wgt[1] = 32 * fx * (32 - fy); wgt[2] = 32 * (32 - fx) * fy; wgt[3] = 32 * fx * fy;
    if (wgt[0] == 32768) { wgt[0] = 32767; wgt[3] = 1; }
}

// The packed record of one table entry (mx, my): the coordinates rounded to 1/32 px, the tap origin clamped to int16, and
// alpha = the bilinear sample of the camera's w x h weight image wk (has == false: a constant 255 inside the image).
__device__ __forceinline__ uint2 pack_record(float mx, float my, const unsigned char *__restrict__ wk, bool has, int w, int h)
{
    const int sx = __float2int_rn(mx * 32.0f), sy = __float2int_rn(my * 32.0f);
    const int ix = max(-32768, min(32767, sx >> 5)), iy = max(-32768, min(32767, sy >> 5));
    const unsigned frac = (unsigned)(sx & 31) | ((unsigned)(sy & 31) << 5);
    int wgt[4];
    tap_weights(frac, wgt);
    int acc = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int x = ix + (q & 1), y = iy + (q >> 1);
        if (x >= 0 && x < w && y >= 0 && y < h) acc += wgt[q] * (has ? (int)wk[(size_t)y * w + x] : 255);
    }
    const int a = max(0, min(255, (acc + (1 << 14)) >> 15));
    return make_uint2(((unsigned)ix & 0xffffu) | ((unsigned)iy << 16), frac | ((unsigned)a << 16));
}

// the arithmetic of k_remap for one output pixel of one image (rows of w * CH bytes)
template <int CH>
__device__ __forceinline__ void sample_px(const unsigned char *__restrict__ img, int w, int h, uint2 pk, int (&px)[CH])
{
    const int ix = (int)(short)(pk.x & 0xffffu), iy = (int)pk.x >> 16;
    int wgt[4];
    tap_weights(pk.y, wgt);
    int acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = ix + (k & 1), y = iy + (k >> 1);
        if (x >= 0 && x < w && y >= 0 && y < h) {
            const unsigned char *q = img + ((size_t)y * w + x) * CH;
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[c] += wgt[k] * q[c];
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) px[c] = max(0, min(255, (acc[c] + (1 << 14)) >> 15));
}

}  // namespace
