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
