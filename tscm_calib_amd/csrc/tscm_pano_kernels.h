// tscm_pano_kernels.h -- the kernels of the panorama composer that do not care where the per-camera samples and masks come from:
// the Q8 gain, the packed output store, the Gaussian pyramid step, the mask sum, the Laplacian blend and the collapse.  Shared
// by tscm_panorama.hip, whose masks are constant per rig, and by the sweep's composer (tscm_sweep.hip), which builds them per
// frame.  In an anonymous namespace like the other kernel headers; behind the kernels the layout of a pyramid plane and the
// launches over its levels (host).
//   k_pano_wsum      W = sum_k M_k over a whole pyramid plane
//   k_pano_reduce    32 x 8 outputs per block from a 67 x 19 halo tile in LDS; the halo load clamps rows and wraps columns
//   k_pano_lapblend  64 x 16 tile of level l: per camera the 34 x 10 coarse halo of G^(l+1) in LDS, Lap = G^l - E(.) in
//                    registers, the weighted sum over the cameras, the floor division by W^l; a camera whose mask is zero
//                    over the whole tile is skipped
//   k_pano_collapse  R^l = B^l + E(R^(l+1)) in place; at level 0 the clamp, the coverage rule and the interleaved bytes
// A pyramid plane holds levels 0..L at offsets that are multiples of 8 elements, Sp elements in all; its padding stays zero.
#pragma once

#include <hip/hip_runtime.h>

#include "tscm_host.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace {

constexpr int kPanoMaxCameras = 16, kPanoMaxLevels = 6;
constexpr int kRedW = 32, kRedH = 8;                  // k_pano_reduce: outputs per block
constexpr int kPanoTileW = 64, kPanoTileH = 16;       // k_pano_lapblend / k_pano_collapse: fine pixels per block
constexpr int kPanoHaloW = kPanoTileW / 2 + 2, kPanoHaloH = kPanoTileH / 2 + 2;

struct Gains { unsigned short g[kPanoMaxCameras]; };

__device__ __forceinline__ int apply_gain(int v, int g) { return min(255, (v * g + 128) >> 8); }

// W = sum_k M_k over a whole pyramid plane (padding included: zero)
__global__ __launch_bounds__(256) void k_pano_wsum(const unsigned char *__restrict__ mpyr, int n, size_t Sp, unsigned short *__restrict__ wsum)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= Sp) return;
    int s = 0;
    for (int k = 0; k < n; ++k) s += mpyr[k * Sp + t];
    wsum[t] = (unsigned short)s;
}

// 4 or 12 output bytes of a quad: packed 32-bit stores when the quad is whole and its first byte is 4-aligned
template <int CH>
__device__ __forceinline__ void store_quad(unsigned char *__restrict__ out, size_t first_px, int nv, const int (&v)[4][CH])
{
    unsigned char b[4 * CH];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < CH; ++c) b[e * CH + c] = (unsigned char)v[e][c];
    unsigned char *q = out + first_px * CH;
    if (nv == 4 && (reinterpret_cast<uintptr_t>(q) & 3) == 0) {
#pragma unroll
        for (int i = 0; i < CH; ++i)
            reinterpret_cast<unsigned *>(q)[i] = (unsigned)b[4 * i] | ((unsigned)b[4 * i + 1] << 8) | ((unsigned)b[4 * i + 2] << 16) | ((unsigned)b[4 * i + 3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < 4 * CH; ++i)
            if (i < nv * CH) q[i] = b[i];
    }
}

// ------------------------------------------------------------------------------------------------ pyramids
__device__ __forceinline__ int col_index(int c, int W, int wrap) { return wrap ? ((c % W) + W) % W : min(max(c, 0), W - 1); }

// grid (ceil(dw / 32), ceil(dh / 8), planes) x 256: level (sw x sh at soff) -> level (sw / 2 x sh / 2 at doff) of every plane
template <typename T>
__global__ __launch_bounds__(256) void k_pano_reduce(T *__restrict__ pyr, int sw, int sh, size_t stride, size_t soff, size_t doff, int wrap)
{
    constexpr int LW = 2 * kRedW + 3, LH = 2 * kRedH + 3;
    __shared__ int tile[LH][LW + 1];
    const int dw = sw >> 1, dh = sh >> 1;
    const int x0 = blockIdx.x * kRedW, y0 = blockIdx.y * kRedH;
    const T *src = pyr + (size_t)blockIdx.z * stride + soff;
    for (int e = threadIdx.x; e < LW * LH; e += 256) {
        const int ty = e / LW, tx = e - ty * LW;
        const int gy = min(max(2 * y0 - 2 + ty, 0), sh - 1), gx = col_index(2 * x0 - 2 + tx, sw, wrap);
        tile[ty][tx] = (int)src[(size_t)gy * sw + gx];
    }
    __syncthreads();
    const int tx = threadIdx.x & (kRedW - 1), ty = threadIdx.x / kRedW;
    if (x0 + tx >= dw || y0 + ty >= dh) return;
    const int t[5] = { 1, 4, 6, 4, 1 };
    int acc = 0;
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = 0; b < 5; ++b) acc += t[a] * t[b] * tile[2 * ty + a][2 * tx + b];
    pyr[(size_t)blockIdx.z * stride + doff + (size_t)(y0 + ty) * dw + x0 + tx] = (T)((acc + 128) >> 8);
}

// the coarse halo of a 64 x 16 fine tile at (x0, y0): coarse rows y0 / 2 - 1 .. y0 / 2 + 8, columns x0 / 2 - 1 .. x0 / 2 + 32
__device__ __forceinline__ void load_halo(short (*halo)[kPanoHaloW + 2], const short *__restrict__ coarse, int Wc, int Hc, int x0, int y0, int wrap)
{
    for (int e = threadIdx.x; e < kPanoHaloW * kPanoHaloH; e += 256) {
        const int ry = e / kPanoHaloW, rx = e - ry * kPanoHaloW;
        const int gy = min(max(y0 / 2 - 1 + ry, 0), Hc - 1), gx = col_index(x0 / 2 - 1 + rx, Wc, wrap);
        halo[ry][rx] = coarse[(size_t)gy * Wc + gx];
    }
}

// E(x) at the tile's local fine pixel (ly, lx): an even coordinate takes coarse neighbours -1, 0, +1 with taps 1, 6, 1, an
// odd one the two it lies between with taps 4, 4
__device__ __forceinline__ int expand_at(const short (*halo)[kPanoHaloW + 2], int ly, int lx)
{
    const int ry = ly >> 1, rx = lx >> 1;
    const int wy0 = (ly & 1) ? 0 : 1, wy1 = (ly & 1) ? 4 : 6, wy2 = (ly & 1) ? 4 : 1;
    const int wx0 = (lx & 1) ? 0 : 1, wx1 = (lx & 1) ? 4 : 6, wx2 = (lx & 1) ? 4 : 1;
    const int r0 = wx0 * halo[ry][rx] + wx1 * halo[ry][rx + 1] + wx2 * halo[ry][rx + 2];
    const int r1 = wx0 * halo[ry + 1][rx] + wx1 * halo[ry + 1][rx + 1] + wx2 * halo[ry + 1][rx + 2];
    const int r2 = wx0 * halo[ry + 2][rx] + wx1 * halo[ry + 2][rx + 1] + wx2 * halo[ry + 2][rx + 2];
    return (wy0 * r0 + wy1 * r1 + wy2 * r2 + 32) >> 6;
}

__device__ __forceinline__ int floor_div(int num, int den)     // den > 0
{
    int q = num / den;
    if (num < 0 && q * den != num) --q;
    return q;
}

// grid (ceil(W / 64), ceil(H / 16)) x 256: thread (tx, ty) of 16 x 16 owns fine pixels (x0 + 4 tx .. + 3, y0 + ty) of level l
// (W x H at off; the coarse level Wc x Hc at offc; top: l == L, Lap = G).  lap != NULL: the Laplacians are written too.
template <int CH>
__global__ __launch_bounds__(256) void k_pano_lapblend(const short *__restrict__ G, const unsigned char *__restrict__ mpyr, const unsigned short *__restrict__ wsum,
                                                       int n, int W, int H, size_t off, size_t offc, size_t Sp, int top, int wrap, short *__restrict__ B,
                                                       short *__restrict__ lap)
{
    __shared__ short halo[CH][kPanoHaloH][kPanoHaloW + 2];
    const int x0 = blockIdx.x * kPanoTileW, y0 = blockIdx.y * kPanoTileH;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x = x0 + 4 * tx, y = y0 + ty;
    const int nv = (y < H && x < W) ? min(4, W - x) : 0;
    const bool vec = nv == 4 && (W & 3) == 0;
    const size_t at = off + (size_t)y * W + x;
    const int Wc = W >> 1, Hc = H >> 1;
    int acc[CH][4];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[c][e] = 0;
    for (int k = 0; k < n; ++k) {
        int m[4] = { 0, 0, 0, 0 };
        if (vec) {
            const unsigned mv = *reinterpret_cast<const unsigned *>(mpyr + k * Sp + at);
            m[0] = mv & 0xff; m[1] = (mv >> 8) & 0xff; m[2] = (mv >> 16) & 0xff; m[3] = mv >> 24;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < nv) m[e] = mpyr[k * Sp + at + e];
        }
        // also the barrier between the previous camera's reads of the halo and this camera's load
        const int used = __syncthreads_or(m[0] | m[1] | m[2] | m[3]);
        if (!used && !lap) continue;                          // block-uniform
        if (!top) {
#pragma unroll
            for (int c = 0; c < CH; ++c) load_halo(halo[c], G + (size_t)(k * CH + c) * Sp + offc, Wc, Hc, x0, y0, wrap);
            __syncthreads();
        }
        if (nv == 0) continue;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const short *g = G + (size_t)(k * CH + c) * Sp + at;
            int gv[4] = { 0, 0, 0, 0 };
            if (vec) {
                const uint2 q = *reinterpret_cast<const uint2 *>(g);
                gv[0] = (short)(q.x & 0xffffu); gv[1] = (int)q.x >> 16; gv[2] = (short)(q.y & 0xffffu); gv[3] = (int)q.y >> 16;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < nv) gv[e] = g[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= nv) continue;
                const int lv = gv[e] - (top ? 0 : expand_at(halo[c], ty, 4 * tx + e));
                if (lap) lap[(size_t)(k * CH + c) * Sp + at + e] = (short)lv;
                acc[c][e] += m[e] * lv;
            }
        }
    }
    if (nv == 0) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e >= nv) continue;
        const int Wsum = wsum[at + e];
#pragma unroll
        for (int c = 0; c < CH; ++c) B[(size_t)c * Sp + at + e] = (short)(Wsum ? floor_div(acc[c][e] + (Wsum >> 1), Wsum) : 0);
    }
}

// same grid and ownership: R^l = B^l + E(R^(l+1)), in place; FINAL (l == 0): the output bytes instead
template <int CH, int FINAL>
__global__ __launch_bounds__(256) void k_pano_collapse(short *__restrict__ B, int W, int H, size_t off, size_t offc, size_t Sp, int wrap,
                                                       const unsigned char *__restrict__ cover, unsigned char *__restrict__ out)
{
    __shared__ short halo[CH][kPanoHaloH][kPanoHaloW + 2];
    const int x0 = blockIdx.x * kPanoTileW, y0 = blockIdx.y * kPanoTileH;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x = x0 + 4 * tx, y = y0 + ty;
    const int nv = (y < H && x < W) ? min(4, W - x) : 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) load_halo(halo[c], B + (size_t)c * Sp + offc, W >> 1, H >> 1, x0, y0, wrap);
    __syncthreads();
    if (nv == 0) return;
    const size_t at = off + (size_t)y * W + x;
    int v[4][CH];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            v[e][c] = 0;
            if (e < nv) v[e][c] = B[(size_t)c * Sp + at + e] + expand_at(halo[c], ty, 4 * tx + e);
        }
    if (FINAL) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool seen = e < nv && cover[at + e] > 0;       // off == 0 at level 0
#pragma unroll
            for (int c = 0; c < CH; ++c) v[e][c] = seen ? max(0, min(255, v[e][c])) : 0;
        }
        store_quad<CH>(out, at, nv, v);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < CH; ++c)
                if (e < nv) B[(size_t)c * Sp + at + e] = (short)v[e][c];
    }
}

// ------------------------------------------------------------------------------------------------ host
// levels 0..L of a pano_w x pano_h plane: on the device at offsets that are multiples of 8 elements (Sp in all), in the stage
// outputs one after the other without padding (S in all)
struct PyramidLayout {
    int levels = 0, lw[kPanoMaxLevels + 1] = {}, lh[kPanoMaxLevels + 1] = {};
    size_t loff[kPanoMaxLevels + 1] = {}, toff[kPanoMaxLevels + 1] = {}, Sp = 0, S = 0;
    void set_levels(int pano_w, int pano_h, int L)
    {
        levels = L; Sp = 0; S = 0;
        for (int l = 0; l <= L; ++l) {
            lw[l] = pano_w >> l; lh[l] = pano_h >> l;
            loff[l] = Sp; toff[l] = S;
            S += (size_t)lw[l] * lh[l];
            Sp = (Sp + (size_t)lw[l] * lh[l] + 7) & ~(size_t)7;
        }
    }
};

inline unsigned quad_blocks(size_t npix) { return (unsigned)((npix + 1023) / 1024); }
inline dim3 tile_grid(int W, int H) { return dim3((unsigned)((W + kPanoTileW - 1) / kPanoTileW), (unsigned)((H + kPanoTileH - 1) / kPanoTileH)); }

// levels 1..L of `planes` planes from their level 0
template <typename T>
void launch_reduce(const PyramidLayout &y, T *pyr, int planes, int wrap)
{
    for (int l = 0; l < y.levels; ++l)
        hipLaunchKernelGGL(k_pano_reduce<T>, dim3((unsigned)((y.lw[l + 1] + kRedW - 1) / kRedW), (unsigned)((y.lh[l + 1] + kRedH - 1) / kRedH), (unsigned)planes), dim3(256), 0,
                           0, pyr, y.lw[l], y.lh[l], y.Sp, y.loff[l], y.loff[l + 1], wrap);
}

// B^l of every level from the image pyramids, the mask pyramids and their sums, then (collapse) the output bytes
template <int CH>
void launch_blend(const PyramidLayout &y, const short *G, const unsigned char *mpyr, const unsigned short *wsum, int n, int wrap, short *B, short *lap, bool collapse,
                  const unsigned char *cover, unsigned char *out)
{
    const int L = y.levels;
    for (int l = 0; l <= L; ++l)
        hipLaunchKernelGGL(k_pano_lapblend<CH>, tile_grid(y.lw[l], y.lh[l]), dim3(256), 0, 0, G, mpyr, wsum, n, y.lw[l], y.lh[l], y.loff[l], l < L ? y.loff[l + 1] : (size_t)0,
                           y.Sp, l == L ? 1 : 0, wrap, B, lap);
    if (!collapse) return;
    for (int l = L - 1; l >= 1; --l)
        hipLaunchKernelGGL((k_pano_collapse<CH, 0>), tile_grid(y.lw[l], y.lh[l]), dim3(256), 0, 0, B, y.lw[l], y.lh[l], y.loff[l], y.loff[l + 1], y.Sp, wrap, cover, out);
    hipLaunchKernelGGL((k_pano_collapse<CH, 1>), tile_grid(y.lw[0], y.lh[0]), dim3(256), 0, 0, B, y.lw[0], y.lh[0], (size_t)0, y.loff[1], y.Sp, wrap, cover, out);
}

// `planes` device planes of Sp elements -> planes of S elements; host == NULL: the output was not asked for
template <typename T>
int download_pyramid(const PyramidLayout &y, const T *dev, int planes, T *host)
{
    if (!host) return 0;
    std::vector<T> tmp((size_t)planes * y.Sp);
    HIP_TRY(hipMemcpy(tmp.data(), dev, tmp.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (int q = 0; q < planes; ++q)
        for (int l = 0; l <= y.levels; ++l)
            std::copy_n(tmp.data() + (size_t)q * y.Sp + y.loff[l], (size_t)y.lw[l] * y.lh[l], host + (size_t)q * y.S + y.toff[l]);
    return 0;
}

// the per-camera gains of a frame: gain_q8[0 .. n), or 256 (= 1.0) for every camera when it is NULL
inline int check_gains(const unsigned short *gain_q8, int n, Gains *gains)
{
    for (int k = 0; k < kPanoMaxCameras; ++k) gains->g[k] = 256;
    for (int k = 0; gain_q8 && k < n; ++k) {
        if (gain_q8[k] < 1 || gain_q8[k] > 4095) return tscm_set_error(TSCM_E_INVALID, "gain_q8[" + std::to_string(k) + "] = " + std::to_string(gain_q8[k]) + " outside 1..4095");
        gains->g[k] = gain_q8[k];
    }
    return 0;
}

}  // namespace
