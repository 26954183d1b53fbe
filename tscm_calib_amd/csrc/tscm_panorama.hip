// tscm_panorama.hip -- the panorama of a calibrated rig (tscm.h: tscm_panorama_*): per-camera bilinear samples through the
// rig's remap tables, composed by seam, feather or multi-band blending.  Integer arithmetic up to the output bytes, defined
// in tscm.h so that a host restatement (tests/pano_ref.py) gives the same bits.
//
// Constant per rig, built once by tscm_panorama_create and kept on the device:
//   pack   [n][plane] uint2: x = ix | iy << 16 (the int16 tap origin), y = fx | fy << 5 | a_k << 16 (1/32 px fractions, alpha)
//   label  [plane] uint8, cover [plane] uint8, mask [plane] uint16 (bit k: a_k > 0)
//   mpyr   [n][Sp] uint8 the mask pyramids M_k^l, wsum [Sp] uint16 their sums W^l
// (plane = pano_w * pano_h rounded up to 4, so that the last quad's vector loads stay inside; a pyramid plane holds levels
// 0..L at offsets that are multiples of 8 elements, Sp elements in all).
// Per frame:
//   k_pano_compose   SEAM / FEATHER in one launch: a thread owns 4 adjacent output pixels, reads label / mask and the packed
//                    samples with 4- to 16-byte loads, skips a camera that no lane of the wave needs (ballot), and stores 4
//                    or 12 packed output bytes; no per-camera plane is written
//   k_pano_sample    MULTIBAND: G^0 of every camera and channel as int16 planes, 4 pixels per thread
//   k_pano_reduce    32 x 8 outputs per block from a 67 x 19 halo tile in LDS; the halo load clamps rows and wraps columns
//   k_pano_lapblend  64 x 16 tile of level l: per camera the 34 x 10 coarse halo of G^(l+1) in LDS, Lap = G^l - E(.) in
//                    registers, the weighted sum over the cameras, the floor division by W^l; a camera whose mask is zero
//                    over the whole tile is skipped
//   k_pano_collapse  R^l = B^l + E(R^(l+1)) in place; at level 0 the clamp, the coverage rule and the interleaved bytes
//   k_pano_overlap   count / sum of the camera pairs: LDS partials per block, then 64-bit integer atomics
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_host.h"
#include "tscm_remap_sample.h"

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

using namespace tscm;

namespace {

constexpr int kMaxCameras = 16, kMaxLevels = 6;
constexpr int kRedW = 32, kRedH = 8;          // k_pano_reduce: outputs per block
constexpr int kTileW = 64, kTileH = 16;       // k_pano_lapblend / k_pano_collapse: fine pixels per block
constexpr int kHaloW = kTileW / 2 + 2, kHaloH = kTileH / 2 + 2;

struct Gains { unsigned short g[kMaxCameras]; };

// ------------------------------------------------------------------------------------------------ sampling
// tap_weights, sample_px: tscm_remap_sample.h
__device__ __forceinline__ int apply_gain(int v, int g) { return min(255, (v * g + 128) >> 8); }

// grid (ceil(npix / 256), n) x 256: the packed sample and a_k of camera blockIdx.y; weight_mask bit k: camera k has a
// weight image (at wimg + k * w * h), otherwise a constant 255 inside the image
__global__ __launch_bounds__(256) void k_pano_prepare(const float *__restrict__ mapx, const float *__restrict__ mapy, const unsigned char *__restrict__ wimg,
                                                      unsigned weight_mask, int w, int h, size_t npix, size_t plane, uint2 *__restrict__ pack,
                                                      unsigned char *__restrict__ alpha)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (t >= npix) return;
    const int sx = __float2int_rn(mapx[k * npix + t] * 32.0f), sy = __float2int_rn(mapy[k * npix + t] * 32.0f);
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
    pack[k * plane + t] = make_uint2(((unsigned)ix & 0xffffu) | ((unsigned)iy << 16), frac | ((unsigned)a << 16));
    alpha[k * plane + t] = (unsigned char)a;
}

// one thread per output pixel: label, coverage, the bit mask of the covering cameras and (mpyr != NULL) level 0 of the masks
__global__ __launch_bounds__(256) void k_pano_label(const unsigned char *__restrict__ alpha, int n, size_t npix, size_t plane, unsigned char *__restrict__ label,
                                                    unsigned char *__restrict__ cover, unsigned short *__restrict__ mask, unsigned char *__restrict__ mpyr, size_t Sp)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= npix) return;
    int best = 0, lab = 255, cnt = 0;
    unsigned bits = 0;
    for (int k = 0; k < n; ++k) {
        const int a = alpha[k * plane + t];
        if (a > 0) { ++cnt; bits |= 1u << k; }
        if (a > best) { best = a; lab = k; }
    }
    label[t] = (unsigned char)lab; cover[t] = (unsigned char)cnt; mask[t] = (unsigned short)bits;
    if (mpyr)
        for (int k = 0; k < n; ++k) mpyr[k * Sp + t] = lab == k ? 255 : 0;
}

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

// grid ceil(npix / 1024) x 256: quad q = output pixels [4q, 4q + 4) of the flat panorama
template <int CH, int MODE>
__global__ __launch_bounds__(256) void k_pano_compose(const uint2 *__restrict__ pack, const unsigned char *__restrict__ label, const unsigned short *__restrict__ mask,
                                                      const unsigned char *__restrict__ img, int n, int w, int h, size_t npix, size_t plane, Gains gains,
                                                      unsigned char *__restrict__ out)
{
    const size_t t0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (t0 >= npix) return;
    const int nv = (int)min((size_t)4, npix - t0);
    const size_t img_bytes = (size_t)w * h * CH;
    int v[4][CH], num[4][CH], A[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        A[e] = 0;
#pragma unroll
        for (int c = 0; c < CH; ++c) { v[e][c] = 0; num[e][c] = 0; }
    }
    unsigned lab4 = 0, bits[4] = { 0, 0, 0, 0 }, any = 0;
    if (MODE == TSCM_PANO_SEAM) lab4 = *reinterpret_cast<const unsigned *>(label + t0);
    else {
        const uint2 m = *reinterpret_cast<const uint2 *>(mask + t0);
        bits[0] = m.x & 0xffffu; bits[1] = m.x >> 16; bits[2] = m.y & 0xffffu; bits[3] = m.y >> 16;
        any = bits[0] | bits[1] | bits[2] | bits[3];
    }
    for (int k = 0; k < n; ++k) {
        bool mine;
        if (MODE == TSCM_PANO_SEAM)
            mine = (lab4 & 0xffu) == (unsigned)k || ((lab4 >> 8) & 0xffu) == (unsigned)k || ((lab4 >> 16) & 0xffu) == (unsigned)k || (lab4 >> 24) == (unsigned)k;
        else mine = (any >> k) & 1u;
        if (__ballot(mine) == 0) continue;                   // no lane of the wave needs camera k: its gathers are skipped
        if (!mine) continue;
        const uint4 p01 = *reinterpret_cast<const uint4 *>(pack + k * plane + t0), p23 = *reinterpret_cast<const uint4 *>(pack + k * plane + t0 + 2);
        const uint2 pk[4] = { make_uint2(p01.x, p01.y), make_uint2(p01.z, p01.w), make_uint2(p23.x, p23.y), make_uint2(p23.z, p23.w) };
        const int g = gains.g[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int a = (int)(pk[e].y >> 16);
            const bool take = MODE == TSCM_PANO_SEAM ? ((lab4 >> (8 * e)) & 0xffu) == (unsigned)k : a > 0;
            if (!take) continue;
            int px[CH];
            sample_px<CH>(img + k * img_bytes, w, h, pk[e], px);
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int s = apply_gain(px[c], g);
                if (MODE == TSCM_PANO_SEAM) v[e][c] = s;
                else num[e][c] += a * s;
            }
            A[e] += a;
        }
    }
    if (MODE == TSCM_PANO_FEATHER) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < CH; ++c) v[e][c] = A[e] ? (int)(((unsigned)num[e][c] + ((unsigned)A[e] >> 1)) / (unsigned)A[e]) : 0;
    }
    store_quad<CH>(out, t0, nv, v);
}

// grid (ceil(npix / 1024), n) x 256: G^0 of camera blockIdx.y, planes (k * CH + c) * Sp
template <int CH>
__global__ __launch_bounds__(256) void k_pano_sample(const uint2 *__restrict__ pack, const unsigned char *__restrict__ img, int w, int h, size_t npix, size_t plane,
                                                     Gains gains, short *__restrict__ G, size_t Sp)
{
    const size_t t0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const int k = blockIdx.y;
    if (t0 >= npix) return;
    const int nv = (int)min((size_t)4, npix - t0);
    const uint4 p01 = *reinterpret_cast<const uint4 *>(pack + k * plane + t0), p23 = *reinterpret_cast<const uint4 *>(pack + k * plane + t0 + 2);
    const uint2 pk[4] = { make_uint2(p01.x, p01.y), make_uint2(p01.z, p01.w), make_uint2(p23.x, p23.y), make_uint2(p23.z, p23.w) };
    const int g = gains.g[k];
    int v[4][CH];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sample_px<CH>(img + (size_t)k * w * h * CH, w, h, pk[e], v[e]);
#pragma unroll
        for (int c = 0; c < CH; ++c) v[e][c] = apply_gain(v[e][c], g);
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        short *q = G + (size_t)(k * CH + c) * Sp + t0;
        if (nv == 4) *reinterpret_cast<uint2 *>(q) = make_uint2((unsigned)v[0][c] | ((unsigned)v[1][c] << 16), (unsigned)v[2][c] | ((unsigned)v[3][c] << 16));
        else
            for (int e = 0; e < nv; ++e) q[e] = (short)v[e][c];
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
__device__ __forceinline__ void load_halo(short (*halo)[kHaloW + 2], const short *__restrict__ coarse, int Wc, int Hc, int x0, int y0, int wrap)
{
    for (int e = threadIdx.x; e < kHaloW * kHaloH; e += 256) {
        const int ry = e / kHaloW, rx = e - ry * kHaloW;
        const int gy = min(max(y0 / 2 - 1 + ry, 0), Hc - 1), gx = col_index(x0 / 2 - 1 + rx, Wc, wrap);
        halo[ry][rx] = coarse[(size_t)gy * Wc + gx];
    }
}

// E(x) at the tile's local fine pixel (ly, lx): an even coordinate takes coarse neighbours -1, 0, +1 with taps 1, 6, 1, an
// odd one the two it lies between with taps 4, 4
__device__ __forceinline__ int expand_at(const short (*halo)[kHaloW + 2], int ly, int lx)
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
    __shared__ short halo[CH][kHaloH][kHaloW + 2];
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
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
    __shared__ short halo[CH][kHaloH][kHaloW + 2];
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
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

// ------------------------------------------------------------------------------------------------ overlap
// grid ceil(npix / 1024) x 256; acc[a * 16 + b] = count, acc[256 + a * 16 + b] = sum.  A block sees at most 1024 pixels, so
// its partials fit 32 bits.
template <int CH>
__global__ __launch_bounds__(256) void k_pano_overlap(const uint2 *__restrict__ pack, const unsigned short *__restrict__ mask, const unsigned char *__restrict__ img,
                                                      int w, int h, size_t npix, size_t plane, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned cnt[256], sum[256];
    cnt[threadIdx.x] = 0; sum[threadIdx.x] = 0;
    __syncthreads();
    const size_t t0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    for (int e = 0; e < 4; ++e) {
        const size_t t = t0 + e;
        if (t >= npix) break;
        const unsigned bits = mask[t];
        for (unsigned ra = bits; ra; ra &= ra - 1) {
            const int a = __ffs(ra) - 1;
            int px[CH];
            sample_px<CH>(img + (size_t)a * w * h * CH, w, h, pack[a * plane + t], px);
            const int lum = CH == 3 ? (px[0] * 1868 + px[CH > 1 ? 1 : 0] * 9617 + px[CH > 2 ? 2 : 0] * 4899 + (1 << 13)) >> 14 : px[0];
            for (unsigned rb = bits; rb; rb &= rb - 1) {
                const int b = __ffs(rb) - 1;
                atomicAdd(&cnt[a * 16 + b], 1u);
                atomicAdd(&sum[a * 16 + b], (unsigned)lum);
            }
        }
    }
    __syncthreads();
    if (cnt[threadIdx.x]) {
        atomicAdd(&acc[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
        atomicAdd(&acc[256 + threadIdx.x], (unsigned long long)sum[threadIdx.x]);
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host
struct tscm_panorama {
    int n = 0, w = 0, h = 0, ch = 0, pw = 0, ph = 0, mode = 0, levels = 0, wrap = 0, device = 0;
    size_t npix = 0, plane = 0;             // output pixels; the same rounded up to 4
    int lw[kMaxLevels + 1] = {}, lh[kMaxLevels + 1] = {};
    size_t loff[kMaxLevels + 1] = {}, toff[kMaxLevels + 1] = {}, Sp = 0, S = 0;    // level offsets on the device / in the stage outputs
    DeviceMem mem;
    uint2 *pack = nullptr;
    unsigned char *alpha = nullptr, *label = nullptr, *cover = nullptr, *mpyr = nullptr, *img = nullptr, *out = nullptr;
    unsigned short *mask = nullptr, *wsum = nullptr;
    short *G = nullptr, *B = nullptr;
    unsigned long long *acc = nullptr;
    hipEvent_t ev[2] = { nullptr, nullptr };
    ~tscm_panorama() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
};

namespace {

int check_frame(const tscm_panorama *p, const unsigned char *const *images, int stride, const unsigned short *gain_q8, Gains *gains)
{
    if (!p) return tscm_set_error(TSCM_E_INVALID, "p is NULL");
    if (!images) return tscm_set_error(TSCM_E_INVALID, "images is NULL");
    for (int k = 0; k < p->n; ++k)
        if (!images[k]) return tscm_set_error(TSCM_E_INVALID, "images[" + std::to_string(k) + "] is NULL");
    if (stride < p->w * p->ch) return tscm_set_error(TSCM_E_INVALID, "stride " + std::to_string(stride) + " < width * channels = " + std::to_string(p->w * p->ch));
    for (int k = 0; k < kMaxCameras; ++k) gains->g[k] = 256;
    for (int k = 0; gain_q8 && k < p->n; ++k) {
        if (gain_q8[k] < 1 || gain_q8[k] > 4095) return tscm_set_error(TSCM_E_INVALID, "gain_q8[" + std::to_string(k) + "] = " + std::to_string(gain_q8[k]) + " outside 1..4095");
        gains->g[k] = gain_q8[k];
    }
    return 0;
}

int upload_frame(tscm_panorama *p, const unsigned char *const *images, int stride)
{
    HIP_TRY(hipSetDevice(p->device));
    const size_t row = (size_t)p->w * p->ch;
    for (int k = 0; k < p->n; ++k) HIP_TRY(hipMemcpy2D(p->img + (size_t)k * row * p->h, row, images[k], (size_t)stride, row, (size_t)p->h, hipMemcpyHostToDevice));
    return 0;
}

unsigned quad_blocks(size_t npix) { return (unsigned)((npix + 1023) / 1024); }

template <int CH>
void launch_sample(const tscm_panorama *p, const Gains &g, short *G, size_t stride)
{
    hipLaunchKernelGGL(k_pano_sample<CH>, dim3(quad_blocks(p->npix), (unsigned)p->n), dim3(256), 0, 0, p->pack, p->img, p->w, p->h, p->npix, p->plane, g, G, stride);
}

dim3 tile_grid(int W, int H) { return dim3((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH)); }

// MULTIBAND up to B^l (collapse == false) or to the output bytes
template <int CH>
void launch_multiband(const tscm_panorama *p, const Gains &g, short *lap, bool collapse)
{
    const int L = p->levels;
    launch_sample<CH>(p, g, p->G, p->Sp);
    for (int l = 0; l < L; ++l)
        hipLaunchKernelGGL(k_pano_reduce<short>, dim3((unsigned)((p->lw[l + 1] + kRedW - 1) / kRedW), (unsigned)((p->lh[l + 1] + kRedH - 1) / kRedH), (unsigned)(p->n * CH)),
                           dim3(256), 0, 0, p->G, p->lw[l], p->lh[l], p->Sp, p->loff[l], p->loff[l + 1], p->wrap);
    for (int l = 0; l <= L; ++l)
        hipLaunchKernelGGL(k_pano_lapblend<CH>, tile_grid(p->lw[l], p->lh[l]), dim3(256), 0, 0, p->G, p->mpyr, p->wsum, p->n, p->lw[l], p->lh[l], p->loff[l],
                           l < L ? p->loff[l + 1] : (size_t)0, p->Sp, l == L ? 1 : 0, p->wrap, p->B, lap);
    if (!collapse) return;
    for (int l = L - 1; l >= 1; --l)
        hipLaunchKernelGGL((k_pano_collapse<CH, 0>), tile_grid(p->lw[l], p->lh[l]), dim3(256), 0, 0, p->B, p->lw[l], p->lh[l], p->loff[l], p->loff[l + 1], p->Sp, p->wrap,
                           p->cover, p->out);
    hipLaunchKernelGGL((k_pano_collapse<CH, 1>), tile_grid(p->pw, p->ph), dim3(256), 0, 0, p->B, p->pw, p->ph, (size_t)0, p->loff[1], p->Sp, p->wrap, p->cover, p->out);
}

template <int CH>
void launch_compose(const tscm_panorama *p, const Gains &g)
{
    if (p->mode == TSCM_PANO_MULTIBAND) { launch_multiband<CH>(p, g, nullptr, true); return; }
    if (p->mode == TSCM_PANO_SEAM)
        hipLaunchKernelGGL((k_pano_compose<CH, TSCM_PANO_SEAM>), dim3(quad_blocks(p->npix)), dim3(256), 0, 0, p->pack, p->label, p->mask, p->img, p->n, p->w, p->h, p->npix,
                           p->plane, g, p->out);
    else
        hipLaunchKernelGGL((k_pano_compose<CH, TSCM_PANO_FEATHER>), dim3(quad_blocks(p->npix)), dim3(256), 0, 0, p->pack, p->label, p->mask, p->img, p->n, p->w, p->h,
                           p->npix, p->plane, g, p->out);
}

// `planes` device planes of Sp elements -> planes of S elements, the levels one after the other without padding
template <typename T>
int download_pyramid(const tscm_panorama *p, const T *dev, int planes, T *host)
{
    std::vector<T> tmp((size_t)planes * p->Sp);
    HIP_TRY(hipMemcpy(tmp.data(), dev, tmp.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (int q = 0; q < planes; ++q)
        for (int l = 0; l <= p->levels; ++l)
            std::copy_n(tmp.data() + (size_t)q * p->Sp + p->loff[l], (size_t)p->lw[l] * p->lh[l], host + (size_t)q * p->S + p->toff[l]);
    return 0;
}

int create_on_device(tscm_panorama *p, const unsigned char *const *weights, const float *mapx, const float *mapy)
{
    const int n = p->n;
    const size_t simg = (size_t)p->w * p->h;
    HIP_TRY(hipEventCreate(&p->ev[0])); HIP_TRY(hipEventCreate(&p->ev[1]));
    HIP_TRY(p->mem.alloc(&p->pack, n * p->plane)); HIP_TRY(hipMemset(p->pack, 0, n * p->plane * sizeof(uint2)));
    HIP_TRY(p->mem.alloc(&p->alpha, n * p->plane)); HIP_TRY(hipMemset(p->alpha, 0, n * p->plane));
    HIP_TRY(p->mem.alloc(&p->label, p->plane)); HIP_TRY(hipMemset(p->label, 0xff, p->plane));
    HIP_TRY(p->mem.alloc(&p->cover, p->plane)); HIP_TRY(hipMemset(p->cover, 0, p->plane));
    HIP_TRY(p->mem.alloc(&p->mask, p->plane)); HIP_TRY(hipMemset(p->mask, 0, p->plane * sizeof(unsigned short)));
    HIP_TRY(p->mem.alloc(&p->img, n * simg * p->ch));
    HIP_TRY(p->mem.alloc(&p->out, p->plane * p->ch));
    HIP_TRY(p->mem.alloc(&p->acc, 512));
    if (p->mode == TSCM_PANO_MULTIBAND) {
        HIP_TRY(p->mem.alloc(&p->mpyr, n * p->Sp)); HIP_TRY(hipMemset(p->mpyr, 0, n * p->Sp));
        HIP_TRY(p->mem.alloc(&p->wsum, p->Sp));
        HIP_TRY(p->mem.alloc(&p->G, (size_t)n * p->ch * p->Sp)); HIP_TRY(hipMemset(p->G, 0, (size_t)n * p->ch * p->Sp * sizeof(short)));
        HIP_TRY(p->mem.alloc(&p->B, (size_t)p->ch * p->Sp)); HIP_TRY(hipMemset(p->B, 0, (size_t)p->ch * p->Sp * sizeof(short)));
    }
    // the tables and the weight images are needed only here
    float *d_mx = nullptr, *d_my = nullptr;
    unsigned char *d_w = nullptr;
    unsigned weight_mask = 0;
    HIP_TRY(p->mem.upload(&d_mx, mapx, n * p->npix)); HIP_TRY(p->mem.upload(&d_my, mapy, n * p->npix));
    HIP_TRY(p->mem.alloc(&d_w, n * simg));
    for (int k = 0; weights && k < n; ++k)
        if (weights[k]) {
            weight_mask |= 1u << k;
            HIP_TRY(hipMemcpy(d_w + k * simg, weights[k], simg, hipMemcpyHostToDevice));
        }
    const unsigned blocks = (unsigned)((p->npix + 255) / 256);
    hipLaunchKernelGGL(k_pano_prepare, dim3(blocks, (unsigned)n), dim3(256), 0, 0, d_mx, d_my, d_w, weight_mask, p->w, p->h, p->npix, p->plane, p->pack, p->alpha);
    hipLaunchKernelGGL(k_pano_label, dim3(blocks), dim3(256), 0, 0, p->alpha, n, p->npix, p->plane, p->label, p->cover, p->mask, p->mpyr, p->Sp);
    if (p->mode == TSCM_PANO_MULTIBAND) {
        for (int l = 0; l < p->levels; ++l)
            hipLaunchKernelGGL(k_pano_reduce<unsigned char>, dim3((unsigned)((p->lw[l + 1] + kRedW - 1) / kRedW), (unsigned)((p->lh[l + 1] + kRedH - 1) / kRedH), (unsigned)n),
                               dim3(256), 0, 0, p->mpyr, p->lw[l], p->lh[l], p->Sp, p->loff[l], p->loff[l + 1], p->wrap);
        hipLaunchKernelGGL(k_pano_wsum, dim3((unsigned)((p->Sp + 255) / 256)), dim3(256), 0, 0, p->mpyr, n, p->Sp, p->wsum);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    p->mem.release(d_mx); p->mem.release(d_my); p->mem.release(d_w);
    return 0;
}

}  // namespace

extern "C" void tscm_panorama_default_params(tscm_panorama_params *p)
{
    if (!p) return;
    p->struct_size = (int)sizeof(tscm_panorama_params);
    p->mode = TSCM_PANO_MULTIBAND; p->levels = 4; p->wrap_x = 1;
}

extern "C" int tscm_panorama_create(int n_cameras, int width, int height, int channels, const unsigned char *const *weights, const float *mapx, const float *mapy,
                                    int pano_w, int pano_h, const tscm_panorama_params *params, int device_index, tscm_panorama **out)
{
    if (!out) return tscm_set_error(TSCM_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!mapx) return tscm_set_error(TSCM_E_INVALID, "mapx is NULL");
    if (!mapy) return tscm_set_error(TSCM_E_INVALID, "mapy is NULL");
    if (!params) return tscm_set_error(TSCM_E_INVALID, "params is NULL");
    if (params->struct_size != (int)sizeof(tscm_panorama_params))
        return tscm_set_error(TSCM_E_INVALID, "params: struct_size " + std::to_string(params->struct_size) + " is not sizeof(tscm_panorama_params) = " + std::to_string(sizeof(tscm_panorama_params)));
    if (n_cameras < 1 || n_cameras > kMaxCameras) return tscm_set_error(TSCM_E_INVALID, "n_cameras " + std::to_string(n_cameras) + " outside 1..16");
    if (channels != 1 && channels != 3) return tscm_set_error(TSCM_E_INVALID, "channels " + std::to_string(channels) + " is not 1 or 3");
    if (width < 1 || height < 1 || width > 32767 || height > 32767)
        return tscm_set_error(TSCM_E_INVALID, "width " + std::to_string(width) + ", height " + std::to_string(height) + ": a source image has 1..32767 pixels per side");
    if (params->mode != TSCM_PANO_SEAM && params->mode != TSCM_PANO_FEATHER && params->mode != TSCM_PANO_MULTIBAND)
        return tscm_set_error(TSCM_E_INVALID, "params: unknown mode " + std::to_string(params->mode));
    const bool multiband = params->mode == TSCM_PANO_MULTIBAND;
    if (multiband && (params->levels < 1 || params->levels > kMaxLevels)) return tscm_set_error(TSCM_E_INVALID, "params: levels " + std::to_string(params->levels) + " outside 1..6");
    if (pano_w < 1 || pano_h < 1) return tscm_set_error(TSCM_E_INVALID, "pano_w " + std::to_string(pano_w) + ", pano_h " + std::to_string(pano_h) + ": below 1");
    const int L = multiband ? params->levels : 0;
    if (pano_w % (1 << L)) return tscm_set_error(TSCM_E_INVALID, "pano_w " + std::to_string(pano_w) + " is no multiple of 2^levels = " + std::to_string(1 << L));
    if (pano_h % (1 << L)) return tscm_set_error(TSCM_E_INVALID, "pano_h " + std::to_string(pano_h) + " is no multiple of 2^levels = " + std::to_string(1 << L));
    if (int rc = select_device(device_index, "tscm_panorama_create")) return rc;
    std::unique_ptr<tscm_panorama> p(new tscm_panorama);
    p->n = n_cameras; p->w = width; p->h = height; p->ch = channels; p->pw = pano_w; p->ph = pano_h;
    p->mode = params->mode; p->levels = L; p->wrap = params->wrap_x ? 1 : 0; p->device = device_index;
    p->npix = (size_t)pano_w * pano_h;
    p->plane = (p->npix + 3) & ~(size_t)3;
    for (int l = 0; l <= L; ++l) {
        p->lw[l] = pano_w >> l; p->lh[l] = pano_h >> l;
        p->loff[l] = p->Sp; p->toff[l] = p->S;
        p->S += (size_t)p->lw[l] * p->lh[l];
        p->Sp = (p->Sp + (size_t)p->lw[l] * p->lh[l] + 7) & ~(size_t)7;
    }
    if (int rc = create_on_device(p.get(), weights, mapx, mapy)) return rc;
    *out = p.release();
    return 0;
}

extern "C" int tscm_panorama_compose(tscm_panorama *p, const unsigned char *const *images, int stride, const unsigned short *gain_q8, unsigned char *dst,
                                     int dst_stride, unsigned char *coverage, double *seconds_kernel)
{
    Gains g;
    if (int rc = check_frame(p, images, stride, gain_q8, &g)) return rc;
    if (!dst) return tscm_set_error(TSCM_E_INVALID, "dst is NULL");
    if (dst_stride < p->pw * p->ch) return tscm_set_error(TSCM_E_INVALID, "dst_stride " + std::to_string(dst_stride) + " < pano_w * channels = " + std::to_string(p->pw * p->ch));
    if (seconds_kernel) *seconds_kernel = 0.0;
    if (int rc = upload_frame(p, images, stride)) return rc;
    HIP_TRY(hipEventRecord(p->ev[0], 0));
    if (p->ch == 1) launch_compose<1>(p, g);
    else launch_compose<3>(p, g);
    HIP_TRY(hipEventRecord(p->ev[1], 0));
    HIP_TRY(hipEventSynchronize(p->ev[1]));
    HIP_TRY(hipGetLastError());
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev[0], p->ev[1]));
    if (seconds_kernel) *seconds_kernel = 1e-3 * ms;
    const size_t row = (size_t)p->pw * p->ch;
    HIP_TRY(hipMemcpy2D(dst, (size_t)dst_stride, p->out, row, row, (size_t)p->ph, hipMemcpyDeviceToHost));
    if (coverage) HIP_TRY(hipMemcpy(coverage, p->cover, p->npix, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tscm_panorama_stages(tscm_panorama *p, const unsigned char *const *images, int stride, const unsigned short *gain_q8, unsigned char *sampled,
                                    unsigned char *alpha, unsigned char *label, unsigned char *mask_pyramid, short *lap_pyramid, short *blend_pyramid)
{
    Gains g;
    if (int rc = check_frame(p, images, stride, gain_q8, &g)) return rc;
    const bool multiband = p->mode == TSCM_PANO_MULTIBAND;
    if (!multiband && (mask_pyramid || lap_pyramid || blend_pyramid))
        return tscm_set_error(TSCM_E_INVALID, std::string(mask_pyramid ? "mask_pyramid" : lap_pyramid ? "lap_pyramid" : "blend_pyramid") + ": the mode is not MULTIBAND");
    if (int rc = upload_frame(p, images, stride)) return rc;
    const int n = p->n, ch = p->ch;
    DeviceMem tmp;
    short *d_lap = nullptr, *d_G = p->G;
    size_t gstride = p->Sp;
    if (multiband) {
        if (lap_pyramid) HIP_TRY(tmp.alloc(&d_lap, (size_t)n * ch * p->Sp));
        if (ch == 1) launch_multiband<1>(p, g, d_lap, false);
        else launch_multiband<3>(p, g, d_lap, false);
    } else if (sampled) {
        gstride = p->plane;
        HIP_TRY(tmp.alloc(&d_G, (size_t)n * ch * gstride));
        if (ch == 1) launch_sample<1>(p, g, d_G, gstride);
        else launch_sample<3>(p, g, d_G, gstride);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (sampled) {                                            // planes -> interleaved bytes
        std::vector<short> planes((size_t)n * ch * gstride);
        HIP_TRY(hipMemcpy(planes.data(), d_G, planes.size() * sizeof(short), hipMemcpyDeviceToHost));
        for (int k = 0; k < n; ++k)
            for (int c = 0; c < ch; ++c)
                for (size_t t = 0; t < p->npix; ++t) sampled[((size_t)k * p->npix + t) * ch + c] = (unsigned char)planes[(size_t)(k * ch + c) * gstride + t];
    }
    if (alpha) HIP_TRY(hipMemcpy2D(alpha, p->npix, p->alpha, p->plane, p->npix, (size_t)n, hipMemcpyDeviceToHost));
    if (label) HIP_TRY(hipMemcpy(label, p->label, p->npix, hipMemcpyDeviceToHost));
    if (mask_pyramid) if (int rc = download_pyramid(p, p->mpyr, n, mask_pyramid)) return rc;
    if (lap_pyramid) if (int rc = download_pyramid(p, d_lap, n * ch, lap_pyramid)) return rc;
    if (blend_pyramid) if (int rc = download_pyramid(p, p->B, ch, blend_pyramid)) return rc;
    return 0;
}

extern "C" int tscm_panorama_overlap(tscm_panorama *p, const unsigned char *const *images, int stride, long long *count, long long *sum)
{
    Gains g;
    if (int rc = check_frame(p, images, stride, nullptr, &g)) return rc;
    if (!count) return tscm_set_error(TSCM_E_INVALID, "count is NULL");
    if (!sum) return tscm_set_error(TSCM_E_INVALID, "sum is NULL");
    if (int rc = upload_frame(p, images, stride)) return rc;
    HIP_TRY(hipMemset(p->acc, 0, 512 * sizeof(unsigned long long)));
    if (p->ch == 1) hipLaunchKernelGGL(k_pano_overlap<1>, dim3(quad_blocks(p->npix)), dim3(256), 0, 0, p->pack, p->mask, p->img, p->w, p->h, p->npix, p->plane, p->acc);
    else hipLaunchKernelGGL(k_pano_overlap<3>, dim3(quad_blocks(p->npix)), dim3(256), 0, 0, p->pack, p->mask, p->img, p->w, p->h, p->npix, p->plane, p->acc);
    HIP_TRY(hipGetLastError());
    unsigned long long host[512];
    HIP_TRY(hipMemcpy(host, p->acc, sizeof(host), hipMemcpyDeviceToHost));
    for (int a = 0; a < p->n; ++a)
        for (int b = 0; b < p->n; ++b) {
            count[a * p->n + b] = (long long)host[a * 16 + b];
            sum[a * p->n + b] = (long long)host[256 + a * 16 + b];
        }
    return 0;
}

extern "C" void tscm_panorama_destroy(tscm_panorama *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}
