// tscm_stereo_kernels.h -- the kernels behind a cost volume C [h][w][D] (uint8, entries <= 64) that the stereo matcher
// (tscm_stereo.hip) and the sphere sweep (tscm_sweep.hip) share: the path aggregation k_aggregate and the winner with its
// uniqueness rule and parabola term.  Device code only.  Everything sits in an anonymous namespace, so each translation
// unit that includes the header compiles and registers kernels of its own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace {

constexpr int kInf = 0x3fff;          // above every path cost (<= 64 + 255), small enough that + p1 / + p2 stay far from overflow
constexpr int kPrefetch = 4;          // steps of a scanline whose loads are in flight ahead of the chain


// ------------------------------------------------------------------------------------------------ cross-lane helpers
// lane i <- lane i - 1 (lane 0 keeps `edge`) and lane i <- lane i + 1 (lane 63 keeps `edge`)
__device__ __forceinline__ int lane_from_below(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }
__device__ __forceinline__ int lane_from_above(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false); }

// minimum over the 64 lanes, wave-uniform result: row_shr 1, 2, 4, 8 leave each row's minimum in its lane 15,
// row_bcast15 / row_bcast31 carry it to lane 63
__device__ __forceinline__ int wave_min(int v)
{
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));
    return __builtin_amdgcn_readlane(v, 63);
}

// ------------------------------------------------------------------------------------------------ aggregation
// Lane l holds disparities k = l * NPL + j, j < NPL (k >= D: idle, held at kInf so that minima pass over it).
template <int NPL>
__device__ __forceinline__ void load_cost(const unsigned char *p, int k0, int D, int (&c)[NPL])
{
    if (NPL == 2) {
        if (k0 < D) { const unsigned v = *reinterpret_cast<const unsigned short *>(p); c[0] = v & 0xff; c[1] = v >> 8; }
    } else if (NPL == 4) {
        if (k0 < D) { const unsigned v = *reinterpret_cast<const unsigned *>(p); c[0] = v & 0xff; c[1] = (v >> 8) & 0xff; c[2] = (v >> 16) & 0xff; c[3] = v >> 24; }
    } else {
#pragma unroll
        for (int j = 0; j < NPL; ++j)
            if (k0 + j < D) c[j] = p[j];
    }
}

template <int NPL>
__device__ __forceinline__ void load_sum(const unsigned short *p, int k0, int D, int (&s)[NPL])
{
    if (NPL == 2) {
        if (k0 < D) { const unsigned v = *reinterpret_cast<const unsigned *>(p); s[0] = v & 0xffff; s[1] = v >> 16; }
    } else if (NPL == 4) {
        if (k0 < D) { const uint2 v = *reinterpret_cast<const uint2 *>(p); s[0] = v.x & 0xffff; s[1] = v.x >> 16; s[2] = v.y & 0xffff; s[3] = v.y >> 16; }
    } else {
#pragma unroll
        for (int j = 0; j < NPL; ++j)
            if (k0 + j < D) s[j] = p[j];
    }
}

template <int NPL>
__device__ __forceinline__ void store_sum(unsigned short *p, int k0, int D, const int (&s)[NPL])
{
    if (NPL == 2) {
        if (k0 < D) *reinterpret_cast<unsigned *>(p) = (unsigned)s[0] | ((unsigned)s[1] << 16);
    } else if (NPL == 4) {
        if (k0 < D) *reinterpret_cast<uint2 *>(p) = make_uint2((unsigned)s[0] | ((unsigned)s[1] << 16), (unsigned)s[2] | ((unsigned)s[3] << 16));
    } else {
#pragma unroll
        for (int j = 0; j < NPL; ++j)
            if (k0 + j < D) p[j] = (unsigned short)s[j];
    }
}

// One wave per scanline of direction (DX, DY), 4 scanlines per block.
//   DY == 0: line = row, step i visits x = i (DX = 1) or w - 1 - i; the path starts at i == 0.
//   DY != 0: line = start column c, step i visits row i (DY = 1) or h - 1 - i and column (c + DX * i) mod w; a diagonal
//            that runs over the image edge starts a new path there, which is where its predecessor p - r leaves the image.
// accumulate == 0: S = L (the first direction), otherwise S += L.
template <int NPL, int DX, int DY>
__global__ __launch_bounds__(256) void k_aggregate(const unsigned char *__restrict__ cost, unsigned short *__restrict__ sum, int w, int h, int D, int p1, int p2,
                                                   int accumulate)
{
    const int lane = threadIdx.x & 63;
    const int line = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_lines = DY == 0 ? h : w, n_steps = DY == 0 ? w : h;
    if (line >= n_lines) return;                             // whole waves
    const int k0 = lane * NPL;
    int prev[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) prev[j] = kInf;
    int m = 0;
    int x = DY == 0 ? (DX > 0 ? 0 : w - 1) : line;
    int y = DY == 0 ? line : (DY > 0 ? 0 : h - 1);
    for (int i0 = 0; i0 < n_steps; i0 += kPrefetch) {
        int c[kPrefetch][NPL], s[kPrefetch][NPL];
        size_t at[kPrefetch];
        bool first[kPrefetch];
#pragma unroll
        for (int u = 0; u < kPrefetch; ++u) {
#pragma unroll
            for (int j = 0; j < NPL; ++j) { c[u][j] = 0; s[u][j] = 0; }
            at[u] = 0; first[u] = false;
            if (i0 + u < n_steps) {                          // wave-uniform
                at[u] = ((size_t)y * w + x) * D + k0;
                first[u] = i0 + u == 0 || (DY != 0 && DX > 0 && x == 0) || (DY != 0 && DX < 0 && x == w - 1);
                load_cost<NPL>(cost + at[u], k0, D, c[u]);
                if (accumulate) load_sum<NPL>(sum + at[u], k0, D, s[u]);
                x += DX; y += DY;
                if (DY != 0 && x == w) x = 0;
                if (DY != 0 && x < 0) x = w - 1;
            }
        }
#pragma unroll
        for (int u = 0; u < kPrefetch; ++u) {
            if (i0 + u >= n_steps) break;
            const int below = lane_from_below(prev[NPL - 1], kInf), above = lane_from_above(prev[0], kInf);
            int cur[NPL], lowest = kInf;
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
                const int a = j > 0 ? prev[j - 1] : below, b = j < NPL - 1 ? prev[j + 1] : above;
                const int best = min(min(prev[j], min(a, b) + p1), m + p2);
                int v = first[u] ? c[u][j] : c[u][j] + best - m;
                v = k0 + j < D ? v : kInf;
                cur[j] = v;
                lowest = min(lowest, v);
                s[u][j] += v;
            }
#pragma unroll
            for (int j = 0; j < NPL; ++j) prev[j] = cur[j];
            m = wave_min(lowest);
            store_sum<NPL>(sum + at[u], k0, D, s[u]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ winner
// The output value of one pixel, computed by one wave: k*, uniqueness, left-right check (disp12 >= 0, with kr), sub-pixel.
// cost != NULL (the sphere sweep): C of the same pixel, and the pixel is invalid when C(k*) == 64; the matcher passes a
// literal NULL and the rule drops out of its kernels.
template <int NPL>
__device__ __forceinline__ int winner_value(const unsigned short *__restrict__ S, const short *__restrict__ kr, const unsigned char *__restrict__ cost, int lane, int w,
                                            int x, int y, int D, int dmin, int uniqueness, int disp12)
{
    const int k0 = lane * NPL;
    int s[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) s[j] = 0;
    load_sum<NPL>(S + k0, k0, D, s);
    int key = 0x7fffffff;                                    // S < 2^15 (8 paths of at most 64 + 255), so (S << 16 | k) is a positive int
#pragma unroll
    for (int j = 0; j < NPL; ++j)
        if (k0 + j < D) key = min(key, (s[j] << 16) | (k0 + j));
    key = wave_min(key);
    const int ks = key & 0xffff, smin = key >> 16;
    bool ok = true;
    if (uniqueness > 0) {
        int other = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int k = k0 + j;
            if (k < D && (k < ks - 1 || k > ks + 1)) other = min(other, s[j]);
        }
        other = wave_min(other);
        if (other != 0x7fffffff && other * (100 - uniqueness) < smin * 100) ok = false;
    }
    const int d = dmin + ks;
    if (disp12 >= 0) {
        const int x2 = x - d;
        if (x2 < 0 || x2 >= w) ok = false;
        else {
            const int other = kr[(size_t)y * w + x2];
            if (abs(other - ks) > disp12) ok = false;
        }
    }
    if (cost && cost[ks] == 64) ok = false;
    int out = 16 * (dmin - 1);
    if (ok) {
        out = 16 * d;
        if (ks > 0 && ks < D - 1) {
            const int sm = S[ks - 1], sp = S[ks + 1];
            const int den = max(sm + sp - 2 * smin, 1), num = (sm - sp) * 16 + den;
            int q = num / (2 * den);
            if (num < 0 && q * 2 * den != num) --q;          // floor division
            out += q;
        }
    }
    return out;
}

// one wave per pixel, 4 pixels per block
template <int NPL>
__global__ __launch_bounds__(256) void k_winner(const unsigned short *__restrict__ sum, const short *__restrict__ kr, int w, int h, int D, int dmin, int uniqueness,
                                                int disp12, short *__restrict__ disp)
{
    const size_t pix = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= (size_t)w * h) return;                        // whole waves
    const int lane = threadIdx.x & 63;
    const int y = (int)(pix / (size_t)w), x = (int)(pix - (size_t)y * w);
    const int out = winner_value<NPL>(sum + pix * D, kr, nullptr, lane, w, x, y, D, dmin, uniqueness, disp12);
    if (lane == 0) disp[pix] = (short)out;
}

// ------------------------------------------------------------------------------------------------ host
// f(std::integral_constant<int, NPL>()) for the NPL = 1..4 planes of 64 hypotheses that hold D of them: the one place that
// picks among the <1> .. <4> instantiations of k_aggregate and the winner kernels
template <typename F>
inline auto with_planes(int D, F &&f)
{
    const int npl = (D + 63) / 64;
    if (npl == 1) return f(std::integral_constant<int, 1>());
    if (npl == 2) return f(std::integral_constant<int, 2>());
    if (npl == 3) return f(std::integral_constant<int, 3>());
    return f(std::integral_constant<int, 4>());
}

using AggregateKernel = void (*)(const unsigned char *, unsigned short *, int, int, int, int, int, int);

template <int NPL>
AggregateKernel aggregate_kernel(int dir)
{
    switch (dir) {                                           // tscm.h: the order of the directions
    case 0: return k_aggregate<NPL, 1, 0>;
    case 1: return k_aggregate<NPL, -1, 0>;
    case 2: return k_aggregate<NPL, 0, 1>;
    case 3: return k_aggregate<NPL, 0, -1>;
    case 4: return k_aggregate<NPL, 1, 1>;
    case 5: return k_aggregate<NPL, -1, -1>;
    case 6: return k_aggregate<NPL, 1, -1>;
    default: return k_aggregate<NPL, -1, 1>;
    }
}

// the `paths` launches of one volume on the current stream: S = sum of L_r over the directions
inline void launch_aggregate(const unsigned char *cost, unsigned short *sum, int w, int h, int D, int p1, int p2, int paths)
{
    for (int dir = 0; dir < paths; ++dir) {
        const AggregateKernel f = with_planes(D, [dir](auto npl) { return aggregate_kernel<decltype(npl)::value>(dir); });
        const int n_lines = dir < 2 ? h : w;
        hipLaunchKernelGGL(f, dim3((n_lines + 3) / 4), dim3(256), 0, 0, cost, sum, w, h, D, p1, p2, dir > 0 ? 1 : 0);
    }
}

}  // namespace
