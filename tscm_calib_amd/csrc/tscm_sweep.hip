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
// The frame composed at the swept depth (tscm_sweep_compose): the panorama's blends on the record (k, z(i, j)) of every pixel,
// z the hypothesis the index map names.  Labels, coverage and mask pyramids depend on the index map, so they are per frame:
//   k_sweep_compose  SEAM / FEATHER in one launch: a thread owns 4 adjacent output pixels, forms their z, reads the n records
//                    at (k, z) with 8-byte loads (the 4 pixels lie in different hypothesis planes), and stores 4 or 12 packed
//                    output bytes and 4 coverage bytes; no per-camera plane is written.  SEAM keeps the record of the largest
//                    alpha and samples once per pixel; FEATHER skips the gathers of a camera that no lane of the wave sees
//                    (ballot)
//   k_sweep_gather   MULTIBAND: G^0 of every camera and channel as int16 planes, label, coverage and level 0 of the masks
//   then k_pano_reduce on the images and the masks, k_pano_wsum, k_pano_lapblend, k_pano_collapse (tscm_pano_kernels.h)
// Per-camera visibility at the swept depth (tscm_sweep_visibility, tscm_sweep_compose_visible): a depth buffer of every camera
// over cells of its image, in ranks of the hypothesis, and the test of every (pixel, camera) against it:
//   hipMemsetAsync   zbuf [n][ch][cw] uint32 = 0
//   k_sweep_splat    the composer's quads; every tested pixel raises the cell of its record in every camera that sees it to
//                    rank + 1 with a no-return atomic max (order-independent)
//   k_sweep_vis_test the composer's quads; per pixel the n-bit masks seen / visible, then state and use: 4 use bytes per quad
//                    and camera and 4 state bytes per quad in one 32-bit store each
//   k_sweep_compose / k_sweep_gather with VIS = true read the 4 use bytes of a quad and camera and zero the alpha
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_host.h"
#include "tscm_pano_kernels.h"
#include "tscm_remap_sample.h"
#include "tscm_stereo_kernels.h"

#include <cmath>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

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
    pack[at] = pack_record(mapx[at], mapy[at], wimg + (size_t)k * w * h, (weight_mask >> k) & 1u, w, h);
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

// ------------------------------------------------------------------------------------------------ compose
// z of the quad at t0 (tscm.h: hypothesis index) and where the record of pixel t0 + e lies inside a camera's D planes;
// elements at and beyond nv are not read
__device__ __forceinline__ void quad_records(const short *__restrict__ index16, size_t t0, int nv, int D, int fallback, size_t npix, int (&z)[4], size_t (&at)[4])
{
    int raw[4] = { -1, -1, -1, -1 };
    if (nv == 4) {
        const uint2 q = *reinterpret_cast<const uint2 *>(index16 + t0);
        raw[0] = (short)(q.x & 0xffffu); raw[1] = (int)q.x >> 16; raw[2] = (short)(q.y & 0xffffu); raw[3] = (int)q.y >> 16;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < nv) raw[e] = index16[t0 + e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        z[e] = raw[e] < 0 ? fallback : min(D - 1, (raw[e] + 8) >> 4);
        at[e] = (size_t)z[e] * npix + t0 + e;
    }
}

// the 4 use bytes of a quad and camera; planes of `use` are padded to whole quads
__device__ __forceinline__ unsigned quad_use(const unsigned char *__restrict__ use, size_t first) { return *reinterpret_cast<const unsigned *>(use + first); }

// grid ceil(npix / 1024) x 256: quad q = output pixels [4q, 4q + 4) of the flat panorama
// VIS: use [n][plane] (tscm.h, visibility: state and use) zeroes the alpha of the cameras a pixel does not use
template <int CH, int MODE, bool VIS>
__global__ __launch_bounds__(256) void k_sweep_compose(const uint2 *__restrict__ pack, const short *__restrict__ index16, const unsigned char *__restrict__ img, int n,
                                                       int w, int h, int D, int fallback, size_t npix, Gains gains, unsigned char *__restrict__ out,
                                                       unsigned char *__restrict__ cover, const unsigned char *__restrict__ use, size_t plane)
{
    const size_t t0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (t0 >= npix) return;
    const int nv = (int)min((size_t)4, npix - t0);
    const size_t img_bytes = (size_t)w * h * CH, cam = (size_t)D * npix;
    int z[4];
    size_t at[4];
    quad_records(index16, t0, nv, D, fallback, npix, z, at);
    int v[4][CH], cnt[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        cnt[e] = 0;
#pragma unroll
        for (int c = 0; c < CH; ++c) v[e][c] = 0;
    }
    if (MODE == TSCM_PANO_SEAM) {
        // the record, camera and gain of the largest alpha so far: the first of equal maxima stays
        uint2 rec[4];
        int best[4] = { 0, 0, 0, 0 }, lab[4] = { 0, 0, 0, 0 }, g[4] = { 256, 256, 256, 256 };
#pragma unroll
        for (int e = 0; e < 4; ++e) rec[e] = make_uint2(0, 0);
        for (int k = 0; k < n; ++k) {
            const int gk = gains.g[k];
            const unsigned used = VIS ? quad_use(use, k * plane + t0) : 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= nv) continue;
                const uint2 r = pack[k * cam + at[e]];
                const int a = VIS && !((used >> (8 * e)) & 0xffu) ? 0 : (int)(r.y >> 16);
                if (a > 0) ++cnt[e];
                if (a > best[e]) { best[e] = a; rec[e] = r; lab[e] = k; g[e] = gk; }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (best[e] == 0) continue;
            int px[CH];
            sample_px<CH>(img + lab[e] * img_bytes, w, h, rec[e], px);
#pragma unroll
            for (int c = 0; c < CH; ++c) v[e][c] = apply_gain(px[c], g[e]);
        }
    } else {
        int num[4][CH], A[4] = { 0, 0, 0, 0 };
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < CH; ++c) num[e][c] = 0;
        for (int k = 0; k < n; ++k) {
            uint2 r[4];
            int any = 0;
            const unsigned used = VIS ? quad_use(use, k * plane + t0) : 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                r[e] = e < nv ? pack[k * cam + at[e]] : make_uint2(0, 0);
                if (VIS && !((used >> (8 * e)) & 0xffu)) r[e].y &= 0xffffu;
                any |= (int)(r[e].y >> 16);
            }
            if (__ballot(any != 0) == 0) continue;               // no lane of the wave sees camera k: its gathers are skipped
            const int g = gains.g[k];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int a = (int)(r[e].y >> 16);
                if (a == 0) continue;
                int px[CH];
                sample_px<CH>(img + k * img_bytes, w, h, r[e], px);
#pragma unroll
                for (int c = 0; c < CH; ++c) num[e][c] += a * apply_gain(px[c], g);
                A[e] += a;
                ++cnt[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < CH; ++c) v[e][c] = A[e] ? (int)(((unsigned)num[e][c] + ((unsigned)A[e] >> 1)) / (unsigned)A[e]) : 0;
    }
    store_quad<CH>(out, t0, nv, v);
    int cv[4][1] = { { cnt[0] }, { cnt[1] }, { cnt[2] }, { cnt[3] } };
    store_quad<1>(cover, t0, nv, cv);
}

// same grid and ownership.  G^0 of every camera at planes (k * CH + c) * Sp, label, cover and (mpyr != NULL) level 0 of the
// masks; hypothesis [npix], sampled [n][npix][CH], alpha [n][npix]: the stage outputs, any of them NULL.
template <int CH, bool VIS>
__global__ __launch_bounds__(256) void k_sweep_gather(const uint2 *__restrict__ pack, const short *__restrict__ index16, const unsigned char *__restrict__ img, int n,
                                                      int w, int h, int D, int fallback, size_t npix, Gains gains, short *__restrict__ G, size_t Sp,
                                                      unsigned char *__restrict__ label, unsigned char *__restrict__ cover, unsigned char *__restrict__ mpyr,
                                                      unsigned char *__restrict__ hypothesis, unsigned char *__restrict__ sampled, unsigned char *__restrict__ alpha,
                                                      const unsigned char *__restrict__ use, size_t plane)
{
    const size_t t0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (t0 >= npix) return;
    const int nv = (int)min((size_t)4, npix - t0);
    const size_t img_bytes = (size_t)w * h * CH, cam = (size_t)D * npix;
    int z[4];
    size_t at[4];
    quad_records(index16, t0, nv, D, fallback, npix, z, at);
    int best[4] = { 0, 0, 0, 0 }, lab[4][1] = { { 255 }, { 255 }, { 255 }, { 255 } }, cnt[4][1] = { { 0 }, { 0 }, { 0 }, { 0 } };
    for (int k = 0; k < n; ++k) {
        const int g = gains.g[k];
        const unsigned used = VIS ? quad_use(use, k * plane + t0) : 0u;
        int v[4][CH];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int c = 0; c < CH; ++c) v[e][c] = 0;
            if (e >= nv) continue;
            const uint2 r = pack[k * cam + at[e]];
            const int a = VIS && !((used >> (8 * e)) & 0xffu) ? 0 : (int)(r.y >> 16);
            sample_px<CH>(img + k * img_bytes, w, h, r, v[e]);
#pragma unroll
            for (int c = 0; c < CH; ++c) v[e][c] = apply_gain(v[e][c], g);
            if (a > 0) ++cnt[e][0];
            if (a > best[e]) { best[e] = a; lab[e][0] = k; }
            if (alpha) alpha[k * npix + t0 + e] = (unsigned char)a;
        }
        if (sampled) store_quad<CH>(sampled + k * npix * CH, t0, nv, v);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            short *q = G + (size_t)(k * CH + c) * Sp + t0;
            if (nv == 4) *reinterpret_cast<uint2 *>(q) = make_uint2((unsigned)v[0][c] | ((unsigned)v[1][c] << 16), (unsigned)v[2][c] | ((unsigned)v[3][c] << 16));
            else
                for (int e = 0; e < nv; ++e) q[e] = (short)v[e][c];
        }
    }
    store_quad<1>(label, t0, nv, lab);
    store_quad<1>(cover, t0, nv, cnt);
    if (mpyr)
        for (int k = 0; k < n; ++k) {
            const int m[4][1] = { { lab[0][0] == k ? 255 : 0 }, { lab[1][0] == k ? 255 : 0 }, { lab[2][0] == k ? 255 : 0 }, { lab[3][0] == k ? 255 : 0 } };
            store_quad<1>(mpyr + k * Sp, t0, nv, m);
        }
    if (hypothesis) {
        const int zz[4][1] = { { z[0] }, { z[1] }, { z[2] }, { z[3] } };
        store_quad<1>(hypothesis, t0, nv, zz);
    }
}

// ------------------------------------------------------------------------------------------------ visibility
// the depth-buffer cell of a record (tscm.h, visibility: cell): always inside the cw x ch grid
__device__ __forceinline__ void record_cell(const uint2 r, int w, int h, int shift, int &cx, int &cy)
{
    const int ix = (short)(r.x & 0xffffu), iy = (int)r.x >> 16;
    cx = min(max(ix, 0), w - 1) >> shift;
    cy = min(max(iy, 0), h - 1) >> shift;
}

// Same grid and ownership as k_sweep_compose.  zbuf [n][cells], cells = cw * ch, cleared before: the maximum of rank + 1 over
// the tested pixels that a camera sees in a cell.  An untested pixel has z = -1 here (the fallback of quad_records).
__global__ __launch_bounds__(256) void k_sweep_splat(const uint2 *__restrict__ pack, const short *__restrict__ index16, int n, int w, int h, int D, size_t npix, int shift,
                                                     int cw, size_t cells, int near_is_high, unsigned *__restrict__ zbuf)
{
    const size_t t0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (t0 >= npix) return;
    const int nv = (int)min((size_t)4, npix - t0);
    const size_t cam = (size_t)D * npix;
    int z[4];
    size_t at[4];
    quad_records(index16, t0, nv, D, -1, npix, z, at);
#pragma unroll 1
    for (int k = 0; k < n; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (z[e] < 0) continue;
            const uint2 r = pack[k * cam + at[e]];
            if ((r.y >> 16) == 0) continue;
            int cx, cy;
            record_cell(r, w, h, shift, cx, cy);
            const unsigned rank1 = (unsigned)(near_is_high ? z[e] : D - 1 - z[e]) + 1u;
            // relaxed, agent scope, the result unused: one vector atomic without return
            (void)__hip_atomic_fetch_max(zbuf + k * cells + (size_t)cy * cw + cx, rank1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Same grid and ownership.  use [n][plane] and state [plane], plane = npix rounded up to 4 (the bytes behind npix are written
// too); hypothesis [npix], cell [n][npix], visible [n][npix]: the stage outputs, any of them NULL.
__global__ __launch_bounds__(256) void k_sweep_vis_test(const uint2 *__restrict__ pack, const short *__restrict__ index16, int n, int w, int h, int D, size_t npix,
                                                        size_t plane, int shift, int cw, int ch, int tolerance, int dilate, int near_is_high,
                                                        const unsigned *__restrict__ zbuf, unsigned char *__restrict__ use, unsigned char *__restrict__ state,
                                                        unsigned char *__restrict__ hypothesis, int *__restrict__ cell, unsigned char *__restrict__ visible)
{
    const size_t t0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (t0 >= npix) return;
    const int nv = (int)min((size_t)4, npix - t0);
    const size_t cam = (size_t)D * npix, cells = (size_t)cw * ch;
    int z[4];
    size_t at[4];
    quad_records(index16, t0, nv, D, -1, npix, z, at);
    unsigned seen[4] = { 0, 0, 0, 0 }, vis[4] = { 0, 0, 0, 0 };                 // bit k: a_k > 0, visible_k
#pragma unroll 1
    for (int k = 0; k < n; ++k) {
        const unsigned *zk = zbuf + k * cells;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int c = -1, ok = 0;
            if (z[e] >= 0) {
                const uint2 r = pack[k * cam + at[e]];
                if ((r.y >> 16) != 0) {
                    int cx, cy;
                    record_cell(r, w, h, shift, cx, cy);
                    c = cy * cw + cx;
                    unsigned m = 0;
                    for (int yy = max(cy - dilate, 0); yy <= min(cy + dilate, ch - 1); ++yy)
                        for (int xx = max(cx - dilate, 0); xx <= min(cx + dilate, cw - 1); ++xx) m = max(m, zk[(size_t)yy * cw + xx]);
                    const unsigned rank1 = (unsigned)(near_is_high ? z[e] : D - 1 - z[e]) + 1u;
                    ok = m <= rank1 + (unsigned)tolerance;
                    seen[e] |= 1u << k;
                    vis[e] |= (unsigned)ok << k;
                }
            }
            if (cell && e < nv) cell[k * npix + t0 + e] = c;
            if (visible && e < nv) visible[k * npix + t0 + e] = (unsigned char)ok;
        }
    }
    unsigned st = 0, used[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        // 0 untested, 1 nobody sees it, 2 all visible, 3 some occluded, 4 all occluded: the guard keeps every source
        const unsigned s = z[e] < 0 ? 0u : seen[e] == 0 ? 1u : vis[e] == seen[e] ? 2u : vis[e] == 0 ? 4u : 3u;
        used[e] = s == 0 ? 0xffu : s == 3 ? vis[e] : seen[e];
        st |= s << (8 * e);
    }
    *reinterpret_cast<unsigned *>(state + t0) = st;
    for (int k = 0; k < n; ++k)
        *reinterpret_cast<unsigned *>(use + k * plane + t0) = ((used[0] >> k) & 1u) | (((used[1] >> k) & 1u) << 8) | (((used[2] >> k) & 1u) << 16) | (((used[3] >> k) & 1u) << 24);
    if (hypothesis) {
        const int zz[4][1] = { { max(z[0], 0) }, { max(z[1], 0) }, { max(z[2], 0) }, { max(z[3], 0) } };
        store_quad<1>(hypothesis, t0, nv, zz);
    }
}

thread_local double g_stage_seconds[3];

}  // namespace

// ------------------------------------------------------------------------------------------------ host
struct tscm_sweep : PyramidLayout {         // the base: the levels of the composer's pyramids
    int n = 0, w = 0, h = 0, pw = 0, ph = 0, D = 0, p1 = 0, p2 = 0, paths = 0, uniqueness = 0, wrap = 0, device = 0;
    size_t npix = 0;
    DeviceMem mem;
    uint2 *pack = nullptr;
    unsigned char *img = nullptr, *cost = nullptr;
    unsigned short *sum = nullptr;
    short *index16 = nullptr;
    bool has_index = false;                 // index16 holds the map of a tscm_sweep_depth
    // the composer's buffers, allocated by the first tscm_sweep_compose for (c_ch, c_mode, levels)
    int c_ch = 0, c_mode = -1;
    size_t plane = 0;                       // npix rounded up to 4
    unsigned char *c_img = nullptr, *c_out = nullptr, *c_label = nullptr, *c_cover = nullptr, *c_mpyr = nullptr;
    unsigned short *c_wsum = nullptr;
    short *c_G = nullptr, *c_B = nullptr, *c_index = nullptr;
    // the buffers of the visibility pass, allocated by its first call: the depth buffers for cell_shift = 0 (the largest grid)
    unsigned *v_zbuf = nullptr;
    unsigned char *v_use = nullptr, *v_state = nullptr;
    short *v_index = nullptr;
    size_t v_plane = 0;                     // npix rounded up to 4
    EventSpan span;
};

namespace {

int check_params(const tscm_sweep_params *p)
{
    if (!p) return tscm_set_error(TSCM_E_INVALID, "params is NULL");
    if (int rc = check_struct_size(p, "tscm_sweep_params")) return rc;
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
    return check_image_list(images, s->n, stride, s->w, "width ");
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
    for (int k = 0; k < s->n; ++k) HIP_TRY(copy_rows(s->img + k * simg, s->w, images[k], stride, s->w, s->h, hipMemcpyHostToDevice));
    HIP_TRY(s->span.mark(0));
    const dim3 grid((unsigned)((s->pw + kTileW - 1) / kTileW), (unsigned)((s->ph + kTileH - 1) / kTileH), (unsigned)(s->D / kZGroup));
    hipLaunchKernelGGL(cost_kernel(s->n), grid, dim3(256), 0, 0, s->pack, s->img, s->w, s->h, s->pw, s->ph, s->D, s->wrap, s->cost, d_sampled, d_alpha, d_census);
    HIP_TRY(s->span.mark(1));
    launch_aggregate(s->cost, s->sum, s->pw, s->ph, s->D, s->p1, s->p2, s->paths);
    HIP_TRY(s->span.mark(2));
    if (with_winner)
        with_planes(s->D, [s](auto npl) {
            hipLaunchKernelGGL(k_sweep_winner<decltype(npl)::value>, dim3((unsigned)((s->npix + 3) / 4)), dim3(256), 0, 0, s->sum, s->cost, s->pw, s->ph, s->D, s->uniqueness,
                               s->index16);
        });
    HIP_TRY(s->span.finish(3, g_stage_seconds, seconds_kernel));
    if (with_winner) s->has_index = true;
    return 0;
}

int create_on_device(tscm_sweep *s, const unsigned char *const *weights, const float *mapx, const float *mapy)
{
    const int n = s->n;
    const size_t simg = (size_t)s->w * s->h, ntab = (size_t)n * s->D * s->npix, nvol = s->npix * s->D;
    HIP_TRY(s->span.create(4));
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
    HIP_TRY(copy_rows(index16, out_stride, s->index16, s->pw, s->pw, s->ph, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tscm_sweep_stages(tscm_sweep *s, const unsigned char *const *images, int stride, unsigned char *sampled, unsigned char *alpha, unsigned long long *census,
                                 unsigned char *cost, unsigned short *aggregated)
{
    if (int rc = check_frame(s, images, stride)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t ntab = (size_t)s->n * s->D * s->npix, nvol = s->npix * s->D;
    DeviceMem tmp;
    StageOutputs stages(tmp);
    unsigned char *d_sampled = nullptr, *d_alpha = nullptr;
    unsigned long long *d_census = nullptr;
    HIP_TRY(stages.scratch(&d_sampled, sampled, ntab));
    HIP_TRY(stages.scratch(&d_alpha, alpha, ntab));
    HIP_TRY(stages.scratch(&d_census, census, ntab));
    stages.from(cost, s->cost, nvol);
    stages.from(aggregated, s->sum, nvol);
    if (int rc = run_frame(s, images, stride, d_sampled, d_alpha, d_census, false, nullptr)) return rc;
    HIP_TRY(stages.fetch());
    return 0;
}

extern "C" int tscm_sweep_stage_times(double *seconds)
{
    if (!seconds) return tscm_set_error(TSCM_E_INVALID, "seconds is NULL");
    for (int k = 0; k < 3; ++k) seconds[k] = g_stage_seconds[k];
    return 0;
}

// ------------------------------------------------------------------------------------------------ compose: host
namespace {

struct ComposeStages {
    unsigned char *hypothesis, *sampled, *alpha, *label, *mask_pyramid;
    short *lap_pyramid, *blend_pyramid;
};

// the checks of tscm_sweep_compose / _stages that they share, in the panorama's wording
int check_compose(const tscm_sweep *s, const unsigned char *const *images, int stride, int channels, const short *index16, int index_stride,
                  const tscm_sweep_compose_params *p, const unsigned short *gain_q8, Gains *gains)
{
    if (!s) return tscm_set_error(TSCM_E_INVALID, "s is NULL");
    if (int rc = check_image_pointers(images, s->n)) return rc;
    if (channels != 1 && channels != 3) return tscm_set_error(TSCM_E_INVALID, "channels " + std::to_string(channels) + " is not 1 or 3");
    if (int rc = check_image_stride(stride, s->w * channels, "width * channels = ")) return rc;
    if (!p) return tscm_set_error(TSCM_E_INVALID, "params is NULL");
    if (int rc = check_struct_size(p, "tscm_sweep_compose_params")) return rc;
    if (p->mode != TSCM_PANO_SEAM && p->mode != TSCM_PANO_FEATHER && p->mode != TSCM_PANO_MULTIBAND)
        return tscm_set_error(TSCM_E_INVALID, "params: unknown mode " + std::to_string(p->mode));
    const bool multiband = p->mode == TSCM_PANO_MULTIBAND;
    if (multiband && (p->levels < 1 || p->levels > kPanoMaxLevels)) return tscm_set_error(TSCM_E_INVALID, "params: levels " + std::to_string(p->levels) + " outside 1..6");
    if (p->fallback_index < 0 || p->fallback_index >= s->D)
        return tscm_set_error(TSCM_E_INVALID, "params: fallback_index " + std::to_string(p->fallback_index) + " outside 0.." + std::to_string(s->D - 1));
    const int L = multiband ? p->levels : 0;
    if (s->pw % (1 << L)) return tscm_set_error(TSCM_E_INVALID, "pano_w " + std::to_string(s->pw) + " is no multiple of 2^levels = " + std::to_string(1 << L));
    if (s->ph % (1 << L)) return tscm_set_error(TSCM_E_INVALID, "pano_h " + std::to_string(s->ph) + " is no multiple of 2^levels = " + std::to_string(1 << L));
    if (int rc = check_index_map(index16, index_stride, s->has_index, s->pw)) return rc;
    return check_gains(gain_q8, s->n, gains);
}

// the composer's buffers for (channels, mode, levels); kept until one of the three changes
int compose_buffers(tscm_sweep *s, int ch, int mode, int L)
{
    if (s->c_ch == ch && s->c_mode == mode && s->levels == L) return 0;
    for (const void *q : { (const void *)s->c_img, (const void *)s->c_out, (const void *)s->c_label, (const void *)s->c_cover, (const void *)s->c_mpyr,
                           (const void *)s->c_wsum, (const void *)s->c_G, (const void *)s->c_B, (const void *)s->c_index })
        s->mem.release(q);
    s->c_img = s->c_out = s->c_label = s->c_cover = s->c_mpyr = nullptr;
    s->c_wsum = nullptr;
    s->c_G = s->c_B = s->c_index = nullptr;
    s->c_mode = -1;
    s->plane = (s->npix + 3) & ~(size_t)3;
    s->set_levels(s->pw, s->ph, L);
    const size_t n = (size_t)s->n;
    HIP_TRY(s->mem.alloc(&s->c_img, n * s->w * s->h * ch));
    HIP_TRY(s->mem.alloc(&s->c_out, s->plane * ch));
    HIP_TRY(s->mem.alloc(&s->c_label, s->plane));
    HIP_TRY(s->mem.alloc(&s->c_cover, s->plane));
    HIP_TRY(s->mem.alloc(&s->c_index, s->plane));
    if (mode == TSCM_PANO_MULTIBAND) {                        // the padding between the levels is never written: it stays zero
        HIP_TRY(s->mem.alloc(&s->c_mpyr, n * s->Sp)); HIP_TRY(hipMemset(s->c_mpyr, 0, n * s->Sp));
        HIP_TRY(s->mem.alloc(&s->c_wsum, s->Sp));
        HIP_TRY(s->mem.alloc(&s->c_G, n * ch * s->Sp)); HIP_TRY(hipMemset(s->c_G, 0, n * ch * s->Sp * sizeof(short)));
        HIP_TRY(s->mem.alloc(&s->c_B, (size_t)ch * s->Sp)); HIP_TRY(hipMemset(s->c_B, 0, (size_t)ch * s->Sp * sizeof(short)));
    }
    s->c_ch = ch; s->c_mode = mode;
    return 0;
}

// use: NULL, or the use planes of the visibility pass
template <int CH>
void launch_gather(const tscm_sweep *s, const short *idx, int fallback, const Gains &g, short *G, size_t stride, unsigned char *mpyr, unsigned char *d_hyp,
                   unsigned char *d_sampled, unsigned char *d_alpha, const unsigned char *use)
{
    if (use)
        hipLaunchKernelGGL((k_sweep_gather<CH, true>), dim3(quad_blocks(s->npix)), dim3(256), 0, 0, s->pack, idx, s->c_img, s->n, s->w, s->h, s->D, fallback, s->npix, g, G,
                           stride, s->c_label, s->c_cover, mpyr, d_hyp, d_sampled, d_alpha, use, s->v_plane);
    else
        hipLaunchKernelGGL((k_sweep_gather<CH, false>), dim3(quad_blocks(s->npix)), dim3(256), 0, 0, s->pack, idx, s->c_img, s->n, s->w, s->h, s->D, fallback, s->npix, g, G,
                           stride, s->c_label, s->c_cover, mpyr, d_hyp, d_sampled, d_alpha, nullptr, (size_t)0);
}

template <int CH, int MODE>
void launch_direct(const tscm_sweep *s, const short *idx, int fallback, const Gains &g, const unsigned char *use)
{
    if (use)
        hipLaunchKernelGGL((k_sweep_compose<CH, MODE, true>), dim3(quad_blocks(s->npix)), dim3(256), 0, 0, s->pack, idx, s->c_img, s->n, s->w, s->h, s->D, fallback, s->npix, g,
                           s->c_out, s->c_cover, use, s->v_plane);
    else
        hipLaunchKernelGGL((k_sweep_compose<CH, MODE, false>), dim3(quad_blocks(s->npix)), dim3(256), 0, 0, s->pack, idx, s->c_img, s->n, s->w, s->h, s->D, fallback, s->npix, g,
                           s->c_out, s->c_cover, nullptr, (size_t)0);
}

// MULTIBAND behind the gather, up to B^l (collapse == false) or to the output bytes: the mask pyramids and their sums are
// per frame here, next to the image pyramids
template <int CH>
void launch_pyramids(const tscm_sweep *s, int wrap, short *lap, bool collapse)
{
    launch_reduce(*s, s->c_G, s->n * CH, wrap);
    launch_reduce(*s, s->c_mpyr, s->n, wrap);
    hipLaunchKernelGGL(k_pano_wsum, dim3((unsigned)((s->Sp + 255) / 256)), dim3(256), 0, 0, s->c_mpyr, s->n, s->Sp, s->c_wsum);
    launch_blend<CH>(*s, s->c_G, s->c_mpyr, s->c_wsum, s->n, wrap, s->c_B, lap, collapse, s->c_cover, s->c_out);
}

template <int CH>
void launch_compose(const tscm_sweep *s, const short *idx, int fallback, int wrap, const Gains &g, const unsigned char *use)
{
    if (s->c_mode == TSCM_PANO_MULTIBAND) {
        launch_gather<CH>(s, idx, fallback, g, s->c_G, s->Sp, s->c_mpyr, nullptr, nullptr, nullptr, use);
        launch_pyramids<CH>(s, wrap, nullptr, true);
    } else if (s->c_mode == TSCM_PANO_SEAM) launch_direct<CH, TSCM_PANO_SEAM>(s, idx, fallback, g, use);
    else launch_direct<CH, TSCM_PANO_FEATHER>(s, idx, fallback, g, use);
}

// buffers, the colour images and the index map (the caller's, or the one tscm_sweep_depth left) on the device
int upload_compose(tscm_sweep *s, const unsigned char *const *images, int stride, int ch, const short *index16, int index_stride,
                   const tscm_sweep_compose_params *p, const short **idx)
{
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = compose_buffers(s, ch, p->mode, p->mode == TSCM_PANO_MULTIBAND ? p->levels : 0)) return rc;
    const size_t row = (size_t)s->w * ch;
    for (int k = 0; k < s->n; ++k) HIP_TRY(copy_rows(s->c_img + (size_t)k * row * s->h, row, images[k], stride, row, s->h, hipMemcpyHostToDevice));
    *idx = s->index16;
    if (index16) {
        HIP_TRY(copy_rows(s->c_index, s->pw, index16, index_stride, s->pw, s->ph, hipMemcpyHostToDevice));
        *idx = s->c_index;
    }
    return 0;
}

// ---- visibility
struct VisibilityStages {
    unsigned char *hypothesis;
    unsigned short *depth_buffer;
    int *cell;
    unsigned char *visible;
};

int check_visibility(const tscm_sweep_visibility_params *p)
{
    if (!p) return tscm_set_error(TSCM_E_INVALID, "vparams is NULL");
    if (int rc = check_struct_size(p, "tscm_sweep_visibility_params", "vparams")) return rc;
    if (p->cell_shift < 0 || p->cell_shift > 8) return tscm_set_error(TSCM_E_INVALID, "vparams: cell_shift " + std::to_string(p->cell_shift) + " outside 0..8");
    if (p->tolerance < 0 || p->tolerance > 255) return tscm_set_error(TSCM_E_INVALID, "vparams: tolerance " + std::to_string(p->tolerance) + " outside 0..255");
    if (p->dilate < 0 || p->dilate > 2) return tscm_set_error(TSCM_E_INVALID, "vparams: dilate " + std::to_string(p->dilate) + " outside 0..2");
    if (p->near_is_high != 0 && p->near_is_high != 1) return tscm_set_error(TSCM_E_INVALID, "vparams: near_is_high " + std::to_string(p->near_is_high) + " is not 0 or 1");
    return 0;
}

int visibility_buffers(tscm_sweep *s)
{
    if (s->v_zbuf) return 0;
    s->v_plane = (s->npix + 3) & ~(size_t)3;
    HIP_TRY(s->mem.alloc(&s->v_use, (size_t)s->n * s->v_plane));
    HIP_TRY(s->mem.alloc(&s->v_state, s->v_plane));
    HIP_TRY(s->mem.alloc(&s->v_index, s->v_plane));
    HIP_TRY(s->mem.alloc(&s->v_zbuf, (size_t)s->n * s->w * s->h));
    return 0;
}

// clear, splat and test on the index map `idx` on the device, into v_use and v_state; st (may be NULL): device pointers of
// the stage outputs.  The caller synchronises.
int launch_visibility(const tscm_sweep *s, const short *idx, const tscm_sweep_visibility_params *p, const VisibilityStages *st)
{
    const int cw = ((s->w - 1) >> p->cell_shift) + 1, ch = ((s->h - 1) >> p->cell_shift) + 1;
    const size_t cells = (size_t)cw * ch;
    HIP_TRY(hipMemsetAsync(s->v_zbuf, 0, (size_t)s->n * cells * sizeof(unsigned), 0));
    hipLaunchKernelGGL(k_sweep_splat, dim3(quad_blocks(s->npix)), dim3(256), 0, 0, s->pack, idx, s->n, s->w, s->h, s->D, s->npix, p->cell_shift, cw, cells, p->near_is_high,
                       s->v_zbuf);
    hipLaunchKernelGGL(k_sweep_vis_test, dim3(quad_blocks(s->npix)), dim3(256), 0, 0, s->pack, idx, s->n, s->w, s->h, s->D, s->npix, s->v_plane, p->cell_shift, cw, ch,
                       p->tolerance, p->dilate, p->near_is_high, s->v_zbuf, s->v_use, s->v_state, st ? st->hypothesis : nullptr, st ? st->cell : nullptr,
                       st ? st->visible : nullptr);
    return 0;
}

// use [n][npix] and state [npix] of the last launch_visibility, either may be NULL
int download_use_state(const tscm_sweep *s, unsigned char *use, unsigned char *state)
{
    if (use) HIP_TRY(copy_rows(use, s->npix, s->v_use, s->v_plane, s->npix, s->n, hipMemcpyDeviceToHost));
    if (state) HIP_TRY(hipMemcpy(state, s->v_state, s->npix, hipMemcpyDeviceToHost));
    return 0;
}

int visibility_call(tscm_sweep *s, const short *index16, int index_stride, const tscm_sweep_visibility_params *p, const VisibilityStages *host, unsigned char *use,
                    unsigned char *state, double *seconds_kernel)
{
    if (!s) return tscm_set_error(TSCM_E_INVALID, "s is NULL");
    if (int rc = check_visibility(p)) return rc;
    if (int rc = check_index_map(index16, index_stride, s->has_index, s->pw)) return rc;
    if (seconds_kernel) *seconds_kernel = 0.0;
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = visibility_buffers(s)) return rc;
    const short *idx = s->index16;
    if (index16) {
        HIP_TRY(copy_rows(s->v_index, s->pw, index16, index_stride, s->pw, s->ph, hipMemcpyHostToDevice));
        idx = s->v_index;
    }
    const size_t nplane = (size_t)s->n * s->npix;
    DeviceMem tmp;
    StageOutputs stages(tmp);
    VisibilityStages dev = { nullptr, nullptr, nullptr, nullptr };
    if (host) {
        HIP_TRY(stages.scratch(&dev.hypothesis, host->hypothesis, s->npix, s->v_plane));
        HIP_TRY(stages.scratch(&dev.cell, host->cell, nplane));
        HIP_TRY(stages.scratch(&dev.visible, host->visible, nplane));
    }
    HIP_TRY(s->span.mark(0));
    if (int rc = launch_visibility(s, idx, p, host ? &dev : nullptr)) return rc;
    HIP_TRY(s->span.finish(1, nullptr, seconds_kernel));
    if (int rc = download_use_state(s, use, state)) return rc;
    HIP_TRY(stages.fetch());
    if (host && host->depth_buffer) {                         // rank + 1 <= 256: the 32-bit cells of the atomics as uint16
        const size_t cells = (size_t)s->n * (((s->w - 1) >> p->cell_shift) + 1) * (((s->h - 1) >> p->cell_shift) + 1);
        std::vector<unsigned> z(cells);
        HIP_TRY(hipMemcpy(z.data(), s->v_zbuf, cells * sizeof(unsigned), hipMemcpyDeviceToHost));
        for (size_t t = 0; t < cells; ++t) host->depth_buffer[t] = (unsigned short)z[t];
    }
    return 0;
}

// tscm_sweep_compose (visible == false) and tscm_sweep_compose_visible
int compose_call(tscm_sweep *s, const unsigned char *const *images, int stride, int channels, const short *index16, int index_stride,
                 const tscm_sweep_compose_params *params, const tscm_sweep_visibility_params *vp, bool visible, const unsigned short *gain_q8, unsigned char *dst,
                 int dst_stride, unsigned char *coverage, double *seconds_kernel)
{
    Gains g;
    if (int rc = check_compose(s, images, stride, channels, index16, index_stride, params, gain_q8, &g)) return rc;
    if (!dst) return tscm_set_error(TSCM_E_INVALID, "dst is NULL");
    if (dst_stride < s->pw * channels) return tscm_set_error(TSCM_E_INVALID, "dst_stride " + std::to_string(dst_stride) + " < pano_w * channels = " + std::to_string(s->pw * channels));
    if (visible)
        if (int rc = check_visibility(vp)) return rc;
    if (seconds_kernel) *seconds_kernel = 0.0;
    const short *idx = nullptr;
    if (int rc = upload_compose(s, images, stride, channels, index16, index_stride, params, &idx)) return rc;
    if (visible)
        if (int rc = visibility_buffers(s)) return rc;
    const int wrap = params->wrap_x ? 1 : 0;                 // the pyramids' wrap is the composer's own, not the census window's
    HIP_TRY(s->span.mark(0));
    if (visible)
        if (int rc = launch_visibility(s, idx, vp, nullptr)) return rc;
    if (channels == 1) launch_compose<1>(s, idx, params->fallback_index, wrap, g, visible ? s->v_use : nullptr);
    else launch_compose<3>(s, idx, params->fallback_index, wrap, g, visible ? s->v_use : nullptr);
    HIP_TRY(s->span.finish(1, nullptr, seconds_kernel));
    const size_t row = (size_t)s->pw * channels;
    HIP_TRY(copy_rows(dst, dst_stride, s->c_out, row, row, s->ph, hipMemcpyDeviceToHost));
    if (coverage) HIP_TRY(hipMemcpy(coverage, s->c_cover, s->npix, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" void tscm_sweep_compose_default_params(tscm_sweep_compose_params *p)
{
    if (!p) return;
    p->struct_size = (int)sizeof(tscm_sweep_compose_params);
    p->mode = TSCM_PANO_MULTIBAND; p->levels = 4; p->wrap_x = 1; p->fallback_index = 0;
}

extern "C" int tscm_sweep_compose(tscm_sweep *s, const unsigned char *const *images, int stride, int channels, const short *index16, int index_stride,
                                  const tscm_sweep_compose_params *params, const unsigned short *gain_q8, unsigned char *dst, int dst_stride, unsigned char *coverage,
                                  double *seconds_kernel)
{
    return compose_call(s, images, stride, channels, index16, index_stride, params, nullptr, false, gain_q8, dst, dst_stride, coverage, seconds_kernel);
}

namespace {

// tscm_sweep_compose_stages (visible == false) and tscm_sweep_compose_visible_stages
int compose_stages_call(tscm_sweep *s, const unsigned char *const *images, int stride, int channels, const short *index16, int index_stride,
                        const tscm_sweep_compose_params *params, const tscm_sweep_visibility_params *vp, bool visible, const unsigned short *gain_q8,
                        unsigned char *hypothesis, unsigned char *sampled, unsigned char *alpha, unsigned char *label, unsigned char *mask_pyramid, short *lap_pyramid,
                        short *blend_pyramid, unsigned char *use_out, unsigned char *state_out)
{
    Gains g;
    if (int rc = check_compose(s, images, stride, channels, index16, index_stride, params, gain_q8, &g)) return rc;
    const bool multiband = params->mode == TSCM_PANO_MULTIBAND;
    if (!multiband && (mask_pyramid || lap_pyramid || blend_pyramid))
        return tscm_set_error(TSCM_E_INVALID, std::string(mask_pyramid ? "mask_pyramid" : lap_pyramid ? "lap_pyramid" : "blend_pyramid") + ": the mode is not MULTIBAND");
    if (visible)
        if (int rc = check_visibility(vp)) return rc;
    const short *idx = nullptr;
    if (int rc = upload_compose(s, images, stride, channels, index16, index_stride, params, &idx)) return rc;
    const unsigned char *use = nullptr;
    if (visible) {
        if (int rc = visibility_buffers(s)) return rc;
        if (int rc = launch_visibility(s, idx, vp, nullptr)) return rc;
        use = s->v_use;
    }
    const int n = s->n, ch = channels;
    const size_t nplane = (size_t)n * s->npix;
    DeviceMem tmp;
    StageOutputs stages(tmp);
    unsigned char *d_hyp = nullptr, *d_sampled = nullptr, *d_alpha = nullptr;
    short *d_lap = nullptr, *d_G = s->c_G;
    size_t gstride = s->Sp;
    HIP_TRY(stages.scratch(&d_hyp, hypothesis, s->npix, s->plane));
    HIP_TRY(stages.scratch(&d_sampled, sampled, nplane * ch));
    HIP_TRY(stages.scratch(&d_alpha, alpha, nplane));
    stages.from(label, s->c_label, s->npix);
    if (!multiband) {                                         // SEAM and FEATHER keep no planes: the gather writes into a scratch set
        gstride = s->plane;
        HIP_TRY(tmp.alloc(&d_G, (size_t)n * ch * gstride));
    } else if (lap_pyramid) HIP_TRY(tmp.alloc(&d_lap, (size_t)n * ch * s->Sp));
    const int wrap = params->wrap_x ? 1 : 0;
    if (ch == 1) {
        launch_gather<1>(s, idx, params->fallback_index, g, d_G, gstride, s->c_mpyr, d_hyp, d_sampled, d_alpha, use);
        if (multiband) launch_pyramids<1>(s, wrap, d_lap, false);
    } else {
        launch_gather<3>(s, idx, params->fallback_index, g, d_G, gstride, s->c_mpyr, d_hyp, d_sampled, d_alpha, use);
        if (multiband) launch_pyramids<3>(s, wrap, d_lap, false);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(stages.fetch());
    if (int rc = download_pyramid(*s, s->c_mpyr, n, mask_pyramid)) return rc;
    if (int rc = download_pyramid(*s, d_lap, n * ch, lap_pyramid)) return rc;
    if (int rc = download_pyramid(*s, s->c_B, ch, blend_pyramid)) return rc;
    if (visible) return download_use_state(s, use_out, state_out);
    return 0;
}

}  // namespace

extern "C" int tscm_sweep_compose_stages(tscm_sweep *s, const unsigned char *const *images, int stride, int channels, const short *index16, int index_stride,
                                         const tscm_sweep_compose_params *params, const unsigned short *gain_q8, unsigned char *hypothesis, unsigned char *sampled,
                                         unsigned char *alpha, unsigned char *label, unsigned char *mask_pyramid, short *lap_pyramid, short *blend_pyramid)
{
    return compose_stages_call(s, images, stride, channels, index16, index_stride, params, nullptr, false, gain_q8, hypothesis, sampled, alpha, label, mask_pyramid,
                               lap_pyramid, blend_pyramid, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------------ visibility: entry points
extern "C" void tscm_sweep_visibility_default_params(tscm_sweep_visibility_params *p)
{
    if (!p) return;
    p->struct_size = (int)sizeof(tscm_sweep_visibility_params);
    p->cell_shift = 2; p->tolerance = 2; p->dilate = 0; p->near_is_high = 1;
}

extern "C" int tscm_sweep_visibility(tscm_sweep *s, const short *index16, int index_stride, const tscm_sweep_visibility_params *vparams, unsigned char *use,
                                     unsigned char *state, double *seconds_kernel)
{
    return visibility_call(s, index16, index_stride, vparams, nullptr, use, state, seconds_kernel);
}

extern "C" int tscm_sweep_visibility_stages(tscm_sweep *s, const short *index16, int index_stride, const tscm_sweep_visibility_params *vparams, unsigned char *hypothesis,
                                            unsigned short *depth_buffer, int *cell, unsigned char *visible, unsigned char *use, unsigned char *state)
{
    const VisibilityStages host = { hypothesis, depth_buffer, cell, visible };
    return visibility_call(s, index16, index_stride, vparams, &host, use, state, nullptr);
}

extern "C" int tscm_sweep_compose_visible(tscm_sweep *s, const unsigned char *const *images, int stride, int channels, const short *index16, int index_stride,
                                          const tscm_sweep_compose_params *params, const tscm_sweep_visibility_params *vparams, const unsigned short *gain_q8,
                                          unsigned char *dst, int dst_stride, unsigned char *coverage, double *seconds_kernel)
{
    return compose_call(s, images, stride, channels, index16, index_stride, params, vparams, true, gain_q8, dst, dst_stride, coverage, seconds_kernel);
}

extern "C" int tscm_sweep_compose_visible_stages(tscm_sweep *s, const unsigned char *const *images, int stride, int channels, const short *index16, int index_stride,
                                                 const tscm_sweep_compose_params *params, const tscm_sweep_visibility_params *vparams, const unsigned short *gain_q8,
                                                 unsigned char *hypothesis, unsigned char *sampled, unsigned char *alpha, unsigned char *label, unsigned char *mask_pyramid,
                                                 short *lap_pyramid, short *blend_pyramid, unsigned char *use, unsigned char *state)
{
    return compose_stages_call(s, images, stride, channels, index16, index_stride, params, vparams, true, gain_q8, hypothesis, sampled, alpha, label, mask_pyramid,
                               lap_pyramid, blend_pyramid, use, state);
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
    HIP_TRY(copy_rows(d_idx, pano_w, index16, stride, pano_w, pano_h, hipMemcpyHostToDevice));
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
