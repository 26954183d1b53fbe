// tscm_stereo_filter.hip -- the post-filter of a disparity map (tscm.h: tscm_stereo_filter*): 4-connected components of
// the "neighbours within speckle_range" graph by union-find, their sizes, the speckle rule and a masked median.  Integer
// arithmetic and order-independent reductions only (integer atomicMin / atomicAdd), so a host restatement
// (tests/stereo_filter_ref.py) gives the same bits.
//
// Arrays [h][w], dense: d int16, parent / label / cnt / rootsize int32.  A pixel's linear index is y * w + x.
//   k_ccl_tile        64 x 16 tile: disparities and a parent array in LDS, union-find over the tile's row edges, then its
//                     column edges (LDS atomicMin, the larger root goes under the smaller); writes each pixel's tile root as
//                     a global index (-1: invalid) and, at each tile root, the number of tile pixels under it (cnt)
//   k_ccl_seams       one thread per pixel pair across a tile border: find + union on the global parent array, atomicMin at
//                     agent scope, repeated until the union sticks
//   k_ccl_flatten     every pixel chases its root -> label; clears rootsize
//   k_ccl_count       rootsize[label] += cnt, one atomicAdd per (tile, component)
//   k_speckle_median  tile + halo of despeckled values in LDS (size test through rootsize[label]), median by rank counting
// Launch boundaries are the only ordering between workgroups.
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_host.h"

#include <climits>
#include <string>

using namespace tscm;

namespace {

constexpr int kTileW = 64, kTileH = 16, kTilePixels = kTileW * kTileH;       // the tile of k_census

// ------------------------------------------------------------------------------------------------ union-find
// Invariant of both forests: parent[x] <= x, so a chain of parents ends, and a root is the smallest index seen so far.
__device__ __forceinline__ int find_lds(int *P, int x)
{
    int p;
    while ((p = __hip_atomic_load(&P[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = p;
    return x;
}

__device__ __forceinline__ int find_global(int *P, int x)
{
    int p;
    while ((p = __hip_atomic_load(&P[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = p;
    return x;
}

// Links the larger of the two roots under the smaller.  atomicMin returns what the larger root's entry held: if that is
// no longer itself another union came first, and this one goes on with (that parent, the smaller root), which keeps all
// three connected whichever value the entry now holds.  Nothing waits for another thread: a failed attempt means that
// some other union has succeeded.
#define TSCM_UNITE(FIND, P, a, b)                        \
    for (;;) {                                           \
        a = FIND(P, a);                                  \
        b = FIND(P, b);                                  \
        if (a == b) break;                               \
        const int hi_ = max(a, b), lo_ = min(a, b);      \
        const int old_ = atomicMin(&P[hi_], lo_);        \
        if (old_ == hi_) break;                          \
        a = old_;                                        \
        b = lo_;                                         \
    }

__device__ __forceinline__ void unite_lds(int *P, int a, int b) { TSCM_UNITE(find_lds, P, a, b) }
__device__ __forceinline__ void unite_global(int *P, int a, int b) { TSCM_UNITE(find_global, P, a, b) }

__device__ __forceinline__ bool joined(int u, int v, int invalid, int thr) { return u != invalid && v != invalid && abs(u - v) <= thr; }

// ------------------------------------------------------------------------------------------------ components of a tile
// grid (tiles_x * tiles_y) x 256: thread t owns the tile pixels l = t + 256 i, i < 4 (column l & 63, row l >> 6).  Pixels
// of the tile outside the image hold `invalid`, so no edge needs a bounds test.  A tile's local order l is the raster
// order of its pixels, so the smallest l of a component is its smallest global index inside the tile.
__global__ __launch_bounds__(256) void k_ccl_tile(const short *__restrict__ d, int w, int h, int tiles_x, int invalid, int thr, int *__restrict__ parent,
                                                  int *__restrict__ cnt)
{
    __shared__ short sd[kTilePixels];
    __shared__ int sp[kTilePixels], sc[kTilePixels];
    const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int x0 = bx * kTileW, y0 = by * kTileH;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int l = threadIdx.x + 256 * i, x = x0 + (l & 63), y = y0 + (l >> 6);
        sd[l] = (x < w && y < h) ? d[(size_t)y * w + x] : (short)invalid;
        sp[l] = l;
        sc[l] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {                            // row edges: runs of a row become chains l -> l - 1
        const int l = threadIdx.x + 256 * i;
        if ((l & 63) < 63 && joined(sd[l], sd[l + 1], invalid, thr)) unite_lds(sp, l, l + 1);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {                            // shorten them to one step before the column edges walk them
        const int l = threadIdx.x + 256 * i;
        __hip_atomic_store(&sp[l], find_lds(sp, l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int l = threadIdx.x + 256 * i;
        if (l + kTileW < kTilePixels && joined(sd[l], sd[l + kTileW], invalid, thr)) unite_lds(sp, l, l + kTileW);
    }
    __syncthreads();
    int root[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int l = threadIdx.x + 256 * i;
        root[i] = -1;
        if (sd[l] != invalid) {
            root[i] = find_lds(sp, l);
            atomicAdd(&sc[root[i]], 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int l = threadIdx.x + 256 * i, x = x0 + (l & 63), y = y0 + (l >> 6);
        if (x >= w || y >= h) continue;
        const size_t g = (size_t)y * w + x;
        parent[g] = root[i] < 0 ? -1 : (y0 + (root[i] >> 6)) * w + x0 + (root[i] & 63);
        cnt[g] = sc[l];                                      // non-zero at tile roots only
    }
}

// ------------------------------------------------------------------------------------------------ tile borders
// Threads [0, nv * h): pair (x - 1, x) at x = 64 (k + 1), row y, k = t / h.  Threads after them: pair (y - 1, y) at
// y = 16 (k + 1), column x, k = t' / w.  nv = tiles_x - 1, nh = tiles_y - 1.
__global__ __launch_bounds__(256) void k_ccl_seams(const short *__restrict__ d, int w, int h, int nv, int nh, int invalid, int thr, int *parent)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, n_vert = (long long)nv * h;
    size_t p, q;
    if (t < n_vert) {
        const int k = (int)(t / h), y = (int)(t - (long long)k * h);
        q = (size_t)y * w + (size_t)kTileW * (k + 1);
        p = q - 1;
    } else {
        const long long u = t - n_vert;
        if (u >= (long long)nh * w) return;
        const int k = (int)(u / w), x = (int)(u - (long long)k * w);
        q = (size_t)kTileH * (k + 1) * w + x;
        p = q - w;
    }
    if (joined(d[p], d[q], invalid, thr)) unite_global(parent, (int)p, (int)q);
}

// one thread per pixel; parent is read-only here
__global__ __launch_bounds__(256) void k_ccl_flatten(const int *__restrict__ parent, int n, int *__restrict__ label, int *__restrict__ rootsize)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int x = parent[i];
    if (x >= 0)
        for (int p; (p = parent[x]) != x;) x = p;
    label[i] = x;
    rootsize[i] = 0;
}

__global__ __launch_bounds__(256) void k_ccl_count(const int *__restrict__ cnt, const int *__restrict__ label, int n, int *rootsize)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = cnt[i];
    if (c > 0) atomicAdd(&rootsize[label[i]], c);
}

// ------------------------------------------------------------------------------------------------ speckle rule + median
// grid (tiles_x * tiles_y) x 256.  The tile and its M / 2 halo hold the map after the speckle rule; positions outside the
// image hold `invalid`, which is what "only the window's pixels inside the image" needs.  label == NULL: no speckle rule.
// size_out / desp_out (the stages; may be NULL) are written by the block whose tile owns the pixel.
// Median of the n valid entries: invalid ones get a key above every int16, so they sort last; the element at index
// k = (n - 1) >> 1 is the smallest key with more than k keys <= it.  M * M keys in registers, all loops unrolled.
template <int M>
__global__ __launch_bounds__(256) void k_speckle_median(const short *__restrict__ d, const int *__restrict__ label, const int *__restrict__ rootsize, int w, int h,
                                                        int tiles_x, int invalid, int window, short *__restrict__ out, int *__restrict__ size_out,
                                                        short *__restrict__ desp_out)
{
    constexpr int R = M / 2, LW = kTileW + 2 * R, LH = kTileH + 2 * R;
    __shared__ short tile[LH * LW];
    const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int x0 = bx * kTileW, y0 = by * kTileH;
    for (int e = threadIdx.x; e < LW * LH; e += 256) {
        const int ty = e / LW, tx = e - ty * LW;
        const int gx = x0 + tx - R, gy = y0 + ty - R;
        int v = invalid;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t g = (size_t)gy * w + gx;
            v = d[g];
            int sz = 0;
            if (label) {
                const int lab = label[g];
                if (lab >= 0) sz = rootsize[lab];
                if (window > 0 && sz <= window) v = invalid;
            }
            if (tx >= R && tx < R + kTileW && ty >= R && ty < R + kTileH) {
                if (size_out) size_out[g] = sz;
                if (desp_out) desp_out[g] = (short)v;
            }
        }
        tile[e] = (short)v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int l = threadIdx.x + 256 * i, lx = l & 63, ly = l >> 6;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= w || y >= h) continue;
        int res = tile[(ly + R) * LW + lx + R];
        if constexpr (M > 0) {
            if (res != invalid) {
                constexpr int kAbove = 0x10000;
                int key[M * M], n = 0;
#pragma unroll
                for (int dy = 0; dy < M; ++dy)
#pragma unroll
                    for (int dx = 0; dx < M; ++dx) {
                        const int v = tile[(ly + dy) * LW + lx + dx];
                        n += v != invalid;
                        key[dy * M + dx] = v != invalid ? v : kAbove;
                    }
                const int k = (n - 1) >> 1;
                res = kAbove;
#pragma unroll
                for (int a = 0; a < M * M; ++a) {
                    int le = 0;
#pragma unroll
                    for (int b = 0; b < M * M; ++b) le += key[b] <= key[a];
                    res = min(res, le > k ? key[a] : kAbove);
                }
            }
        }
        out[(size_t)y * w + x] = (short)res;
    }
}

// ------------------------------------------------------------------------------------------------ host
int check_filter_args(const short *disparity, int width, int height, int disp_stride, const tscm_stereo_filter_params *p)
{
    if (int rc = check_map_args(disparity, width, height, disp_stride, p, "tscm_stereo_filter_params")) return rc;
    if (p->speckle_window_size < 0) return tscm_set_error(TSCM_E_INVALID, "params: speckle_window_size " + std::to_string(p->speckle_window_size) + " is negative");
    if (p->speckle_range < 0 || p->speckle_range > 255) return tscm_set_error(TSCM_E_INVALID, "params: speckle_range " + std::to_string(p->speckle_range) + " outside 0..255");
    if (p->median != 0 && p->median != 3 && p->median != 5) return tscm_set_error(TSCM_E_INVALID, "params: median " + std::to_string(p->median) + " is not 0, 3 or 5");
    if (int rc = check_map_min_disparity(p->min_disparity)) return rc;
    if ((long long)width * height > (long long)INT_MAX)
        return tscm_set_error(TSCM_E_INVALID, "width * height = " + std::to_string((long long)width * height) + " does not fit the int32 labels");
    return 0;
}

// The kernels of one map.  Outputs are host pointers, any of them NULL.  The component kernels run when the speckle rule
// is on or a stage asks for them.
int filter_run(const short *disparity, int w, int h, int disp_stride, const tscm_stereo_filter_params &p, int device, const char *who, short *out, int out_stride,
               int *label, int *size, short *despeckled, double *seconds_kernel)
{
    if (int rc = select_device(device, who)) return rc;
    const int n = w * h, invalid = 16 * (p.min_disparity - 1), thr = 16 * p.speckle_range;
    const int tiles_x = (w + kTileW - 1) / kTileW, tiles_y = (h + kTileH - 1) / kTileH;
    const bool components = p.speckle_window_size > 0 || label || size;
    DeviceMem mem;
    StageOutputs stages(mem);
    EventSpan span;
    short *d_in = nullptr, *d_out = nullptr, *d_desp = nullptr;
    int *d_parent = nullptr, *d_cnt = nullptr, *d_label = nullptr, *d_rootsize = nullptr, *d_size = nullptr;
    HIP_TRY(mem.alloc(&d_in, (size_t)n));
    HIP_TRY(mem.alloc(&d_out, (size_t)n));
    HIP_TRY(copy_rows(d_in, w, disparity, disp_stride, w, h, hipMemcpyHostToDevice));
    if (components) {
        HIP_TRY(mem.alloc(&d_parent, (size_t)n)); HIP_TRY(mem.alloc(&d_cnt, (size_t)n));
        HIP_TRY(mem.alloc(&d_label, (size_t)n)); HIP_TRY(mem.alloc(&d_rootsize, (size_t)n));
    }
    stages.from(label, d_label, (size_t)n);
    HIP_TRY(stages.scratch(&d_size, size, (size_t)n));
    HIP_TRY(stages.scratch(&d_desp, despeckled, (size_t)n));
    HIP_TRY(span.create(2));
    const dim3 tiles((unsigned)(tiles_x * tiles_y)), pixels((unsigned)((n + 255) / 256)), block(256);
    HIP_TRY(span.mark(0));
    if (components) {
        hipLaunchKernelGGL(k_ccl_tile, tiles, block, 0, 0, d_in, w, h, tiles_x, invalid, thr, d_parent, d_cnt);
        const long long seam_pairs = (long long)(tiles_x - 1) * h + (long long)(tiles_y - 1) * w;
        if (seam_pairs > 0)
            hipLaunchKernelGGL(k_ccl_seams, dim3((unsigned)((seam_pairs + 255) / 256)), block, 0, 0, d_in, w, h, tiles_x - 1, tiles_y - 1, invalid, thr, d_parent);
        hipLaunchKernelGGL(k_ccl_flatten, pixels, block, 0, 0, d_parent, n, d_label, d_rootsize);
        hipLaunchKernelGGL(k_ccl_count, pixels, block, 0, 0, d_cnt, d_label, n, d_rootsize);
    }
    auto *const f = p.median == 0 ? k_speckle_median<0> : p.median == 3 ? k_speckle_median<3> : k_speckle_median<5>;
    hipLaunchKernelGGL(f, tiles, block, 0, 0, d_in, d_label, d_rootsize, w, h, tiles_x, invalid, p.speckle_window_size, d_out, d_size, d_desp);
    HIP_TRY(span.finish(1, nullptr, seconds_kernel));
    if (out) HIP_TRY(copy_rows(out, out_stride, d_out, w, w, h, hipMemcpyDeviceToHost));
    HIP_TRY(stages.fetch());
    return 0;
}

}  // namespace

extern "C" void tscm_stereo_filter_default_params(tscm_stereo_filter_params *p)
{
    if (!p) return;
    p->struct_size = (int)sizeof(tscm_stereo_filter_params);
    p->min_disparity = 0;
    p->speckle_window_size = 100; p->speckle_range = 2;
    p->median = 0;
}

extern "C" int tscm_stereo_filter(const short *disparity, int width, int height, int disp_stride, const tscm_stereo_filter_params *params, int device,
                                  short *out, int out_stride, double *seconds_kernel)
{
    if (int rc = check_filter_args(disparity, width, height, disp_stride, params)) return rc;
    if (int rc = check_map_out(out, out_stride, width)) return rc;
    if (seconds_kernel) *seconds_kernel = 0.0;
    if (width == 0 || height == 0) return 0;
    return filter_run(disparity, width, height, disp_stride, *params, device, "tscm_stereo_filter", out, out_stride, nullptr, nullptr, nullptr, seconds_kernel);
}

extern "C" int tscm_stereo_filter_stages(const short *disparity, int width, int height, int disp_stride, const tscm_stereo_filter_params *params, int device,
                                         int *label, int *size, short *despeckled)
{
    if (int rc = check_filter_args(disparity, width, height, disp_stride, params)) return rc;
    if (width == 0 || height == 0) return 0;
    return filter_run(disparity, width, height, disp_stride, *params, device, "tscm_stereo_filter_stages", nullptr, 0, label, size, despeckled, nullptr);
}
