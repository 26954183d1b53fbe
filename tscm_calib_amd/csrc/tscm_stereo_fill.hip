// tscm_stereo_fill.hip -- hole filling of a disparity or sweep index map (tscm.h: tscm_stereo_fill*): for every pixel and
// each of the 8 path directions the nearest valid value and its distance, then for the invalid pixels a rank of those
// candidates.  Integers only and no atomics; every candidate comes from the input map, so a host restatement
// (tests/stereo_fill_ref.py) gives the same bits.
//
// No loop's trip count depends on the map: a candidate is the carry (last valid value, steps since) of a scan that runs
// against its direction, so the work is paths * w * h whatever the holes look like.
//
// Arrays: d int16 [h][w] dense; cand uint32 [paths][h][w], one packed candidate (distance << 16 | value & 0xffff) per
// direction and pixel, distance 0 = none.
//   k_fill_rows     directions 0, 1 (+x, -x): one wave per (row, direction), 64 columns per step, inclusive max-scan of
//                   the keys (position << 16 | value) over the lanes with __shfl_up, the carry between steps in a register;
//                   with wrap_x a first pass over the row finds the key that enters it from the other side of the seam
//   k_fill_lines    directions 2..7 (vertical, diagonal): one thread per scanline, enumerated as k_aggregate does: start
//                   column c, step i visits row i (or h - 1 - i) and column (c - dx i) mod w, so the threads of a wave read
//                   and write consecutive elements of a row; loads are issued kPrefetch rows ahead of the carry chain
//   k_fill_select   one thread per pixel: its candidates through a fixed 19-exchange sorting network, the pick by rule
// Launch boundaries are the only ordering between workgroups.
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_host.h"

#include <climits>
#include <string>
#include <vector>

using namespace tscm;

namespace {

constexpr int kPrefetch = 16;                 // rows of loads in flight per scanline thread
constexpr int kNone = INT_MAX;                // sorts behind every int16

__device__ __forceinline__ unsigned pack_candidate(int value, int dist) { return ((unsigned)dist << 16) | ((unsigned)value & 0xffffu); }

// ------------------------------------------------------------------------------------------------ rows
// grid (ceil(h / 4), 2) x 256: wave = row, blockIdx.y = direction.  The scan runs against the direction, over the scan
// position m = 0 .. w - 1: column x = m for direction 1 (-x: the scan runs left to right), x = w - 1 - m for direction 0.
// Key of a valid pixel: (m + w + 1) << 16 | value; 0 = none.  The key that enters over the seam is the row's largest
// key moved back by one revolution, (m + 1) << 16 | value: any pixel of the row itself beats it, and its distance to
// position m' is m' + w - m, which the rule "a horizontal walk ends after t = w - 1" cuts off exactly at the pixel itself.
__global__ __launch_bounds__(256) void k_fill_rows(const short *__restrict__ d, int w, int h, int invalid, int maxd, int wrap, unsigned *__restrict__ cand)
{
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6), dir = blockIdx.y;
    if (y >= h) return;                                     // whole waves leave: the shuffles below stay among 64 live lanes
    const short *row = d + (size_t)y * w;
    unsigned *crow = cand + ((size_t)dir * h + y) * w;
    const int steps = (w + 63) >> 6;
    unsigned carry = 0;
    if (wrap) {
        unsigned best = 0;
        for (int s = 0; s < steps; ++s) {
            const int m = 64 * s + lane;
            if (m < w) {
                const int v = row[dir ? m : w - 1 - m];
                if (v != invalid) best = max(best, ((unsigned)(m + w + 1) << 16) | ((unsigned)v & 0xffffu));
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, off));
        carry = best ? best - ((unsigned)w << 16) : 0u;
    }
    for (int s = 0; s < steps; ++s) {
        const int m = 64 * s + lane, x = dir ? m : w - 1 - m;
        unsigned key = 0;
        if (m < w) {
            const int v = row[x];
            if (v != invalid) key = ((unsigned)(m + w + 1) << 16) | ((unsigned)v & 0xffffu);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned t = (unsigned)__shfl_up((int)key, off);
            if (lane >= off) key = max(key, t);
        }
        unsigned before = (unsigned)__shfl_up((int)key, 1);          // exclusive: the pixels behind this one
        if (lane == 0) before = 0;
        before = max(before, carry);
        carry = max(carry, (unsigned)__shfl((int)key, 63));
        if (m < w) {
            const int dist = before ? m + w + 1 - (int)(before >> 16) : 0;
            crow[x] = (dist >= 1 && dist < w && dist <= maxd) ? pack_candidate((int)(before & 0xffffu), dist) : 0u;
        }
    }
}

// ------------------------------------------------------------------------------------------------ columns and diagonals
// grid (ceil(w / 64), paths - 2) x 64: thread = scanline c, blockIdx.y + 2 = direction (dx, dy).  The scan runs against
// the direction: step i is at row i for dy < 0 and h - 1 - i for dy > 0, and at column (c - dx i) mod w.  Every line has
// h steps and the w lines of a direction cover every pixel once.  Where the column passes an end of the row the carry is
// dropped, or kept with wrap_x.  age = steps since the carried value's pixel, which is the walk's t at the current pixel.
__global__ __launch_bounds__(64) void k_fill_lines(const short *__restrict__ d, int w, int h, int invalid, int maxd, int wrap, unsigned *__restrict__ cand)
{
    const int c = blockIdx.x * 64 + threadIdx.x, dir = blockIdx.y + 2;
    if (c >= w) return;
    const int dx = dir < 4 ? 0 : ((dir == 4 || dir == 6) ? 1 : -1);
    const bool down = dir == 2 || dir == 4 || dir == 7;     // dy = +1: the scan climbs from the last row
    unsigned *plane = cand + (size_t)dir * h * w;
    int col = c, value = 0, age = 0;                         // age 0: nothing carried
    for (int i0 = 0; i0 < h; i0 += kPrefetch) {
        int v[kPrefetch], cols[kPrefetch];
        unsigned crossed = 0;
#pragma unroll
        for (int j = 0; j < kPrefetch; ++j) {
            const int i = i0 + j;
            if (i > 0) {                                     // the move onto step i
                col -= dx;
                if (col < 0) { col += w; crossed |= 1u << j; }
                if (col >= w) { col -= w; crossed |= 1u << j; }
            }
            cols[j] = col;
            v[j] = i < h ? (int)d[(size_t)(down ? h - 1 - i : i) * w + col] : invalid;
        }
#pragma unroll
        for (int j = 0; j < kPrefetch; ++j) {
            const int i = i0 + j;
            if (i < h) {
                if (((crossed >> j) & 1u) && !wrap) age = 0;
                plane[(size_t)(down ? h - 1 - i : i) * w + cols[j]] = (age >= 1 && age <= maxd) ? pack_candidate(value, age) : 0u;
                if (v[j] != invalid) { value = v[j]; age = 0; }
                age += (v[j] != invalid || age > 0) ? 1 : 0;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ select
#define TSCM_CX(a, b) { const int lo_ = min(k[a], k[b]), hi_ = max(k[a], k[b]); k[a] = lo_; k[b] = hi_; }

// grid ceil(n / 256) x 256, one thread per pixel.  Absent candidates (and directions 4..7 with paths = 4) hold kNone and
// sort last; Batcher's odd-even merge sort of 8 keys, all indices constants, so the keys stay in registers.
template <int PATHS>
__global__ __launch_bounds__(256) void k_fill_select(const short *__restrict__ d, const unsigned *__restrict__ cand, int n, int invalid, int rule, int min_directions,
                                                     short *__restrict__ out, unsigned char *__restrict__ mask)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int res = d[i], m = 0;
    int k[8], cnt = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        k[r] = kNone;
        if (r < PATHS) {
            const unsigned cv = cand[(size_t)r * n + i];
            if (cv >> 16) { k[r] = (int)(short)(cv & 0xffffu); ++cnt; }
        }
    }
    if (res == invalid) {
        TSCM_CX(0, 1) TSCM_CX(2, 3) TSCM_CX(4, 5) TSCM_CX(6, 7)
        TSCM_CX(0, 2) TSCM_CX(1, 3) TSCM_CX(4, 6) TSCM_CX(5, 7)
        TSCM_CX(1, 2) TSCM_CX(5, 6)
        TSCM_CX(0, 4) TSCM_CX(1, 5) TSCM_CX(2, 6) TSCM_CX(3, 7)
        TSCM_CX(2, 4) TSCM_CX(3, 5)
        TSCM_CX(1, 2) TSCM_CX(3, 4) TSCM_CX(5, 6)
        m = 2;
        if (cnt >= min_directions) {                         // min_directions >= 1, so cnt >= 1 here
            const int pick = rule == TSCM_FILL_LOWEST ? 0 : rule == TSCM_FILL_SECOND_LOWEST ? min(1, cnt - 1) : (cnt - 1) >> 1;     // 0..3
            res = pick == 0 ? k[0] : pick == 1 ? k[1] : pick == 2 ? k[2] : k[3];
            m = 1;
        }
    }
    out[i] = (short)res;
    if (mask) mask[i] = (unsigned char)m;
}

// ------------------------------------------------------------------------------------------------ host
int check_fill_args(const short *disparity, int width, int height, int disp_stride, const tscm_stereo_fill_params *p)
{
    if (int rc = check_map_args(disparity, width, height, disp_stride, p, "tscm_stereo_fill_params")) return rc;
    if (p->rule < TSCM_FILL_LOWEST || p->rule > TSCM_FILL_MEDIAN) return tscm_set_error(TSCM_E_INVALID, "params: rule " + std::to_string(p->rule) + " outside 0..2");
    if (p->paths != 4 && p->paths != 8) return tscm_set_error(TSCM_E_INVALID, "params: paths " + std::to_string(p->paths) + " is not 4 or 8");
    if (p->min_directions < 1 || p->min_directions > p->paths)
        return tscm_set_error(TSCM_E_INVALID, "params: min_directions " + std::to_string(p->min_directions) + " outside 1.." + std::to_string(p->paths) + " (paths)");
    if (p->max_distance < 0 || p->max_distance > 32767) return tscm_set_error(TSCM_E_INVALID, "params: max_distance " + std::to_string(p->max_distance) + " outside 0..32767");
    if (p->wrap_x != 0 && p->wrap_x != 1) return tscm_set_error(TSCM_E_INVALID, "params: wrap_x " + std::to_string(p->wrap_x) + " is not 0 or 1");
    if (int rc = check_map_min_disparity(p->min_disparity)) return rc;
    if (width > 32767 || height > 32767)
        return tscm_set_error(TSCM_E_INVALID, "width " + std::to_string(width) + " or height " + std::to_string(height) + " above 32767: distances are int16");
    return 0;
}

// The kernels of one map.  Outputs are host pointers, any of them NULL; the select kernel runs only for `out`.
int fill_run(const short *disparity, int w, int h, int disp_stride, const tscm_stereo_fill_params &p, int device, const char *who, short *out, int out_stride,
             unsigned char *mask, short *value, short *distance, double *seconds_kernel)
{
    if (int rc = select_device(device, who)) return rc;
    const int n = w * h, invalid = 16 * (p.min_disparity - 1), maxd = p.max_distance > 0 ? p.max_distance : INT_MAX;
    DeviceMem mem;
    StageOutputs stages(mem);
    EventSpan span;
    short *d_in = nullptr, *d_out = nullptr;
    unsigned *d_cand = nullptr;
    unsigned char *d_mask = nullptr;
    HIP_TRY(mem.alloc(&d_in, (size_t)n));
    HIP_TRY(mem.alloc(&d_cand, (size_t)p.paths * n));
    if (out) HIP_TRY(mem.alloc(&d_out, (size_t)n));
    if (out) HIP_TRY(stages.scratch(&d_mask, mask, (size_t)n));
    HIP_TRY(copy_rows(d_in, w, disparity, disp_stride, w, h, hipMemcpyHostToDevice));
    HIP_TRY(span.create(2));
    HIP_TRY(span.mark(0));
    hipLaunchKernelGGL(k_fill_rows, dim3((unsigned)((h + 3) / 4), 2), dim3(256), 0, 0, d_in, w, h, invalid, maxd, p.wrap_x, d_cand);
    hipLaunchKernelGGL(k_fill_lines, dim3((unsigned)((w + 63) / 64), (unsigned)(p.paths - 2)), dim3(64), 0, 0, d_in, w, h, invalid, maxd, p.wrap_x, d_cand);
    if (out) {
        auto *const f = p.paths == 4 ? k_fill_select<4> : k_fill_select<8>;
        hipLaunchKernelGGL(f, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, d_cand, n, invalid, p.rule, p.min_directions, d_out, d_mask);
    }
    HIP_TRY(span.finish(1, nullptr, seconds_kernel));
    if (out) HIP_TRY(copy_rows(out, out_stride, d_out, w, w, h, hipMemcpyDeviceToHost));
    HIP_TRY(stages.fetch());
    if (value || distance) {                                 // the packed planes, taken apart on the host
        std::vector<unsigned> c((size_t)p.paths * n);
        HIP_TRY(hipMemcpy(c.data(), d_cand, c.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < c.size(); ++i) {
            const int dist = (int)(c[i] >> 16);
            if (value) value[i] = dist ? (short)(c[i] & 0xffffu) : (short)invalid;
            if (distance) distance[i] = (short)dist;
        }
    }
    return 0;
}

}  // namespace

extern "C" void tscm_stereo_fill_default_params(tscm_stereo_fill_params *p)
{
    if (!p) return;
    p->struct_size = (int)sizeof(tscm_stereo_fill_params);
    p->min_disparity = 0;
    p->rule = TSCM_FILL_MEDIAN;
    p->paths = 8;
    p->max_distance = 0;
    p->min_directions = 1;
    p->wrap_x = 0;
}

extern "C" int tscm_stereo_fill(const short *disparity, int width, int height, int disp_stride, const tscm_stereo_fill_params *params, int device, short *out,
                                int out_stride, unsigned char *mask, double *seconds_kernel)
{
    if (int rc = check_fill_args(disparity, width, height, disp_stride, params)) return rc;
    if (int rc = check_map_out(out, out_stride, width)) return rc;
    if (seconds_kernel) *seconds_kernel = 0.0;
    if (width == 0 || height == 0) return 0;
    return fill_run(disparity, width, height, disp_stride, *params, device, "tscm_stereo_fill", out, out_stride, mask, nullptr, nullptr, seconds_kernel);
}

extern "C" int tscm_stereo_fill_stages(const short *disparity, int width, int height, int disp_stride, const tscm_stereo_fill_params *params, int device,
                                       short *value, short *distance)
{
    if (int rc = check_fill_args(disparity, width, height, disp_stride, params)) return rc;
    if (width == 0 || height == 0) return 0;
    return fill_run(disparity, width, height, disp_stride, *params, device, "tscm_stereo_fill_stages", nullptr, 0, nullptr, value, distance, nullptr);
}
