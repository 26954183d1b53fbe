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
//   k_pano_reduce, k_pano_lapblend, k_pano_collapse (and k_pano_wsum at create): tscm_pano_kernels.h, shared with the
//                    sweep's composer
//   k_pano_overlap   count / sum of the camera pairs: LDS partials per block, then 64-bit integer atomics
#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include "tscm_host.h"
#include "tscm_pano_kernels.h"
#include "tscm_remap_sample.h"

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

using namespace tscm;

namespace {

constexpr int kMaxCameras = kPanoMaxCameras, kMaxLevels = kPanoMaxLevels;

// ------------------------------------------------------------------------------------------------ sampling
// pack_record, sample_px: tscm_remap_sample.h; Gains, apply_gain: tscm_pano_kernels.h

// grid (ceil(npix / 256), n) x 256: the packed sample and a_k of camera blockIdx.y; weight_mask bit k: camera k has a
// weight image (at wimg + k * w * h), otherwise a constant 255 inside the image
__global__ __launch_bounds__(256) void k_pano_prepare(const float *__restrict__ mapx, const float *__restrict__ mapy, const unsigned char *__restrict__ wimg,
                                                      unsigned weight_mask, int w, int h, size_t npix, size_t plane, uint2 *__restrict__ pack,
                                                      unsigned char *__restrict__ alpha)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (t >= npix) return;
    const uint2 rec = pack_record(mapx[k * npix + t], mapy[k * npix + t], wimg + (size_t)k * w * h, (weight_mask >> k) & 1u, w, h);
    pack[k * plane + t] = rec;
    alpha[k * plane + t] = (unsigned char)(rec.y >> 16);
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
struct tscm_panorama : PyramidLayout {
    int n = 0, w = 0, h = 0, ch = 0, pw = 0, ph = 0, mode = 0, wrap = 0, device = 0;      // levels: 0 unless MULTIBAND
    size_t npix = 0, plane = 0;             // output pixels; the same rounded up to 4
    DeviceMem mem;
    uint2 *pack = nullptr;
    unsigned char *alpha = nullptr, *label = nullptr, *cover = nullptr, *mpyr = nullptr, *img = nullptr, *out = nullptr;
    unsigned short *mask = nullptr, *wsum = nullptr;
    short *G = nullptr, *B = nullptr;
    unsigned long long *acc = nullptr;
    EventSpan span;
};

namespace {

int check_frame(const tscm_panorama *p, const unsigned char *const *images, int stride, const unsigned short *gain_q8, Gains *gains)
{
    if (!p) return tscm_set_error(TSCM_E_INVALID, "p is NULL");
    if (int rc = check_image_list(images, p->n, stride, p->w * p->ch, "width * channels = ")) return rc;
    return check_gains(gain_q8, p->n, gains);
}

int upload_frame(tscm_panorama *p, const unsigned char *const *images, int stride)
{
    HIP_TRY(hipSetDevice(p->device));
    const size_t row = (size_t)p->w * p->ch;
    for (int k = 0; k < p->n; ++k) HIP_TRY(copy_rows(p->img + (size_t)k * row * p->h, row, images[k], stride, row, p->h, hipMemcpyHostToDevice));
    return 0;
}

template <int CH>
void launch_sample(const tscm_panorama *p, const Gains &g, short *G, size_t stride)
{
    hipLaunchKernelGGL(k_pano_sample<CH>, dim3(quad_blocks(p->npix), (unsigned)p->n), dim3(256), 0, 0, p->pack, p->img, p->w, p->h, p->npix, p->plane, g, G, stride);
}

// MULTIBAND up to B^l (collapse == false) or to the output bytes
template <int CH>
void launch_multiband(const tscm_panorama *p, const Gains &g, short *lap, bool collapse)
{
    launch_sample<CH>(p, g, p->G, p->Sp);
    launch_reduce(*p, p->G, p->n * CH, p->wrap);
    launch_blend<CH>(*p, p->G, p->mpyr, p->wsum, p->n, p->wrap, p->B, lap, collapse, p->cover, p->out);
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

int create_on_device(tscm_panorama *p, const unsigned char *const *weights, const float *mapx, const float *mapy)
{
    const int n = p->n;
    const size_t simg = (size_t)p->w * p->h;
    HIP_TRY(p->span.create(2));
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
        launch_reduce(*p, p->mpyr, n, p->wrap);
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
    if (int rc = check_struct_size(params, "tscm_panorama_params")) return rc;
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
    p->mode = params->mode; p->wrap = params->wrap_x ? 1 : 0; p->device = device_index;
    p->npix = (size_t)pano_w * pano_h;
    p->plane = (p->npix + 3) & ~(size_t)3;
    p->set_levels(pano_w, pano_h, L);
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
    HIP_TRY(p->span.mark(0));
    if (p->ch == 1) launch_compose<1>(p, g);
    else launch_compose<3>(p, g);
    HIP_TRY(p->span.finish(1, nullptr, seconds_kernel));
    const size_t row = (size_t)p->pw * p->ch;
    HIP_TRY(copy_rows(dst, dst_stride, p->out, row, row, p->ph, hipMemcpyDeviceToHost));
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
    if (alpha) HIP_TRY(copy_rows(alpha, p->npix, p->alpha, p->plane, p->npix, n, hipMemcpyDeviceToHost));
    if (label) HIP_TRY(hipMemcpy(label, p->label, p->npix, hipMemcpyDeviceToHost));
    if (int rc = download_pyramid(*p, p->mpyr, n, mask_pyramid)) return rc;
    if (int rc = download_pyramid(*p, d_lap, n * ch, lap_pyramid)) return rc;
    return download_pyramid(*p, p->B, ch, blend_pyramid);
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
