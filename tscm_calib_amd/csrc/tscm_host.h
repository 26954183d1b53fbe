// tscm_host.h -- host plumbing shared by the .hip files: the one error path of HIP calls, device selection, the owners of
// device allocations, timing events and optional stage outputs, the strided copy, and the argument checks that several
// entry points share.  Host code only: the kernel headers do not include it.
#pragma once

#include "tscm/tscm.h"
#include "tscm_spec.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

int tscm_set_error(int code, const std::string &msg);   // tscm_solver.hip: the text of tscm_last_error(); returns code

// tscm_solver.hip: what tscm_eval_normal_equations_weighted and its siblings wrap -- the blocks from the Gram kernel a solve with
// `opt` runs, under the loss and the weights of `in` (spec_args; a mask plays no part in an evaluation)
int tscm_eval_normal_equations_spec(const tscm_problem *p, int device, const tscm_options *opt, const tscm::SolveSpec &in, double *board_gram,
                                    double *board_grad, double *view_cross, double *cam_gram, double *cam_grad, double *cost);

// a service of one .hip file to the others: linked across the library's objects, not exported from it
#define TSCM_INTERNAL __attribute__((visibility("hidden")))

// tscm_solver.hip, for the batched mono route (tscm_mono_batch.hip) and the exchange back-ends (tscm_comm.hip):
namespace tscm { struct CtrlHead; struct IterLog; }
TSCM_INTERNAL double wall();                            // seconds of the steady clock
// the caller's options (NULL: the defaults of a mono / multi solve) in this library's struct; refuses an unknown struct_size
TSCM_INTERNAL int read_options(const tscm_options *opt_in, int mono, tscm_options &opt);
// tscm_spec.h's check_corner_weights with its text in tscm_last_error()
TSCM_INTERNAL int check_corner_weights(const int *view_count, int n_views, const double *w, double *sum = nullptr, long *kept = nullptr);
// a terminated control block and its iteration log as a summary (times excepted); rmse: that of a plain loss, sqrt(2 cost / N)
TSCM_INTERNAL void fill_summary(const tscm::CtrlHead &h, const tscm::IterLog *log, long N, tscm_summary *sum);
// one solve on the calling thread's device, with a checked spec
TSCM_INTERNAL int solve_configured(const tscm_problem *p, const tscm_options *opt, const tscm::SolveSpec &spec, tscm_summary *sum);

// a failed HIP call ends the calling function with TSCM_E_HIP
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return tscm_set_error(TSCM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
    } while (0)

namespace tscm {

// Makes `device` the calling thread's device.  TSCM_E_NO_DEVICE without a HIP runtime or device and for an index outside
// [0, count); `who` names the entry point in the message.
inline int select_device(int device, const char *who)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return tscm_set_error(TSCM_E_NO_DEVICE, std::string("no HIP device available (") + who + " has no CPU fallback)");
    if (device < 0 || device >= n) return tscm_set_error(TSCM_E_NO_DEVICE, std::string(who) + ": device index " + std::to_string(device) + " out of range");
    HIP_TRY(hipSetDevice(device));
    return 0;
}

// Owner of device allocations: a list of pointers that the destructor frees.  The calls return the HIP error; the call
// site chooses the status code (HIP_TRY, or TSCM_E_NOMEM where that is the entry point's answer).
class DeviceMem {
public:
    DeviceMem() = default;
    DeviceMem(const DeviceMem &) = delete;
    DeviceMem &operator=(const DeviceMem &) = delete;
    ~DeviceMem() { for (void *q : ptrs_) (void)hipFree(q); }

    // n elements (never a zero-byte allocation)
    template <typename T>
    hipError_t alloc(T **out, size_t n)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) adopt(q);
        *out = static_cast<T *>(q);
        return e;
    }
    // n elements holding a copy of host[0 .. n)
    template <typename T, typename U>
    hipError_t upload(U **out, const T *host, size_t n)
    {
        T *q = nullptr;
        hipError_t e = alloc(&q, n);
        if (e == hipSuccess && n) e = hipMemcpy(q, host, n * sizeof(T), hipMemcpyHostToDevice);
        *out = q;
        return e;
    }
    template <typename T, typename U>
    hipError_t upload(U **out, const std::vector<T> &host) { return upload(out, host.data(), host.size()); }
    // takes over a pointer allocated elsewhere (fine-grained memory of hipExtMallocWithFlags)
    void adopt(void *q) { ptrs_.push_back(q); }
    // frees one allocation ahead of the destructor; NULL and pointers this object does not own are left alone
    void release(const void *p)
    {
        const auto it = std::find(ptrs_.begin(), ptrs_.end(), p);
        if (it == ptrs_.end()) return;
        (void)hipFree(*it);
        ptrs_.erase(it);
    }

private:
    std::vector<void *> ptrs_;
};

// Owner of the events that time a call on the null stream: create(n) once per call or per handle, mark(i) ahead of stage i,
// finish() behind the last stage.  The destructor destroys the events, on every exit of the caller.
class EventSpan {
public:
    static constexpr int kMaxMarks = 6;
    EventSpan() = default;
    EventSpan(const EventSpan &) = delete;
    EventSpan &operator=(const EventSpan &) = delete;
    ~EventSpan() { for (int i = 0; i < n_; ++i) (void)hipEventDestroy(ev_[i]); }

    hipError_t create(int n)
    {
        if (n > kMaxMarks) return hipErrorInvalidValue;
        for (; n_ < n; ++n_)
            if (const hipError_t e = hipEventCreate(&ev_[n_])) return e;
        return hipSuccess;
    }
    hipError_t mark(int i) { return i >= 0 && i < n_ ? hipEventRecord(ev_[i], 0) : hipErrorInvalidValue; }
    // Records mark `last`, waits for it and asks for the launches' error.  stage[i] (stage may be NULL) = seconds between
    // marks i and i + 1, *total (may be NULL too) = their sum, added in stage order.
    hipError_t finish(int last, double *stage, double *total)
    {
        hipError_t e = mark(last);
        if (e == hipSuccess) e = hipEventSynchronize(ev_[last]);
        if (e == hipSuccess) e = hipGetLastError();
        double sum = 0.0;
        for (int i = 0; i < last && e == hipSuccess; ++i) {
            float ms = 0.f;
            e = hipEventElapsedTime(&ms, ev_[i], ev_[i + 1]);
            if (stage) stage[i] = 1e-3 * ms;
            sum += 1e-3 * ms;
        }
        if (total && e == hipSuccess) *total = sum;
        return e;
    }

private:
    hipEvent_t ev_[kMaxMarks] = {};
    int n_ = 0;
};

// `rows` rows of `width` elements between arrays with row strides in elements; the only hipMemcpy2D.  Row padding of the
// destination (a caller's array, on the way back) keeps its values.
template <typename T>
hipError_t copy_rows(T *dst, size_t dst_stride, const T *src, size_t src_stride, size_t width, size_t rows, hipMemcpyKind kind)
{
    return hipMemcpy2D(dst, dst_stride * sizeof(T), src, src_stride * sizeof(T), width * sizeof(T), rows, kind);
}

// The optional outputs of a call (host pointers of n elements, any of them NULL): scratch() gives the kernels a device array
// for an output that was asked for (of n_alloc > n elements where they write whole quads), from() names a device array
// that exists anyway, fetch() downloads exactly those.
class StageOutputs {
public:
    explicit StageOutputs(DeviceMem &mem) : mem_(mem) {}
    template <typename T>
    hipError_t scratch(T **dev, T *host, size_t n, size_t n_alloc = 0)
    {
        *dev = nullptr;
        if (!host) return hipSuccess;
        const hipError_t e = mem_.alloc(dev, std::max(n, n_alloc));
        if (e == hipSuccess) from(host, *dev, n);
        return e;
    }
    template <typename T>
    void from(T *host, const T *dev, size_t n)
    {
        if (host) items_.push_back({ host, dev, n * sizeof(T) });
    }
    hipError_t fetch() const
    {
        for (const Item &it : items_)
            if (const hipError_t e = hipMemcpy(it.host, it.dev, it.bytes, hipMemcpyDeviceToHost)) return e;
        return hipSuccess;
    }

private:
    struct Item { void *host; const void *dev; size_t bytes; };
    DeviceMem &mem_;
    std::vector<Item> items_;
};

// ---- argument checks that more than one entry point makes, in one wording
template <typename P>
int check_struct_size(const P *p, const char *type, const char *arg = "params")
{
    if (p->struct_size == (int)sizeof(P)) return 0;
    return tscm_set_error(TSCM_E_INVALID, std::string(arg) + ": struct_size " + std::to_string(p->struct_size) + " is not sizeof(" + type + ") = " + std::to_string(sizeof(P)));
}

// what the map stages (filter, fill, refine) ask of their input map and their params ahead of the stage's own fields;
// guide (NULL for a stage without one) points at the guide image's pointer, checked where refine always checked it
template <typename P>
int check_map_args(const short *disparity, int width, int height, int disp_stride, const P *p, const char *type, const unsigned char *const *guide = nullptr,
                   int guide_stride = 0)
{
    if (!disparity) return tscm_set_error(TSCM_E_INVALID, "disparity is NULL");
    if (guide && !*guide) return tscm_set_error(TSCM_E_INVALID, "guide is NULL");
    if (!p) return tscm_set_error(TSCM_E_INVALID, "params is NULL");
    if (width < 0 || height < 0) return tscm_set_error(TSCM_E_INVALID, "negative width or height");
    if (disp_stride < width) return tscm_set_error(TSCM_E_INVALID, "disp_stride " + std::to_string(disp_stride) + " < width " + std::to_string(width));
    if (guide && guide_stride < width) return tscm_set_error(TSCM_E_INVALID, "guide_stride " + std::to_string(guide_stride) + " < width " + std::to_string(width));
    return check_struct_size(p, type);
}

// ... and behind them: the matcher's range at its smallest num_disparities
inline int check_map_min_disparity(int min_disparity)
{
    if (min_disparity >= -2047 && min_disparity <= 2047 - 16) return 0;
    return tscm_set_error(TSCM_E_INVALID, "params: min_disparity " + std::to_string(min_disparity) + " outside -2047..2031, what the matcher accepts");
}

inline int check_map_out(const short *out, int out_stride, int width)
{
    if (!out) return tscm_set_error(TSCM_E_INVALID, "out is NULL");
    if (out_stride < width) return tscm_set_error(TSCM_E_INVALID, "out_stride " + std::to_string(out_stride) + " < width " + std::to_string(width));
    return 0;
}

// n images with rows of `row` bytes; row_name: "width " for grey images, "width * channels = " for colour ones.  The two
// halves are callable on their own for an entry point that checks `channels` between them.
inline int check_image_pointers(const unsigned char *const *images, int n)
{
    if (!images) return tscm_set_error(TSCM_E_INVALID, "images is NULL");
    for (int k = 0; k < n; ++k)
        if (!images[k]) return tscm_set_error(TSCM_E_INVALID, "images[" + std::to_string(k) + "] is NULL");
    return 0;
}
inline int check_image_stride(int stride, int row, const char *row_name)
{
    if (stride < row) return tscm_set_error(TSCM_E_INVALID, "stride " + std::to_string(stride) + " < " + row_name + std::to_string(row));
    return 0;
}
inline int check_image_list(const unsigned char *const *images, int n, int stride, int row, const char *row_name)
{
    if (int rc = check_image_pointers(images, n)) return rc;
    return check_image_stride(stride, row, row_name);
}

// a caller's index map (NULL: the one the handle's tscm_sweep_depth left, if it ran)
inline int check_index_map(const short *index16, int index_stride, bool has_index, int pano_w)
{
    if (!index16 && !has_index) return tscm_set_error(TSCM_E_INVALID, "index16 is NULL and the handle has not run tscm_sweep_depth yet");
    if (index16 && index_stride < pano_w) return tscm_set_error(TSCM_E_INVALID, "index_stride " + std::to_string(index_stride) + " < pano_w " + std::to_string(pano_w));
    return 0;
}

}  // namespace tscm
