// tscm_host.h -- host plumbing shared by the .hip files: the one error path of HIP calls, device selection, and the
// owner of device allocations.  Host code only: the kernel headers do not include it.
#pragma once

#include "tscm/tscm.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

int tscm_set_error(int code, const std::string &msg);   // tscm_solver.hip: the text of tscm_last_error(); returns code

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

}  // namespace tscm
