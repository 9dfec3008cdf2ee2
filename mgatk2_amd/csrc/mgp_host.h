// mgp_host.h — what the host code of mgp_engine.hip and mgp_jobs.hip shares (internal):
// the C-ABI's error message and return-code plumbing, and the owning device buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/mgpileup.h"

// the calling thread's message (mgp_last_error reads it); returns `code`. Defined in
// mgp_engine.hip
int set_err(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e__ = (expr);                                                        \
        if (e__ != hipSuccess) {                                                        \
            return set_err(e__ == hipErrorOutOfMemory ? MGP_E_OOM : MGP_E_HIP,          \
                           std::string(#expr) + ": " + hipGetErrorString(e__));         \
        }                                                                               \
    } while (0)

#define MGP_TRY(expr)             \
    do {                          \
        int r__ = (expr);         \
        if (r__ != MGP_OK) return r__; \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t bytes, bool preserve = false, size_t used = 0, hipStream_t s = 0) {
        if (bytes <= cap) return MGP_OK;
        size_t ncap = std::max(bytes, cap + cap / 2);
        ncap = (ncap + 255) & ~size_t(255);
        void* np = nullptr;
        hipError_t e = hipMalloc(&np, ncap);
        if (e != hipSuccess) {
            ncap = (bytes + 255) & ~size_t(255);
            e = hipMalloc(&np, ncap);
            if (e != hipSuccess)
                return set_err(MGP_E_OOM, "hipMalloc(" + std::to_string(ncap) + ") failed: " +
                                              hipGetErrorString(e));
        }
        if (preserve && p && used) {
            HIP_TRY(hipMemcpyAsync(np, p, used, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        if (p) (void)hipFree(p);
        p = np;
        cap = ncap;
        return MGP_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(p); }
};
