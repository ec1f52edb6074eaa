// Host-side helpers shared by the three C-ABI translation units (at3hip.hip, at1hip.hip, at3phip.hip).
#pragma once
#include <cstdio>

#include <hip/hip_runtime.h>

#include "../../include/at3hip.h"

namespace at3host {

// Records `what` (with the HIP error string when `e` is an error) as the context's last error and returns `code`.
template <typename Ctx>
int fail(Ctx* c, int code, const char* what, hipError_t e = hipSuccess)
{
    if (c) {
        if (e != hipSuccess) snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString(e));
        else snprintf(c->err, sizeof(c->err), "%s", what);
    }
    return code;
}

#define HIPCHK(c, call)                                                              \
    do {                                                                             \
        hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) return at3host::fail((c), AT3HIP_EDEVICE, #call, e_);  \
    } while (0)

template <typename Ctx, typename Tp>
int dev_alloc(Ctx* c, Tp** p, size_t count)
{
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, count * sizeof(Tp) + 256);
    if (e != hipSuccess) return fail(c, AT3HIP_ENOMEM, "hipMalloc", e);
    *p = (Tp*)q;
    return AT3HIP_OK;
}

// Every entry point works on the device its context was created on, whatever device the calling thread has current
// (torch, another context on another GPU ...), and leaves the caller's current device as it found it.
class DeviceGuard {
public:
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
        err_ = (prev_ == device) ? hipSuccess : hipSetDevice(device);
        changed_ = (err_ == hipSuccess && prev_ != device);
    }
    ~DeviceGuard()
    {
        if (changed_ && prev_ >= 0) (void)hipSetDevice(prev_);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
    hipError_t error() const { return err_; }

private:
    int prev_ = -1;
    bool changed_ = false;
    hipError_t err_ = hipSuccess;
};

constexpr int kMaxGridY = 65535;   // gridDim.y / gridDim.z limit of the HIP launch interface

}  // namespace at3host
