// Host-side helpers shared by the C-ABI translation units (at3hip.hip, at1hip.hip, at3phip.hip, resample.hip, loudness.hip):
// error recording, device allocation, the device guard, and the engine base - what every context with one stream (the three
// decoders, the resampler, the loudness meter) does the same way: create prologue, table upload, destroy, sync, set_stream,
// last_error and the tail of a call that gives host memory. The decoders' further shared part is at3_decoder_host.hpp.
#pragma once
#include <cstdio>
#include <initializer_list>
#include <new>

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

// The part of a context every single-stream engine has; an engine's context derives from it.
struct EngineBase {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // own_stream, or the caller's (*_set_stream)
    char err[256] = {0};
};

// *_create after the engine's own configuration checks. Checks device_id, makes the engine on that device with a non-blocking
// stream of its own, then runs setup(e) for its tables, buffers and state. A failure destroys the half-made engine and returns
// the code.
template <typename Eng, typename Destroy, typename Setup>
int create_engine(int device_id, Eng** out, Destroy destroy, Setup setup)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return AT3HIP_EDEVICE;
    if (device_id < 0 || device_id >= ndev) return AT3HIP_EINVAL;
    Eng* e = new (std::nothrow) Eng();
    if (!e) return AT3HIP_ENOMEM;
    e->device = device_id;
    DeviceGuard guard(e->device);
    int rc = AT3HIP_EDEVICE;
    if (guard.error() == hipSuccess && hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking) == hipSuccess) {
        e->stream = e->own_stream;
        rc = setup(e);
    }
    if (rc != AT3HIP_OK) {
        destroy(e);
        return rc;
    }
    *out = e;
    return AT3HIP_OK;
}

// Uploads a table built in pageable host memory: the blocking copy may return once the data is staged, so the device is
// drained before anything on a non-blocking stream can read the table (see at3hip_create).
inline int upload_table(void* dst, const void* src, size_t bytes)
{
    if (hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return AT3HIP_EDEVICE;
    return AT3HIP_OK;
}

// *_destroy of a non-null engine: waits for its stream, frees `bufs` and its own stream, deletes it.
template <typename Eng>
void destroy_engine(Eng* e, std::initializer_list<void*> bufs)
{
    {
        DeviceGuard guard(e->device);
        if (e->stream) (void)hipStreamSynchronize(e->stream);
        for (void* b : bufs)
            if (b) (void)hipFree(b);
        if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
    }
    delete e;
}

inline const char* engine_last_error(const EngineBase* e) { return e ? e->err : "null context"; }

inline int engine_sync(EngineBase* e)
{
    if (!e) return AT3HIP_EINVAL;
    DeviceGuard guard(e->device);
    HIPCHK(e, guard.error());
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return AT3HIP_OK;
}

inline int engine_set_stream(EngineBase* e, void* hip_stream)
{
    if (!e) return AT3HIP_EINVAL;
    DeviceGuard guard(e->device);
    HIPCHK(e, guard.error());
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->stream = hip_stream ? (hipStream_t)hip_stream : e->own_stream;
    return AT3HIP_OK;
}

// The tail of a call that may give host memory: `bytes` from the staging buffer d_out to `out` unless the output stays on the
// device, then the wait for the stream unless the call is AT3HIP_ASYNC.
inline int copy_out_and_wait(EngineBase* e, void* out, const void* d_out, size_t bytes, uint32_t flags)
{
    if (!(flags & AT3HIP_OUT_ON_DEVICE) && bytes) HIPCHK(e, hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, e->stream));
    if (flags & AT3HIP_ASYNC) return AT3HIP_OK;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return AT3HIP_OK;
}

}  // namespace at3host
