// Host-side helpers shared by the C-ABI translation units (at3hip.hip, at1hip.hip, at3phip.hip, resample.hip, loudness.hip):
// error recording, the device guard, and the engine base - what every context (the three encoders, the three decoders, the
// resampler, the loudness meter) does the same way: create prologue, table upload, device allocations the engine owns and
// destroy releases, last_error, the guarded call (null check, device guard, one function), and for those with one stream
// sync, set_stream and the host staging of a call: stage_in (host samples into a staging buffer that the first such call
// allocates), stage_out (where the kernels write) and copy_out_and_wait (the tail of a call that may give host memory). The
// decoders' further shared part is at3_decoder_host.hpp. Outside these on purpose: at3hip_encode's pipelined staging (copy
// stream, parity buffers, events) and at3phip.hip's run_stage, which copy on other streams or bracket the copies with events.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <new>
#include <vector>

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

constexpr int kMaxGridY = 65535;   // gridDim.y / gridDim.z limit of the HIP launch interface

// The part of a context every engine has; an engine's context derives from it.
struct EngineBase {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // own_stream, or the caller's (*_set_stream)
    std::vector<void*> owned;      // what dev_alloc_bytes returned and dev_free has not released: destroy_engine frees it
    char err[256] = {0};
};

// `bytes` of device memory that the engine owns from here on, whenever in its life they are allocated.
inline int dev_alloc_bytes(EngineBase* c, void** p, size_t bytes, const char* what = "hipMalloc")
{
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(c, AT3HIP_ENOMEM, what, e);
    try {
        c->owned.push_back(q);
    } catch (const std::bad_alloc&) {
        (void)hipFree(q);
        return fail(c, AT3HIP_ENOMEM, "out of host memory");
    }
    *p = q;
    return AT3HIP_OK;
}

// `count` elements and a pad of 256 bytes behind them.
template <typename Tp>
int dev_alloc(EngineBase* c, Tp** p, size_t count)
{
    void* q = nullptr;
    const int rc = dev_alloc_bytes(c, &q, count * sizeof(Tp) + 256);
    if (rc == AT3HIP_OK) *p = (Tp*)q;
    return rc;
}

// Releases an allocation of the engine before its destroy does (null: nothing).
inline void dev_free(EngineBase* c, void* p)
{
    for (size_t i = 0; p && i < c->owned.size(); ++i)
        if (c->owned[i] == p) {
            (void)hipFree(p);
            c->owned.erase(c->owned.begin() + i);
            return;
        }
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

// *_create after the engine's own configuration checks. Checks device_id, makes the engine on that device with a stream of its
// own - make_stream(&own_stream), by default a non-blocking one -, then runs setup(e) for its further streams, tables, buffers
// and state. A failure destroys the half-made engine and returns the code.
template <typename Eng, typename Destroy, typename Setup, typename MakeStream>
int create_engine(int device_id, Eng** out, Destroy destroy, Setup setup, MakeStream make_stream)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return AT3HIP_EDEVICE;
    if (device_id < 0 || device_id >= ndev) return AT3HIP_EINVAL;
    Eng* e = new (std::nothrow) Eng();
    if (!e) return AT3HIP_ENOMEM;
    e->device = device_id;
    DeviceGuard guard(e->device);
    int rc = AT3HIP_EDEVICE;
    if (guard.error() == hipSuccess && make_stream(&e->own_stream) == hipSuccess) {
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
template <typename Eng, typename Destroy, typename Setup>
int create_engine(int device_id, Eng** out, Destroy destroy, Setup setup)
{
    return create_engine(device_id, out, destroy, setup, [](hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); });
}

// Uploads a table built in pageable host memory. From pageable memory a blocking copy may return once the data is STAGED: the
// transfer itself may then still run on the null stream, which the contexts' non-blocking streams do not wait for. As a
// precaution - no wrong table has been observed - the device is drained here, once per table, before anything can read it.
inline int upload_table(void* dst, const void* src, size_t bytes)
{
    if (hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return AT3HIP_EDEVICE;
    return AT3HIP_OK;
}

// A table block of a context: allocated on the host, filled by build(block) (false: out of memory), uploaded to a device
// allocation of its own (*d_tables), freed on the host.
template <typename Ctx, typename Tables, typename Build>
int make_device_tables(Ctx* c, Tables** d_tables, Build build)
{
    Tables* host_tables = new (std::nothrow) Tables();
    if (!host_tables) return AT3HIP_ENOMEM;
    int rc = build(host_tables) ? dev_alloc(c, d_tables, 1) : AT3HIP_ENOMEM;
    if (rc == AT3HIP_OK) rc = upload_table(*d_tables, host_tables, sizeof(Tables));
    delete host_tables;
    return rc;
}

// Fills the device array d[0 .. n) with `value` on the engine's stream and waits for it.
inline int fill_and_wait(EngineBase* e, float* d, size_t n, float value)
{
    float* init = (float*)malloc(n * sizeof(float));
    if (!init) return fail(e, AT3HIP_ENOMEM, "malloc");
    for (size_t i = 0; i < n; ++i) init[i] = value;
    hipError_t err = hipMemcpyAsync(d, init, n * sizeof(float), hipMemcpyHostToDevice, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    free(init);
    if (err != hipSuccess) return fail(e, AT3HIP_EDEVICE, "state upload", err);
    return AT3HIP_OK;
}

// *_destroy of a non-null engine, half-made ones included: waits for its stream and for `streams` (further ones of its own),
// frees what it owns, runs destroy_events() for the engine's events, destroys `streams` and its own stream, deletes it.
template <typename Eng, typename DestroyEvents>
void destroy_engine(Eng* e, std::initializer_list<hipStream_t> streams, DestroyEvents destroy_events)
{
    {
        DeviceGuard guard(e->device);
        if (e->stream) (void)hipStreamSynchronize(e->stream);
        for (hipStream_t s : streams)
            if (s) (void)hipStreamSynchronize(s);
        for (void* b : e->owned) (void)hipFree(b);
        destroy_events();
        for (hipStream_t s : streams)
            if (s) (void)hipStreamDestroy(s);
        if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
    }
    delete e;
}
template <typename Eng>
void destroy_engine(Eng* e)
{
    destroy_engine(e, {}, [] {});
}

inline const char* engine_last_error(const EngineBase* e) { return e ? e->err : "null context"; }

// An entry point that is a null check, the device guard and one function of the engine (*_reset, *_sync ...).
template <typename Eng, typename F>
int guarded(Eng* e, F f)
{
    if (!e) return AT3HIP_EINVAL;
    DeviceGuard guard(e->device);
    HIPCHK(e, guard.error());
    return f(e);
}

inline int engine_sync(EngineBase* e)
{
    return guarded(e, [](EngineBase* e) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        return AT3HIP_OK;
    });
}

inline int engine_set_stream(EngineBase* e, void* hip_stream)
{
    return guarded(e, [hip_stream](EngineBase* e) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        e->stream = hip_stream ? (hipStream_t)hip_stream : e->own_stream;
        return AT3HIP_OK;
    });
}

// The staging slot of a call's sample type, of the two a context keeps: float, or 16-bit samples, which cross the bus as they
// are (half the bytes) and are widened by the first kernel's loads.
template <typename T>
T*& pick(float*& f32, int16_t*& s16)
{
    if constexpr (sizeof(T) == sizeof(int16_t)) return s16;
    else return f32;
}

// Where a call reads its `count` input elements: the caller's pointer under AT3HIP_PCM_ON_DEVICE, else the staging buffer
// `slot` of `capacity` elements - allocated here if it is still null - filled from `in` on the engine's stream.
template <typename T>
int stage_in(EngineBase* e, T*& slot, size_t capacity, const T* in, size_t count, uint32_t flags, const T** d_in)
{
    *d_in = in;
    if (flags & AT3HIP_PCM_ON_DEVICE) return AT3HIP_OK;
    if (!slot) {
        const int rc = dev_alloc(e, &slot, capacity);
        if (rc != AT3HIP_OK) return rc;
    }
    HIPCHK(e, hipMemcpyAsync(slot, in, count * sizeof(T), hipMemcpyHostToDevice, e->stream));
    *d_in = slot;
    return AT3HIP_OK;
}

// Where a call's kernels write: the caller's pointer under AT3HIP_OUT_ON_DEVICE, else the staging buffer `slot` of `capacity`
// elements - allocated here if it is still null -, which copy_out_and_wait hands to the host.
template <typename T>
int stage_out(EngineBase* e, T*& slot, size_t capacity, T* out, uint32_t flags, T** d_out)
{
    *d_out = out;
    if (flags & AT3HIP_OUT_ON_DEVICE) return AT3HIP_OK;
    if (!slot) {
        const int rc = dev_alloc(e, &slot, capacity);
        if (rc != AT3HIP_OK) return rc;
    }
    *d_out = slot;
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
