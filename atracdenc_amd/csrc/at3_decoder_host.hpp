// Host-side core shared by the C-ABI decoders (at1hip_decoder_* in at1hip.hip, at3hip_decoder_* in at3hip.hip): what a
// decoder does the same way whatever it decodes. Each decoder keeps its configuration checks, buffers, state reset, table
// builder, kernel launches and counter names.
#pragma once
#include <initializer_list>
#include <new>

#include "at3_host_util.hpp"

namespace at3host {

// The part of a decoder context every decoder has; a decoder's context derives from it.
struct DecoderBase {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // own_stream, or the caller's (*_decoder_set_stream)
    unsigned long long* d_rejected = nullptr;   // the decoder's rejection counters
    char err[256] = {0};
};

// *_decoder_create after the decoder's own configuration checks. Checks cfg->device_id, makes the decoder on that device
// with a non-blocking stream of its own, builds its table block on the host with build_tables (false: out of memory) and
// uploads it to d_tables, then runs setup(d) for the decoder's buffers and state. A failure destroys the half-made decoder
// and returns the code.
template <typename Dec, typename Cfg, typename Tables, typename Setup>
int create_decoder(const Cfg* cfg, Dec** out, bool (*build_tables)(Tables*), void (*destroy)(Dec*), Setup setup)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return AT3HIP_EDEVICE;
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return AT3HIP_EINVAL;
    Dec* d = new (std::nothrow) Dec();
    if (!d) return AT3HIP_ENOMEM;
    d->cfg = *cfg;
    d->device = cfg->device_id;
    auto bail = [&](int code) {
        destroy(d);
        return code;
    };
    DeviceGuard guard(d->device);
    if (guard.error() != hipSuccess) return bail(AT3HIP_EDEVICE);
    if (hipStreamCreateWithFlags(&d->own_stream, hipStreamNonBlocking) != hipSuccess) return bail(AT3HIP_EDEVICE);
    d->stream = d->own_stream;
    Tables* host_tables = new (std::nothrow) Tables();
    if (!host_tables) return bail(AT3HIP_ENOMEM);
    int rc = build_tables(host_tables) ? dev_alloc(d, &d->d_tables, 1) : AT3HIP_ENOMEM;
    if (rc == AT3HIP_OK && (hipMemcpy(d->d_tables, host_tables, sizeof(Tables), hipMemcpyHostToDevice) != hipSuccess ||
                            hipDeviceSynchronize() != hipSuccess))   // (pageable source, see at3hip_create)
        rc = AT3HIP_EDEVICE;
    delete host_tables;
    if (rc != AT3HIP_OK || (rc = setup(d)) != AT3HIP_OK) return bail(rc);
    *out = d;
    return AT3HIP_OK;
}

// *_decoder_destroy of a non-null decoder: waits for its stream, frees `bufs` and its own stream, deletes it.
template <typename Dec>
void destroy_decoder(Dec* d, std::initializer_list<void*> bufs)
{
    {
        DeviceGuard guard(d->device);
        if (d->stream) (void)hipStreamSynchronize(d->stream);
        for (void* b : bufs)
            if (b) (void)hipFree(b);
        if (d->own_stream) (void)hipStreamDestroy(d->own_stream);
    }
    delete d;
}

inline const char* decoder_last_error(const DecoderBase* d) { return d ? d->err : "null context"; }

inline int decoder_sync(DecoderBase* d)
{
    if (!d) return AT3HIP_EINVAL;
    DeviceGuard guard(d->device);
    HIPCHK(d, guard.error());
    HIPCHK(d, hipStreamSynchronize(d->stream));
    return AT3HIP_OK;
}

inline int decoder_set_stream(DecoderBase* d, void* hip_stream)
{
    if (!d) return AT3HIP_EINVAL;
    DeviceGuard guard(d->device);
    HIPCHK(d, guard.error());
    HIPCHK(d, hipStreamSynchronize(d->stream));
    d->stream = hip_stream ? (hipStream_t)hip_stream : d->own_stream;
    return AT3HIP_OK;
}

// Reads the decoder's N rejection counters into h, clears them on the device when `reset` is set, and waits for both.
template <size_t N>
int read_counters(DecoderBase* d, unsigned long long (&h)[N], int32_t reset)
{
    DeviceGuard guard(d->device);
    HIPCHK(d, guard.error());
    HIPCHK(d, hipMemcpyAsync(h, d->d_rejected, sizeof(h), hipMemcpyDeviceToHost, d->stream));
    if (reset) HIPCHK(d, hipMemsetAsync(d->d_rejected, 0, sizeof(h), d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    return AT3HIP_OK;
}

}  // namespace at3host
