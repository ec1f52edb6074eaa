// Host-side core shared by the C-ABI decoders (at1hip_decoder_* in at1hip.hip, at3hip_decoder_* in at3hip.hip,
// at3phip_decoder_* in at3phip.hip) on top of the engine base of at3_host_util.hpp (create prologue, destroy, sync, set_stream,
// last_error): the table block and the rejection counters. Each decoder keeps its configuration checks, buffers, state reset,
// table builder, kernel launches and counter names.
#pragma once
#include "at3_host_util.hpp"

namespace at3host {

// The part of a decoder context every decoder has; a decoder's context derives from it.
struct DecoderBase : EngineBase {
    unsigned long long* d_rejected = nullptr;   // the decoder's rejection counters
};

// *_decoder_create after the decoder's own configuration checks: create_engine on cfg->device_id, whose setup makes the
// decoder's table block d_tables with build_tables (false: out of memory), then runs setup(d) for the decoder's buffers and
// state.
template <typename Dec, typename Cfg, typename Tables, typename Setup>
int create_decoder(const Cfg* cfg, Dec** out, bool (*build_tables)(Tables*), void (*destroy)(Dec*), Setup setup)
{
    return create_engine(cfg->device_id, out, destroy, [&](Dec* d) {
        d->cfg = *cfg;
        const int rc = make_device_tables(d, &d->d_tables, build_tables);
        return rc != AT3HIP_OK ? rc : setup(d);
    });
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
