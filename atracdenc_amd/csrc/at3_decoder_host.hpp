// Host-side core shared by the C-ABI decoders (at1hip_decoder_* in at1hip.hip, at3hip_decoder_* in at3hip.hip,
// at3phip_decoder_* in at3phip.hip) on top of the engine base of at3_host_util.hpp (create prologue, destroy, sync, set_stream,
// last_error, host staging): the table block, the rejection counters and the decode call - everything around the launches.
// Each decoder keeps its configuration checks, buffers, state reset, table builder, parameter structs, kernel launches and
// counter names.
#pragma once
#include "at3_host_util.hpp"

namespace at3host {

// The part of a decoder context every decoder has; a decoder's context derives from it.
struct DecoderBase : EngineBase {
    unsigned long long* d_rejected = nullptr;   // the decoder's rejection counters
    uint8_t* d_in = nullptr;                    // staging for host frames [S][max_frames][bytes per frame], made by *_decoder_create
    float* d_out = nullptr;                     // staging for host output [S][max_frames][elements per frame], likewise (16-bit output uses its first half)
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

// *_decode: the argument check (`extra`: the decoder's flags beyond the three of every call, s16_flag among them), the device
// guard, the frames from host memory (frame_bytes each), launch(d_frames, d_pcm) for the decoder's kernels, and the tail:
// frame_elems float or 16-bit samples per frame to host memory, the wait unless the call is AT3HIP_ASYNC.
template <typename Dec, typename Launch>
int decode_call(Dec* d, const uint8_t* frames, int32_t n_frames, void* pcm, uint32_t flags, uint32_t extra, uint32_t s16_flag,
                size_t frame_bytes, size_t frame_elems, Launch launch)
{
    const uint32_t known = AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE | AT3HIP_ASYNC | extra;
    if (!d || !frames || !pcm || n_frames < 1 || n_frames > d->cfg.max_frames || (flags & ~known))
        return d ? fail(d, AT3HIP_EINVAL, "bad argument") : AT3HIP_EINVAL;
    DeviceGuard guard(d->device);
    HIPCHK(d, guard.error());
    const size_t items = (size_t)d->cfg.n_streams * n_frames;
    const uint8_t* d_frames = nullptr;
    float* d_pcm = nullptr;
    int rc = stage_in(d, d->d_in, 0, frames, items * frame_bytes, flags, &d_frames);   // (both stagings exist since create)
    if (rc == AT3HIP_OK) rc = stage_out(d, d->d_out, 0, (float*)pcm, flags, &d_pcm);
    if (rc == AT3HIP_OK) rc = launch(d_frames, (void*)d_pcm);
    if (rc != AT3HIP_OK) return rc;
    return copy_out_and_wait(d, pcm, d->d_out, items * frame_elems * ((flags & s16_flag) ? sizeof(int16_t) : sizeof(float)), flags);
}

}  // namespace at3host
