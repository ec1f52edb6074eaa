// C ABI of the ATRAC1 encode path (include/at1hip.h): context, device buffers, kernel launches.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include <hip/hip_runtime.h>

#include "../../include/at1hip.h"
#include "at1_kernels.hpp"
#include "at3_host_util.hpp"

using namespace at1;
using at3host::dev_alloc;
using at3host::fail;

static_assert(sizeof(Tables) == AT1HIP_TABLES_BYTES, "at1hip.h documents the table block's size");

struct at1hip_ctx : at3host::EngineBase {   // (no at1hip_set_stream: stream == own_stream)
    at1hip_config cfg;
    hipEvent_t ev[4] = {};
    bool tm_pending = false;      // a call's stage events have not been read yet (AT3HIP_ASYNC)
    Tables* d_tables = nullptr;
    float* d_pcm_in = nullptr;    // staging for host PCM [S][max_blocks][512][nch]
    int16_t* d_pcm_s16 = nullptr; // the same as 16-bit samples, allocated by the first at1hip_encode_short that takes host memory
    float* d_hist = nullptr;      // [S][512][nch] last PCM block of the previous call
    float* d_specs = nullptr;     // [S][B][nch][512]
    float* d_values = nullptr;    // [S][B][nch][512]
    float* d_energy = nullptr;    // [S][B][nch][52]
    uint8_t* d_sfi = nullptr;     // [S][B][nch][64]
    int32_t* d_mask = nullptr;    // [S][B][nch]
    float* d_loud_ch = nullptr;   // [S][B][nch]
    float* d_loud_state = nullptr;  // [S]
    float* d_loud_track = nullptr;  // [S][B]
    uint8_t* d_out = nullptr;     // staging for host output [S][B][nch][212]
    long long blocks_fed = 0;
    int last_blocks = 0;
    at1hip_timings tm = {};
};

namespace {

int reset_state(at1hip_ctx* c)
{
    const size_t S = c->cfg.n_streams;
    HIPCHK(c, hipMemsetAsync(c->d_hist, 0, S * 512 * c->cfg.channels * sizeof(float), c->stream));
    const int rc = at3host::fill_and_wait(c, c->d_loud_state, S, 0.006f);   // LoudFactor, atrac1denc.h:101-102
    if (rc != AT3HIP_OK) return rc;
    c->blocks_fed = 0;
    return AT3HIP_OK;
}

}  // namespace

extern "C" {

int at1hip_create(const at1hip_config* cfg, at1hip_ctx** out)
{
    if (!cfg || !out) return AT3HIP_EINVAL;
    *out = nullptr;
    if ((cfg->channels != 1 && cfg->channels != 2) || cfg->n_streams < 1 || cfg->max_blocks < 1 || cfg->bfu_idx_const < 0 ||
        cfg->bfu_idx_const > 8 || cfg->window_mask < 0 || cfg->window_mask > 7)
        return AT3HIP_EINVAL;
    if ((long long)cfg->n_streams * cfg->channels > at3host::kMaxGridY) return AT3HIP_EINVAL;   // (stream, channel) is gridDim.y
    return at3host::create_engine(cfg->device_id, out, at1hip_destroy, [cfg](at1hip_ctx* c) {
        c->cfg = *cfg;
        for (auto& e : c->ev)
            if (hipEventCreate(&e) != hipSuccess) return AT3HIP_EDEVICE;
        int rc = at3host::make_device_tables(c, &c->d_tables, [](Tables* t) { build_tables(t); return true; });
        if (rc != AT3HIP_OK) return rc;
        const size_t S = cfg->n_streams, B = cfg->max_blocks, C = cfg->channels;
        if ((rc = dev_alloc(c, &c->d_pcm_in, S * B * 512 * C)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_hist, S * 512 * C)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_specs, S * B * C * 512)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_values, S * B * C * 512)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_energy, S * B * C * kMaxBfus)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_sfi, S * B * C * 64)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_mask, S * B * C)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_loud_ch, S * B * C)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_loud_state, S)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_loud_track, S * B)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_out, S * B * C * kFrame)) != AT3HIP_OK) return rc;
        return reset_state(c);
    });
}

void at1hip_destroy(at1hip_ctx* c)
{
    if (c)
        at3host::destroy_engine(c, {}, [c] {
            for (hipEvent_t e : c->ev)
                if (e) (void)hipEventDestroy(e);
        });
}

const char* at1hip_last_error(const at1hip_ctx* c) { return at3host::engine_last_error(c); }

int at1hip_reset(at1hip_ctx* c) { return at3host::guarded(c, reset_state); }

}  // extern "C"

namespace {

// at1hip_encode (T = float) and at1hip_encode_short (T = int16_t): the sample type is the front kernel's and the state kernel's
// template parameter, everything behind them is shared.
template <typename T>
int encode_impl(at1hip_ctx* c, const T* pcm, int32_t n_blocks, uint8_t* out_frames, uint32_t flags)
{
    if (!c || !pcm || !out_frames || n_blocks < 1 || n_blocks > c->cfg.max_blocks)
        return c ? fail(c, AT3HIP_EINVAL, "bad argument") : AT3HIP_EINVAL;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    const size_t S = c->cfg.n_streams, C = c->cfg.channels, F = (size_t)n_blocks;
    hipStream_t st = c->stream;
    const bool timed = !(flags & AT3HIP_ASYNC);   // a queued call carries no stage-timing events (not free between the kernels): its timings read zero
    // 16-bit samples cross the bus as they are (half the bytes) and are widened by the front kernel's loads
    T*& staging = at3host::pick<T>(c->d_pcm_in, c->d_pcm_s16);
    const T* d_pcm = nullptr;
    if (const int rc = at3host::stage_in(c, staging, S * (size_t)c->cfg.max_blocks * 512 * C, pcm, S * F * 512 * C, flags, &d_pcm)) return rc;
    uint8_t* d_out = (flags & AT3HIP_OUT_ON_DEVICE) ? out_frames : c->d_out;

    if (timed) HIPCHK(c, hipEventRecord(c->ev[0], st));
    FrontParams fp;
    fp.T = c->d_tables;
    fp.pcm = d_pcm;
    fp.hist = c->d_hist;
    fp.n_frames = n_blocks;
    fp.nch = (int)C;
    fp.first = c->blocks_fed == 0;
    fp.window_auto = c->cfg.window_auto ? 1 : 0;
    fp.window_mask = c->cfg.window_mask;
    fp.specs = c->d_specs;
    fp.values = c->d_values;
    fp.energy = c->d_energy;
    fp.sfi = c->d_sfi;
    fp.mask = c->d_mask;
    fp.loud_ch = c->d_loud_ch;
    hipLaunchKernelGGL(k_at1_front<T>, dim3((unsigned)F, (unsigned)(S * C)), dim3(64), 0, st, fp);
    HIPCHK(c, hipGetLastError());
    LoudParams lp;
    lp.T = c->d_tables;
    lp.specs = c->d_specs;
    lp.loud_ch = c->d_loud_ch;
    lp.n_units = (int32_t)(S * F * C);
    hipLaunchKernelGGL(k_at1_loud, dim3((unsigned)((S * F * C + kAt1LoudUnits - 1) / kAt1LoudUnits)), dim3(256), 0, st, lp);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_at1_state<T>, dim3((unsigned)((S * 512 * C + 255) / 256)), dim3(256), 0, st, d_pcm, c->d_hist, n_blocks, (int)C,
                       (int)S);
    if (timed) HIPCHK(c, hipEventRecord(c->ev[1], st));

    ScanParams sp;
    sp.mask = c->d_mask;
    sp.loud_ch = c->d_loud_ch;
    sp.loud_state = c->d_loud_state;
    sp.loud_track = c->d_loud_track;
    sp.n_streams = (int)S;
    sp.n_frames = n_blocks;
    sp.nch = (int)C;
    hipLaunchKernelGGL(k_at1_loud_scan, dim3((unsigned)S), dim3(64), 0, st, sp);
    if (timed) HIPCHK(c, hipEventRecord(c->ev[2], st));

    PackParams pp;
    pp.T = c->d_tables;
    pp.values = c->d_values;
    pp.energy = c->d_energy;
    pp.sfi = c->d_sfi;
    pp.mask = c->d_mask;
    pp.loud_track = c->d_loud_track;
    pp.out = d_out;
    pp.n_items = (int)(S * F * C);
    pp.nch = (int)C;
    pp.bfu_idx_const = c->cfg.bfu_idx_const;
    hipLaunchKernelGGL(k_at1_alloc_pack, dim3((unsigned)((S * F * C + 3) / 4)), dim3(256), 0, st, pp);
    HIPCHK(c, hipGetLastError());
    if (timed) HIPCHK(c, hipEventRecord(c->ev[3], st));
    if (!(flags & AT3HIP_OUT_ON_DEVICE))
        HIPCHK(c, hipMemcpyAsync(out_frames, c->d_out, S * F * C * kFrame, hipMemcpyDeviceToHost, st));
    c->blocks_fed += n_blocks;
    c->last_blocks = n_blocks;
    c->tm_pending = timed;
    if (!timed) memset(&c->tm, 0, sizeof(c->tm));
    // AT3HIP_ASYNC: the call is queued (one stream: consecutive calls follow each other on the device without the host in between);
    // at1hip_sync waits and reads the last call's timings
    return (flags & AT3HIP_ASYNC) ? AT3HIP_OK : at1hip_sync(c);
}

}  // namespace

extern "C" {

int at1hip_encode(at1hip_ctx* c, const float* pcm, int32_t n_blocks, uint8_t* out_frames, uint32_t flags)
{
    return encode_impl(c, pcm, n_blocks, out_frames, flags);
}

int at1hip_encode_short(at1hip_ctx* c, const int16_t* pcm, int32_t n_blocks, uint8_t* out_frames, uint32_t flags)
{
    return encode_impl(c, pcm, n_blocks, out_frames, flags);
}

int at1hip_sync(at1hip_ctx* c)
{
    return at3host::guarded(c, [](at1hip_ctx* c) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->tm_pending) {
            c->tm_pending = false;
            (void)hipEventElapsedTime(&c->tm.front_ms, c->ev[0], c->ev[1]);
            (void)hipEventElapsedTime(&c->tm.scan_ms, c->ev[1], c->ev[2]);
            (void)hipEventElapsedTime(&c->tm.pack_ms, c->ev[2], c->ev[3]);
            (void)hipEventElapsedTime(&c->tm.total_ms, c->ev[0], c->ev[3]);
        }
        return AT3HIP_OK;
    });
}

int at1hip_host_tables(void* dst, size_t bytes)
{
    if (!dst || bytes != sizeof(Tables)) return AT3HIP_EINVAL;
    build_tables((Tables*)dst);
    return AT3HIP_OK;
}

int at1hip_get_timings(const at1hip_ctx* c, at1hip_timings* out)
{
    if (!c || !out) return AT3HIP_EINVAL;
    *out = c->tm;
    return AT3HIP_OK;
}

int at1hip_read_tap(at1hip_ctx* c, int32_t kind, void* dst, size_t bytes)
{
    if (!c || !dst) return AT3HIP_EINVAL;
    const size_t S = c->cfg.n_streams, C = c->cfg.channels, F = (size_t)c->last_blocks;
    const void* src = nullptr;
    size_t need = 0;
    switch (kind) {
        case AT1HIP_TAP_SPECTRA: src = c->d_specs; need = S * F * C * 512 * sizeof(float); break;
        case AT1HIP_TAP_MASKS: src = c->d_mask; need = S * F * C * sizeof(int32_t); break;
        case AT1HIP_TAP_LOUDNESS: src = c->d_loud_track; need = S * F * sizeof(float); break;
        case AT1HIP_TAP_TABLES: src = c->d_tables; need = sizeof(Tables); break;
        default: return fail(c, AT3HIP_EINVAL, "unknown tap");
    }
    if (bytes != need || (kind != AT1HIP_TAP_TABLES && F == 0)) return fail(c, AT3HIP_EINVAL, "tap size");
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
    return AT3HIP_OK;
}

}  // extern "C"

// ---- decoder (include/at1hip.h) ------------------------------------------------------------------------------------------------
#include "at3_decoder_host.hpp"
#include "at1_decode.hpp"

struct at1hip_decoder : at3host::DecoderBase {
    at1hip_decoder_config cfg;
    DecTables* d_tables = nullptr;
    float* d_raw = nullptr;        // [S*C][F][512]
    float* d_tails = nullptr;      // [S*C][F][48]
    int32_t* d_modes = nullptr;    // [S*C][F]
    int4* d_lw = nullptr;          // [S*C][F]
    float* d_st_band = nullptr;    // [S*C][512]
    float* d_st_tail = nullptr;    // [S*C][48]
    // (d_in: the units [S][F][C][212], d_out: [S][F][512][C], d_rejected: [2])
};

namespace {

// false when the encoder's table block cannot be allocated (the decoder is then not created)
__attribute__((optnone, noinline)) bool build_dec_tables(DecTables* t)
{
    Tables* enc = new (std::nothrow) Tables();   // the shared entries: the encoder's builder computes them the reference's way
    if (!enc) return false;
    build_tables(enc);
    memcpy(t->qmf_win, enc->qmf_win, sizeof(t->qmf_win));
    memcpy(t->sine, enc->sine, sizeof(t->sine));
    memcpy(t->scale, enc->scale, sizeof(t->scale));
    memcpy(t->tw128, enc->tw128, sizeof(t->tw128));
    memcpy(t->tw64, enc->tw64, sizeof(t->tw64));
    memcpy(t->tw16, enc->tw16, sizeof(t->tw16));
    delete enc;
    t->maxq[0] = t->maxq[1] = 0.0f;
    for (int wl = 2; wl <= 16; ++wl) t->maxq[wl] = 1.0 / (float)((1 << (wl - 1)) - 1);
    // TMIDCT<n>(2n) (TMIDCT(float scale = TN) : TMDCTBase(TN, scale / 2), atrac1denc.h:52-54)
    at3::mdct_sincos(t->cs512, 512, 512.0f);
    at3::mdct_sincos(t->cs256, 256, 256.0f);
    at3::mdct_sincos(t->cs64, 64, 64.0f);
    return true;
}

int dec_reset_state(at1hip_decoder* d)
{
    const size_t SC = (size_t)d->cfg.n_streams * d->cfg.channels;
    HIPCHK(d, hipMemsetAsync(d->d_st_band, 0, SC * 512 * sizeof(float), d->stream));
    HIPCHK(d, hipMemsetAsync(d->d_st_tail, 0, SC * kDecTailLen * sizeof(float), d->stream));
    HIPCHK(d, hipMemsetAsync(d->d_rejected, 0, 2 * sizeof(unsigned long long), d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    return AT3HIP_OK;
}

}  // namespace

extern "C" {

int at1hip_decoder_create(const at1hip_decoder_config* cfg, at1hip_decoder** out)
{
    if (!cfg || !out) return AT3HIP_EINVAL;
    *out = nullptr;
    if ((cfg->channels != 1 && cfg->channels != 2) || cfg->n_streams < 1 || cfg->max_frames < 1) return AT3HIP_EINVAL;
    if ((long long)cfg->n_streams * cfg->channels > at3host::kMaxGridY) return AT3HIP_EINVAL;   // (stream, channel) is gridDim.y
    // every buffer index stays inside size_t and the kernels' int frame counts
    if ((long long)cfg->max_frames * cfg->n_streams * cfg->channels > (1ll << 31) / 512) return AT3HIP_EINVAL;
    return at3host::create_decoder(cfg, out, build_dec_tables, at1hip_decoder_destroy, [](at1hip_decoder* d) {
        const size_t S = d->cfg.n_streams, F = d->cfg.max_frames, C = d->cfg.channels;
        int rc;
        if ((rc = dev_alloc(d, &d->d_in, S * F * C * kFrame)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_raw, S * C * F * 512)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_tails, S * C * F * kDecTailLen)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_modes, S * C * F)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_lw, S * C * F)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_st_band, S * C * 512)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_st_tail, S * C * kDecTailLen)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_rejected, 2)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_out, S * F * 512 * C)) != AT3HIP_OK) return rc;
        return dec_reset_state(d);
    });
}

void at1hip_decoder_destroy(at1hip_decoder* d)
{
    if (d) at3host::destroy_engine(d);
}

const char* at1hip_decoder_last_error(const at1hip_decoder* d) { return at3host::engine_last_error(d); }

int at1hip_decoder_sync(at1hip_decoder* d) { return at3host::engine_sync(d); }

int at1hip_decoder_reset(at1hip_decoder* d) { return at3host::guarded(d, dec_reset_state); }

int at1hip_decoder_set_stream(at1hip_decoder* d, void* hip_stream) { return at3host::engine_set_stream(d, hip_stream); }

int at1hip_decoder_get_counters(at1hip_decoder* d, at1hip_decoder_counters* out, int32_t reset)
{
    if (!d || !out) return AT3HIP_EINVAL;
    unsigned long long h[2] = {0, 0};
    const int rc = at3host::read_counters(d, h, reset);
    if (rc != AT3HIP_OK) return rc;
    out->bad_block_size = h[0];
    out->read_past_end = h[1];
    return AT3HIP_OK;
}

}  // extern "C"

namespace {

// The kernels of one at1hip_decode call: n_frames units per (stream, channel) from d_units into d_pcm, both device memory.
int dec_launch(at1hip_decoder* d, const uint8_t* d_units, int n_frames, void* d_pcm, bool s16)
{
    const size_t C = d->cfg.channels, F = (size_t)n_frames, SC = (size_t)d->cfg.n_streams * C;
    hipStream_t st = d->stream;
    DecBandsParams bp;
    bp.T = d->d_tables;
    bp.units = d_units;
    bp.n_frames = n_frames;
    bp.nch = (int)C;
    bp.raw = d->d_raw;
    bp.tails = d->d_tails;
    bp.modes = d->d_modes;
    bp.rejected = d->d_rejected;
    hipLaunchKernelGGL(k_at1d_bands, dim3((unsigned)F, (unsigned)SC), dim3(128), 0, st, bp);
    HIPCHK(d, hipGetLastError());
    hipLaunchKernelGGL(k_at1d_scan, dim3((unsigned)SC), dim3(kDecScanThreads), 0, st, (const int32_t*)d->d_modes, d->d_lw, n_frames);
    HIPCHK(d, hipGetLastError());
    DecSynthParams sp;
    sp.T = d->d_tables;
    sp.raw = d->d_raw;
    sp.tails = d->d_tails;
    sp.lw = d->d_lw;
    sp.st_band = d->d_st_band;
    sp.st_tail = d->d_st_tail;
    sp.out = d_pcm;
    sp.n_frames = n_frames;
    sp.nch = (int)C;
    sp.s16 = s16 ? 1 : 0;
    hipLaunchKernelGGL(k_at1d_synth, dim3((unsigned)F, (unsigned)SC), dim3(256), 0, st, sp);
    HIPCHK(d, hipGetLastError());
    hipLaunchKernelGGL(k_at1d_state, dim3((unsigned)SC), dim3(256), 0, st, (const float*)d->d_raw, (const float*)d->d_tails,
                       (const int4*)d->d_lw, d->d_st_band, d->d_st_tail, n_frames);
    HIPCHK(d, hipGetLastError());
    return AT3HIP_OK;
}

}  // namespace

extern "C" int at1hip_decode(at1hip_decoder* d, const uint8_t* units, int32_t n_frames, void* pcm, uint32_t flags)
{
    const size_t C = d ? d->cfg.channels : 0;
    return at3host::decode_call(d, units, n_frames, pcm, flags, AT1HIP_DECODE_S16, AT1HIP_DECODE_S16, C * kFrame, 512 * C,
                                [&](const uint8_t* d_units, void* d_pcm) { return dec_launch(d, d_units, n_frames, d_pcm, flags & AT1HIP_DECODE_S16); });
}
