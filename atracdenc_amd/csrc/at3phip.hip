// C ABI of the ATRAC3plus front end (include/at3phip.h): context, device buffers, kernel launches.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include <hip/hip_runtime.h>

#include "../../include/at3phip.h"
#include "at3p_kernels.hpp"
#include "at3p_write.hpp"
#include "at3p_gha.hpp"
#include "at3_host_util.hpp"

using namespace at3p;
using at3host::dev_alloc;
using at3host::fail;

static_assert(sizeof(Tables) == AT3PHIP_TABLES_BYTES, "at3phip.h documents the table block's size");
static_assert(sizeof(WriteTables) == AT3PHIP_WRITE_TABLES_BYTES, "at3phip.h documents the frame writer's table block size");
// at3phip_tonal_block is the writer's record, field for field
static_assert(sizeof(at3phip_tonal_block) == sizeof(TonalBlock) && offsetof(at3phip_tonal_block, tone_sharing) == offsetof(TonalBlock, tone_sharing) &&
                  offsetof(at3phip_tonal_block, band) == offsetof(TonalBlock, band) && offsetof(at3phip_tonal_block, wave) == offsetof(TonalBlock, wave) &&
                  sizeof(at3phip_tonal_band) == 4 && AT3PHIP_TONAL_MAX_WAVES == kTonalMaxWaves && AT3PHIP_TONAL_MAX_BAND_WAVES == kTonalMaxBandWaves,
              "at3phip.h documents the tonal record's layout");
static_assert(sizeof(ToneFindTables) == AT3PHIP_TONE_FIND_TABLES_BYTES, "at3phip.h documents the tone analysis' table block size");
static_assert(AT3PHIP_TONE_MAX_BAND_WAVES == kToneBandWaves && AT3PHIP_TONE_FINE_SPAN == kToneSpan && AT3PHIP_TONE_PEAK_RATIO == 16.0 &&
                  AT3PHIP_TONE_MIN_AMP == 8.0 && AT3PHIP_TONE_GATE_MIN == kToneGateMin && AT3PHIP_TONE_GATE_RATIO == kToneGateRatio,
              "at3phip.h names the constants of at3p_gha.hpp");

struct at3phip_ctx : at3host::EngineBase {   // (no at3phip_set_stream: stream == own_stream)
    at3phip_config cfg;
    hipEvent_t ev[5] = {};
    Tables* d_tables = nullptr;
    float* d_pcm_in = nullptr;     // staging for host PCM   [S][F][2048][nch]
    int16_t* d_pcm_s16 = nullptr;  // the same as 16-bit samples, allocated by the first at3phip_encode_frames_short that takes host memory
    float* d_bands = nullptr;      // subband samples        [S][F][nch][16][128]
    float* d_specs = nullptr;      // staging for host specs [S][F][nch][2048]
    uint16_t* d_flags = nullptr;   // [S][F][nch]
    float* d_pqf_hist = nullptr;   // [S][nch][368]
    float* d_mdct_hist = nullptr;  // [S][nch][16][128]
    WriteTables* d_wtables = nullptr;
    uint8_t* d_frames = nullptr;   // staging for host frames [S][F][2048]
    TonalBlock* d_tonal = nullptr; // the tonal records of a call [S][F], allocated by the first at3phip_write_frames_tonal that has any
    // the tone analysis (at3p_gha.hpp): tables, buffers and state, all set up by the first call that analyses (ensure_tones)
    ToneFindTables* d_tone_tables = nullptr;
    ToneCand* d_tone_cand = nullptr;             // [S][F][nch][16][3]
    TonalBlock* d_tone_blocks = nullptr;         // [S][F]
    TonalBlock* d_tone_writer[2] = {nullptr, nullptr};   // [S][F] each: the writer's records, double-buffered like the spectra
    float* d_tone_resid = nullptr;               // [S][F][nch][16][128]
    float* d_tone_prev = nullptr;                // state: the last frame's subband samples [S][nch][16][128]
    TonalBlock* d_tone_last = nullptr;           // state: the last block [S], then the block before it [S] (its points: GATES)
    // at3phip_encode_frames: the frame writer only needs the spectra of ITS call, so it runs on a stream of its own behind
    // an event and the next call's filter bank and transform overlap it; the spectra in between are double-buffered
    hipStream_t write_stream = nullptr;
    float* d_specs_b[2] = {nullptr, nullptr};
    hipEvent_t ev_specs[2] = {}, ev_write_done[2] = {};
    bool write_done_valid[2] = {false, false};
    long long enc_calls = 0;
    bool ev_from_encode = false;   // the timing events were last recorded by at3phip_encode_frames (at3phip_sync may read all of them)
    float pqf_ms = 0.0f, mdct_ms = 0.0f, write_ms = 0.0f;
    int32_t frame_bytes = kFrameBytes;   // at3phip_set_frame_bytes: `frames` of every frame-writing call is [S][F][frame_bytes]; d_frames is sized for 2048
};

namespace at3p {
// The fixed writer's two instantiations under the names they are launched by. Here and not in at3p_write.hpp: at3p_alloc.hip
// includes that header too, and must not hold a second copy of these kernels.
constexpr auto k_at3p_write = k_at3p_write_with<WriteParams>;
constexpr auto k_at3p_write_tonal = k_at3p_write_with<WriteParamsTonal>;

// The launches of the adaptive writer's kernels (wp.tonal null: without records) and of the sparse unpack kernels (sized: the frame
// size is not 2048). The kernels are translation units of their own - at3p_alloc.hip, at3p_sparse.hip, at3p_rd.hip, at3p_psy.hip - so that this
// one's device code stays instruction for instruction what it was; weak, because the stand-alone host programs that link this file
// without them (tests/test_owned_alloc_cpu.py) must still link: there resolve_alloc_mode and choose_unpack refuse the flags.
__attribute__((weak, visibility("default"))) void launch_write_adaptive(const WriteParamsTonal& wp, int32_t frame_bytes, hipStream_t on);
__attribute__((weak, visibility("default"))) void launch_write_adaptive_sparse(const WriteParamsTonal& wp, int32_t frame_bytes, hipStream_t on);
__attribute__((weak, visibility("default"))) void launch_write_adaptive_rd(const WriteParamsTonal& wp, int32_t frame_bytes, hipStream_t on);
__attribute__((weak, visibility("default"))) void launch_write_adaptive_psy(const WriteParamsTonal& wp, int32_t frame_bytes, hipStream_t on);
struct DecUnpackParams;
__attribute__((weak, visibility("default"))) void launch_unpack_sparse(const DecUnpackParams& up, bool sized, dim3 grid, hipStream_t on);
}

namespace {

#include "at3p_tone_vlc.inc"

int reset_state(at3phip_ctx* c)
{
    const size_t S = c->cfg.n_streams, C = c->cfg.channels;
    HIPCHK(c, hipMemsetAsync(c->d_pqf_hist, 0, S * C * kOverlap * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_mdct_hist, 0, S * C * 2048 * sizeof(float), c->stream));
    if (c->d_tone_last) {   // the tone analysis has been used: a zero frame before the stream, no block
        HIPCHK(c, hipMemsetAsync(c->d_tone_prev, 0, S * C * 2048 * sizeof(float), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_tone_last, 0, 2 * S * sizeof(TonalBlock), c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AT3HIP_OK;
}

// Entry points other than at3phip_encode_frames work on the context's main stream only: whatever asynchronous calls left
// on the writer's stream is waited for first.
int quiesce(at3phip_ctx* c)
{
    if (c->write_stream) HIPCHK(c, hipStreamSynchronize(c->write_stream));
    return AT3HIP_OK;
}

// the setters' last-error text for a size that is not admissible (admissible_frame_bytes, at3p_write.hpp)
struct FrameBytesError {
    char text[96];
};
FrameBytesError frame_bytes_error(int32_t fb, int channels)
{
    FrameBytesError e;
    snprintf(e.text, sizeof(e.text), "frame_bytes %d: not a multiple of 8 in %d..%d", (int)fb, min_frame_bytes(channels), kFrameBytes);
    return e;
}

// How a frame-writing call chooses its word lengths: the fixed table, or one of the adaptive writer's four units.
enum AllocMode { kAllocFixed, kAllocAdaptive, kAllocSparse, kAllocRd, kAllocPsy };
struct AllocWriter {
    void (*launch)(const WriteParamsTonal& wp, int32_t frame_bytes, hipStream_t on);   // null: this build was linked without the unit
    const char *flag, *name, *unit;   // for the refusal's text
};
const AllocWriter kAllocWriters[] = {
    {nullptr, nullptr, nullptr, nullptr},   // kAllocFixed: k_at3p_write, k_at3p_write_tonal
    {launch_write_adaptive, "AT3PHIP_ALLOC_ADAPTIVE", "adaptive", "at3p_alloc.hip"},
    {launch_write_adaptive_sparse, "AT3PHIP_ALLOC_SPARSE", "sparse", "at3p_alloc.hip, at3p_sparse.hip"},
    {launch_write_adaptive_rd, "AT3PHIP_ALLOC_RD", "rate-distortion", "at3p_rd.hip"},
    {launch_write_adaptive_psy, "AT3PHIP_ALLOC_PSY", "masking-weighted", "at3p_psy.hip"},
};

// The allocation mode of a frame-writing call with these flags at the context's frame size, or the call's refusal. The fixed table is
// the reference's and fills 2048 bytes only, so at any other size the call needs AT3PHIP_ALLOC_ADAPTIVE; AT3PHIP_ALLOC_SPARSE counts
// only together with it, AT3PHIP_ALLOC_RD only together with both, AT3PHIP_ALLOC_PSY only together with all three; each needs its writer in the build. Every frame-writing call asks
// directly after its argument checks: a refused call queues nothing, allocates nothing and moves no state.
int resolve_alloc_mode(at3phip_ctx* c, uint32_t flags, AllocMode* mode)
{
    const bool adaptive = flags & AT3PHIP_ALLOC_ADAPTIVE, sparse = flags & AT3PHIP_ALLOC_SPARSE, rd = flags & AT3PHIP_ALLOC_RD,
               psy = flags & AT3PHIP_ALLOC_PSY;
    auto missing = [c](AllocMode m) {
        const AllocWriter& w = kAllocWriters[m];
        char msg[128];
        snprintf(msg, sizeof(msg), "%s: this build has no %s writer (%s)", w.flag, w.name, w.unit);
        return fail(c, AT3HIP_EINVAL, msg);
    };
    if (c->frame_bytes != kFrameBytes) {
        if (!adaptive)
            return fail(c, AT3HIP_EINVAL, "the fixed table is defined for 2048-byte frames only: this context's frame size needs AT3PHIP_ALLOC_ADAPTIVE");
        if (!kAllocWriters[kAllocAdaptive].launch) return missing(kAllocAdaptive);
    }
    if (psy) {
        if (!adaptive || !sparse || !rd)
            return fail(c, AT3HIP_EINVAL, "AT3PHIP_ALLOC_PSY needs AT3PHIP_ALLOC_ADAPTIVE, AT3PHIP_ALLOC_SPARSE and AT3PHIP_ALLOC_RD in the same call");
        if (!kAllocWriters[kAllocPsy].launch) return missing(kAllocPsy);
    }
    if (rd) {
        if (!adaptive || !sparse) return fail(c, AT3HIP_EINVAL, "AT3PHIP_ALLOC_RD needs AT3PHIP_ALLOC_ADAPTIVE and AT3PHIP_ALLOC_SPARSE in the same call");
        if (!kAllocWriters[kAllocRd].launch) return missing(kAllocRd);
    }
    if (sparse) {
        if (!adaptive) return fail(c, AT3HIP_EINVAL, "AT3PHIP_ALLOC_SPARSE needs AT3PHIP_ALLOC_ADAPTIVE in the same call");
        if (!kAllocWriters[kAllocSparse].launch) return missing(kAllocSparse);
    }
    if (adaptive && !kAllocWriters[kAllocAdaptive].launch) return missing(kAllocAdaptive);
    *mode = psy ? kAllocPsy : rd ? kAllocRd : sparse ? kAllocSparse : adaptive ? kAllocAdaptive : kAllocFixed;
    return AT3HIP_OK;
}

template <typename T>
int launch_pqf(at3phip_ctx* c, const T* d_pcm, int n_frames, float* d_bands)
{
    const size_t S = c->cfg.n_streams, C = c->cfg.channels;
    PqfParams pp;
    pp.T = c->d_tables;
    pp.pcm = d_pcm;
    pp.hist = c->d_pqf_hist;
    pp.bands = d_bands;
    pp.n_frames = n_frames;
    pp.nch = (int)C;
    hipLaunchKernelGGL(k_at3p_pqf<T>, dim3((unsigned)n_frames, (unsigned)(S * C)), dim3(256), 0, c->stream, pp);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_at3p_pqf_state<T>, dim3((unsigned)((S * C * kOverlap + 255) / 256)), dim3(256), 0, c->stream, d_pcm, c->d_pqf_hist,
                       n_frames, (int)C, (int)S);
    HIPCHK(c, hipGetLastError());
    return AT3HIP_OK;
}

int launch_mdct(at3phip_ctx* c, const float* d_bands, int n_frames, const uint16_t* win_flags, float* d_specs, uint32_t flags)
{
    const size_t S = c->cfg.n_streams, C = c->cfg.channels;
    if (win_flags) HIPCHK(c, hipMemcpyAsync(c->d_flags, win_flags, S * n_frames * C * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    MdctParams mp;
    mp.T = c->d_tables;
    mp.bands = d_bands;
    mp.flags = win_flags ? c->d_flags : nullptr;
    mp.hist = c->d_mdct_hist;
    mp.specs = d_specs;
    mp.n_frames = n_frames;
    mp.nch = (int)C;
    mp.residual_scale = (flags & AT3PHIP_RESIDUAL_SCALE) ? 1 : 0;
    hipLaunchKernelGGL(k_at3p_mdct, dim3((unsigned)n_frames, (unsigned)(S * C)), dim3(256), 0, c->stream, mp);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_at3p_mdct_state, dim3((unsigned)((S * C * 2048 + 255) / 256)), dim3(256), 0, c->stream, mp, c->d_mdct_hist, (int)S);
    HIPCHK(c, hipGetLastError());
    return AT3HIP_OK;
}

// What a frame-writing call hands to the writer, all device memory but win_flags and tonal.
struct WriteCall {
    const float* d_specs;
    int n_frames;
    const uint16_t* win_flags;           // host memory, or null: sine windows
    uint8_t* d_frames;
    hipStream_t on;
    const at3phip_tonal_block* tonal;    // the call's records [S][n_frames] in host memory, already checked (check_tonal), or null
    const TonalBlock* d_records;         // the same in device memory, as the tone analysis left them (valid by construction), or null
};

// mode: what resolve_alloc_mode gave the call. Without records from either source: the writer without records.
int launch_write(at3phip_ctx* c, AllocMode mode, const WriteCall& w)
{
    const size_t S = c->cfg.n_streams, C = c->cfg.channels;
    if (w.win_flags) HIPCHK(c, hipMemcpyAsync(c->d_flags, w.win_flags, S * w.n_frames * C * sizeof(uint16_t), hipMemcpyHostToDevice, w.on));
    WriteParamsTonal wp;
    wp.W = c->d_wtables;
    wp.specs = w.d_specs;
    wp.flags = w.win_flags ? c->d_flags : nullptr;
    wp.out = w.d_frames;
    wp.nch = (int)C;
    wp.n_items = (int)(S * w.n_frames);
    wp.tonal = w.d_records;
    if (w.tonal && !w.d_records) {
        if (!c->d_tonal) {
            const int rc = dev_alloc(c, &c->d_tonal, S * (size_t)c->cfg.max_frames);
            if (rc != AT3HIP_OK) return rc;
        }
        HIPCHK(c, hipMemcpyAsync(c->d_tonal, w.tonal, S * w.n_frames * sizeof(TonalBlock), hipMemcpyHostToDevice, w.on));
        wp.tonal = c->d_tonal;
    }
    if (wp.tonal) memcpy(wp.tone_vlc, AT3P_TONE_BANDS_VLC, sizeof(wp.tone_vlc));
    if (mode != kAllocFixed) kAllocWriters[mode].launch(wp, c->frame_bytes, w.on);
    else if (wp.tonal) hipLaunchKernelGGL(k_at3p_write_tonal, dim3(wp.n_items), dim3(256), 0, w.on, wp);
    else hipLaunchKernelGGL(k_at3p_write, dim3(wp.n_items), dim3(256), 0, w.on, static_cast<const WriteParams&>(wp));
    HIPCHK(c, hipGetLastError());
    return AT3HIP_OK;
}

// The tone analysis' tables with the host's libm (never constant-folded: optnone), as the decoder's tone tables are built.
__attribute__((optnone, noinline)) void build_tone_find_tables(ToneFindTables* t)
{
    memset(t, 0, sizeof(*t));
    for (int i = 0; i < 2048; ++i) t->sine[i] = (float)sin(2 * M_PI * i / 2048);
    for (int i = 0; i < 256; ++i) t->hann[i] = (float)((1.0f - cos(2 * M_PI * i / 256.0f)) * 0.5f);
    for (int i = 0; i < 64; ++i) t->amp_sf[i] = exp2f((i - 3) / 4.0f);
    const double pi = 3.141592653589793238462643383279502884197169399375105820974944;   // kiss_fft.c:357-363
    for (int i = 0; i < 256; ++i) {
        const double ph = -2 * pi * i / 256;
        t->tw[i].r = (float)cos(ph);
        t->tw[i].i = (float)sin(ph);
    }
    for (int i = 0; i < 64; ++i) {
        const double a = (double)t->amp_sf[i] * exp2(-0.125);
        t->thr[i] = a * a;
    }
    for (int f = 0; f < 1024; ++f) {   // the projections' normalisers: sums over t = 0 .. 255 in order
        double ns = 0, nc = 0;
        for (int k = 0; k < 256; ++k) {
            const int pos = ((k - 128) * f) & 2047;
            const double sn = (double)t->sine[pos], cs = (double)t->sine[(pos + 512) & 2047];
            ns = ns + (double)t->hann[k] * (sn * sn);
            nc = nc + (double)t->hann[k] * (cs * cs);
        }
        t->rs[f] = ns > 0 ? 1.0 / ns : 0.0;
        t->rc[f] = nc > 0 ? 1.0 / nc : 0.0;
    }
}

// Tables, buffers and start-of-stream state of the tone analysis, on the first call that needs them (at3phip_create's runtime
// calls stay what they were).
int ensure_tones(at3phip_ctx* c)
{
    if (c->d_tone_tables) return AT3HIP_OK;
    const size_t S = c->cfg.n_streams, F = c->cfg.max_frames, C = c->cfg.channels;
    int rc;
    if (!c->d_tone_cand && (rc = dev_alloc(c, &c->d_tone_cand, S * F * C * 16 * kToneBandWaves)) != AT3HIP_OK) return rc;
    if (!c->d_tone_blocks && (rc = dev_alloc(c, &c->d_tone_blocks, S * F)) != AT3HIP_OK) return rc;
    for (auto& w : c->d_tone_writer)
        if (!w && (rc = dev_alloc(c, &w, S * F)) != AT3HIP_OK) return rc;
    if (!c->d_tone_resid && (rc = dev_alloc(c, &c->d_tone_resid, S * F * C * 2048)) != AT3HIP_OK) return rc;
    if (!c->d_tone_prev && (rc = dev_alloc(c, &c->d_tone_prev, S * C * 2048)) != AT3HIP_OK) return rc;
    if (!c->d_tone_last && (rc = dev_alloc(c, &c->d_tone_last, 2 * S)) != AT3HIP_OK) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_tone_prev, 0, S * C * 2048 * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_tone_last, 0, 2 * S * sizeof(TonalBlock), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return at3host::make_device_tables(c, &c->d_tone_tables, [](ToneFindTables* t) { build_tone_find_tables(t); return true; });
}

// Steps 1-8 on d_bands: the blocks into d_tone_blocks, the residuals into d_resid, the writer's records (or none) into d_writer.
// flags: AT3PHIP_TONES_GATED (steps G1-G5), AT3PHIP_TONES_SHARED (steps S1-S5; a mono context has nothing to share).
int launch_tones(at3phip_ctx* c, const float* d_bands, int n_frames, float* d_resid, TonalBlock* d_writer, uint32_t flags)
{
    const unsigned S = (unsigned)c->cfg.n_streams, C = (unsigned)c->cfg.channels, F = (unsigned)n_frames;
    const bool gated = (flags & AT3PHIP_TONES_GATED) != 0, shared = (flags & AT3PHIP_TONES_SHARED) != 0 && C == 2;
    ToneParams tp;
    tp.T = c->d_tone_tables;
    tp.bands = d_bands;
    tp.prev_x = c->d_tone_prev;
    tp.cand = c->d_tone_cand;
    tp.blocks = c->d_tone_blocks;
    tp.last = c->d_tone_last;
    tp.writer = d_writer;
    tp.resid = d_resid;
    tp.n_frames = n_frames;
    tp.nch = (int)C;
    tp.n_streams = (int)S;
    tp.gated = gated ? 1 : 0;
    // (slot, four subbands) x (stream, channel)
    if (gated) hipLaunchKernelGGL(k_at3p_tone_find<true>, dim3(F * 4, S * C), dim3(256), 0, c->stream, tp);
    else hipLaunchKernelGGL(k_at3p_tone_find<false>, dim3(F * 4, S * C), dim3(256), 0, c->stream, tp);
    HIPCHK(c, hipGetLastError());
    if (shared) hipLaunchKernelGGL(k_at3p_tone_select<true>, dim3(F, S), dim3(128), 0, c->stream, tp);
    else hipLaunchKernelGGL(k_at3p_tone_select<false>, dim3(F, S), dim3(128), 0, c->stream, tp);
    HIPCHK(c, hipGetLastError());
    if (shared) {
        if (gated) hipLaunchKernelGGL((k_at3p_tone_sub<true, true>), dim3(F, S * C), dim3(256), 0, c->stream, tp);
        else hipLaunchKernelGGL((k_at3p_tone_sub<false, true>), dim3(F, S * C), dim3(256), 0, c->stream, tp);
    } else if (gated) {
        hipLaunchKernelGGL((k_at3p_tone_sub<true, false>), dim3(F, S * C), dim3(256), 0, c->stream, tp);
    } else {
        hipLaunchKernelGGL((k_at3p_tone_sub<false, false>), dim3(F, S * C), dim3(256), 0, c->stream, tp);
    }
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_at3p_tone_state, dim3(S), dim3(256), 0, c->stream, tp, c->d_tone_prev);
    HIPCHK(c, hipGetLastError());
    return AT3HIP_OK;
}

// The contract of at3phip_tonal_block for one record of a context with `channels` channels: null, or the field that breaks it.
const char* check_tonal(const at3phip_tonal_block& t, int channels)
{
    const int nb = t.num_tone_bands;
    if (nb == 0) return nullptr;   // no tonal block: nothing else is read
    if (nb > 16) return "num_tone_bands above 16";
    if (t.second_is_leader > 1) return "second_is_leader above 1";
    if (channels == 1 && t.second_is_leader) return "second_is_leader in a mono context";
    if (channels == 1 && t.tone_sharing) return "tone_sharing in a mono context";
    int at = 0;
    for (int ch = 0; ch < channels; ++ch)
        for (int b = 0; b < nb; ++b) {
            const at3phip_tonal_band& bd = t.band[ch][b];
            if (ch == 1 && ((t.tone_sharing >> b) & 1)) {
                if (bd.n_waves) return "n_waves of a shared band of channel 1";
                continue;
            }
            if (bd.start > 32) return "start above 32 (point 31)";
            if (bd.stop > 32) return "stop above 32 (point 31)";
            if (bd.n_waves > AT3PHIP_TONAL_MAX_BAND_WAVES) return "n_waves above 15";
            if (at + bd.n_waves > AT3PHIP_TONAL_MAX_WAVES) return "more than 48 waves";
            for (int i = 0; i < bd.n_waves; ++i, ++at) {
                if (t.wave[at] >> 21) return "wave outside FreqIndex 0..1023, AmpSf 0..63, PhaseIndex 0..31";
                if (i && (t.wave[at] & 1023u) < (t.wave[at - 1] & 1023u)) return "FreqIndex decreasing within a band";
            }
        }
    return nullptr;
}

// A stage-level entry point (at3phip_pqf_analyse, at3phip_mdct, at3phip_pqf_mdct, at3phip_write_frames): which buffers it
// stages and which of the context's events bracket its launches.
struct StageOut {
    void* host;            // null: an optional output the caller did not ask for
    const void* staging;
    size_t bytes;
};
struct Stage {
    const void* in;        // the input, copied to in_staging unless AT3HIP_PCM_ON_DEVICE
    void* in_staging;
    size_t in_bytes;
    StageOut out[2];       // the outputs, copied from their staging unless AT3HIP_OUT_ON_DEVICE
    int first_ev;          // step k runs between ev[first_ev + k] and ev[first_ev + k + 1] ...
    float at3phip_ctx::*ms[2];   // ... and its time is read into this member (null: no such step)
};

// Runs a stage on the main stream and waits: stage-in, launch(step) per step between its events, stage-out, wait, timings. Of
// the filter bank's and the transform's times the ones this call did not measure read zero.
template <typename Launch>
int run_stage(at3phip_ctx* c, uint32_t flags, const Stage& s, Launch launch)
{
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    if (int qrc = quiesce(c)) return qrc;
    if (!(flags & AT3HIP_PCM_ON_DEVICE)) HIPCHK(c, hipMemcpyAsync(s.in_staging, s.in, s.in_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[s.first_ev], c->stream));
    // (from here the timing events are no longer all at3phip_encode_frames': a later at3phip_sync must not mix them with an older encode's)
    c->ev_from_encode = false;
    for (int step = 0; step < 2 && s.ms[step]; ++step) {
        const int rc = launch(step);
        if (rc != AT3HIP_OK) return rc;
        HIPCHK(c, hipEventRecord(c->ev[s.first_ev + step + 1], c->stream));
    }
    if (!(flags & AT3HIP_OUT_ON_DEVICE))
        for (const StageOut& o : s.out)
            if (o.host) HIPCHK(c, hipMemcpyAsync(o.host, o.staging, o.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bool pqf = false, mdct = false;
    for (int step = 0; step < 2 && s.ms[step]; ++step) {
        (void)hipEventElapsedTime(&(c->*s.ms[step]), c->ev[s.first_ev + step], c->ev[s.first_ev + step + 1]);
        pqf |= s.ms[step] == &at3phip_ctx::pqf_ms;
        mdct |= s.ms[step] == &at3phip_ctx::mdct_ms;
    }
    if (!pqf) c->pqf_ms = 0.0f;
    if (!mdct) c->mdct_ms = 0.0f;
    return AT3HIP_OK;
}

}  // namespace

extern "C" {

int at3phip_create(const at3phip_config* cfg, at3phip_ctx** out)
{
    if (!cfg || !out) return AT3HIP_EINVAL;
    *out = nullptr;
    if ((cfg->channels != 1 && cfg->channels != 2) || cfg->n_streams < 1 || cfg->max_frames < 1) return AT3HIP_EINVAL;
    if ((long long)cfg->n_streams * cfg->channels > at3host::kMaxGridY) return AT3HIP_EINVAL;   // (stream, channel) is gridDim.y
    // (the order counts, see at3hip_create: the main stream with its events, tables and buffers, then the writer's stream with its events)
    return at3host::create_engine(cfg->device_id, out, at3phip_destroy, [cfg](at3phip_ctx* c) {
        c->cfg = *cfg;
        for (auto& e : c->ev)
            if (hipEventCreate(&e) != hipSuccess) return AT3HIP_EDEVICE;
        int rc = at3host::make_device_tables(c, &c->d_tables, [](Tables* t) { build_tables(t); return true; });
        if (rc != AT3HIP_OK) return rc;
        const size_t S = cfg->n_streams, F = cfg->max_frames, C = cfg->channels;
        if ((rc = dev_alloc(c, &c->d_pcm_in, S * F * C * 2048)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_bands, S * F * C * 2048)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_specs, S * F * C * 2048)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_flags, S * F * C)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_pqf_hist, S * C * kOverlap)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_mdct_hist, S * C * 2048)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_frames, S * F * kFrameBytes)) != AT3HIP_OK) return rc;
        c->d_specs_b[0] = c->d_specs;
        if ((rc = dev_alloc(c, &c->d_specs_b[1], S * F * C * 2048)) != AT3HIP_OK) return rc;
        if (hipStreamCreateWithFlags(&c->write_stream, hipStreamNonBlocking) != hipSuccess) return AT3HIP_EDEVICE;
        for (int q = 0; q < 2; ++q)
            if (hipEventCreateWithFlags(&c->ev_specs[q], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&c->ev_write_done[q], hipEventDisableTiming) != hipSuccess)
                return AT3HIP_EDEVICE;
        rc = at3host::make_device_tables(c, &c->d_wtables, [](WriteTables* t) { build_write_tables(t); return true; });
        return rc != AT3HIP_OK ? rc : reset_state(c);
    });
}

void at3phip_destroy(at3phip_ctx* c)
{
    if (c)
        at3host::destroy_engine(c, {c->write_stream}, [c] {
            for (hipEvent_t e : {c->ev[0], c->ev[1], c->ev[2], c->ev[3], c->ev[4], c->ev_specs[0], c->ev_specs[1], c->ev_write_done[0],
                                 c->ev_write_done[1]})
                if (e) (void)hipEventDestroy(e);
        });
}

const char* at3phip_last_error(const at3phip_ctx* c) { return at3host::engine_last_error(c); }

int at3phip_reset(at3phip_ctx* c)
{
    return at3host::guarded(c, [](at3phip_ctx* c) {
        const int qrc = quiesce(c);
        return qrc != AT3HIP_OK ? qrc : reset_state(c);
    });
}

int at3phip_pqf_analyse(at3phip_ctx* c, const float* pcm, int32_t n_frames, float* bands, uint32_t flags)
{
    if (!c || !pcm || !bands || n_frames < 1 || n_frames > c->cfg.max_frames) return c ? fail(c, AT3HIP_EINVAL, "bad argument") : AT3HIP_EINVAL;
    const size_t bytes = (size_t)c->cfg.n_streams * n_frames * c->cfg.channels * 2048 * sizeof(float);
    const float* d_pcm = (flags & AT3HIP_PCM_ON_DEVICE) ? pcm : c->d_pcm_in;
    float* d_bands = (flags & AT3HIP_OUT_ON_DEVICE) ? bands : c->d_bands;
    const Stage stage = {pcm, c->d_pcm_in, bytes, {{bands, c->d_bands, bytes}}, 0, {&at3phip_ctx::pqf_ms}};
    return run_stage(c, flags, stage, [&](int) { return launch_pqf(c, d_pcm, n_frames, d_bands); });
}

int at3phip_mdct(at3phip_ctx* c, const float* bands, int32_t n_frames, const uint16_t* win_flags, float* specs, uint32_t flags)
{
    if (!c || !bands || !specs || n_frames < 1 || n_frames > c->cfg.max_frames) return c ? fail(c, AT3HIP_EINVAL, "bad argument") : AT3HIP_EINVAL;
    const size_t bytes = (size_t)c->cfg.n_streams * n_frames * c->cfg.channels * 2048 * sizeof(float);
    const float* d_bands = (flags & AT3HIP_PCM_ON_DEVICE) ? bands : c->d_bands;
    float* d_specs = (flags & AT3HIP_OUT_ON_DEVICE) ? specs : c->d_specs;
    const Stage stage = {bands, c->d_bands, bytes, {{specs, c->d_specs, bytes}}, 1, {&at3phip_ctx::mdct_ms}};
    return run_stage(c, flags, stage, [&](int) { return launch_mdct(c, d_bands, n_frames, win_flags, d_specs, flags); });
}

int at3phip_pqf_mdct(at3phip_ctx* c, const float* pcm, int32_t n_frames, const uint16_t* win_flags, float* bands, float* specs, uint32_t flags)
{
    if (!c || !pcm || !specs || n_frames < 1 || n_frames > c->cfg.max_frames) return c ? fail(c, AT3HIP_EINVAL, "bad argument") : AT3HIP_EINVAL;
    const size_t bytes = (size_t)c->cfg.n_streams * n_frames * c->cfg.channels * 2048 * sizeof(float);
    const float* d_pcm = (flags & AT3HIP_PCM_ON_DEVICE) ? pcm : c->d_pcm_in;
    const bool out_dev = (flags & AT3HIP_OUT_ON_DEVICE) != 0;
    float* d_bands = (out_dev && bands) ? bands : c->d_bands;   // (the subbands are optional)
    float* d_specs = out_dev ? specs : c->d_specs;
    const Stage stage = {pcm, c->d_pcm_in, bytes, {{bands, c->d_bands, bytes}, {specs, c->d_specs, bytes}}, 0, {&at3phip_ctx::pqf_ms, &at3phip_ctx::mdct_ms}};
    return run_stage(c, flags, stage, [&](int step) {
        return step == 0 ? launch_pqf(c, d_pcm, n_frames, d_bands) : launch_mdct(c, d_bands, n_frames, win_flags, d_specs, flags);
    });
}

int at3phip_write_frames(at3phip_ctx* c, const float* specs, int32_t n_frames, const uint16_t* win_flags, uint8_t* frames, uint32_t flags)
{
    return at3phip_write_frames_tonal(c, specs, n_frames, win_flags, nullptr, frames, flags);
}

int at3phip_write_frames_tonal(at3phip_ctx* c, const float* specs, int32_t n_frames, const uint16_t* win_flags, const at3phip_tonal_block* tonal,
                               uint8_t* frames, uint32_t flags)
{
    if (!c || !specs || !frames || n_frames < 1 || n_frames > c->cfg.max_frames) return c ? fail(c, AT3HIP_EINVAL, "bad argument") : AT3HIP_EINVAL;
    AllocMode mode;
    if (const int rc = resolve_alloc_mode(c, flags, &mode)) return rc;
    // (The records' contract is all that is checked here at every frame size: the smallest admissible sizes,
    // AT3PHIP_MIN_FRAME_BYTES_*, hold the largest tail a record can give beside one unit per channel, so no record needs a tail check.)
    bool any = false;   // records without a block are the writer without records
    if (tonal)
        for (int s = 0; s < c->cfg.n_streams; ++s)
            for (int f = 0; f < n_frames; ++f) {
                const at3phip_tonal_block& t = tonal[(size_t)s * n_frames + f];
                any |= t.num_tone_bands != 0;
                if (const char* why = check_tonal(t, c->cfg.channels)) {
                    char msg[160];
                    snprintf(msg, sizeof(msg), "tonal block of stream %d, frame %d: %s", s, f, why);
                    return fail(c, AT3HIP_EINVAL, msg);
                }
            }
    if (!any) tonal = nullptr;
    const size_t items = (size_t)c->cfg.n_streams * n_frames;
    const float* d_specs = (flags & AT3HIP_PCM_ON_DEVICE) ? specs : c->d_specs;
    uint8_t* d_frames = (flags & AT3HIP_OUT_ON_DEVICE) ? frames : c->d_frames;
    const Stage stage = {specs, c->d_specs, items * c->cfg.channels * 2048 * sizeof(float), {{frames, c->d_frames, items * (size_t)c->frame_bytes}}, 2, {&at3phip_ctx::write_ms}};
    const WriteCall call = {d_specs, n_frames, win_flags, d_frames, c->stream, tonal, nullptr};
    return run_stage(c, flags, stage, [&](int) { return launch_write(c, mode, call); });
}

}  // extern "C"

namespace {

// at3phip_encode_frames (T = float) and at3phip_encode_frames_short (T = int16_t): the sample type is the filter bank's and its
// state kernel's template parameter, everything behind them is shared.
// kTones: at3phip_encode_frames_tonal(_short): the tone analysis between the filter bank and the transform, the transform on
// its residual, the writer with its records.
template <typename T, bool kTones = false>
int encode_frames_impl(at3phip_ctx* c, const T* pcm, int32_t n_frames, uint8_t* frames, uint32_t flags)
{
    if (!c || !pcm || !frames || n_frames < 1 || n_frames > c->cfg.max_frames) return c ? fail(c, AT3HIP_EINVAL, "bad argument") : AT3HIP_EINVAL;
    AllocMode mode;
    if (const int mrc = resolve_alloc_mode(c, flags, &mode)) return mrc;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    if constexpr (kTones) {
        const int rc = ensure_tones(c);
        if (rc != AT3HIP_OK) return rc;
    }
    const size_t items = (size_t)c->cfg.n_streams * n_frames;
    const size_t n = items * c->cfg.channels * 2048;
    const T* d_pcm = nullptr;   // (16-bit samples are widened by the filter bank's loads)
    int rc = at3host::stage_in(c, at3host::pick<T>(c->d_pcm_in, c->d_pcm_s16), (size_t)c->cfg.n_streams * c->cfg.max_frames * c->cfg.channels * 2048,
                               pcm, n, flags, &d_pcm);
    if (rc != AT3HIP_OK) return rc;
    uint8_t* d_frames = (flags & AT3HIP_OUT_ON_DEVICE) ? frames : c->d_frames;
    const int par = (int)(c->enc_calls & 1);
    float* d_specs = c->d_specs_b[par];
    hipStream_t ws = c->write_stream;
    // the writer of the call before the previous one must be done with this parity's spectra
    if (c->write_done_valid[par]) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_write_done[par], 0));
    // the stage timings are events between the kernels and not free (the ATRAC3 path measured ~1.5 us of the dependent chain per record):
    // a call that is only queued carries none - its timings read zero -, a synchronous one carries all five
    const bool timed = !(flags & AT3HIP_ASYNC);
    if (timed) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    rc = launch_pqf(c, d_pcm, n_frames, c->d_bands);
    if (rc != AT3HIP_OK) return rc;
    if (timed) HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    const float* d_mdct_in = c->d_bands;
    if constexpr (kTones) {   // (its time counts as the transform's)
        rc = launch_tones(c, c->d_bands, n_frames, c->d_tone_resid, c->d_tone_writer[par], flags);
        if (rc != AT3HIP_OK) return rc;
        d_mdct_in = c->d_tone_resid;
    }
    rc = launch_mdct(c, d_mdct_in, n_frames, nullptr, d_specs, AT3PHIP_RESIDUAL_SCALE);   // sine windows: EncodeFrame's default Win
    if (rc != AT3HIP_OK) return rc;
    if (timed) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    HIPCHK(c, hipEventRecord(c->ev_specs[par], c->stream));
    HIPCHK(c, hipStreamWaitEvent(ws, c->ev_specs[par], 0));
    if (timed) HIPCHK(c, hipEventRecord(c->ev[4], ws));
    rc = launch_write(c, mode, {d_specs, n_frames, nullptr, d_frames, ws, nullptr, kTones ? c->d_tone_writer[par] : nullptr});
    if (rc != AT3HIP_OK) return rc;
    if (timed) HIPCHK(c, hipEventRecord(c->ev[3], ws));
    if (!(flags & AT3HIP_OUT_ON_DEVICE)) HIPCHK(c, hipMemcpyAsync(frames, c->d_frames, items * (size_t)c->frame_bytes, hipMemcpyDeviceToHost, ws));
    HIPCHK(c, hipEventRecord(c->ev_write_done[par], ws));
    c->write_done_valid[par] = true;
    c->enc_calls++;
    c->ev_from_encode = timed;
    if (!timed) c->pqf_ms = c->mdct_ms = c->write_ms = 0.0f;
    if (flags & AT3HIP_ASYNC) return AT3HIP_OK;   // at3phip_sync is the completion point
    return at3phip_sync(c);
}

}  // namespace

extern "C" {

int at3phip_encode_frames(at3phip_ctx* c, const float* pcm, int32_t n_frames, uint8_t* frames, uint32_t flags)
{
    return encode_frames_impl(c, pcm, n_frames, frames, flags);
}

int at3phip_encode_frames_short(at3phip_ctx* c, const int16_t* pcm, int32_t n_frames, uint8_t* frames, uint32_t flags)
{
    return encode_frames_impl(c, pcm, n_frames, frames, flags);
}

int at3phip_encode_frames_tonal(at3phip_ctx* c, const float* pcm, int32_t n_frames, uint8_t* frames, uint32_t flags)
{
    return encode_frames_impl<float, true>(c, pcm, n_frames, frames, flags);
}

int at3phip_encode_frames_tonal_short(at3phip_ctx* c, const int16_t* pcm, int32_t n_frames, uint8_t* frames, uint32_t flags)
{
    return encode_frames_impl<int16_t, true>(c, pcm, n_frames, frames, flags);
}

int at3phip_analyse_tones(at3phip_ctx* c, const float* bands, int32_t n_frames, at3phip_tonal_block* blocks, float* residual, uint32_t flags)
{
    if (!c || !bands || n_frames < 1 || n_frames > c->cfg.max_frames) return c ? fail(c, AT3HIP_EINVAL, "bad argument") : AT3HIP_EINVAL;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    if (int qrc = quiesce(c)) return qrc;
    int rc = ensure_tones(c);
    if (rc != AT3HIP_OK) return rc;
    const size_t items = (size_t)c->cfg.n_streams * n_frames;
    const size_t bytes = items * c->cfg.channels * 2048 * sizeof(float);
    const float* d_bands = nullptr;
    if ((rc = at3host::stage_in(c, c->d_bands, 0, bands, bytes / sizeof(float), flags, &d_bands)) != AT3HIP_OK) return rc;
    const bool out_dev = (flags & AT3HIP_OUT_ON_DEVICE) != 0;
    float* d_resid = (out_dev && residual) ? residual : c->d_tone_resid;
    c->ev_from_encode = false;
    rc = launch_tones(c, d_bands, n_frames, d_resid, nullptr, flags);
    if (rc != AT3HIP_OK) return rc;
    if (blocks) HIPCHK(c, hipMemcpyAsync(blocks, c->d_tone_blocks, items * sizeof(TonalBlock), hipMemcpyDeviceToHost, c->stream));
    if (residual && !out_dev) HIPCHK(c, hipMemcpyAsync(residual, c->d_tone_resid, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AT3HIP_OK;
}

int at3phip_host_tone_find_tables(void* dst, size_t bytes)
{
    if (!dst || bytes != sizeof(ToneFindTables)) return AT3HIP_EINVAL;
    build_tone_find_tables((ToneFindTables*)dst);
    return AT3HIP_OK;
}

// G1 of include/at3phip.h on the host: k_at3p_tone_find's gate, operation for operation (this file is compiled without contraction)
int at3phip_host_tone_gates(const float* bands, int32_t n_frames, int32_t channels, uint8_t* out)
{
    if (!bands || !out || n_frames < 0 || channels < 1 || channels > 2) return AT3HIP_EINVAL;
    for (size_t i = 0; i < (size_t)n_frames * channels * 16; ++i) {
        const float* x = bands + i * 128;
        double P[33], e[32];
        P[0] = 0.0;
        for (int j = 0; j < 32; ++j) {
            float v = x[4 * j] * x[4 * j];
            v = v + x[4 * j + 1] * x[4 * j + 1];
            v = v + x[4 * j + 2] * x[4 * j + 2];
            v = v + x[4 * j + 3] * x[4 * j + 3];
            e[j] = (double)v;
            P[j + 1] = P[j] + e[j];
        }
        int bs = 0;
        double bd = 0.0, before = 0.0, after = 0.0;
        for (int s = kToneGateMin; s <= 32 - kToneGateMin; ++s) {
            const double b = P[s] / (double)s, a = (P[32] - P[s]) / (double)(32 - s);
            const double d = fabs(a - b);
            if (bs == 0 || d > bd) {
                bs = s;
                bd = d;
                before = b;
                after = a;
            }
        }
        // the loud side holds at least MIN loud cells next to the split: each over R times the quiet side's mean, and not zero
        uint8_t gate = 0;
        if (after >= kToneGateRatio * before && after > 0.0) {
            bool ok = true;
            for (int j = bs; j < bs + kToneGateMin; ++j) ok = ok && e[j] >= kToneGateRatio * before && e[j] > 0.0;
            if (ok) gate = (uint8_t)bs;
        } else if (before >= kToneGateRatio * after && before > 0.0) {
            bool ok = true;
            for (int j = bs - kToneGateMin; j < bs; ++j) ok = ok && e[j] >= kToneGateRatio * after && e[j] > 0.0;
            if (ok) gate = (uint8_t)(0x80 | (bs - 1));
        }
        out[i] = gate;
    }
    return AT3HIP_OK;
}

uint32_t at3phip_host_tone_flags(void)
{
    return AT3PHIP_TONES_GATED | AT3PHIP_TONES_SHARED;
}

int at3phip_sync(at3phip_ctx* c)
{
    return at3host::guarded(c, [](at3phip_ctx* c) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipStreamSynchronize(c->write_stream));
        if (c->ev_from_encode) {
            float a = 0.0f, b = 0.0f, w = 0.0f;
            if (hipEventElapsedTime(&a, c->ev[0], c->ev[1]) == hipSuccess && hipEventElapsedTime(&b, c->ev[1], c->ev[2]) == hipSuccess &&
                hipEventElapsedTime(&w, c->ev[4], c->ev[3]) == hipSuccess) {
                c->pqf_ms = a;
                c->mdct_ms = b;
                c->write_ms = w;
            }
        }
        return AT3HIP_OK;
    });
}

// An admissible size: waits for queued work (a queued call still writes frames of the old size), then only stores the size: the
// staging buffers are sized for 2048 bytes, the upper bound, and stream state does not depend on the size.
int at3phip_set_frame_bytes(at3phip_ctx* c, int32_t frame_bytes)
{
    if (!c) return AT3HIP_EINVAL;
    if (!admissible_frame_bytes(frame_bytes, c->cfg.channels)) return fail(c, AT3HIP_EINVAL, frame_bytes_error(frame_bytes, c->cfg.channels).text);
    const int rc = at3phip_sync(c);
    if (rc != AT3HIP_OK) return rc;
    c->frame_bytes = frame_bytes;
    return AT3HIP_OK;
}

int at3phip_get_frame_bytes(const at3phip_ctx* c, int32_t* frame_bytes)
{
    if (!c || !frame_bytes) return AT3HIP_EINVAL;
    *frame_bytes = c->frame_bytes;
    return AT3HIP_OK;
}

int at3phip_get_write_timing(const at3phip_ctx* c, float* write_ms)
{
    if (!c) return AT3HIP_EINVAL;
    if (write_ms) *write_ms = c->write_ms;
    return AT3HIP_OK;
}

int at3phip_host_write_tables(void* dst, size_t bytes)
{
    if (!dst || bytes != sizeof(WriteTables)) return AT3HIP_EINVAL;
    build_write_tables((WriteTables*)dst);
    return AT3HIP_OK;
}

int at3phip_get_timings(const at3phip_ctx* c, float* pqf_ms, float* mdct_ms)
{
    if (!c) return AT3HIP_EINVAL;
    if (pqf_ms) *pqf_ms = c->pqf_ms;
    if (mdct_ms) *mdct_ms = c->mdct_ms;
    return AT3HIP_OK;
}

int at3phip_host_tables(void* dst, size_t bytes)
{
    if (!dst || bytes != sizeof(Tables)) return AT3HIP_EINVAL;
    build_tables((Tables*)dst);
    return AT3HIP_OK;
}

}  // extern "C"

// ---- decoder (include/at3phip.h, decoder section) ------------------------------------------------------------------------------
#include <cmath>

#include "at3_decoder_host.hpp"
#include "at3p_decode.hpp"

namespace at3p {
// The unpack kernel's two unflagged instantiations under the names they are launched by (here and not in at3p_decode.hpp, which
// at3p_sparse.hip includes too).
constexpr auto k_at3pd_unpack = k_at3pd_unpack_with<false>;
constexpr auto k_at3pd_unpack_sized = k_at3pd_unpack_with<true>;
}

static_assert(sizeof(DecTables) == AT3PHIP_DECODER_TABLES_BYTES, "at3phip.h documents the decoder's table block size");
static_assert(sizeof(DecToneTables) == AT3PHIP_DECODER_TONE_TABLES_BYTES, "at3phip.h documents the tone table block size");

struct at3phip_decoder : at3host::DecoderBase {
    at3phip_decoder_config cfg;
    DecTables* d_tables = nullptr;
    float* d_raw = nullptr;        // [F + 2][S][C][16][256]: slots 0, 1 = the carried frames -2, -1
    uint16_t* d_flags = nullptr;   // [F + 2][S][C]
    TonalRec* d_tonal = nullptr;   // [F + 3][S]: slots 0 .. 2 = the carried records of frames -3 .. -1
    DecToneTables* d_tone_tables = nullptr;
    int32_t frame_bytes = 2048;    // at3phip_decoder_set_frame_bytes: `frames` of at3phip_decode is [S][F][frame_bytes]; d_in is sized for 2048
    // (d_in: the frames [S][F][2048], d_out: [S][F][2048][C], d_rejected: [kDecReasons])
};

namespace {

#include "at3p_mant.inc"

// The tone synthesis' tables as ff_atrac3p_init_dsp_static builds them, with the host's libm (never constant-folded: optnone).
__attribute__((optnone, noinline)) void build_decp_tone_tables(DecToneTables* t)
{
    memset(t, 0, sizeof(*t));
    for (int i = 0; i < 2048; ++i) t->sine[i] = (float)sin(2 * M_PI * i / 2048);
    for (int i = 0; i < 256; ++i) t->hann[i] = (float)((1.0f - cos(2 * M_PI * i / 256.0f)) * 0.5f);
    for (int i = 0; i < 64; ++i) t->amp_sf[i] = exp2f((i - 3) / 4.0f);
    memcpy(t->vlc, AT3P_TONE_BANDS_VLC, sizeof(t->vlc));
}

// The decoder's table block: the shared entries from the encoder's builder, the cosines of the synthesis's DCT-IV with the
// host's libm (never constant-folded: optnone), and the two-level VLC look-up expanded from the frame writer's code tables.
// false when the encoder's table block cannot be allocated (the decoder is then not created).
__attribute__((optnone, noinline)) bool build_decp_tables(DecTables* t)
{
    memset(t, 0, sizeof(*t));
    Tables* enc = new (std::nothrow) Tables();
    if (!enc) return false;
    build_tables(enc);
    memcpy(t->fir, enc->fir, sizeof(t->fir));
    memcpy(t->tw64, enc->tw64, sizeof(t->tw64));
    memcpy(t->sine128, enc->sine128, sizeof(t->sine128));
    memcpy(t->sine64, enc->sine64, sizeof(t->sine64));
    delete enc;
    for (int k = 0; k < 16; ++k)
        for (int n = 0; n < 16; ++n) t->cos16[k][n] = cos((M_PI / 16) * ((double)n + 0.5) * ((double)k + 0.5));
    at3::mdct_sincos(t->cs256, 256, 128.0f);   // TMIDCT<256>(): TMIDCT(float scale = TN) : TMDCTBase(TN, scale / 2)
    memcpy(t->mant, AT3P_MANT, sizeof(t->mant));
    memcpy(t->scale, AT3P_SCALE, sizeof(t->scale));
    memcpy(t->spec_tab, AT3P_SPEC_TAB, sizeof(t->spec_tab));
    memcpy(t->wl_vlc, AT3P_WL_VLC, sizeof(t->wl_vlc));
    memcpy(t->qu_to_sb, AT3P_QU_TO_SB, sizeof(t->qu_to_sb));
    memcpy(t->sb_powgrps, AT3P_SB_POWGRPS, sizeof(t->sb_powgrps));
    int blocks = 0;
    for (int tb = 0; tb < 56; ++tb) {
        for (int sym = 0; sym < AT3P_VLC_OFF[tb + 1] - AT3P_VLC_OFF[tb]; ++sym) {
            const uint16_t e = AT3P_VLC[AT3P_VLC_OFF[tb] + sym];
            const int len = e >> 12, code = e & 0xfff;
            const uint16_t entry = (uint16_t)(sym | (len << 8));
            if (!len) continue;
            if (len <= 8) {
                for (int x = 0; x < (1 << (8 - len)); ++x) t->lut1[tb][(code << (8 - len)) | x] = entry;
                continue;
            }
            const int pre = code >> (len - 8);
            if (!(t->lut1[tb][pre] & 0x8000u)) {
                if (blocks == kDecLut2Blocks) return false;
                t->lut1[tb][pre] = (uint16_t)(0x8000u | blocks++);
            }
            uint16_t* blk = t->lut2[t->lut1[tb][pre] & 0x7fffu];
            const int low = code & ((1 << (len - 8)) - 1);   // the code's bits after the first 8
            for (int x = 0; x < (1 << (12 - len)); ++x) blk[(low << (12 - len)) | x] = entry;
        }
    }
    return true;
}

int decp_reset_state(at3phip_decoder* d)
{
    const size_t S = d->cfg.n_streams, C = d->cfg.channels;
    HIPCHK(d, hipMemsetAsync(d->d_raw, 0, 2 * S * C * 4096 * sizeof(float), d->stream));
    HIPCHK(d, hipMemsetAsync(d->d_flags, 0, 2 * S * C * sizeof(uint16_t), d->stream));
    HIPCHK(d, hipMemsetAsync(d->d_tonal, 0, kTonalCarry * S * sizeof(TonalRec), d->stream));   // no tonal block
    HIPCHK(d, hipMemsetAsync(d->d_rejected, 0, kDecReasons * sizeof(unsigned long long), d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    return AT3HIP_OK;
}

}  // namespace

extern "C" {

int at3phip_decoder_create(const at3phip_decoder_config* cfg, at3phip_decoder** out)
{
    if (!cfg || !out) return AT3HIP_EINVAL;
    *out = nullptr;
    if ((cfg->channels != 1 && cfg->channels != 2) || cfg->n_streams < 1 || cfg->max_frames < 1) return AT3HIP_EINVAL;
    if ((long long)cfg->n_streams * cfg->channels > at3host::kMaxGridY) return AT3HIP_EINVAL;   // (stream, channel) is gridDim.y
    // every buffer index stays inside size_t and the kernels' int frame counts
    if (((long long)cfg->max_frames + 2) * cfg->n_streams * cfg->channels > (1ll << 31) / 16) return AT3HIP_EINVAL;
    return at3host::create_decoder(cfg, out, build_decp_tables, at3phip_decoder_destroy, [](at3phip_decoder* d) {
        const size_t S = d->cfg.n_streams, F = d->cfg.max_frames, C = d->cfg.channels;
        int rc;
        if ((rc = dev_alloc(d, &d->d_in, S * F * 2048)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_raw, (F + 2) * S * C * 4096)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_flags, (F + 2) * S * C)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_rejected, kDecReasons)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_tonal, (F + kTonalCarry) * S)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_tone_tables, 1)) != AT3HIP_OK) return rc;
        {
            DecToneTables* h = new (std::nothrow) DecToneTables();
            if (!h) return fail(d, AT3HIP_ENOMEM, "out of host memory");
            build_decp_tone_tables(h);
            hipError_t e = hipMemcpy(d->d_tone_tables, h, sizeof(DecToneTables), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipDeviceSynchronize();   // (pageable source, as the decoder's table block)
            delete h;
            HIPCHK(d, e);
        }
        if ((rc = dev_alloc(d, &d->d_out, S * F * 2048 * C)) != AT3HIP_OK) return rc;
        return decp_reset_state(d);
    });
}

void at3phip_decoder_destroy(at3phip_decoder* d)
{
    if (d) at3host::destroy_engine(d);
}

const char* at3phip_decoder_last_error(const at3phip_decoder* d) { return at3host::engine_last_error(d); }

int at3phip_decoder_sync(at3phip_decoder* d) { return at3host::engine_sync(d); }

int at3phip_decoder_reset(at3phip_decoder* d) { return at3host::guarded(d, decp_reset_state); }

int at3phip_decoder_set_stream(at3phip_decoder* d, void* hip_stream) { return at3host::engine_set_stream(d, hip_stream); }

int at3phip_decoder_get_counters(at3phip_decoder* d, at3phip_decoder_counters* out, int32_t reset)
{
    if (!d || !out) return AT3HIP_EINVAL;
    unsigned long long h[kDecReasons] = {0, 0, 0, 0, 0, 0};
    const int rc = at3host::read_counters(d, h, reset);
    if (rc != AT3HIP_OK) return rc;
    out->bad_header = h[0];
    out->unsupported_syntax = h[1];
    out->tonal_present = h[2];
    out->bad_code = h[3];
    out->read_past_end = h[4];
    out->no_terminator = h[5];
    return AT3HIP_OK;
}

}  // extern "C"

namespace {

// The unpack kernel of an at3phip_decode call. The parse is one lane's serial code, so AT3PHIP_DECODE_SPARSE and a frame size other
// than 2048 select instantiations of their own and are no tests in the kernel; the sparse two are in at3p_sparse.hip as the sparse
// writer is, and a build without it refuses the flag.
enum Unpack { kUnpack, kUnpackSized, kUnpackSparse, kUnpackSparseSized };
int choose_unpack(at3phip_decoder* d, uint32_t flags, Unpack* unpack)
{
    const bool sized = d->frame_bytes != 2048;
    if (!(flags & AT3PHIP_DECODE_SPARSE)) *unpack = sized ? kUnpackSized : kUnpack;
    else if (launch_unpack_sparse) *unpack = sized ? kUnpackSparseSized : kUnpackSparse;
    else return fail(d, AT3HIP_EINVAL, "AT3PHIP_DECODE_SPARSE: this build has no sparse unpack kernels (at3p_sparse.hip)");
    return AT3HIP_OK;
}

// The kernels of one at3phip_decode call: n_frames frames per stream from d_frames into d_pcm, both device memory.
int decp_launch(at3phip_decoder* d, const uint8_t* d_frames, int n_frames, void* d_pcm, uint32_t flags, Unpack unpack)
{
    const size_t S = d->cfg.n_streams, F = (size_t)n_frames, C = d->cfg.channels;
    const int tones = (flags & AT3PHIP_DECODE_TONES) ? 1 : 0;
    hipStream_t st = d->stream;
    DecUnpackParams up;
    up.T = d->d_tables;
    up.frames = d_frames;
    up.frame_bytes = d->frame_bytes;
    up.n_frames = n_frames;
    up.n_streams = (int)S;
    up.nch = (int)C;
    up.raw = d->d_raw;
    up.flags = d->d_flags;
    up.rejected = d->d_rejected;
    up.tonal = d->d_tonal;
    up.tone_vlc = d->d_tone_tables->vlc;
    up.tones = tones;
    const dim3 grid((unsigned)F, (unsigned)S);
    if (unpack == kUnpack) hipLaunchKernelGGL(k_at3pd_unpack, grid, dim3(kDecUnpackThreads), 0, st, up);
    else if (unpack == kUnpackSized) hipLaunchKernelGGL(k_at3pd_unpack_sized, grid, dim3(kDecUnpackThreads), 0, st, up);
    else launch_unpack_sparse(up, unpack == kUnpackSparseSized, grid, st);
    HIPCHK(d, hipGetLastError());
    DecSynthParams sp;
    sp.T = d->d_tables;
    sp.raw = d->d_raw;
    sp.flags = d->d_flags;
    sp.out = d_pcm;
    sp.n_frames = n_frames;
    sp.n_streams = (int)S;
    sp.nch = (int)C;
    sp.s16 = (flags & AT3PHIP_DECODE_S16) ? 1 : 0;
    sp.tonal = d->d_tonal;
    sp.TT = d->d_tone_tables;
    sp.tones = tones;
    hipLaunchKernelGGL(k_at3pd_synth, dim3((unsigned)F, (unsigned)(S * C)), dim3(256), 0, st, sp);
    HIPCHK(d, hipGetLastError());
    hipLaunchKernelGGL(k_at3pd_state, dim3((unsigned)(S * C)), dim3(256), 0, st, d->d_raw, d->d_flags, d->d_tonal, n_frames, (int32_t)S,
                       (int32_t)C);
    HIPCHK(d, hipGetLastError());
    return AT3HIP_OK;
}

}  // namespace

extern "C" {

int at3phip_decode(at3phip_decoder* d, const uint8_t* frames, int32_t n_frames, void* pcm, uint32_t flags)
{
    Unpack unpack = kUnpack;
    if (d)
        if (const int rc = choose_unpack(d, flags, &unpack)) return rc;
    return at3host::decode_call(d, frames, n_frames, pcm, flags, AT3PHIP_DECODE_S16 | AT3PHIP_DECODE_TONES | AT3PHIP_DECODE_SPARSE, AT3PHIP_DECODE_S16,
                                d ? (size_t)d->frame_bytes : 0, d ? (size_t)2048 * d->cfg.channels : 0,
                                [&](const uint8_t* d_frames, void* d_pcm) { return decp_launch(d, d_frames, n_frames, d_pcm, flags, unpack); });
}

// As at3phip_set_frame_bytes: an admissible size waits for queued work, then is stored.
int at3phip_decoder_set_frame_bytes(at3phip_decoder* d, int32_t frame_bytes)
{
    if (!d) return AT3HIP_EINVAL;
    if (!admissible_frame_bytes(frame_bytes, d->cfg.channels)) return fail(d, AT3HIP_EINVAL, frame_bytes_error(frame_bytes, d->cfg.channels).text);
    const int rc = at3host::engine_sync(d);
    if (rc != AT3HIP_OK) return rc;
    d->frame_bytes = frame_bytes;
    return AT3HIP_OK;
}

int at3phip_decoder_get_frame_bytes(const at3phip_decoder* d, int32_t* frame_bytes)
{
    if (!d || !frame_bytes) return AT3HIP_EINVAL;
    *frame_bytes = d->frame_bytes;
    return AT3HIP_OK;
}

int at3phip_decoder_host_tables(void* dst, size_t bytes)
{
    if (!dst || bytes != sizeof(DecTables)) return AT3HIP_EINVAL;
    DecTables* t = new (std::nothrow) DecTables();
    if (!t) return AT3HIP_ENOMEM;
    const bool ok = build_decp_tables(t);
    if (ok) memcpy(dst, t, sizeof(DecTables));
    delete t;
    return ok ? AT3HIP_OK : AT3HIP_ENOMEM;
}

int at3phip_decoder_host_tone_tables(void* dst, size_t bytes)
{
    if (!dst || bytes != sizeof(DecToneTables)) return AT3HIP_EINVAL;
    build_decp_tone_tables((DecToneTables*)dst);
    return AT3HIP_OK;
}

}  // extern "C"
