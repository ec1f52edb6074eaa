// libat3hip: C-ABI host layer (include/at3hip.h) over the gfx950 kernels. No CPU fallback: every
// compute entry point launches HIP kernels; failures are reported as error codes.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "../../include/at3hip.h"
#include "at3_common.hpp"
#include "at3_host_util.hpp"
#include "at3_k_backend.hpp"
#include "at3_k_alloc.hpp"
#include "at3_k_frontend.hpp"
#include "at3_k_front2.hpp"
#include "at3_k_gain.hpp"

using namespace at3;
using at3host::dev_alloc;
using at3host::fail;

namespace {

const struct {
    uint32_t bitrate;
    uint16_t frame_sz;
    uint8_t js;
} kContainer[8] = {{66150, 192, 1},  {93713, 272, 1},  {104738, 304, 0}, {132300, 384, 0},
                   {146081, 424, 0}, {176400, 512, 0}, {264600, 768, 0}, {352800, 1024, 0}};  // atrac3.h:211-220

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

}  // namespace

// AT3HIP_TAP_CLOCK: 16 words, of which k_alloc_pack writes words 0 and 1
constexpr size_t kClkWords = 16;
struct at3hip_ctx : at3host::EngineBase {
    // An event of the context's own, and whether anything has been recorded on it yet: waiting for a fresh one is no call at all.
    struct Event {
        hipEvent_t ev = nullptr;
        bool recorded = false;
        hipError_t record(hipStream_t s)
        {
            const hipError_t e = hipEventRecord(ev, s);
            if (e == hipSuccess) recorded = true;
            return e;
        }
        hipError_t make_wait(hipStream_t s) const { return recorded ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }   // `s` waits for the last record
        hipError_t host_wait() const { return recorded ? hipEventSynchronize(ev) : hipSuccess; }
    };

    at3hip_config cfg;
    int frame_sz = 0;
    int js = 0;
    // The M/S matrixing (atrac3denc.cpp:665-677) runs for two input channels only. A one-channel context in a joint-stereo container takes
    // its (x, x) pairs through the front half unmatrixed, as the reference does: (x + x) * 0.5 is x only while x + x is finite, and a subband
    // sample above FLT_MAX / 2 (input near +-FLT_MAX) would leave the front half as an infinity the reference never forms. The second
    // channel is then a copy of the first; the rate / pack kernel replaces its sound unit by the empty element either way (mono_js).
    int ms = 0;
    // The back half of call N only consumes what the front half of call N produced (spectra, curves, energy scales),
    // and the front half of call N+1 only depends on the front half of call N (carried state): the two halves run on
    // HIP streams of their own (three with gain control, see mid_stream below), buffers that cross between them are double-buffered by call parity, and consecutive calls overlap.
    // (EngineBase::stream: the front half - QMF, gain control, fused QMF+MDCT, carried state)
    hipStream_t back_stream = nullptr;   // back half: psychoacoustics, quantisation, rate loop, packing
    // With gain control the front half is two stages: the heavy one (QMF, spectra of the gain analysis, upsampled envelopes)
    // depends only on the PCM, the light one (curve context scan, curves, energy scales, MDCT) on it and on the previous
    // call's light stage. The light stage is a chain of short latency-bound kernels; on a stream of its own it runs under
    // the next call's heavy stage and the current call's back half instead of holding the GPU nearly idle between them.
    hipStream_t mid_stream = nullptr;
    // Host PCM: staged through a copy stream into device staging that is double-buffered by call parity, so that the
    // H2D copy of call N+1 runs beside the kernels of call N (pinned host memory: at3hip_host_alloc).
    hipStream_t h2d_stream = nullptr;

    // ---- events; the context owns all of them but the two `*_of` handles (for_each_event lists them in creation order) ----
    hipEvent_t ev_h2d[2] = {};           // by call parity: the parity's PCM has arrived in its staging (copy stream -> front stream)
    Event pcm_free[2];                   // by call parity: the staging has been consumed, the front half is done with it (front stream -> copy stream)
    static constexpr int kSlots = 32;    // timing history (events per call)
    hipEvent_t ev[kSlots][8] = {};       // a call's stage timestamps
    Event front_done;                    // everything the most recent call queued on `stream` when that is the caller's (at3hip_destroy)
    hipEvent_t ev_heavy_done[kSlots] = {}, ev_mdct_done[kSlots] = {};   // a call's own hand-overs between its streams: heavy -> light stage, front -> back half
    // what the HOST waits for (at3hip_wait_input / at3hip_wait_frames), per call in a ring of four: the parity events are
    // re-recorded by the call after next, so a caller with three calls in flight would wait for the newest of them
    static constexpr int kHostRing = 4;
    Event host_in[kHostRing];            // the call's host PCM has been copied (nothing recorded: the call copied none)
    Event host_out[kHostRing];           // the call's frames are out and its back half is done (nothing recorded: the call produced none)
    hipEvent_t ev_mid_done[2] = {};      // by call parity: light stage of a call WITHOUT frames finished
    // What the next call of the same parity waits for before it reuses the parity's buffers; null: nothing yet.
    hipEvent_t mid_done_of[2] = {};      // light stage done with the subbands and gain records: the call's ev_mdct_done, or ev_mid_done (light -> heavy stage)
    hipEvent_t back_done_of[2] = {};     // back half done with the spectra, curves and energy scales: the call's host_out (back half -> light stage)

    float* d_sub_b[2] = {nullptr, nullptr};      // subbands, by call parity (the heavy stage runs one call ahead)
    GainRec* d_rec_b[2] = {nullptr, nullptr};
    float* d_pcm_in_b[2] = {nullptr, nullptr};      // host PCM staging [S][max_blocks][1024][channels]
    int16_t* d_s16_b[2] = {nullptr, nullptr};       // the same as 16-bit samples (at3hip_encode_s16 with host memory), by call parity
    long long enc_calls = 0;             // at3hip_encode calls so far
    int last_slot = -1;                  // slot of the most recent call that produced frames
    bool slot_has_frames[kSlots] = {};
    int slot_k1_launches[kSlots] = {};   // kernels the QMF + MDCT work of the slot's call was spread over (1 = fused, 2)
    long long blocks_fed = 0;   // per stream
    int chain_mode = 0;      // AT3HIP_OPT_CHAIN: 0 = chosen per call, 1 = never, 2 = whenever the geometry allows
    int timing_every = 1;    // AT3HIP_OPT_TIMING_EVERY: stage timings on every Nth call with frames (0 = never)
    unsigned timing_tick = 0;
    bool slot_timed[kSlots] = {};
    int runs_override = 0;   // AT3HIP_OPT_RUNS: runs per (stream, channel) of the front-end kernels (tuning aid; output is invariant)
    int flat_literal = 0;    // AT3HIP_OPT_LITERAL_FORMS
    int gain_form = AT3HIP_GAIN_FORM_TWO_WAVES;   // AT3HIP_OPT_GAIN_FORM: the two-wavefront workgroups (default) or one wavefront per item (k_gain_analysis1)
    int gain_wgs_per_cu = 0; // AT3HIP_OPT_GAIN_WGS_PER_CU: k_gain_analysis1 workgroups per CU (dynamic LDS padding; 0 = chosen per launch)
    int n_cus = 256;
    size_t lds_per_cu = 0;     // hipDeviceProp_t::maxSharedMemoryPerMultiProcessor; the whole-round LDS padding below is tuned for 160 KB
    int wgs_per_cu = 3;        // resident workgroups per CU of the QMF kernel this context uses (k_qmf_sub8 or the fused one)
    int wgs_per_cu_mdct = 3;   // the same of k_mdct_sub

    Tables* d_tables = nullptr;
    float* d_pcm_in = nullptr;       // one-channel contexts: the samples as (x, x) pairs [S][max_blocks][1024][2]
    float* d_hist[2] = {nullptr, nullptr};
    int hist_cur = 0;
    float* d_sub = nullptr;
    float* d_sub_tail = nullptr;     // [S][8][512] subbands of the last two blocks of the previous call
    GainRec* d_rec = nullptr;
    cpx* d_bins = nullptr;           // [S][B][6][kGainBins] high-passed rfft bins, k_gain_spec -> k_gain_analysis
    BandState* d_state = nullptr;
    Curve* d_curves[2] = {nullptr, nullptr};   // by call parity
    float* d_specs[2] = {nullptr, nullptr};
    float* d_ges[2] = {nullptr, nullptr};
    PsyRec* d_psy = nullptr;
    float* d_loud = nullptr;
    float* d_loud_state = nullptr;
    uint8_t* d_out = nullptr;
    QuantRec* d_quant = nullptr;     // allocated by AT3HIP_OPT_QUANT_TAP
    unsigned long long* d_clk = nullptr;   // AT3HIP_TAP_CLOCK (kClkWords)
    unsigned long long* d_counters = nullptr;   // at3hip_get_counters: [0] "Scale error" blocks, [1] "clipping" values (k_psy adds)
    at3hip_timings tm = {};
    // grow-only device staging of the stage-level entry points (at3hip_mdct, at3hip_gain_energy_scale) for host buffers
    void* d_stage = nullptr;
    size_t stage_bytes = 0;
};

namespace {

// Device staging area of at least `bytes` bytes (reallocated only when a call needs more than any call before).
int stage_reserve(at3hip_ctx* c, size_t bytes)
{
    if (bytes <= c->stage_bytes) return AT3HIP_OK;
    at3host::dev_free(c, c->d_stage);
    c->d_stage = nullptr;
    c->stage_bytes = 0;
    const size_t want = bytes + bytes / 2 + 4096;
    const int rc = at3host::dev_alloc_bytes(c, &c->d_stage, want, "hipMalloc (staging)");
    if (rc == AT3HIP_OK) c->stage_bytes = want;
    return rc;
}

// One call's layout of the staging area: the total is reserved first, then consecutive regions are handed out in the order
// they are asked for, with or without a host array copied into them on the context's stream.
struct StageLayout {
    at3hip_ctx* c;
    size_t at = 0;
    template <typename T>
    T* take(size_t count)
    {
        T* p = reinterpret_cast<T*>((char*)c->d_stage + at);
        at += count * sizeof(T);
        return p;
    }
    template <typename T, typename D>
    int put(const T* host, size_t count, D** d)   // (D: T or const T)
    {
        T* p = take<T>(count);
        HIPCHK(c, hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
        *d = p;
        return AT3HIP_OK;
    }
    // the three arrays of n_curves gain curves behind each other (absent: their regions stay unused)
    int put_curves(const int32_t*& n_points, const int32_t*& level, const int32_t*& loc, size_t n_curves)
    {
        if (!n_points) return AT3HIP_OK;
        int rc = put(n_points, n_curves, &n_points);
        if (rc == AT3HIP_OK) rc = put(level, n_curves * 8, &level);
        if (rc == AT3HIP_OK) rc = put(loc, n_curves * 8, &loc);
        return rc;
    }
};

// The stage-level entry points take their buffers all from the host or all from the device (*dev), and the three arrays of
// n_curves gain curves together or not at all; curves in host memory are checked for their ranges.
int check_buffers(at3hip_ctx* c, uint32_t flags, bool* dev, const int32_t* n_points, const int32_t* level, const int32_t* loc, size_t n_curves)
{
    if ((n_points != nullptr) != (level != nullptr) || (n_points != nullptr) != (loc != nullptr))
        return fail(c, AT3HIP_EINVAL, "n_points/level/loc must be all null or all set");
    *dev = (flags & AT3HIP_PCM_ON_DEVICE) && (flags & AT3HIP_OUT_ON_DEVICE);
    if (!*dev && (flags & (AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE))) return fail(c, AT3HIP_EINVAL, "buffers must be all host or all device");
    if (*dev || !n_points) return AT3HIP_OK;
    for (size_t i = 0; i < n_curves; ++i) {
        if (n_points[i] < 0 || n_points[i] > 7) return fail(c, AT3HIP_EINVAL, "n_points out of range");
        for (int k = 0; k < n_points[i]; ++k)
            if (level[i * 8 + k] < 0 || level[i * 8 + k] > 15 || loc[i * 8 + k] < 0 || loc[i * 8 + k] > 31)
                return fail(c, AT3HIP_EINVAL, "gain point out of range");
    }
    return AT3HIP_OK;
}

// Waits for everything this context has queued on its streams.
int drain(at3hip_ctx* c)
{
    if (c->h2d_stream) HIPCHK(c, hipStreamSynchronize(c->h2d_stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->mid_stream) HIPCHK(c, hipStreamSynchronize(c->mid_stream));
    HIPCHK(c, hipStreamSynchronize(c->back_stream));
    return AT3HIP_OK;
}

// Stage timings of the call recorded in `slot` (its events must have completed).
void read_timings(const at3hip_ctx* c, int slot, at3hip_timings* tm)
{
    memset(tm, 0, sizeof(*tm));
    if (slot < 0 || !c->slot_has_frames[slot] || !c->slot_timed[slot]) return;   // (all zero, qmf_mdct_launches 0: the call was not timed)
    hipEvent_t const* ev = c->ev[slot];
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, ev[0], ev[1]); tm->qmf_ms = ms;
    (void)hipEventElapsedTime(&ms, ev[1], ev[2]); tm->gain_ms = ms;
    (void)hipEventElapsedTime(&ms, ev[2], ev[3]); tm->curve_ms = ms;
    (void)hipEventElapsedTime(&ms, ev[3], ev[4]); tm->qmf_mdct_ms = ms;
    (void)hipEventElapsedTime(&ms, ev[5], ev[6]); tm->psy_ms = ms;
    (void)hipEventElapsedTime(&ms, ev[6], ev[7]); tm->alloc_ms = ms;
    (void)hipEventElapsedTime(&ms, ev[0], ev[7]); tm->total_ms = ms;   // first front-half kernel to last back-half kernel
    tm->qmf_mdct_launches = c->slot_k1_launches[slot];
}

// Runs per (stream, channel) for the wavefront-per-run kernels (QMF, MDCT, fused): `items` blocks or frames are cut
// into runs of at most 32, one wavefront each. A run costs its items plus a prologue of `prologue` items (FIR histories,
// overlap priming); a SIMD with w resident wavefronts issues at roughly eff(w) of its peak. The run count with the
// smallest estimated time wins: small batches get as many equal runs as one round of the grid holds, large batches long
// runs.
int pick_runs(const at3hip_ctx* c, int items, int wgs_per_cu, double prologue, int step = 1)
{
    if (c->runs_override > 0) return c->runs_override < items ? c->runs_override : items;
    if (items < step) step = 1;   // (`step`: only multiples of it are considered - whole workgroups per (stream, channel), see xcd_pair)
    const long long pairs = 2LL * c->cfg.n_streams;   // (stream, channel)
    const long long simds = (long long)c->n_cus * 4;
    const int cap = wgs_per_cu;                        // resident wavefronts per SIMD (a workgroup is one per SIMD)
    static const double eff[5] = {0.0, 0.55, 0.85, 0.95, 1.0};
    int best = 1;
    double best_t = 1e300;
    const int r_min = (items + 31) / 32;
    const int r_max = r_min > 128 ? r_min + 16 : 128;   // (a run holds at most 32 items: long calls need more than 128 runs)
    for (int r = (r_min + step - 1) / step * step; r <= items && r <= r_max; r += step) {
        const long long waves = pairs * r;
        const long long per_simd = (waves + simds - 1) / simds;   // the fullest SIMD
        const double work = (double)((items + r - 1) / r) + prologue;   // the longest run
        const long long resident = per_simd < cap ? per_simd : cap;
        const double t = (double)per_simd * work / eff[resident > 4 ? 4 : resident];
        if (t < best_t * 0.999) {
            best_t = t;
            best = r;
        }
    }
    return best;
}

// The fused kernel's cut: runs per (stream, channel) and whether the runs of a workgroup are CHAINED (k_qmf_mdct8: kFusedWaves consecutive
// runs share one priming block and hand their overlap on through LDS instead of each re-deriving it from a whole block of PCM). A chained
// wavefront costs its share of (the group's frames + 1) blocks, its FIR prologue and the hand-over with the deferred transform (~0.65 block);
// an unchained one its frames + 1.35. Same time model as pick_runs; chaining wins whenever runs are short (small batches).
struct FusedCut {
    int runs, chain;
};
FusedCut pick_fused(const at3hip_ctx* c, int items)
{
    const int NW = kFusedWaves;
    FusedCut cut = {pick_runs(c, items, c->wgs_per_cu, 1.35), 0};
    if (items < NW) return cut;
    if (c->runs_override > 0) {
        // a forced run count is chained when it can be: a multiple of NW with at least NW frames per group
        const int r = cut.runs;
        if (c->chain_mode != 1 && r % NW == 0 && items / (r / NW) >= NW) cut.chain = 1;
        return cut;
    }
    const long long pairs = 2LL * c->cfg.n_streams;
    const long long simds = (long long)c->n_cus * 4;
    const int cap = c->wgs_per_cu;
    static const double eff[5] = {0.0, 0.55, 0.85, 0.95, 1.0};
    auto cost = [&](int r, double work) {
        const long long waves = pairs * r;
        const long long per_simd = (waves + simds - 1) / simds;
        const long long resident = per_simd < cap ? per_simd : cap;
        return (double)per_simd * work / eff[resident > 4 ? 4 : resident];
    };
    // Whole workgroups of one (stream, channel) - run counts that are multiples of NW - let the kernel put a stream's two channels on
    // the same XCD (xcd_pair): its interleaved PCM then crosses the fabric once instead of twice. Only such cuts are considered.
    const int g_min = (items + 32 * NW - 1) / (32 * NW);   // (a run holds at most ~32 blocks)
    double best_t = 1e300;
    for (int g = g_min; g * NW <= items && g <= 64; ++g) {
        const int r = g * NW;
        if (c->chain_mode != 2) {
            const double t = cost(r, (double)((items + r - 1) / r) + 1.35);
            if (t < best_t * 0.999) {
                best_t = t;
                cut = {r, 0};
            }
        }
        if (c->chain_mode != 1 && items / g >= NW) {
            const int per_group = (items + g - 1) / g + 1;      // the longest group's frames + its priming block
            const double t = cost(r, (double)((per_group + NW - 1) / NW) + 0.65);
            if (t < best_t * 0.999) {
                best_t = t;
                cut = {r, 1};
            }
        }
    }
    return cut;
}

// Dynamic LDS added to k_gain_analysis' launch: it decides how many of its 17 KB workgroups share a CU (nine without). A
// launch of few rounds wants WHOLE rounds - 24 576 workgroups (4096 frames) are 10.67 rounds of 256 x 9 but exactly 16 of
// 256 x 6 - and fewer, fatter slots leave the light stage's and the back half's kernels room beside it: measured on the
// step at 4096 frames 0.333 ms (nine per CU), 0.329 (eight), 0.333 (seven), 0.326 (six), 0.357 (five); at the 1024 x 128
// shard (342 rounds, nothing to round) any padding costs 3 %.
struct LdsChoice {
    int per_cu;
    size_t pad;
};
size_t whole_rounds_pad(const at3hip_ctx* c, long long n_wgs, const LdsChoice* choice, int n_choices, bool ties_to_fewer)
{
    // the per-CU counts of the choices hold for a 160 KB LDS (gfx950): on any other geometry the launch is left alone
    if (c->lds_per_cu != 160u * 1024u) return 0;
    const long long cus = c->n_cus > 0 ? c->n_cus : 256;
    if (n_wgs >= 32 * choice[0].per_cu * cus) return 0;
    double best_waste = 1e30;
    size_t best_pad = 0;
    for (int i = 0; i < n_choices; ++i) {
        const long long slots = cus * choice[i].per_cu;
        const double waste = (double)(((n_wgs + slots - 1) / slots) * slots) / (double)n_wgs;
        if (ties_to_fewer ? waste <= best_waste + 0.005 : waste < best_waste - 0.005) {
            best_waste = waste < best_waste ? waste : best_waste;
            best_pad = choice[i].pad;
        }
    }
    return best_pad;
}
size_t analysis_lds_pad(const at3hip_ctx* c, long long n_wgs)
{
    if (c->lds_per_cu == 160u * 1024u && c->gain_wgs_per_cu > 0 && c->gain_wgs_per_cu < 9) {   // AT3HIP_OPT_GAIN_WGS_PER_CU (tuning aid)
        const size_t each = ((160u * 1024u) / (size_t)c->gain_wgs_per_cu) & ~(size_t)255;
        return each > sizeof(GainLds) + 256 ? each - sizeof(GainLds) - 256 : 0;
    }
    if (c->lds_per_cu == 160u * 1024u && c->gain_wgs_per_cu >= 256) return (size_t)c->gain_wgs_per_cu;   // (values from 256: the pad itself)
    if (c->gain_wgs_per_cu >= 9) return 0;
    // (six per CU at 26 KB each leave 4 KB of the CU's LDS: with the 8704-byte pad of round 3 they left exactly the 10 KB of one
    // k_alloc_pack wavefront, and the step was 0.8 % slower for every CU carrying that lodger - tools/ab_step.sh, --gain-wgs)
    // Since k_mdct_sub's workgroups are three wavefronts (20.3 KB) the fat slot is 22.5 KB, SEVEN per CU: what counts is that the slot ONE retiring
    // analysis workgroup frees takes a workgroup of the light stage - with mdct at 25.5 KB that needed the 26 KB slots of six per CU (a 2 KB larger
    // mdct block cost the step 5 %: EXPERIMENTS round 5), now seven fit the same launches (+1.2 % on the step, `tones` +2 %;
    // 23.3 KB slots, which leave under 1 KB of the CU, lose 7 %). The choice is still scored as the six-per-CU one it replaces.
    static const LdsChoice kChoice[3] = {{9, 0}, {8, 3328}, {6, 5632}};
    return whole_rounds_pad(c, n_wgs, kChoice, 3, true);   // (equally whole rounds: the fewer, fatter slots measured better)
}
// The one-wavefront form (k_gain_analysis1, 9.5 KB per workgroup): sixteen per CU without padding.
size_t analysis1_lds_pad(const at3hip_ctx* c, long long n_wgs)
{
    if (c->lds_per_cu != 160u * 1024u) return 0;
    if (c->gain_wgs_per_cu > 0 && c->gain_wgs_per_cu < 16) {
        const size_t each = ((160u * 1024u) / (size_t)c->gain_wgs_per_cu) & ~(size_t)255;
        return each > 9728 ? each - 9728 : 0;
    }
    static const LdsChoice kChoice[3] = {{16, 0}, {12, 3584}, {8, 10240}};
    return whole_rounds_pad(c, n_wgs, kChoice, 3, true);
}
// The same for k_gain_spec (9.5 KB per one-wavefront workgroup, sixteen per CU without padding): the 6144 workgroups of
// 4096 frames are one and a half rounds of 256 x 16 and exactly two of 256 x 12 (+0.8 % on the step).
size_t spec_lds_pad(const at3hip_ctx* c, long long n_wgs)
{
    static const LdsChoice kChoice[2] = {{16, 0}, {12, 3584}};
    return whole_rounds_pad(c, n_wgs, kChoice, 2, false);   // (only when it removes a partial round: 16384 frames are six whole rounds as they are)
}

int reset_state(at3hip_ctx* c)
{
    const size_t S = c->cfg.n_streams;
    HIPCHK(c, hipMemsetAsync(c->d_hist[0], 0, S * kHist * 2 * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_hist[1], 0, S * kHist * 2 * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_state, 0, S * 8 * sizeof(BandState), c->stream));
    if (c->d_sub_tail) HIPCHK(c, hipMemsetAsync(c->d_sub_tail, 0, S * 8 * 512 * sizeof(float), c->stream));   // silence before the stream
    HIPCHK(c, hipMemsetAsync(c->d_counters, 0, 2 * sizeof(unsigned long long), c->stream));
    const int rc = at3host::fill_and_wait(c, c->d_loud_state, S, 0.006f);   // LoudFactor, atrac3denc.h:115-116
    if (rc != AT3HIP_OK) return rc;
    c->blocks_fed = 0;
    c->hist_cur = 0;
    return AT3HIP_OK;
}

// Every event the context owns, in the order at3hip_create makes them: f(event, creation flags) until one returns false.
template <typename F>
bool for_each_event(at3hip_ctx* c, F f)
{
    const unsigned untimed = hipEventDisableTiming;
    for (int q = 0; q < 2; ++q)
        if (!f(c->ev_h2d[q], untimed) || !f(c->pcm_free[q].ev, untimed)) return false;
    for (auto& row : c->ev)
        for (auto& e : row)
            if (!f(e, 0u)) return false;
    if (!f(c->front_done.ev, untimed)) return false;
    for (int q = 0; q < at3hip_ctx::kSlots; ++q)
        if (!f(c->ev_heavy_done[q], untimed) || !f(c->ev_mdct_done[q], untimed)) return false;
    for (int q = 0; q < at3hip_ctx::kHostRing; ++q)
        if (!f(c->host_in[q].ev, untimed) || !f(c->host_out[q].ev, untimed)) return false;
    for (auto& e : c->ev_mid_done)
        if (!f(e, untimed)) return false;
    return true;
}

}  // namespace

extern "C" {

uint32_t at3hip_version(void) { return (uint32_t)AT3HIP_VERSION; }

int at3hip_create(const at3hip_config* cfg, at3hip_ctx** out)
{
    if (!cfg || !out) return AT3HIP_EINVAL;
    *out = nullptr;
    if ((cfg->channels != 1 && cfg->channels != 2) || cfg->n_streams < 1 || cfg->max_blocks < 1 || cfg->bfu_idx_const < 0 ||
        cfg->bfu_idx_const > 32)
        return AT3HIP_EINVAL;
    // the largest grid is one workgroup per (stream, frame, channel, band < 3); gridDim.x is a 31-bit quantity
    if ((long long)cfg->n_streams * cfg->max_blocks * 6 > 0x7fffffffLL) return AT3HIP_EINVAL;
    // The back half's stream gets the higher priority: its rate loop is the longest kernel of a call and fills every CU's
    // LDS, so a front-half workgroup placed between two of its rounds only delays it, while the front-half kernels of the
    // NEXT call have a whole rate loop's time to spare (measured with the three streams: back high / front low beats
    // the opposite by 0.7 % on white noise, 3-4 % on `tones` and LP4, 6.5 % on `burst`; equal priorities sit between).
    int prio_lo = 0, prio_hi = 0;
    auto make_front_stream = [&](hipStream_t* own) {
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);   // lo = numerically greatest = lowest priority
        return hipStreamCreateWithPriority(own, hipStreamNonBlocking, prio_lo);
    };
    auto setup = [&](at3hip_ctx* c) {
        c->cfg = *cfg;
        const uint32_t br = cfg->bitrate == 0 ? 132300u : (uint32_t)cfg->bitrate;
        int idx = 0;
        while (idx < 7 && kContainer[idx].bitrate < br) ++idx;  // lower_bound, atrac3.cpp:47-53
        c->frame_sz = kContainer[idx].frame_sz;
        c->js = kContainer[idx].js;
        c->ms = c->js && cfg->channels == 2;

        // All streams are made before any event, table or buffer, in this order.
        if (hipStreamCreateWithPriority(&c->back_stream, hipStreamNonBlocking, prio_hi) != hipSuccess) return AT3HIP_EDEVICE;
        // The light front stage (curve context, curves, energy scales, MDCT) sits on the step's critical path - the next rate
        // loop waits for its spectra - while the heavy stage it shares the chip with (the NEXT step's spectra and envelopes,
        // whose workgroups fill the LDS) has a whole rate loop of slack: high priority lets its short kernels take the
        // slots the heavy stage's workgroups free (+3 % on the step; a middle priority does nothing).
        if (!cfg->no_gain_control && hipStreamCreateWithPriority(&c->mid_stream, hipStreamNonBlocking, prio_hi) != hipSuccess) return AT3HIP_EDEVICE;
        // (Round 6 tried creating the copy stream only at the first call that copies from host memory - one claim less on the runtime's few hardware queues for
        // contexts fed from device memory. Created that late it shares a hardware queue with one of the kernel streams and the host-fed pipeline halves:
        // 12.4 -> 6.3 M frames/s with 16-bit samples. It is created here, right behind the kernel streams.)
        if (hipStreamCreateWithFlags(&c->h2d_stream, hipStreamNonBlocking) != hipSuccess) return AT3HIP_EDEVICE;
        if (!for_each_event(c, [](hipEvent_t& e, unsigned flags) { return (flags ? hipEventCreateWithFlags(&e, flags) : hipEventCreate(&e)) == hipSuccess; }))
            return AT3HIP_EDEVICE;

        const size_t S = cfg->n_streams, B = cfg->max_blocks;
        int rc = at3host::make_device_tables(c, &c->d_tables, [](Tables* t) { build_tables(t); return true; });
        if (rc != AT3HIP_OK) return rc;

        if (cfg->channels == 1 && (rc = dev_alloc(c, &c->d_pcm_in, S * B * 2048)) != AT3HIP_OK) return rc;
        // (the host-PCM staging pair is allocated by the first call that hands over host memory)
        if ((rc = dev_alloc(c, &c->d_hist[0], S * kHist * 2)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_hist[1], S * kHist * 2)) != AT3HIP_OK) return rc;
        // subbands go through HBM when gain control analyses them, and for joint stereo (the M/S matrixing needs both channels'
        // subbands, which the one-channel wavefronts of the fused kernel do not have)
        if (!cfg->no_gain_control || c->js) {
            if ((rc = dev_alloc(c, &c->d_sub, S * 8 * (B + 2) * 256)) != AT3HIP_OK) return rc;
            if ((rc = dev_alloc(c, &c->d_sub_tail, S * 8 * 512)) != AT3HIP_OK) return rc;
        }
        if (!cfg->no_gain_control) {
            if ((rc = dev_alloc(c, &c->d_rec, S * B * 6)) != AT3HIP_OK) return rc;
            c->d_rec_b[0] = c->d_rec;
            c->d_sub_b[0] = c->d_sub;
            if ((rc = dev_alloc(c, &c->d_rec_b[1], S * B * 6)) != AT3HIP_OK) return rc;
            if ((rc = dev_alloc(c, &c->d_sub_b[1], S * 8 * (B + 2) * 256)) != AT3HIP_OK) return rc;
            if ((rc = dev_alloc(c, &c->d_bins, S * B * 6 * kGainBins)) != AT3HIP_OK) return rc;
            for (int q = 0; q < 2; ++q)
                if ((rc = dev_alloc(c, &c->d_ges[q], S * B * 8)) != AT3HIP_OK) return rc;
        }
        if ((rc = dev_alloc(c, &c->d_state, S * 8)) != AT3HIP_OK) return rc;
        for (int q = 0; q < 2; ++q) {
            if ((rc = dev_alloc(c, &c->d_curves[q], S * B * 8)) != AT3HIP_OK) return rc;
            if ((rc = dev_alloc(c, &c->d_specs[q], S * B * 2048)) != AT3HIP_OK) return rc;
        }
        if ((rc = dev_alloc(c, &c->d_psy, S * B * 2)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_loud, S * B)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_loud_state, S)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_out, S * B * (size_t)c->frame_sz)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(c, &c->d_clk, kClkWords)) != AT3HIP_OK) return rc;
        if (hipMemsetAsync(c->d_clk, 0, kClkWords * sizeof(unsigned long long), c->stream) != hipSuccess) return AT3HIP_EDEVICE;   // (reset_state below waits for the stream)
        if ((rc = dev_alloc(c, &c->d_counters, 2)) != AT3HIP_OK) return rc;   // (zeroed by reset_state)
        if ((rc = reset_state(c)) != AT3HIP_OK) return rc;
        hipDeviceProp_t prop;
        const bool have_prop = hipGetDeviceProperties(&prop, c->device) == hipSuccess;
        c->n_cus = (have_prop && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
        c->lds_per_cu = have_prop ? (size_t)prop.maxSharedMemoryPerMultiProcessor : 0;
        int nb = 0;
        const bool gain = !c->cfg.no_gain_control;
        const hipError_t e = (gain || c->js) ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_qmf_sub8, 256, 0)
                                             : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_qmf_mdct8, 64 * kFusedWaves, 0);
        // (pick_runs' unit is resident wavefronts per SIMD: a four-wavefront workgroup is one per SIMD)
        c->wgs_per_cu = (e == hipSuccess && nb > 0) ? ((gain || c->js) ? nb : nb * kFusedWaves / 4) : 3;
        nb = 0;
        c->wgs_per_cu_mdct = ((c->js ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (k_mdct_sub<true, 4>), 256, 0)
                                     : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (k_mdct_sub<false, 4>), 256, 0)) == hipSuccess && nb > 0) ? nb : 3;   // (wavefronts per SIMD, pick_runs' unit: the same three for the three-wavefront form, four workgroups per CU)
        return AT3HIP_OK;
    };
    return at3host::create_engine(cfg->device_id, out, at3hip_destroy, setup, make_front_stream);
}

void at3hip_destroy(at3hip_ctx* c)
{
    if (!c) return;
    {
        // only the context's own streams are waited for: a caller-owned stream (at3hip_set_stream) may already be gone. What
        // the last call queued there (the carried-state update writes buffers freed below) is covered by an event, which
        // outlives the stream
        at3host::DeviceGuard guard(c->device);
        (void)c->front_done.host_wait();
    }
    c->stream = c->own_stream;   // (destroy_engine waits for `stream`: it must not be the caller's any more)
    at3host::destroy_engine(c, {c->mid_stream, c->back_stream, c->h2d_stream}, [c] {
        for_each_event(c, [](hipEvent_t& e, unsigned) {
            if (e) (void)hipEventDestroy(e);
            return true;
        });
    });
}

int at3hip_frame_size(const at3hip_ctx* c) { return c ? c->frame_sz : AT3HIP_EINVAL; }
int at3hip_joint_stereo(const at3hip_ctx* c) { return c ? c->js : AT3HIP_EINVAL; }
const char* at3hip_last_error(const at3hip_ctx* c) { return at3host::engine_last_error(c); }

int at3hip_set_stream(at3hip_ctx* c, void* hip_stream)
{
    return at3host::guarded(c, [hip_stream](at3hip_ctx* c) {
        const int rc = drain(c);
        if (rc == AT3HIP_OK) c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
        return rc;
    });
}

int at3hip_host_alloc(at3hip_ctx* c, size_t bytes, void** out)
{
    if (!c || !out || bytes == 0) return AT3HIP_EINVAL;
    *out = nullptr;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, AT3HIP_ENOMEM, "hipHostMalloc", e);
    *out = p;
    return AT3HIP_OK;
}

int at3hip_device_numa_node(int32_t device_id)
{
    // an ordinal the runtime does not know is answered here: a failed runtime call would stay behind as the thread's last
    // error, which the caller's next kernel launch check (torch's, for one) then reports as its own
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) {
        (void)hipGetLastError();
        return -1;
    }
    char bus[32] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device_id) != hipSuccess || !bus[0]) {
        (void)hipGetLastError();
        return -1;
    }
    for (char* q = bus; *q; ++q)
        if (*q >= 'A' && *q <= 'F') *q = (char)(*q - 'A' + 'a');   // sysfs spells the address in lower case
    char path[96];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE* f = fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

int at3hip_host_free(at3hip_ctx* c, void* p)
{
    if (!c) return AT3HIP_EINVAL;
    if (!p) return AT3HIP_OK;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    HIPCHK(c, hipHostFree(p));
    return AT3HIP_OK;
}

int at3hip_wait_input(at3hip_ctx* c, int32_t ago)
{
    if (!c || ago < 0 || ago >= at3hip_ctx::kHostRing || ago >= c->enc_calls) return AT3HIP_EINVAL;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    const int q = (int)((c->enc_calls - 1 - ago) % at3hip_ctx::kHostRing);
    HIPCHK(c, c->host_in[q].host_wait());
    return AT3HIP_OK;
}

int at3hip_wait_frames(at3hip_ctx* c, int32_t ago)
{
    if (!c || ago < 0 || ago >= at3hip_ctx::kHostRing || ago >= c->enc_calls) return AT3HIP_EINVAL;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    const int q = (int)((c->enc_calls - 1 - ago) % at3hip_ctx::kHostRing);
    HIPCHK(c, c->host_out[q].host_wait());
    return AT3HIP_OK;
}

int at3hip_host_tables(void* dst, size_t bytes)
{
    if (!dst || bytes != sizeof(Tables)) return AT3HIP_EINVAL;
    build_tables((Tables*)dst);
    return AT3HIP_OK;
}

int at3hip_set_option(at3hip_ctx* c, int32_t option, int32_t value)
{
    if (!c) return AT3HIP_EINVAL;
    switch (option) {
        case AT3HIP_OPT_RUNS:
            if (value < 0) return fail(c, AT3HIP_EINVAL, "runs must be >= 0");
            c->runs_override = value;
            return AT3HIP_OK;
        case AT3HIP_OPT_CHAIN:
            if (value < 0 || value > 2) return fail(c, AT3HIP_EINVAL, "chain: 0 (per call), 1 (never) or 2 (whenever possible)");
            c->chain_mode = value;
            return AT3HIP_OK;
        case AT3HIP_OPT_TIMING_EVERY:
            if (value < 0) return fail(c, AT3HIP_EINVAL, "timing every: 0 (never) or N >= 1 (every Nth call with frames)");
            c->timing_every = value;
            c->timing_tick = 0;
            return AT3HIP_OK;
        case AT3HIP_OPT_LITERAL_FORMS:
            if (value != 0 && value != 1) return fail(c, AT3HIP_EINVAL, "literal forms: 0 or 1");
            c->flat_literal = value;
            return AT3HIP_OK;
        case AT3HIP_OPT_GAIN_FORM:
            if (value == 2) value = AT3HIP_GAIN_FORM_ONE_WAVE;   // (ABI 1.2's number for the one-wavefront form)
            if (value != AT3HIP_GAIN_FORM_TWO_WAVES && value != AT3HIP_GAIN_FORM_ONE_WAVE)
                return fail(c, AT3HIP_EINVAL, "gain form: AT3HIP_GAIN_FORM_TWO_WAVES or AT3HIP_GAIN_FORM_ONE_WAVE");
            c->gain_form = value;
            return AT3HIP_OK;
        case AT3HIP_OPT_GAIN_WGS_PER_CU:
            if (value < 0 || (value > 16 && value < 256) || value > 64 * 1024) return fail(c, AT3HIP_EINVAL, "workgroups per CU must be 0 .. 16 (or a pad of 256 .. 65536 bytes)");
            c->gain_wgs_per_cu = value;
            return AT3HIP_OK;
        case AT3HIP_OPT_QUANT_TAP: {
            if (value != 0 && value != 1) return fail(c, AT3HIP_EINVAL, "quant tap: 0 or 1");
            at3host::DeviceGuard guard(c->device);
            HIPCHK(c, guard.error());
            const int rc = drain(c);
            if (rc != AT3HIP_OK) return rc;
            if (value && !c->d_quant) return dev_alloc(c, &c->d_quant, (size_t)c->cfg.n_streams * c->cfg.max_blocks * 2);
            if (!value) {
                at3host::dev_free(c, c->d_quant);
                c->d_quant = nullptr;
            }
            return AT3HIP_OK;
        }
        default: return fail(c, AT3HIP_EINVAL, "unknown option");
    }
}

int at3hip_reset(at3hip_ctx* c)
{
    return at3host::guarded(c, [](at3hip_ctx* c) {
        const int rc = drain(c);
        return rc != AT3HIP_OK ? rc : reset_state(c);
    });
}

int at3hip_get_timings(const at3hip_ctx* c, at3hip_timings* out)
{
    if (!c || !out) return AT3HIP_EINVAL;
    *out = c->tm;
    return AT3HIP_OK;
}

namespace {
int encode_impl(at3hip_ctx* c, const void* pcm_any, bool s16, int32_t n_blocks, uint8_t* out_frames, int32_t* n_frames_out, uint32_t flags);
}

int at3hip_encode(at3hip_ctx* c, const float* pcm, int32_t n_blocks, uint8_t* out_frames, int32_t* n_frames_out,
                  uint32_t flags)
{
    return encode_impl(c, pcm, false, n_blocks, out_frames, n_frames_out, flags);
}

int at3hip_encode_s16(at3hip_ctx* c, const int16_t* pcm, int32_t n_blocks, uint8_t* out_frames, int32_t* n_frames_out,
                      uint32_t flags)
{
    return encode_impl(c, pcm, true, n_blocks, out_frames, n_frames_out, flags);
}

}  // extern "C"

namespace {

// What one at3hip_encode / at3hip_encode_s16 call works with: its geometry, its places in the context's rings, its streams and
// the buffers of its parity.
struct EncodeCall {
    int n_blocks, f0, n_out;   // blocks given; 1 when the stream starts with this call (its first block only primes the look-ahead); frames produced
    uint32_t flags;
    int par, slot, hq;         // call parity (the double buffers), slot in the timing history, slot in the host-visible event ring
    bool gain, split;          // gain control; QMF and MDCT as two kernels with the subbands in HBM between them (gain control or joint stereo)
    bool staged;               // the call's float samples live in this parity's staging buffer
    bool timed;                // the call records its stage timestamps
    hipStream_t st, md, bk;    // the heavy front stage, the light one (see at3hip_ctx::mid_stream; without gain control md == st), the back half
    hipEvent_t* ev;            // the slot's eight stage timestamps
    const float* d_pcm;        // the samples in device memory as pairs, [S][n_blocks][1024][2]
    const float* hist;         // the PCM history in front of them
    float* hist_next;          // and where the carried-state update leaves the next call's
    float* d_sub;              // the parity's buffers
    GainRec* d_rec;
    Curve* d_curves;
    float* d_specs;
    float* d_ges;
    uint8_t* d_out;            // the frames: the caller's device memory, or the staging of host output
};

// PCM staging: host samples through the copy stream into the parity's staging, 16-bit samples to floats, one channel to pairs.
// Leaves k.d_pcm.
int stage_pcm(at3hip_ctx* c, EncodeCall& k, const void* pcm_any, bool s16)
{
    const int S = c->cfg.n_streams, par = k.par;
    const float* pcm = (const float*)pcm_any;   // (float samples unless s16)
    const size_t n_in = (size_t)S * k.n_blocks * 1024 * c->cfg.channels;
    const size_t n_max = (size_t)S * c->cfg.max_blocks * 1024 * c->cfg.channels;
    const float* d_staged = pcm;   // the call's PCM in device memory, [S][n_blocks][1024][channels]
    if (k.staged && !c->d_pcm_in_b[par]) {
        const int rc = dev_alloc(c, &c->d_pcm_in_b[par], n_max);
        if (rc != AT3HIP_OK) return rc;
    }
    if (!(k.flags & AT3HIP_PCM_ON_DEVICE)) {
        // host memory: the copy runs on its own stream into this parity's staging buffer - beside the previous call's
        // kernels when the memory is pinned - and the front half waits for its arrival. 16-bit samples cross the bus as they
        // are (half the bytes: the host-fed rate is bound by them) and become floats on the device, on the same stream.
        if (s16 && !c->d_s16_b[par]) {
            const int rc = dev_alloc(c, &c->d_s16_b[par], n_max);
            if (rc != AT3HIP_OK) return rc;
        }
        HIPCHK(c, c->pcm_free[par].make_wait(c->h2d_stream));
        if (s16) HIPCHK(c, hipMemcpyAsync(c->d_s16_b[par], pcm_any, n_in * sizeof(int16_t), hipMemcpyHostToDevice, c->h2d_stream));
        else HIPCHK(c, hipMemcpyAsync(c->d_pcm_in_b[par], pcm, n_in * sizeof(float), hipMemcpyHostToDevice, c->h2d_stream));
        HIPCHK(c, hipEventRecord(c->ev_h2d[par], c->h2d_stream));
        HIPCHK(c, c->host_in[k.hq].record(c->h2d_stream));
        HIPCHK(c, hipStreamWaitEvent(k.st, c->ev_h2d[par], 0));
        // (the conversion runs on the front stream, not behind the copy: the copy stream carries nothing but copies, back to back)
        if (s16) hipLaunchKernelGGL(k_s16_to_f32, dim3((unsigned)((n_in / 8 + 255) / 256)), dim3(256), 0, k.st, c->d_s16_b[par], c->d_pcm_in_b[par], n_in / 8);
        d_staged = c->d_pcm_in_b[par];
    } else if (s16) {
        // 16-bit samples already in HBM: converted on the front stream (which also carries everything that reads the staging)
        hipLaunchKernelGGL(k_s16_to_f32, dim3((unsigned)((n_in / 8 + 255) / 256)), dim3(256), 0, k.st, (const int16_t*)pcm_any, c->d_pcm_in_b[par], n_in / 8);
        d_staged = c->d_pcm_in_b[par];
    }
    k.d_pcm = d_staged;
    if (c->cfg.channels == 1) {
        // "No mono mode for atrac3, just make duplicate of first channel" (atrac3_bitstream.cpp:836-843): the one-channel
        // frame is two identical sound units, i.e. the discrete-stereo frame of L = R (TrackLoudness' 0.02 l equals
        // 0.01 (l + l) exactly). The samples are duplicated in HBM and the stereo pipeline runs unchanged.
        // Joint-stereo containers: M = (x + x) / 2 = x exactly, so the M unit is the mono unit (gain analysis, loudness
        // with 0.02 l and all); the rate/pack kernel replaces the S unit by the empty element of atrac3denc.cpp:843-849.
        const size_t n = (size_t)S * k.n_blocks * 1024;
        hipLaunchKernelGGL(k_mono_to_pairs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k.st, d_staged, c->d_pcm_in, n);
        k.d_pcm = c->d_pcm_in;
    }
    return AT3HIP_OK;
}

// The carried-state update on stream `on`: PCM history and subband tail (parts & 1), last curves and band states (parts & 2).
void launch_state(at3hip_ctx* c, const EncodeCall& k, hipStream_t on, int parts)
{
    StateParams sp;
    sp.pcm = k.d_pcm;
    sp.hist_in = k.hist;
    sp.hist_out = k.hist_next;
    sp.curves = k.d_curves;
    sp.state = c->d_state;
    sp.sub = k.split ? k.d_sub : nullptr;
    sp.sub_tail = c->d_sub_tail;
    sp.n_blocks = k.n_blocks;
    sp.n_streams = c->cfg.n_streams;
    sp.parts = parts;
    hipLaunchKernelGGL(k_state_update, dim3((unsigned)(((kHist + 255) / 256) * c->cfg.n_streams)), dim3(256), 0, on, sp);
}

// k_qmf_sub8 on the heavy stage's stream: the subbands of all the call's blocks to HBM, one wavefront per (stream, channel, run).
void launch_qmf_sub(at3hip_ctx* c, const EncodeCall& k, FrontParams& fp)
{
    fp.sub_runs = pick_runs(c, k.n_blocks, c->wgs_per_cu, 0.35, 4);
    const int n_waves = c->cfg.n_streams * 2 * fp.sub_runs;
    hipLaunchKernelGGL(k_qmf_sub8, dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0, k.st, fp, c->d_tables, n_waves);
}

// A call that only primes the look-ahead (n_out == 0) still has to leave its subbands behind for the next call's look-back.
void launch_qmf_sub_priming(at3hip_ctx* c, const EncodeCall& k)
{
    FrontParams fp = {};
    fp.pcm = k.d_pcm;
    fp.hist = k.hist;
    fp.sub = k.d_sub;
    fp.sub_tail = c->d_sub_tail;
    fp.n_blocks = k.n_blocks;
    fp.f0 = k.f0;
    fp.js = c->ms;
    launch_qmf_sub(c, k, fp);
}

// The front half's parameters of a call with frames; the cut of the fused kernel where that is the one to run.
FrontParams front_params(at3hip_ctx* c, const EncodeCall& k)
{
    FrontParams fp;
    fp.pcm = k.d_pcm;
    fp.hist = k.hist;
    fp.curves = k.d_curves;
    fp.state = c->d_state;
    fp.specs = k.d_specs;
    fp.ges = k.d_ges;
    fp.sub = k.d_sub;
    fp.sub_tail = c->d_sub_tail;
    fp.n_blocks = k.n_blocks;
    fp.f0 = k.f0;
    const FusedCut cut = k.split ? FusedCut{0, 0} : pick_fused(c, k.n_out);
    fp.frame_runs = cut.runs;
    fp.chain = cut.chain;
    fp.sub_runs = 0;
    fp.js = c->ms;
    return fp;
}

// k_mdct_sub on the light stage's stream: the subbands are in HBM (k_qmf_sub8 wrote them: for the gain analysis, or for the M/S matrixing).
void launch_mdct_sub(at3hip_ctx* c, const EncodeCall& k)
{
    const int S = c->cfg.n_streams;
    MdctSubParams mp;
    mp.sub = k.d_sub;
    mp.curves = k.gain ? k.d_curves : nullptr;
    mp.state = c->d_state;
    mp.specs = k.d_specs;
    mp.n_blocks = k.n_blocks;
    mp.f0 = k.f0;
    mp.js = c->ms;
    mp.frame_runs = pick_runs(c, k.n_out, c->wgs_per_cu_mdct, 0.3);
    mp.n_waves = S * 2 * mp.frame_runs;
    // three wavefronts per workgroup (20.3 KB) where k_gain_analysis' launch is padded to fat slots - a light-stage workgroup must fit the slot
    // one retiring analysis workgroup frees (analysis_lds_pad) -, four (25.5 KB; one table copy per four runs) where it fills the chip unpadded
    const bool fat_slots = c->gain_form != AT3HIP_GAIN_FORM_ONE_WAVE && analysis_lds_pad(c, (long long)S * k.n_out * 6) != 0;   // (the one-wavefront form's launch has no fat slots)
    if (fat_slots) {
        if (c->ms) hipLaunchKernelGGL((k_mdct_sub<true, 3>), dim3((unsigned)((mp.n_waves + 2) / 3)), dim3(192), 0, k.md, mp, c->d_tables);
        else hipLaunchKernelGGL((k_mdct_sub<false, 3>), dim3((unsigned)((mp.n_waves + 2) / 3)), dim3(192), 0, k.md, mp, c->d_tables);
    } else {
        if (c->ms) hipLaunchKernelGGL((k_mdct_sub<true, 4>), dim3((unsigned)((mp.n_waves + 3) / 4)), dim3(256), 0, k.md, mp, c->d_tables);
        else hipLaunchKernelGGL((k_mdct_sub<false, 4>), dim3((unsigned)((mp.n_waves + 3) / 4)), dim3(256), 0, k.md, mp, c->d_tables);
    }
}

// What every front half starts with: the waits that hand the parity's buffers over to this call, its first timestamp, the zeroed curves.
int front_open(at3hip_ctx* c, const EncodeCall& k)
{
    // the light stage of the call before the previous one must be done with this parity's subbands and gain records
    if (k.gain && c->mid_done_of[k.par]) HIPCHK(c, hipStreamWaitEvent(k.st, c->mid_done_of[k.par], 0));
    if (k.timed) HIPCHK(c, hipEventRecord(k.ev[0], k.st));
    // the back half of the call before the previous one must be done with this parity's spectra / curves / scales
    if (c->back_done_of[k.par]) HIPCHK(c, hipStreamWaitEvent(k.md, c->back_done_of[k.par], 0));
    HIPCHK(c, hipMemsetAsync(k.d_curves, 0, (size_t)c->cfg.n_streams * k.n_blocks * 8 * sizeof(Curve), k.md));
    return AT3HIP_OK;
}

// What every front half with frames ends with: its last timestamp and the hand-over of the spectra to the back half.
int front_close(at3hip_ctx* c, const EncodeCall& k)
{
    if (k.timed) HIPCHK(c, hipEventRecord(k.ev[4], k.md));
    HIPCHK(c, hipEventRecord(c->ev_mdct_done[k.slot], k.md));
    c->slot_k1_launches[k.slot] = k.split ? 2 : 1;
    return AT3HIP_OK;
}

// The front half with gain control: the heavy stage on k.st, the light one on k.md, and what the parity's next call waits for.
int front_with_gain(at3hip_ctx* c, const EncodeCall& k)
{
    const int S = c->cfg.n_streams, n_out = k.n_out, par = k.par;
    hipStream_t st = k.st, md = k.md;
    int rc = front_open(c, k);
    if (rc != AT3HIP_OK) return rc;
    if (n_out == 0) {
        launch_qmf_sub_priming(c, k);
        launch_state(c, k, st, 1);
        launch_state(c, k, md, 2);   // last curves: the light stage's own hand-over
        HIPCHK(c, hipEventRecord(c->ev_mid_done[par], md));
        c->mid_done_of[par] = c->ev_mid_done[par];
        return AT3HIP_OK;
    }
    FrontParams fp = front_params(c, k);
    GainParams gp;
    gp.sub = k.d_sub;
    gp.rec = k.d_rec;
    gp.bins = c->d_bins;
    gp.state = c->d_state;
    gp.curves = k.d_curves;
    gp.n_blocks = k.n_blocks;
    gp.f0 = k.f0;
    gp.js = c->ms;
    gp.n_streams = S;
    gp.literal = c->flat_literal;
    launch_qmf_sub(c, k, fp);
    if (k.timed) HIPCHK(c, hipEventRecord(k.ev[1], st));
    // PCM history and subband tail: the next call's heavy stage needs nothing else from this one. (Round 6: moved behind the gain analysis - off the
    // chain QMF -> spectra -> analysis - it cost the step 8 %: the next call's QMF kernel follows it on this stream and then misses the window
    // between the analysis and the next rate loop in which it gets its only undisturbed microseconds. EXPERIMENTS.md.)
    launch_state(c, k, st, 1);
    const long long spec_wgs = (long long)S * ((n_out + 3) / 4) * 6;   // (four consecutive frames of one (stream, channel, band) per wavefront)
    hipLaunchKernelGGL(k_gain_spec, dim3((unsigned)spec_wgs), dim3(64), spec_lds_pad(c, spec_wgs), st, gp, c->d_tables, S * n_out * 6);
    // default: the two-wavefront form. The one-wavefront form is 11 % faster alone (89 against 101 us at 4096 frames) and
    // leaves the pipelined step 2 % slower at that size, equal at the 1024 x 128 shard (profiles/EXPERIMENTS.md)
    if (c->gain_form != AT3HIP_GAIN_FORM_ONE_WAVE) hipLaunchKernelGGL(k_gain_analysis, dim3(S * n_out * 6), dim3(128), analysis_lds_pad(c, (long long)S * n_out * 6), st, gp, c->d_tables);
    else hipLaunchKernelGGL(k_gain_analysis1, dim3(S * n_out * 6), dim3(64), analysis1_lds_pad(c, (long long)S * n_out * 6), st, gp, c->d_tables);   // one wavefront per item
    if (k.timed) HIPCHK(c, hipEventRecord(k.ev[2], st));
    HIPCHK(c, hipEventRecord(c->ev_heavy_done[k.slot], st));
    HIPCHK(c, hipStreamWaitEvent(md, c->ev_heavy_done[k.slot], 0));   // the light stage starts when this call's heavy stage is done
    hipLaunchKernelGGL(k_gain_tail, dim3((unsigned)((S * n_out * 6 + 7) / 8)), dim3(256), 0, md, gp, S * n_out * 6);
    hipLaunchKernelGGL(k_gain_scan, dim3(S * 6), dim3(64), 0, md, gp, S);
    hipLaunchKernelGGL(k_gain_curve, dim3((S * n_out * 6 + 7) / 8), dim3(256), 0, md, gp, c->d_tables, S);
    hipLaunchKernelGGL(k_gain_energy_scale, dim3(S * n_out), dim3(64), 0, md, fp, c->d_tables, S * n_out);
    if (k.timed) HIPCHK(c, hipEventRecord(k.ev[3], md));
    launch_mdct_sub(c, k);
    if ((rc = front_close(c, k)) != AT3HIP_OK) return rc;
    launch_state(c, k, md, 2);   // last curves: the light stage's own hand-over
    // the MDCT kernel was the last reader of the parity's subbands and gain records (the update above touches the curves and
    // the band states, which only this stream reads and writes): its event serves, one record less between the kernels
    c->mid_done_of[par] = c->ev_mdct_done[k.slot];
    return AT3HIP_OK;
}

// The front half without gain control, all of it on k.st: the fused QMF + MDCT kernel, or for joint stereo the two kernels.
int front_without_gain(at3hip_ctx* c, const EncodeCall& k)
{
    hipStream_t st = k.st;
    int rc = front_open(c, k);
    if (rc != AT3HIP_OK) return rc;
    if (k.n_out == 0 && k.split) launch_qmf_sub_priming(c, k);
    if (k.n_out > 0) {
        FrontParams fp = front_params(c, k);
        if (k.split) launch_qmf_sub(c, k, fp);   // joint stereo without gain control: the QMF kernel, timed as qmf_ms
        if (k.timed) HIPCHK(c, hipEventRecord(k.ev[1], st));
        if (k.timed) HIPCHK(c, hipEventRecord(k.ev[2], st));
        if (k.timed) HIPCHK(c, hipEventRecord(k.ev[3], st));
        if (k.split) {
            launch_mdct_sub(c, k);
        } else {
            const int n_waves = c->cfg.n_streams * 2 * fp.frame_runs;
            hipLaunchKernelGGL(k_qmf_mdct8, dim3((unsigned)((n_waves + kFusedWaves - 1) / kFusedWaves)), dim3(64 * kFusedWaves), 0, st, fp, c->d_tables, n_waves);
        }
        if ((rc = front_close(c, k)) != AT3HIP_OK) return rc;
    }
    launch_state(c, k, st, 3);
    return AT3HIP_OK;
}

// The back half of a call with frames, on its own stream, after the MDCT (or the fused kernel) of THIS call.
// (Round 6, each an 8 - 11 % LOSS on the step although it shortens a chain: the loudness sums and k_psy queued behind the MDCT on the light stage's stream
// (no event hop between the streams in front of them); k_gain_energy_scale on this stream beside the MDCT; TrackLoudness inside k_psy (no k_loudness
// launch); k_loud_sum in 22 KB blocks that fit a slot one retiring analysis workgroup frees. EXPERIMENTS.md: the step's schedule is one of several
// stable ones.)
int back_half(at3hip_ctx* c, const EncodeCall& k, uint8_t* out_frames)
{
    const int S = c->cfg.n_streams, n_out = k.n_out;
    hipStream_t bk = k.bk;
    HIPCHK(c, hipStreamWaitEvent(bk, c->ev_mdct_done[k.slot], 0));
    if (k.timed) HIPCHK(c, hipEventRecord(k.ev[5], bk));
    BackParams bp;
    bp.specs = k.d_specs;
    bp.ges = k.gain ? k.d_ges : nullptr;
    bp.curves = k.d_curves;
    bp.psy = c->d_psy;
    bp.loud = c->d_loud;
    bp.loud_state = c->d_loud_state;
    bp.out = k.d_out;
    bp.n_blocks = k.n_blocks;
    bp.f0 = k.f0;
    bp.n_streams = S;
    bp.no_tonal = c->cfg.no_tonal;
    bp.js = c->js;
    bp.frame_sz = c->frame_sz;
    bp.bfu_idx_const = c->cfg.bfu_idx_const;
    bp.mono_js = (c->cfg.channels == 1 && c->js) ? 1 : 0;
    bp.flat_literal = c->flat_literal;
    bp.quant = c->d_quant;
    bp.clk = c->d_clk;
    bp.counters = c->d_counters;
    bp.one_channel = c->cfg.channels == 1 ? 1 : 0;
    hipLaunchKernelGGL(k_loud_sum, dim3((unsigned)((S * n_out * 2 + kLoudCf - 1) / kLoudCf)), dim3(256), 0, bk, bp, c->d_tables, S * n_out * 2);
    hipLaunchKernelGGL(k_psy, dim3((S * n_out * 2 + kPsyCf - 1) / kPsyCf), dim3(256), 0, bk, bp, c->d_tables, S * n_out * 2);
    if (k.timed) HIPCHK(c, hipEventRecord(k.ev[6], bk));
    hipLaunchKernelGGL(k_loudness, dim3(S), dim3(64), 0, bk, bp);
    hipLaunchKernelGGL(k_alloc_pack, dim3(S * n_out * 2), dim3(64), 0, bk, bp, c->d_tables);
    if (k.timed) HIPCHK(c, hipEventRecord(k.ev[7], bk));
    if (!(k.flags & AT3HIP_OUT_ON_DEVICE))
        HIPCHK(c, hipMemcpyAsync(out_frames, c->d_out, (size_t)S * n_out * c->frame_sz, hipMemcpyDeviceToHost, bk));
    // one event per call on this stream: the frames are out (at3hip_wait_frames) and the back half is done with the parity's buffers
    HIPCHK(c, c->host_out[k.hq].record(bk));
    c->back_done_of[k.par] = c->host_out[k.hq].ev;
    c->slot_has_frames[k.slot] = true;
    c->last_slot = k.slot;
    return AT3HIP_OK;
}

// The end of a call: the events that cover what it left on the front stream, the context's counters, and the wait unless AT3HIP_ASYNC.
int finish_call(at3hip_ctx* c, const EncodeCall& k, int32_t* n_frames_out)
{
    if (c->stream != c->own_stream) HIPCHK(c, c->front_done.record(k.st));   // (at3hip_destroy waits for the context's own streams themselves)
    if (k.staged) HIPCHK(c, c->pcm_free[k.par].record(k.st));   // (the PCM is read by the first stage and by the carried-state update, both on `st`)
    HIPCHK(c, hipGetLastError());
    c->host_in[k.hq].recorded = !(k.flags & AT3HIP_PCM_ON_DEVICE);   // (a call without a host copy / without frames leaves its slot of the ring
    c->host_out[k.hq].recorded = k.n_out > 0;                         // with nothing to wait for)
    c->hist_cur ^= 1;
    c->blocks_fed += k.n_blocks;
    c->enc_calls++;
    if (n_frames_out) *n_frames_out = k.n_out;
    if (!(k.flags & AT3HIP_ASYNC)) {
        const int rc = drain(c);
        if (rc != AT3HIP_OK) return rc;
        if (k.n_out > 0) read_timings(c, k.slot, &c->tm);
    }
    return AT3HIP_OK;
}

int encode_impl(at3hip_ctx* c, const void* pcm_any, bool s16, int32_t n_blocks, uint8_t* out_frames, int32_t* n_frames_out, uint32_t flags)
{
    if (!c || !pcm_any || n_blocks < 1 || n_blocks > c->cfg.max_blocks) return c ? fail(c, AT3HIP_EINVAL, "bad argument") : AT3HIP_EINVAL;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    EncodeCall k;
    k.n_blocks = n_blocks;
    k.f0 = (c->blocks_fed == 0) ? 1 : 0;
    k.n_out = n_blocks - k.f0;
    k.flags = flags;
    if (k.n_out > 0 && !out_frames) return fail(c, AT3HIP_EINVAL, "out_frames is null");
    // k_s16_to_f32 reads the caller's device pointer sixteen bytes at a time
    if (s16 && (flags & AT3HIP_PCM_ON_DEVICE) && ((uintptr_t)pcm_any & 15u) != 0) return fail(c, AT3HIP_EINVAL, "16-bit device PCM must be 16-byte aligned");
    k.par = (int)(c->enc_calls & 1);
    k.slot = (int)(c->enc_calls % at3hip_ctx::kSlots);
    k.hq = (int)(c->enc_calls % at3hip_ctx::kHostRing);
    k.gain = !c->cfg.no_gain_control;
    k.split = k.gain || c->js;
    k.staged = s16 || !(flags & AT3HIP_PCM_ON_DEVICE);
    k.st = c->stream;
    k.md = k.gain ? c->mid_stream : k.st;
    k.bk = c->back_stream;
    k.ev = c->ev[k.slot];
    k.hist = c->d_hist[c->hist_cur];
    k.hist_next = c->d_hist[c->hist_cur ^ 1];
    k.d_sub = k.gain ? c->d_sub_b[k.par] : c->d_sub;
    k.d_rec = k.gain ? c->d_rec_b[k.par] : c->d_rec;
    k.d_curves = c->d_curves[k.par];
    k.d_specs = c->d_specs[k.par];
    k.d_ges = c->d_ges[k.par];
    k.d_out = (flags & AT3HIP_OUT_ON_DEVICE) ? out_frames : c->d_out;
    int rc = stage_pcm(c, k, pcm_any, s16);
    if (rc != AT3HIP_OK) return rc;
    c->slot_has_frames[k.slot] = false;
    // The timing events sit between the kernels of the three streams; at 4096 frames a step recording all eight takes 3.3 % longer than one recording none
    // (EXPERIMENTS.md, round 6), so a caller that only samples the stage timings asks for every Nth call.
    k.timed = k.n_out > 0 && c->timing_every > 0 && (c->timing_tick++ % (unsigned)c->timing_every) == 0;
    c->slot_timed[k.slot] = k.timed;
    rc = k.gain ? front_with_gain(c, k) : front_without_gain(c, k);
    if (rc == AT3HIP_OK && k.n_out > 0) rc = back_half(c, k, out_frames);
    return rc != AT3HIP_OK ? rc : finish_call(c, k, n_frames_out);
}

}  // namespace

extern "C" {

int at3hip_sync(at3hip_ctx* c)
{
    return at3host::guarded(c, [](at3hip_ctx* c) {
        const int rc = drain(c);
        if (rc == AT3HIP_OK) read_timings(c, c->last_slot, &c->tm);
        return rc;
    });
}

int at3hip_read_tap(at3hip_ctx* c, int32_t kind, void* dst, size_t bytes)
{
    if (!c || !dst) return AT3HIP_EINVAL;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    const int rc = drain(c);
    if (rc != AT3HIP_OK) return rc;
    if (c->enc_calls == 0 && kind != AT3HIP_TAP_CLOCK) return fail(c, AT3HIP_EINVAL, "no encode call yet");
    const int par = (int)((c->enc_calls - 1) & 1);
    const size_t S = c->cfg.n_streams, B = c->cfg.max_blocks;
    const void* src = nullptr;
    size_t cap = 0;
    switch (kind) {
        case AT3HIP_TAP_SPECTRA: src = c->d_specs[par]; cap = S * B * 2048 * sizeof(float); break;
        case AT3HIP_TAP_CURVES: src = c->d_curves[par]; cap = S * B * 8 * sizeof(Curve); break;
        case AT3HIP_TAP_ENERGY_SCALE: src = c->d_ges[par]; cap = c->d_ges[par] ? S * B * 8 * sizeof(float) : 0; break;
        case AT3HIP_TAP_PSY: src = c->d_psy; cap = S * B * 2 * sizeof(PsyRec); break;
        case AT3HIP_TAP_LOUDNESS: src = c->d_loud; cap = S * B * sizeof(float); break;
        case AT3HIP_TAP_QUANT: src = c->d_quant; cap = c->d_quant ? S * B * 2 * sizeof(QuantRec) : 0; break;
        case AT3HIP_TAP_GAIN_ANALYSIS: src = c->d_rec_b[par]; cap = c->d_rec_b[par] ? S * B * 6 * sizeof(GainRec) : 0; break;
        case AT3HIP_TAP_CLOCK: src = c->d_clk; cap = kClkWords * sizeof(unsigned long long); break;
        default: return fail(c, AT3HIP_EINVAL, "unknown tap");
    }
    if (!src || bytes > cap) return fail(c, AT3HIP_EINVAL, "tap not available or request too large");
    HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return AT3HIP_OK;
}

int at3hip_get_counters(at3hip_ctx* c, at3hip_counters* out, int32_t reset)
{
    if (!c || !out) return AT3HIP_EINVAL;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    const int rc = drain(c);
    if (rc != AT3HIP_OK) return rc;
    unsigned long long v[2] = {0ull, 0ull};
    HIPCHK(c, hipMemcpy(v, c->d_counters, sizeof(v), hipMemcpyDeviceToHost));
    out->scale_overflow = v[0];
    out->clipped_values = v[1];
    if (reset) {
        HIPCHK(c, hipMemsetAsync(c->d_counters, 0, sizeof(v), c->back_stream));   // (the stream whose kernels add to them)
        HIPCHK(c, hipStreamSynchronize(c->back_stream));
    }
    return AT3HIP_OK;
}

int at3hip_get_timings_ago(at3hip_ctx* c, int32_t ago, at3hip_timings* out)
{
    if (!c || !out || ago < 0 || ago >= at3hip_ctx::kSlots || ago >= c->enc_calls) return AT3HIP_EINVAL;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    const int rc = drain(c);
    if (rc != AT3HIP_OK) return rc;
    read_timings(c, (int)((c->enc_calls - 1 - ago) % at3hip_ctx::kSlots), out);
    return AT3HIP_OK;
}

namespace {

int mdct_impl(at3hip_ctx* c, float* bands, float* specs, float* max_levels, const int32_t* n_points, const int32_t* level,
              const int32_t* loc, int32_t n_items, uint32_t flags)
{
    if (!c || !bands || !specs || n_items < 1) return c ? fail(c, AT3HIP_EINVAL, "bad argument") : AT3HIP_EINVAL;
    const size_t n = n_items;
    bool dev = false;
    int rc = check_buffers(c, flags, &dev, n_points, level, loc, n * 4);
    if (rc != AT3HIP_OK) return rc;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    hipStream_t st = c->stream;
    MdctItemsParams mp;
    mp.bands = bands;
    mp.specs = specs;
    mp.max_levels = max_levels;
    if (!dev) {
        // host buffers: one staging block per context, laid out [bands | specs | max_levels | n_points | level | loc]
        if ((rc = stage_reserve(c, n * (2048 + 1024 + 4) * sizeof(float) + n * (4 + 32 + 32) * sizeof(int32_t))) != AT3HIP_OK) return rc;
        StageLayout lay{c};
        if ((rc = lay.put(bands, n * 2048, &mp.bands)) != AT3HIP_OK) return rc;
        mp.specs = lay.take<float>(n * 1024);
        mp.max_levels = lay.take<float>(n * 4);
        if (!max_levels) mp.max_levels = nullptr;
        if ((rc = lay.put_curves(n_points, level, loc, n * 4)) != AT3HIP_OK) return rc;
    }
    mp.n_points = n_points;
    mp.level = level;
    mp.loc = loc;
    hipLaunchKernelGGL(k_mdct_items, dim3((unsigned)n), dim3(128), 0, st, mp, c->d_tables);
    HIPCHK(c, hipGetLastError());
    if (!dev) {
        HIPCHK(c, hipMemcpyAsync(bands, mp.bands, n * 2048 * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(specs, mp.specs, n * 1024 * sizeof(float), hipMemcpyDeviceToHost, st));
        if (max_levels) HIPCHK(c, hipMemcpyAsync(max_levels, mp.max_levels, n * 4 * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return AT3HIP_OK;
}

}  // namespace

int at3hip_mdct(at3hip_ctx* c, float* bands, float* specs, const int32_t* n_points, const int32_t* level,
                const int32_t* loc, int32_t n_items, uint32_t flags)
{
    return mdct_impl(c, bands, specs, nullptr, n_points, level, loc, n_items, flags);
}

int at3hip_mdct_levels(at3hip_ctx* c, float* bands, float* specs, float* max_levels, const int32_t* n_points,
                       const int32_t* level, const int32_t* loc, int32_t n_items, uint32_t flags)
{
    if (!max_levels) return c ? fail(c, AT3HIP_EINVAL, "max_levels is null") : AT3HIP_EINVAL;
    return mdct_impl(c, bands, specs, max_levels, n_points, level, loc, n_items, flags);
}

int at3hip_gain_energy_scale(at3hip_ctx* c, const float* prev_overlap, const float* cur_input, const int32_t* n_points,
                             const int32_t* level, const int32_t* loc, const float* prev_overlap_scale, float* out,
                             int32_t n_items, uint32_t flags)
{
    if (!c || !prev_overlap || !cur_input || !prev_overlap_scale || !out || n_items < 1)
        return c ? fail(c, AT3HIP_EINVAL, "bad argument") : AT3HIP_EINVAL;
    const size_t n = n_items;
    bool dev = false;
    int rc = check_buffers(c, flags, &dev, n_points, level, loc, n);
    if (rc != AT3HIP_OK) return rc;
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    hipStream_t st = c->stream;
    GesItemsParams gp;
    gp.prev_overlap = prev_overlap;
    gp.cur_input = cur_input;
    gp.prev_scale = prev_overlap_scale;
    gp.out = out;
    if (!dev) {
        // host buffers: the staging block laid out [prev_overlap | cur_input | prev_scale | out | n_points | level | loc]
        if ((rc = stage_reserve(c, n * (256 + 256 + 1 + 4) * sizeof(float) + n * (1 + 8 + 8) * sizeof(int32_t))) != AT3HIP_OK) return rc;
        StageLayout lay{c};
        if ((rc = lay.put(prev_overlap, n * 256, &gp.prev_overlap)) != AT3HIP_OK) return rc;
        if ((rc = lay.put(cur_input, n * 256, &gp.cur_input)) != AT3HIP_OK) return rc;
        if ((rc = lay.put(prev_overlap_scale, n, &gp.prev_scale)) != AT3HIP_OK) return rc;
        gp.out = lay.take<float>(n * 4);
        if ((rc = lay.put_curves(n_points, level, loc, n)) != AT3HIP_OK) return rc;
    }
    gp.n_points = n_points;
    gp.level = level;
    gp.loc = loc;
    hipLaunchKernelGGL(k_ges_items, dim3((unsigned)n), dim3(64), 0, st, gp, c->d_tables);
    HIPCHK(c, hipGetLastError());
    if (!dev) HIPCHK(c, hipMemcpyAsync(out, gp.out, n * 4 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return AT3HIP_OK;
}

int at3hip_qmf_mdct(at3hip_ctx* c, const float* pcm, int32_t n_blocks, float* specs, uint32_t flags)
{
    if (!c || !pcm || !specs || n_blocks < 2) return c ? fail(c, AT3HIP_EINVAL, "bad argument") : AT3HIP_EINVAL;
    if ((flags & (AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE)) != (AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE))
        return fail(c, AT3HIP_EINVAL, "qmf_mdct needs device pointers");
    at3host::DeviceGuard guard(c->device);
    HIPCHK(c, guard.error());
    {
        const int rc = drain(c);
        if (rc != AT3HIP_OK) return rc;
    }
    hipStream_t st = c->stream;
    const int S = c->cfg.n_streams;
    // start-of-stream history: an all-zero buffer (the spare history buffer is kept zeroed for this)
    float* zero_hist = c->d_hist[c->hist_cur ^ 1];
    HIPCHK(c, hipMemsetAsync(zero_hist, 0, (size_t)S * kHist * 2 * sizeof(float), st));
    FrontParams fp;
    fp.pcm = pcm;
    fp.hist = zero_hist;
    fp.curves = nullptr;
    fp.state = nullptr;
    fp.specs = specs;
    fp.ges = nullptr;
    fp.sub = nullptr;
    fp.sub_runs = 0;
    fp.n_blocks = n_blocks;
    fp.f0 = 1;
    const int n_out = n_blocks - 1;
    fp.js = c->js;
    {
        const FusedCut cut = c->js ? FusedCut{0, 0} : pick_fused(c, n_out);
        fp.frame_runs = cut.runs;
        fp.chain = cut.chain;
    }
    HIPCHK(c, hipEventRecord(c->ev[0][0], st));
    if (c->js) {
        // joint stereo: the M/S matrixing needs both channels' subbands, which go through HBM (as in at3hip_encode)
        if (n_blocks > c->cfg.max_blocks) return fail(c, AT3HIP_EINVAL, "n_blocks exceeds max_blocks");
        // the carried subbands must be the start-of-stream zeros this entry point is defined on
        if (c->blocks_fed != 0) return fail(c, AT3HIP_EINVAL, "qmf_mdct on a joint-stereo context needs a fresh or reset context");
        fp.sub = c->d_sub;
        fp.sub_tail = c->d_sub_tail;
        fp.sub_runs = pick_runs(c, n_blocks, c->wgs_per_cu, 0.35, 4);
        const int n_waves = S * 2 * fp.sub_runs;
        hipLaunchKernelGGL(k_qmf_sub8, dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0, st, fp, c->d_tables, n_waves);
        MdctSubParams mp;
        mp.sub = c->d_sub;
        mp.curves = nullptr;
        mp.state = nullptr;
        mp.specs = specs;
        mp.n_blocks = n_blocks;
        mp.f0 = 1;
        mp.js = 1;
        mp.frame_runs = pick_runs(c, n_out, c->wgs_per_cu_mdct, 0.3);
        mp.n_waves = S * 2 * mp.frame_runs;
        hipLaunchKernelGGL((k_mdct_sub<true, 4>), dim3((unsigned)((mp.n_waves + 3) / 4)), dim3(256), 0, st, mp, c->d_tables);
    } else {
        const int n_waves = S * 2 * fp.frame_runs;
        hipLaunchKernelGGL(k_qmf_mdct8, dim3((unsigned)((n_waves + kFusedWaves - 1) / kFusedWaves)), dim3(64 * kFusedWaves), 0, st, fp, c->d_tables, n_waves);
    }
    HIPCHK(c, hipEventRecord(c->ev[0][1], st));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    memset(&c->tm, 0, sizeof(c->tm));
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, c->ev[0][0], c->ev[0][1]);
    c->tm.qmf_mdct_ms = ms;
    c->tm.total_ms = ms;
    c->tm.qmf_mdct_launches = 1;
    return AT3HIP_OK;
}

}  // extern "C"

#ifdef AT3_EMU_HOST
// SIMT HARNESS BUILDS ONLY (not in include/at3hip.h): the divisors of all 256 samples under n arbitrary
// curves (16 bytes each: n, level[7], loc[7], pad - any byte values) from the select walk the pipeline's kernels use (cell_divisors_packed) and from the
// sample-by-sample restatement of TGainProcessor::Modulate (curve_divisor), side by side: tests/test_kernels_simt_harness.py compares the bit patterns.
namespace {
__global__ __launch_bounds__(64) void k_debug_cell_divisors(const Curve* curves, const Tables* T, float* out_packed, float* out_ref, int n)
{
    __shared__ float s_gi[32];
    const int lane = threadIdx.x;
    if (lane < 32) s_gi[lane] = T->gain_interp[lane < 31 ? lane : 30];
    __syncthreads();
    const int item = blockIdx.x * 2 + (lane >> 5), cell = lane & 31;   // two curves per wavefront, a lane per cell of eight samples
    const int it = item < n ? item : n - 1;
    const uint4 w = *reinterpret_cast<const uint4*>(curves + it);
    float d[8];
    cell_divisors_packed((uint64_t)w.x | ((uint64_t)w.y << 32), (uint64_t)w.z | ((uint64_t)w.w << 32), s_gi, 8 * cell, d);
    if (item < n) {
        for (int k = 0; k < 8; ++k) {
            out_packed[(size_t)item * 256 + 8 * cell + k] = d[k];
            out_ref[(size_t)item * 256 + 8 * cell + k] = curve_divisor(s_gi, curves[it], 8 * cell + k);
        }
    }
}
}  // namespace

extern "C" __attribute__((visibility("default"))) int at3hip_debug_cell_divisors(at3hip_ctx* c, const void* curves, int32_t n, float* out_packed, float* out_ref)
{
    if (!c || !curves || n < 1 || !out_packed || !out_ref) return AT3HIP_EINVAL;
    at3host::DeviceGuard guard(c->device);
    Curve* d_cv = nullptr;
    float* d_out = nullptr;
    const size_t nb = (size_t)n * 256 * sizeof(float);
    if (hipMalloc((void**)&d_cv, (size_t)n * sizeof(Curve)) != hipSuccess || hipMalloc((void**)&d_out, 2 * nb) != hipSuccess) return AT3HIP_EDEVICE;
    int rc = AT3HIP_OK;
    if (hipMemcpy(d_cv, curves, (size_t)n * sizeof(Curve), hipMemcpyHostToDevice) != hipSuccess) rc = AT3HIP_EDEVICE;
    if (rc == AT3HIP_OK) {
        hipLaunchKernelGGL(k_debug_cell_divisors, dim3((unsigned)((n + 1) / 2)), dim3(64), 0, c->stream, d_cv, c->d_tables, d_out, d_out + (size_t)n * 256, n);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(out_packed, d_out, nb, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out_ref, d_out + (size_t)n * 256, nb, hipMemcpyDeviceToHost) != hipSuccess)
            rc = AT3HIP_EDEVICE;
    }
    (void)hipFree(d_cv);
    (void)hipFree(d_out);
    return rc;
}

// SIMT HARNESS BUILDS ONLY: k_psy's split flatness sum (flat_sums, at3_k_backend.hpp) over n BFUs of `len` lines (32 or 64) given as
// their spectral lines: per BFU the sum flat_sums hands the leader, the reference's chain over the same energies restated as a plain
// loop, and whether the chunks' sums were added (1) or the serial chain was walked (0). tests/test_flatness_split_simt_harness.py.
namespace {
__global__ __launch_bounds__(64) void k_debug_flat_sums(const float* lines, int len, double* out_sum, double* out_chain, int32_t* out_split, int n)
{
    __shared__ __attribute__((aligned(16))) float s_x[64 * 16];
    const int lane = threadIdx.x;
    const int nch = len / 16, per_wave = 64 / nch;
    const int first = blockIdx.x * per_wave;
    for (int i = lane; i < 64 * 16; i += 64) {
        const int bfu = first + i / len;
        s_x[i] = bfu < n ? lines[(size_t)bfu * len + i % len] : 0.0f;
    }
    __syncthreads();
    const int chunk = lane % nch;
    double arith, prod;
    int esum;
    bool split;
    flat_sums(s_x + 16 * lane, chunk, nch, arith, prod, esum, split);
    const int bfu = first + lane / nch;
    if (chunk == 0 && bfu < n) {
        double chain = 0.0;
        const float* x = s_x + 16 * lane;
        for (int i = 0; i < len; ++i) chain += (double)fmaxf(0.0f, x[i] * x[i]);
        out_sum[bfu] = arith;
        out_chain[bfu] = chain;
        out_split[bfu] = split ? 1 : 0;
    }
}
}  // namespace

extern "C" __attribute__((visibility("default"))) int at3hip_debug_flat_sums(at3hip_ctx* c, const float* lines, int32_t len, int32_t n, double* out_sum, double* out_chain, int32_t* out_split)
{
    if (!c || !lines || (len != 32 && len != 64) || n < 1 || !out_sum || !out_chain || !out_split) return AT3HIP_EINVAL;
    at3host::DeviceGuard guard(c->device);
    float* d_x = nullptr;
    double* d_out = nullptr;
    int32_t* d_split = nullptr;
    const size_t xb = (size_t)n * len * sizeof(float), ob = (size_t)n * sizeof(double);
    if (hipMalloc((void**)&d_x, xb) != hipSuccess || hipMalloc((void**)&d_out, 2 * ob) != hipSuccess || hipMalloc((void**)&d_split, (size_t)n * sizeof(int32_t)) != hipSuccess) {
        (void)hipFree(d_x);
        (void)hipFree(d_out);
        return AT3HIP_EDEVICE;
    }
    int rc = AT3HIP_OK;
    if (hipMemcpy(d_x, lines, xb, hipMemcpyHostToDevice) != hipSuccess) rc = AT3HIP_EDEVICE;
    if (rc == AT3HIP_OK) {
        const int per_wave = 64 / (len / 16);
        hipLaunchKernelGGL(k_debug_flat_sums, dim3((unsigned)((n + per_wave - 1) / per_wave)), dim3(64), 0, c->stream, d_x, (int)len, d_out, d_out + n, d_split, (int)n);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(out_sum, d_out, ob, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out_chain, d_out + n, ob, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out_split, d_split, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
            rc = AT3HIP_EDEVICE;
    }
    (void)hipFree(d_x);
    (void)hipFree(d_out);
    (void)hipFree(d_split);
    return rc;
}
#endif

// ---- decoder (include/at3hip.h, decoder section) -------------------------------------------------------------------------------
#include "at3_decoder_host.hpp"
#include "at3_decode.hpp"

struct at3hip_decoder : at3host::DecoderBase {
    at3hip_decoder_config cfg;
    Dec3Tables* d_tables = nullptr;
    float* d_raw = nullptr;        // [F + 2][S][2][4][512]: slots 0, 1 = the carried frames -2, -1
    Dec3Gains* d_gains = nullptr;  // [F + 2][S][2]
    // (d_in: the frames [S][F][frame_size], d_out: [S][F][1024][2], d_rejected: [kDec3Reasons])
};

namespace {

// false when the encoder's table block cannot be allocated (the decoder is then not created)
__attribute__((optnone, noinline)) bool build_dec3_tables(Dec3Tables* t)
{
    Tables* enc = new (std::nothrow) Tables();   // the shared entries: the encoder's builder computes them the reference's way
    if (!enc) return false;
    build_tables(enc);
    memcpy(t->qmf_win, enc->qmf_win, sizeof(t->qmf_win));
    memcpy(t->scale, enc->scale, sizeof(t->scale));
    memcpy(t->gain_level, enc->gain_level, sizeof(t->gain_level));
    memcpy(t->gain_interp, enc->gain_interp, sizeof(t->gain_interp));
    memcpy(t->tw128, enc->tw128, sizeof(t->tw128));
    for (int i = 0; i < 256; ++i) {   // DecodeWindow (atrac3.h) from the float EncodeWindow, times 2 as Midct applies it
        const double a = enc->enc_win[i], b = enc->enc_win[255 - i];
        const float dw = 2.0 * a / (a * a + b * b);
        t->dwin2[i] = 2 * dw;
    }
    delete enc;
    static const float max_quant[8] = {0.0f, 1.5f, 2.5f, 3.5f, 4.5f, 7.5f, 15.5f, 31.5f};   // MaxQuant (atrac3.h)
    t->inv_maxq[0] = 0.0f;
    for (int wl = 1; wl < 8; ++wl) t->inv_maxq[wl] = 1.0 / (double)max_quant[wl];
    mdct_sincos(t->cs512, 512, 256.0f);   // TMIDCT<512>(): TMIDCT(float scale = TN) : TMDCTBase(TN, scale / 2)
    memset(t->vlc, 0, sizeof(t->vlc));    // filled on the device from c_huff (k_at3d_vlc_lut)
    return true;
}

int dec3_reset_state(at3hip_decoder* d)
{
    const size_t S = d->cfg.n_streams;
    HIPCHK(d, hipMemsetAsync(d->d_raw, 0, 2 * S * 2 * 2048 * sizeof(float), d->stream));
    HIPCHK(d, hipMemsetAsync(d->d_gains, 0, 2 * S * 2 * sizeof(Dec3Gains), d->stream));
    HIPCHK(d, hipMemsetAsync(d->d_rejected, 0, kDec3Reasons * sizeof(unsigned long long), d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    return AT3HIP_OK;
}

bool dec3_row_ok(int frame_size, int js)
{
    static const int rows[8][2] = {{192, 1}, {272, 1}, {304, 0}, {384, 0}, {424, 0}, {512, 0}, {768, 0}, {1024, 0}};
    for (const auto& r : rows)
        if (r[0] == frame_size && r[1] == js) return true;
    return false;
}

}  // namespace

extern "C" {

int at3hip_decoder_create(const at3hip_decoder_config* cfg, at3hip_decoder** out)
{
    if (!cfg || !out) return AT3HIP_EINVAL;
    *out = nullptr;
    if (!dec3_row_ok(cfg->frame_size, cfg->joint_stereo) || cfg->n_streams < 1 || cfg->max_frames < 1) return AT3HIP_EINVAL;
    if ((long long)cfg->n_streams * 2 > at3host::kMaxGridY) return AT3HIP_EINVAL;   // (stream, unit) is gridDim.y
    // every buffer index stays inside size_t and the kernels' int frame counts
    if (((long long)cfg->max_frames + 2) * cfg->n_streams > (1ll << 31) / 4096) return AT3HIP_EINVAL;
    return at3host::create_decoder(cfg, out, build_dec3_tables, at3hip_decoder_destroy, [](at3hip_decoder* d) {
        hipLaunchKernelGGL(k_at3d_vlc_lut, dim3(1), dim3(256), 0, d->stream, d->d_tables);
        if (hipGetLastError() != hipSuccess) return AT3HIP_EDEVICE;
        const size_t S = d->cfg.n_streams, F = d->cfg.max_frames;
        int rc;
        if ((rc = dev_alloc(d, &d->d_in, S * F * d->cfg.frame_size)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_raw, (F + 2) * S * 2 * 2048)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_gains, (F + 2) * S * 2)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_rejected, kDec3Reasons)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(d, &d->d_out, S * F * 2048)) != AT3HIP_OK) return rc;
        return dec3_reset_state(d);
    });
}

void at3hip_decoder_destroy(at3hip_decoder* d)
{
    if (d) at3host::destroy_engine(d);
}

const char* at3hip_decoder_last_error(const at3hip_decoder* d) { return at3host::engine_last_error(d); }

int at3hip_decoder_sync(at3hip_decoder* d) { return at3host::engine_sync(d); }

int at3hip_decoder_reset(at3hip_decoder* d) { return at3host::guarded(d, dec3_reset_state); }

int at3hip_decoder_set_stream(at3hip_decoder* d, void* hip_stream) { return at3host::engine_set_stream(d, hip_stream); }

int at3hip_decoder_get_counters(at3hip_decoder* d, at3hip_decoder_counters* out, int32_t reset)
{
    if (!d || !out) return AT3HIP_EINVAL;
    unsigned long long h[kDec3Reasons] = {0, 0, 0, 0, 0, 0};
    const int rc = at3host::read_counters(d, h, reset);
    if (rc != AT3HIP_OK) return rc;
    out->bad_id = h[0];
    out->unsupported_js = h[1];
    out->read_past_end = h[2];
    out->tonal_past_end = h[3];
    out->bad_tonal_mode = h[4];
    out->bad_tonal_quant = h[5];
    return AT3HIP_OK;
}
}  // extern "C"

namespace {

// The kernels of one at3hip_decode call: n_frames frames per stream from d_frames into d_pcm, both device memory.
int dec3_launch(at3hip_decoder* d, const uint8_t* d_frames, int n_frames, void* d_pcm, bool s16)
{
    const size_t S = d->cfg.n_streams, F = (size_t)n_frames, fsz = d->cfg.frame_size;
    hipStream_t st = d->stream;
    Dec3UnpackParams up;
    up.T = d->d_tables;
    up.frames = d_frames;
    up.n_frames = n_frames;
    up.n_streams = (int)S;
    up.frame_sz = (int)fsz;
    up.js = d->cfg.joint_stereo;
    up.raw = d->d_raw;
    up.gains = d->d_gains;
    up.rejected = d->d_rejected;
    hipLaunchKernelGGL(k_at3d_unpack, dim3((unsigned)F, (unsigned)(2 * S)), dim3(kDec3UnpackThreads), 0, st, up);
    HIPCHK(d, hipGetLastError());
    Dec3SynthParams sp;
    sp.T = d->d_tables;
    sp.raw = d->d_raw;
    sp.gains = d->d_gains;
    sp.out = d_pcm;
    sp.n_frames = n_frames;
    sp.n_streams = (int)S;
    sp.js = d->cfg.joint_stereo;
    sp.s16 = s16 ? 1 : 0;
    hipLaunchKernelGGL(k_at3d_synth, dim3((unsigned)F, (unsigned)S), dim3(256), 0, st, sp);
    HIPCHK(d, hipGetLastError());
    hipLaunchKernelGGL(k_at3d_state, dim3((unsigned)(2 * S)), dim3(256), 0, st, d->d_raw, d->d_gains, n_frames, (int32_t)S);
    HIPCHK(d, hipGetLastError());
    return AT3HIP_OK;
}

}  // namespace

extern "C" int at3hip_decode(at3hip_decoder* d, const uint8_t* frames, int32_t n_frames, void* pcm, uint32_t flags)
{
    return at3host::decode_call(d, frames, n_frames, pcm, flags, AT3HIP_DECODE_S16, AT3HIP_DECODE_S16, d ? (size_t)d->cfg.frame_size : 0, 2048,
                                [&](const uint8_t* d_frames, void* d_pcm) { return dec3_launch(d, d_frames, n_frames, d_pcm, flags & AT3HIP_DECODE_S16); });
}
