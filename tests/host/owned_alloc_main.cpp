// TEST INFRASTRUCTURE: every engine's device allocations, the lazily made ones included, are released by its destroy.
// Stand-alone (tests/test_owned_alloc_cpu.py builds and runs it): the library's sources compiled for the host with
// tools/emu/emu_runtime.cpp, whose hipMalloc / hipFree are malloc / free, under -fsanitize=address,undefined with leak
// detection on. Each engine is created, makes one host-memory call of every kind that allocates on first use, and is
// destroyed; then every device allocation of each create is refused in turn (emu_fail_alloc_after) and the half-made
// context must be released. Exit status 0 and no sanitizer report is a pass. The samples are silence.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/at1hip.h"
#include "../../include/at3hip.h"
#include "../../include/at3hip_loudness.h"
#include "../../include/at3hip_resample.h"
#include "../../include/at3phip.h"

extern "C" void emu_fail_alloc_after(long n);

static int fails = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);      \
            ++fails;                                                   \
        }                                                              \
    } while (0)
#define OK(call) EXPECT((call) == AT3HIP_OK)

// Refuses every device allocation of create(cfg) in turn; returns the number of allocations of a create that succeeds.
template <class Cfg, class Ctx>
static int HalfMadeCreates(int (*create)(const Cfg*, Ctx**), void (*destroy)(Ctx*), const Cfg& cfg)
{
    for (int n = 0; n < 100; ++n) {
        emu_fail_alloc_after(n);
        Ctx* c = nullptr;
        const int rc = create(&cfg, &c);
        emu_fail_alloc_after(-1);
        if (rc == AT3HIP_OK) {
            destroy(c);
            return n;
        }
        EXPECT(rc == AT3HIP_ENOMEM && c == nullptr);
    }
    return -1;
}

int main()
{
    enum { S = 2, C = 2, B = 2 };   // streams, channels, blocks / frames per call
    std::vector<float> f32((size_t)S * 4500 * C, 0.0f), fout(f32.size());
    std::vector<int16_t> i16(f32.size(), 0);
    std::vector<uint8_t> bytes((size_t)S * B * 4096, 0);
    int32_t n = 0;

    at3hip_config c3{};
    c3.channels = C;
    c3.n_streams = S;
    c3.max_blocks = B;
    {   // ---- ATRAC3 encoder: staging pairs by parity, quant tap on / off / on, the stage-level staging growing ----
        at3hip_ctx* c = nullptr;
        OK(at3hip_create(&c3, &c));
        for (int call = 0; call < 2; ++call) OK(at3hip_encode(c, f32.data(), B, bytes.data(), &n, 0));
        for (int call = 0; call < 2; ++call) OK(at3hip_encode_s16(c, i16.data(), B, bytes.data(), &n, 0));
        OK(at3hip_set_option(c, AT3HIP_OPT_QUANT_TAP, 1));
        OK(at3hip_set_option(c, AT3HIP_OPT_QUANT_TAP, 0));
        OK(at3hip_set_option(c, AT3HIP_OPT_QUANT_TAP, 1));
        std::vector<float> bands(4 * 2048, 0.0f), specs(4 * 1024), mx(4 * 4), ges(4 * 4), scale(4, 1.0f);
        std::vector<int32_t> np(16, 0), lv(128, 0), lc(128, 0);
        OK(at3hip_mdct(c, bands.data(), specs.data(), nullptr, nullptr, nullptr, 1, 0));
        OK(at3hip_mdct_levels(c, bands.data(), specs.data(), mx.data(), np.data(), lv.data(), lc.data(), 4, 0));   // (grows)
        OK(at3hip_gain_energy_scale(c, bands.data(), bands.data(), np.data(), lv.data(), lc.data(), scale.data(), ges.data(), 4, 0));
        at3hip_destroy(c);
    }
    at1hip_config c1{};
    c1.channels = C;
    c1.window_auto = 1;
    c1.n_streams = S;
    c1.max_blocks = B;
    {   // ---- ATRAC1 encoder: the 16-bit staging ----
        at1hip_ctx* c = nullptr;
        OK(at1hip_create(&c1, &c));
        OK(at1hip_encode(c, f32.data(), B, bytes.data(), 0));
        OK(at1hip_encode_short(c, i16.data(), B, bytes.data(), 0));
        at1hip_destroy(c);
    }
    at3phip_config cp{};
    cp.channels = C;
    cp.n_streams = S;
    cp.max_frames = B;
    {   // ---- ATRAC3plus encoder: the 16-bit staging, the caller's tonal records, the tone analysis ----
        at3phip_ctx* c = nullptr;
        OK(at3phip_create(&cp, &c));
        OK(at3phip_encode_frames(c, f32.data(), B, bytes.data(), 0));
        OK(at3phip_encode_frames_short(c, i16.data(), B, bytes.data(), 0));
        std::vector<at3phip_tonal_block> tonal((size_t)S * B);
        for (auto& t : tonal) t = at3phip_tonal_block{};
        tonal[0].num_tone_bands = 1;
        tonal[0].band[0][0].n_waves = 1;
        tonal[0].wave[0] = 100u | 20u << 10;
        OK(at3phip_write_frames_tonal(c, f32.data(), B, nullptr, tonal.data(), bytes.data(), 0));
        OK(at3phip_analyse_tones(c, f32.data(), B, tonal.data(), fout.data(), 0));
        OK(at3phip_encode_frames_tonal(c, f32.data(), B, bytes.data(), 0));
        OK(at3phip_encode_frames_tonal_short(c, i16.data(), B, bytes.data(), 0));
        at3phip_destroy(c);
    }
    at1hip_decoder_config d1{};
    d1.channels = C;
    d1.n_streams = S;
    d1.max_frames = B;
    at3hip_decoder_config d3{};
    d3.n_streams = S;
    d3.frame_size = 384;
    d3.max_frames = B;
    at3phip_decoder_config dp{};
    dp.channels = C;
    dp.n_streams = S;
    dp.max_frames = B;
    {   // ---- the three decoders: float and 16-bit output to host memory ----
        at1hip_decoder* a = nullptr;
        OK(at1hip_decoder_create(&d1, &a));
        OK(at1hip_decode(a, bytes.data(), B, fout.data(), 0));
        OK(at1hip_decode(a, bytes.data(), B, fout.data(), AT1HIP_DECODE_S16));
        at1hip_decoder_destroy(a);
        at3hip_decoder* b = nullptr;
        OK(at3hip_decoder_create(&d3, &b));
        OK(at3hip_decode(b, bytes.data(), B, fout.data(), 0));
        OK(at3hip_decode(b, bytes.data(), B, fout.data(), AT3HIP_DECODE_S16));
        at3hip_decoder_destroy(b);
        at3phip_decoder* p = nullptr;
        OK(at3phip_decoder_create(&dp, &p));
        OK(at3phip_decode(p, bytes.data(), B, fout.data(), 0));
        OK(at3phip_decode(p, bytes.data(), B, fout.data(), AT3PHIP_DECODE_S16 | AT3PHIP_DECODE_TONES));
        at3phip_decoder_destroy(p);
    }
    at3hip_resampler_config cr{};
    cr.in_rate = 48000;
    cr.out_rate = 44100;
    cr.channels = C;
    cr.n_streams = S;
    cr.max_in = 64;
    {   // ---- resampler: both input stagings, the output staging made by a flush ----
        at3hip_resampler* r = nullptr;
        OK(at3hip_resampler_create(&cr, &r));
        OK(at3hip_resampler_process(r, f32.data(), 64, fout.data(), &n, AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE));
        OK(at3hip_resampler_flush(r, fout.data(), &n, 0));
        OK(at3hip_resampler_process(r, f32.data(), 64, fout.data(), &n, 0));
        OK(at3hip_resampler_process_s16(r, i16.data(), 64, fout.data(), &n, AT3HIP_RESAMPLE_OUT_S16));
        at3hip_resampler_destroy(r);
    }
    at3hip_loudness_config cl{};
    cl.channels = C;
    cl.n_streams = S;
    cl.max_in = 4500;
    cl.max_hops = 4;
    {   // ---- meter and limiter: input stagings, apply's output, the limiter's buffers, table and output ----
        at3hip_loudness* l = nullptr;
        const float gains[S] = {1.0f, 1.0f};
        OK(at3hip_loudness_create(&cl, &l));
        OK(at3hip_loudness_process(l, f32.data(), 4500, 0));
        OK(at3hip_loudness_process_s16(l, i16.data(), 64, 0));
        OK(at3hip_loudness_apply(l, f32.data(), 64, gains, fout.data(), 0));
        OK(at3hip_loudness_limit_start(l, gains, 0.5f, AT3HIP_LIMIT_TRUE_PEAK));
        OK(at3hip_loudness_limit(l, f32.data(), 512, fout.data(), &n, 0));
        OK(at3hip_loudness_limit_s16(l, i16.data(), 512, fout.data(), &n, 0));
        OK(at3hip_loudness_limit_flush(l, fout.data(), &n, 0));
        OK(at3hip_loudness_limit_start(l, gains, 0.5f, 0));   // (a second start allocates nothing)
        at3hip_loudness_destroy(l);
    }
    // ---- creates that fail half-way ----
    cl.true_peak = 1;
    const int counts[] = {HalfMadeCreates(at3hip_create, at3hip_destroy, c3), HalfMadeCreates(at1hip_create, at1hip_destroy, c1),
                          HalfMadeCreates(at3phip_create, at3phip_destroy, cp), HalfMadeCreates(at1hip_decoder_create, at1hip_decoder_destroy, d1),
                          HalfMadeCreates(at3hip_decoder_create, at3hip_decoder_destroy, d3), HalfMadeCreates(at3phip_decoder_create, at3phip_decoder_destroy, dp),
                          HalfMadeCreates(at3hip_resampler_create, at3hip_resampler_destroy, cr), HalfMadeCreates(at3hip_loudness_create, at3hip_loudness_destroy, cl)};
    for (int k : counts) {
        EXPECT(k > 0);
        printf("half-made creates: %d allocations refused in turn\n", k);
    }
    printf(fails ? "OWNED ALLOCATIONS FAILED\n" : "OWNED ALLOCATIONS OK\n");
    return fails ? 1 : 0;
}
