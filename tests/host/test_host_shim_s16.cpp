// The 16-bit PCM entry points of the host-side C++ mirror (atracdenc_amd/host/at3hip_host.hpp: TAtrac1Encoder::EncodeS16,
// TAt3PEncoder::EncodeS16, TResampler::ProcessS16 and its 16-bit outputs, TLoudnessMeter::ProcessS16 / ApplyS16) against the
// float entry points of the same classes on s / 32768.0f, bit for bit. Stand-alone: links libat3hip.so only. The argument
// checks that need no device come first; on a machine without a GPU the program stops behind them and says so.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../atracdenc_amd/host/at3hip_host.hpp"

using namespace NAtracDEncHip;

struct TMemOut : ICompressedOutput {
    std::vector<std::vector<char>>* Frames;
    size_t Channels;
    TMemOut(std::vector<std::vector<char>>* f, size_t channels) : Frames(f), Channels(channels) {}
    void WriteFrame(std::vector<char> data) override { Frames->push_back(std::move(data)); }
    std::string GetName() const override { return "mem"; }
    size_t GetChannelNum() const override { return Channels; }
};

static int fails = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);      \
            ++fails;                                                   \
        }                                                              \
    } while (0)

// Only in a build of the library's sources through the CPU SIMT harness (tools/emu/emu_runtime.cpp): n more device allocations
// succeed, every later one is refused. Against libat3hip.so the symbol is absent and the part that uses it is skipped.
extern "C" void emu_fail_alloc_after(long n) __attribute__((weak));

// Refuses every device allocation of create(cfg) in turn: each time the create must report AT3HIP_ENOMEM, give no context and
// have released the half-made one (the sanitizers this program is run under see a leak or a double free). Returns the
// number of allocations of a create that succeeds.
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

template <class T>
static bool SameBytes(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main()
{
    // ---- without a device: a null context is AT3HIP_EINVAL at every 16-bit entry point ----
    {
        int16_t in[8] = {0};
        uint8_t out[8];
        float fout[8], g = 1.0f;
        int32_t n = 0;
        EXPECT(at1hip_encode_short(nullptr, in, 1, out, 0) == AT3HIP_EINVAL);
        EXPECT(at3phip_encode_frames_short(nullptr, in, 1, out, 0) == AT3HIP_EINVAL);
        EXPECT(at3hip_resampler_process_s16(nullptr, in, 1, fout, &n, 0) == AT3HIP_EINVAL);
        EXPECT(at3hip_resampler_process_s16(nullptr, in, 1, fout, &n, AT3HIP_RESAMPLE_OUT_S16) == AT3HIP_EINVAL);
        EXPECT(at3hip_loudness_process_s16(nullptr, in, 1, 0) == AT3HIP_EINVAL);
        EXPECT(at3hip_loudness_apply_s16(nullptr, in, 1, &g, fout, 0) == AT3HIP_EINVAL);
        static_assert(AT3HIP_RESAMPLE_OUT_S16 == AT3HIP_DECODE_S16, "the decoders' bit");
        printf("null-context argument checks done\n");
    }
    at1hip_config probe{};
    probe.channels = 2;
    probe.window_auto = 1;
    probe.n_streams = 1;
    probe.max_blocks = 1;
    at1hip_ctx* ctx = nullptr;
    if (at1hip_create(&probe, &ctx) != AT3HIP_OK) {
        printf("no usable device: stopped behind the argument checks\n");
        printf(fails ? "HOST SHIM S16 TEST FAILED\n" : "HOST SHIM S16 TEST OK (argument checks only)\n");
        return fails ? 1 : 0;
    }
    at1hip_destroy(ctx);

    if (emu_fail_alloc_after) {   // ---- creates that fail half-way, for the three encoders ----
        at3phip_config p3{};
        p3.channels = 2;
        p3.n_streams = 2;
        p3.max_frames = 2;
        at3hip_config c3{};
        c3.channels = 2;
        c3.n_streams = 2;
        c3.max_blocks = 2;
        at3hip_config c3m = c3;   // one channel, joint stereo, no gain control: the other set of buffers and streams
        c3m.channels = 1;
        c3m.bitrate = 66150;
        c3m.no_gain_control = 1;
        const int n1 = HalfMadeCreates(at1hip_create, at1hip_destroy, probe), np = HalfMadeCreates(at3phip_create, at3phip_destroy, p3);
        const int n3 = HalfMadeCreates(at3hip_create, at3hip_destroy, c3), n3m = HalfMadeCreates(at3hip_create, at3hip_destroy, c3m);
        EXPECT(n1 > 0 && np > 0 && n3 > 0 && n3m > 0);
        printf("half-made creates: %d (at1hip), %d (at3phip), %d and %d (at3hip) allocations refused in turn\n", n1, np, n3, n3m);
    }

    // full-range noise with both extremes, a silence and a full-scale burst behind it
    const int C = 2, n = 5 * 2048;   // sample frames
    std::vector<int16_t> p16((size_t)n * C);
    std::vector<float> pf(p16.size());
    uint32_t lcg = 12345u;
    for (size_t i = 0; i < p16.size(); ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        p16[i] = (int16_t)(lcg >> 16);
    }
    p16[2] = -32768;
    p16[5] = 32767;
    for (int i = 3000; i < 5000; ++i) p16[2 * i] = p16[2 * i + 1] = 0;
    for (int i = 5000; i < 5200; ++i) p16[2 * i] = p16[2 * i + 1] = ((i / 50) % 2) ? 32767 : -32768;
    for (size_t i = 0; i < p16.size(); ++i) pf[i] = (float)p16[i] / 32768.0f;

    {   // ---- TAtrac1Encoder: 20 blocks, the lambda on floats against EncodeS16 (12 blocks in calls of <= 8) behind 8 lambda calls ----
        std::vector<std::vector<char>> want, got;
        {
            TAtrac1Encoder enc(TCompressedOutputPtr(new TMemOut(&want, C)), TAtrac1EncodeSettings(), 8);
            auto lambda = enc.GetLambda();
            for (int b = 0; b < 20; ++b) lambda(pf.data() + (size_t)b * 512 * C, ProcessMeta{2});
        }
        {
            TAtrac1Encoder enc(TCompressedOutputPtr(new TMemOut(&got, C)), TAtrac1EncodeSettings(), 8);
            auto lambda = enc.GetLambda();
            for (int b = 0; b < 8; ++b) lambda(pf.data() + (size_t)b * 512 * C, ProcessMeta{2});
            enc.EncodeS16(p16.data() + (size_t)8 * 512 * C, 12);
        }
        EXPECT(want.size() == 40 && got == want);
        printf("TAtrac1Encoder::EncodeS16: %d units compared\n", (int)got.size());
    }
    {   // ---- TAt3PEncoder: 5 frames, the lambda against 2 lambda calls and EncodeS16 of 3 frames (calls of <= 2) ----
        std::vector<std::vector<char>> want, got;
        {
            TAt3PEncoder enc(TCompressedOutputPtr(new TMemOut(&want, C)), C, 2);
            auto lambda = enc.GetLambda();
            for (int f = 0; f < 5; ++f) lambda(pf.data() + (size_t)f * 2048 * C, ProcessMeta{2});
        }
        {
            TAt3PEncoder enc(TCompressedOutputPtr(new TMemOut(&got, C)), C, 2);
            auto lambda = enc.GetLambda();
            for (int f = 0; f < 2; ++f) lambda(pf.data() + (size_t)f * 2048 * C, ProcessMeta{2});
            EXPECT(!enc.EncodeS16(p16.data() + (size_t)2 * 2048 * C, 3));
        }
        EXPECT(want.size() == 4 && got == want);
        printf("TAt3PEncoder::EncodeS16: %d frames compared\n", (int)got.size());
    }
    {   // ---- TResampler: 48000 -> 44100, 1001 + 333 samples + flush; float and 16-bit outputs ----
        TResampler a(48000, 44100, C, 1001, 0), b(48000, 44100, C, 1001, 0);
        std::vector<float> want, got;
        b.Process(pf.data(), 1001, want);
        b.Process(pf.data() + (size_t)1001 * C, 333, want);
        b.Flush(want);
        a.ProcessS16(p16.data(), 1001, got);
        a.Process(pf.data() + (size_t)1001 * C, 333, got);
        a.Flush(got);
        EXPECT(!want.empty() && SameBytes(got, want));
        std::vector<int16_t> want16(want.size()), got16;
        for (size_t i = 0; i < want.size(); ++i) want16[i] = (int16_t)lrintf(std::max(-1.0f, std::min(1.0f, want[i])) * 32767.0f);
        a.Process(pf.data(), 1001, got16);
        a.ProcessS16(p16.data() + (size_t)1001 * C, 333, got16);
        a.Flush(got16);
        EXPECT(SameBytes(got16, want16));
        printf("TResampler::ProcessS16 and 16-bit outputs: %d samples compared\n", (int)got.size());
    }
    {   // ---- TLoudnessMeter: ProcessS16 and ApplyS16 ----
        TLoudnessMeter a(C, (uint64_t)n, true, 0), b(C, (uint64_t)n, true, 0);
        b.Process(pf.data(), (size_t)n);
        a.ProcessS16(p16.data(), 5000);
        a.Process(pf.data() + (size_t)5000 * C, (size_t)n - 5000);
        const at3hip_loudness_result rb = b.Finish(), ra = a.Finish();
        EXPECT(rb.n_hops == n / AT3HIP_LOUDNESS_HOP && memcmp(&ra, &rb, sizeof(ra)) == 0);
        std::vector<float> want(pf), got(pf.size());
        b.Apply(want.data(), (size_t)n, 0.7371f);
        a.ApplyS16(p16.data(), (size_t)n, 0.7371f, got.data());
        EXPECT(SameBytes(got, want));
        printf("TLoudnessMeter::ProcessS16 / ApplyS16 compared (integrated %.2f LUFS)\n", ra.integrated);
    }
    printf(fails ? "HOST SHIM S16 TEST FAILED\n" : "HOST SHIM S16 TEST OK\n");
    return fails ? 1 : 0;
}
