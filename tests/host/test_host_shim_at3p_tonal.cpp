// TAt3PEncoder with a tonal analyser (atracdenc_amd/host/at3hip_host.hpp: TAt3PSettings, IAt3PGhaProcessor) against the frames
// the reference's own TAt3PEnc wrote around the same stand-in analyser (tests/host/at3p_fake_gha.h) for UseGha = 0, 1, 5 and 7:
// the schedule cases of tests/golden/at3p_tonal_write.npz, which the caller exports to the file named by argv[1]
// (tests/at3p_tonal_write_lib.export_schedule: PCM and golden frames per case). Stand-alone: links libat3hip.so only. The
// argument checks that need no device come first; on a machine without a GPU the program stops behind them and says so.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../atracdenc_amd/host/at3hip_host.hpp"
#include "at3p_fake_gha.h"

using namespace NAtracDEncHip;

struct TMemOut : ICompressedOutput {
    std::vector<std::vector<char>>* Frames;
    size_t Channels;
    TMemOut(std::vector<std::vector<char>>* f, size_t channels) : Frames(f), Channels(channels) {}
    void WriteFrame(std::vector<char> data) override { Frames->push_back(std::move(data)); }
    std::string GetName() const override { return "mem"; }
    size_t GetChannelNum() const override { return Channels; }
};

// the stand-in analyser behind the mirror's interface; it also checks what the mirror hands it
struct TFakeGha : IAt3PGhaProcessor {
    int Channels, Calls = 0, BadArgs = 0;
    const float* Pcm;   // the case's PCM [calls][2048][C]: raw*Cur of analysis k is input frame k
    at3phip_tonal_block Block;
    TFakeGha(int channels, const float* pcm) : Channels(channels), Pcm(pcm) {}
    const at3phip_tonal_block* DoAnalize(TBufPtr b1, TBufPtr b2, float* w1, float* w2, const float* raw1Cur, const float* raw2Cur) override
    {
        const int k = Calls++;
        if (!b1[0] || !b1[1] || !w1 || !raw1Cur || (Channels == 2) != (b2[0] && b2[1] && w2 && raw2Cur)) ++BadArgs;
        for (int i = 0; i < 2048 && !BadArgs; ++i) {
            if (raw1Cur[i] != Pcm[((size_t)k * 2048 + i) * Channels]) ++BadArgs;
            if (Channels == 2 && raw2Cur[i] != Pcm[((size_t)k * 2048 + i) * 2 + 1]) ++BadArgs;
        }
        at3p_fake_gha_modify(k, w1, w2);
        return at3p_fake_gha_block(k, Channels, &Block) ? &Block : nullptr;
    }
};

static int fails = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);      \
            ++fails;                                                   \
        }                                                              \
    } while (0)

int main(int argc, char** argv)
{
    {   // ---- without a device: a null context is AT3HIP_EINVAL ----
        float specs[1] = {0};
        uint8_t out[1];
        at3phip_tonal_block t{};
        EXPECT(at3phip_write_frames_tonal(nullptr, specs, 1, nullptr, &t, out, 0) == AT3HIP_EINVAL);
        static_assert(sizeof(at3phip_tonal_block) == 324, "the record's documented size");
        printf("null-context argument check done\n");
    }
    if (argc != 2) {
        printf("usage: %s schedule.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    int32_t nCases = 0;
    if (!f || fread(&nCases, 4, 1, f) != 1) {
        printf("cannot read %s\n", argv[1]);
        return 2;
    }
    {
        at3phip_config probe{};
        probe.channels = 2;
        probe.n_streams = 1;
        probe.max_frames = 1;
        at3phip_ctx* ctx = nullptr;
        if (at3phip_create(&probe, &ctx) != AT3HIP_OK) {
            printf("no usable device: stopped behind the argument checks\n");
            printf(fails ? "HOST SHIM AT3P TONAL TEST FAILED\n" : "HOST SHIM AT3P TONAL TEST OK (argument checks only)\n");
            fclose(f);
            return fails ? 1 : 0;
        }
        at3phip_destroy(ctx);
    }
    for (int c = 0; c < nCases; ++c) {
        int32_t h[4];   // channels, UseGha, calls, frames
        if (fread(h, 4, 4, f) != 4) return 2;
        const int C = h[0], nCalls = h[2], nFrames = h[3];
        std::vector<float> pcm((size_t)nCalls * 2048 * C);
        std::vector<uint8_t> want((size_t)nFrames * 2048);
        if (fread(pcm.data(), 4, pcm.size(), f) != pcm.size() || fread(want.data(), 1, want.size(), f) != want.size()) return 2;
        for (int batch : {3, 64}) {   // calls split 3 + 3 + 2 (state carried between flushes), and all in the destructor's flush
            std::vector<std::vector<char>> frames;
            TFakeGha gha(C, pcm.data());
            TAt3PSettings settings;
            settings.UseGha = (uint8_t)h[1];
            {
                TAt3PEncoder enc(TCompressedOutputPtr(new TMemOut(&frames, (size_t)C)), C, batch, 0, settings, &gha);
                auto lambda = enc.GetLambda();
                for (int k = 0; k < nCalls; ++k) {
                    const auto r = lambda(pcm.data() + (size_t)k * 2048 * C, ProcessMeta{(uint16_t)C});
                    EXPECT((k == 0) == (r == EProcessResult::LOOK_AHEAD));
                }
            }   // destructor flushes
            EXPECT((int)frames.size() == nFrames && gha.Calls == nCalls - 1 && gha.BadArgs == 0);
            int bad = 0;
            for (int i = 0; i < nFrames && i < (int)frames.size(); ++i)
                bad += frames[i].size() != 2048 || memcmp(frames[i].data(), want.data() + (size_t)i * 2048, 2048) != 0;
            EXPECT(bad == 0);
            printf("TAt3PEncoder channels %d UseGha %d batch %d: %d frames compared, %d differ\n", C, h[1], batch, (int)frames.size(), bad);
        }
    }
    fclose(f);
    printf(fails ? "HOST SHIM AT3P TONAL TEST FAILED\n" : "HOST SHIM AT3P TONAL TEST OK\n");
    return fails ? 1 : 0;
}
