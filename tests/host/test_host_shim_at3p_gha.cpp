// TAt3PToneAnalyser and TAt3PEncoder's two tone modes (atracdenc_amd/host/at3hip_host.hpp), under any combination of
// AT3PHIP_TONES_GATED and AT3PHIP_TONES_SHARED, against the C restatement of the tone analysis (tests/host/at3p_gha_cpu.c): the
// caller exports cases to the file named by argv[1] (tests/at3p_gha_lib.py, export_shim_cases: per case the analysis flags, the
// PCM, the subband samples, the restatement's records and residuals, and the frames its pipeline predicts; a case without PCM
// compares the analyser alone). Stand-alone: links libat3hip.so - or the host-compiled kernels, which makes it runnable without a
// GPU and under ASan / UBSan by the recipe of DESIGN.md section 1 - and nothing else. The checks that need no context come first.
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

static int differing(const std::vector<std::vector<char>>& frames, const std::vector<uint8_t>& want, int n)
{
    int bad = 0;
    for (int i = 0; i < n; ++i) bad += i >= (int)frames.size() || frames[i].size() != 2048 || memcmp(frames[i].data(), want.data() + (size_t)i * 2048, 2048) != 0;
    return bad;
}

int main(int argc, char** argv)
{
    {   // ---- without a device: null contexts, a wrong table size and a wrong channel count are AT3HIP_EINVAL; the capability call ----
        float x[1] = {0};
        uint8_t out[1];
        at3phip_tonal_block t{};
        char small[16];
        EXPECT(at3phip_analyse_tones(nullptr, x, 1, &t, x, 0) == AT3HIP_EINVAL);
        EXPECT(at3phip_encode_frames_tonal(nullptr, x, 1, out, 0) == AT3HIP_EINVAL);
        EXPECT(at3phip_encode_frames_tonal_short(nullptr, (const int16_t*)x, 1, out, 0) == AT3HIP_EINVAL);
        EXPECT(at3phip_host_tone_find_tables(small, sizeof(small)) == AT3HIP_EINVAL);
        EXPECT(at3phip_host_tone_gates(nullptr, 1, 1, out) == AT3HIP_EINVAL);
        EXPECT(at3phip_host_tone_gates(x, 1, 3, out) == AT3HIP_EINVAL);
        EXPECT(at3phip_host_tone_gates(x, 0, 1, out) == AT3HIP_OK);
        EXPECT(at3phip_host_tone_flags() == (AT3PHIP_TONES_GATED | AT3PHIP_TONES_SHARED));
        printf("argument checks done\nflags understood %u\n", at3phip_host_tone_flags());
    }
    if (argc != 2) {
        printf("usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    int32_t nCases = 0;
    if (!f || fread(&nCases, 4, 1, f) != 1) {
        printf("cannot read %s\n", argv[1]);
        return 2;
    }
    bool device = false;
    {
        at3phip_config probe{};
        probe.channels = 2;
        probe.n_streams = 1;
        probe.max_frames = 1;
        at3phip_ctx* ctx = nullptr;
        device = at3phip_create(&probe, &ctx) == AT3HIP_OK;
        if (device) at3phip_destroy(ctx);
        else printf("no usable device: the analyser alone is compared\n");
    }
    for (int c = 0; c < nCases; ++c) {
        int32_t h[4];   // channels, frames, analysis flags, 1: PCM and predicted frames follow
        if (fread(h, 4, 4, f) != 4) return 2;
        const int C = h[0], n = h[1], withPcm = h[3];
        const bool gated = (h[2] & AT3PHIP_TONES_GATED) != 0, shared = (h[2] & AT3PHIP_TONES_SHARED) != 0;
        const size_t FF = (size_t)2048 * C;
        std::vector<float> pcm(withPcm ? n * FF : 0), bands(n * FF), resid(n * FF);
        std::vector<at3phip_tonal_block> blocks(n);
        std::vector<uint8_t> want(withPcm ? (size_t)n * 2048 : 0);
        if (fread(pcm.data(), 4, pcm.size(), f) != pcm.size() || fread(bands.data(), 4, bands.size(), f) != bands.size() ||
            fread(blocks.data(), sizeof(at3phip_tonal_block), n, f) != (size_t)n || fread(resid.data(), 4, resid.size(), f) != resid.size() ||
            fread(want.data(), 1, want.size(), f) != want.size())
            return 2;
        {   // the analyser alone, driven as TAt3PEncoder drives it: call k gets (previous = frame k-2, current = frame k-1, next = frame k)
            TAt3PToneAnalyser gha(C, gated, shared);
            std::vector<float> prev(FF, 0.0f), cur(FF, 0.0f);
            int badBlocks = 0, badResid = 0, points = 0, bits = 0;
            for (int k = 0; k <= n; ++k) {   // (one more call than frames: the last frame's pair)
                const float* next = k < n ? bands.data() + (size_t)k * FF : cur.data();
                if (k > 0) {
                    const at3phip_tonal_block* b = gha.DoAnalize({cur.data(), next}, {C == 2 ? cur.data() + 2048 : nullptr, C == 2 ? next + 2048 : nullptr},
                                                                 prev.data(), C == 2 ? prev.data() + 2048 : nullptr, nullptr, nullptr);
                    badBlocks += !b || memcmp(b, &blocks[k - 1], sizeof(*b)) != 0;
                    badResid += memcmp(prev.data(), resid.data() + (size_t)(k - 1) * FF, FF * sizeof(float)) != 0;
                    for (int sb = 0; b && sb < 16; ++sb) {
                        bits += (b->tone_sharing >> sb) & 1;
                        for (int ch = 0; ch < C; ++ch) points += (b->band[ch][sb].start != 0) + (b->band[ch][sb].stop != 0);
                    }
                    prev = cur;
                }
                if (k < n) cur.assign(next, next + FF);
            }
            EXPECT(badBlocks == 0 && badResid == 0);
            EXPECT(shared && C == 2 ? bits > 0 : bits == 0);
            EXPECT(gated || points == 0);
            printf("TAt3PToneAnalyser channels %d flags %d: %d records compared, %d differ; %d residuals differ; points %d; sharing bits %d\n", C, h[2], n, badBlocks,
                   badResid, points, bits);
        }
        if (!device || !withPcm) continue;
        for (int mode = 0; mode < 2; ++mode)      // the analyser on the host, then on the device
            for (int batch : {3, 64}) {           // state carried between flushes, and all in the destructor's flush
                std::vector<std::vector<char>> frames;
                TAt3PToneAnalyser gha(C, gated, shared);
                {
                    TAt3PEncoder enc(TCompressedOutputPtr(new TMemOut(&frames, (size_t)C)), C, batch, 0, TAt3PSettings(), mode ? nullptr : &gha, mode == 1, mode == 1 && gated,
                                     mode == 1 && shared);
                    auto lambda = enc.GetLambda();
                    for (int k = 0; k < n; ++k) lambda(pcm.data() + (size_t)k * FF, ProcessMeta{(uint16_t)C});
                }   // destructor flushes
                EXPECT((int)frames.size() == n - 1);
                const int bad = differing(frames, want, n - 1);
                EXPECT(bad == 0);
                printf("TAt3PEncoder channels %d flags %d %s batch %d: %d frames compared, %d differ\n", C, h[2], mode ? "device tones" : "host analyser", batch, n - 1, bad);
            }
    }
    fclose(f);
    printf(fails ? "HOST SHIM AT3P GHA TEST FAILED\n" : "HOST SHIM AT3P GHA TEST OK\n");
    return fails ? 1 : 0;
}
