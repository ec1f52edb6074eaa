// A build of the ATRAC3plus engine WITHOUT the adaptive writer's translation units (csrc/at3p_alloc.hip, csrc/at3p_sparse.hip) and
// AT3PHIP_ALLOC_SPARSE: all six frame-writing calls refuse the flag - alone because it needs AT3PHIP_ALLOC_ADAPTIVE, together with
// it because this build has no sparse writer - and write nothing; at3phip_decode refuses AT3PHIP_DECODE_SPARSE because the build
// has no sparse unpack kernels; without the flags the context and the decoder work as before.
// Built and run by tests/test_at3p_sparse_cpu.py: at3phip.hip compiled for the host with the SIMT harness's runtime (tools/emu).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/at3phip.h"

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

static void refused(at3phip_ctx* c, int rc, const char* why, std::vector<uint8_t>& frames)
{
    CHECK(rc == AT3HIP_EINVAL);
    CHECK(std::strstr(at3phip_last_error(c), why) != nullptr);
    for (uint8_t b : frames) CHECK(b == 0xA5);   // nothing was written
}

int main()
{
    for (int channels = 1; channels <= 2; ++channels) {
        at3phip_config cfg{};
        cfg.channels = channels;
        cfg.n_streams = 1;
        cfg.max_frames = 2;
        at3phip_ctx* c = nullptr;
        CHECK(at3phip_create(&cfg, &c) == AT3HIP_OK);
        if (!c) return 1;
        std::vector<float> in((size_t)2 * 2048 * channels, 0.25f);
        std::vector<int16_t> in16(in.size(), 1000);
        std::vector<at3phip_tonal_block> tonal(2, at3phip_tonal_block{});
        std::vector<uint8_t> frames((size_t)2 * AT3PHIP_FRAME_BYTES, 0xA5), plain(frames);
        for (int pass = 0; pass < 2; ++pass) {
            const uint32_t flag = AT3PHIP_ALLOC_SPARSE | (pass ? AT3PHIP_ALLOC_ADAPTIVE : 0u);
            const char* why = pass ? "no sparse writer" : "AT3PHIP_ALLOC_SPARSE needs AT3PHIP_ALLOC_ADAPTIVE";
            refused(c, at3phip_write_frames(c, in.data(), 2, nullptr, frames.data(), flag), why, frames);
            refused(c, at3phip_write_frames_tonal(c, in.data(), 2, nullptr, tonal.data(), frames.data(), flag), why, frames);
            refused(c, at3phip_encode_frames(c, in.data(), 2, frames.data(), flag), why, frames);
            refused(c, at3phip_encode_frames_short(c, in16.data(), 2, frames.data(), flag), why, frames);
            refused(c, at3phip_encode_frames_tonal(c, in.data(), 2, frames.data(), flag), why, frames);
            refused(c, at3phip_encode_frames_tonal_short(c, in16.data(), 2, frames.data(), flag | AT3PHIP_TONES_GATED), why, frames);
        }
        // without the flags the context is as usable as before
        CHECK(at3phip_write_frames(c, in.data(), 2, nullptr, plain.data(), 0) == AT3HIP_OK);
        CHECK(plain != frames);
        at3phip_destroy(c);

        at3phip_decoder_config dcfg{};
        dcfg.channels = channels;
        dcfg.n_streams = 1;
        dcfg.max_frames = 2;
        at3phip_decoder* d = nullptr;
        CHECK(at3phip_decoder_create(&dcfg, &d) == AT3HIP_OK);
        if (!d) return 1;
        std::vector<float> pcm((size_t)2 * 2048 * channels, 7.0f);
        CHECK(at3phip_decode(d, plain.data(), 2, pcm.data(), AT3PHIP_DECODE_SPARSE) == AT3HIP_EINVAL);
        CHECK(std::strstr(at3phip_decoder_last_error(d), "no sparse unpack kernels") != nullptr);
        for (float v : pcm) CHECK(v == 7.0f);
        CHECK(at3phip_decode(d, plain.data(), 2, pcm.data(), 0) == AT3HIP_OK);
        at3phip_decoder_counters cnt{};
        CHECK(at3phip_decoder_get_counters(d, &cnt, 0) == AT3HIP_OK && cnt.bad_code == 0 && cnt.unsupported_syntax == 0);
        at3phip_decoder_destroy(d);
    }
    if (fails) return 1;
    std::printf("SPARSE WITHOUT THE ADAPTIVE WRITER OK\n");
    return 0;
}
