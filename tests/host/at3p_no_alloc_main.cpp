// A build of the ATRAC3plus engine WITHOUT the adaptive writer's translation unit (csrc/at3p_alloc.hip), as the stand-alone host
// programs that link at3phip.hip from their own source lists have it: at3phip.hip reaches the adaptive launch through a weak
// symbol, so such a build links, and every call that carries AT3PHIP_ALLOC_ADAPTIVE is AT3HIP_EINVAL with an error that says
// so - never the fixed writer's frames in the flag's place. Without the flag the calls work as before.
// Built and run by tests/test_at3p_alloc_cpu.py: at3phip.hip compiled for the host with the SIMT harness's runtime (tools/emu).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/at3phip.h"

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

static void refused(at3phip_ctx* c, int rc, std::vector<uint8_t>& frames)
{
    CHECK(rc == AT3HIP_EINVAL);
    CHECK(std::strstr(at3phip_last_error(c), "no adaptive writer") != nullptr);
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
        refused(c, at3phip_write_frames(c, in.data(), 2, nullptr, frames.data(), AT3PHIP_ALLOC_ADAPTIVE), frames);
        refused(c, at3phip_write_frames_tonal(c, in.data(), 2, nullptr, tonal.data(), frames.data(), AT3PHIP_ALLOC_ADAPTIVE), frames);
        refused(c, at3phip_encode_frames(c, in.data(), 2, frames.data(), AT3PHIP_ALLOC_ADAPTIVE), frames);
        refused(c, at3phip_encode_frames_short(c, in16.data(), 2, frames.data(), AT3PHIP_ALLOC_ADAPTIVE), frames);
        refused(c, at3phip_encode_frames_tonal(c, in.data(), 2, frames.data(), AT3PHIP_ALLOC_ADAPTIVE), frames);
        refused(c, at3phip_encode_frames_tonal_short(c, in16.data(), 2, frames.data(), AT3PHIP_ALLOC_ADAPTIVE | AT3PHIP_TONES_GATED), frames);
        // and the context is as usable as before
        CHECK(at3phip_reset(c) == AT3HIP_OK);
        CHECK(at3phip_write_frames(c, in.data(), 2, nullptr, plain.data(), 0) == AT3HIP_OK);
        CHECK(plain != frames);
        at3phip_destroy(c);
    }
    if (fails) return 1;
    std::printf("NO ADAPTIVE WRITER OK\n");
    return 0;
}
