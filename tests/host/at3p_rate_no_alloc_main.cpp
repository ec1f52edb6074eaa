// A build of the ATRAC3plus engine WITHOUT the adaptive writer's translation unit (csrc/at3p_alloc.hip) and a frame size other
// than 2048 bytes: at3phip_set_frame_bytes succeeds (the size is the context's, whichever writers the build has), and from then
// on every frame-writing call is refused - without AT3PHIP_ALLOC_ADAPTIVE because the fixed table is defined for 2048-byte frames
// only, with it because this build has no adaptive writer. Nothing is written either way, and back at 2048 bytes the context
// works as before.
// Built and run by tests/test_at3p_rate_cpu.py: at3phip.hip compiled for the host with the SIMT harness's runtime (tools/emu).
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
        int32_t fb = 0;
        CHECK(at3phip_get_frame_bytes(c, &fb) == AT3HIP_OK && fb == AT3PHIP_FRAME_BYTES);
        CHECK(at3phip_set_frame_bytes(c, 376) == AT3HIP_OK);
        CHECK(at3phip_get_frame_bytes(c, &fb) == AT3HIP_OK && fb == 376);
        std::vector<float> in((size_t)2 * 2048 * channels, 0.25f);
        std::vector<int16_t> in16(in.size(), 1000);
        std::vector<at3phip_tonal_block> tonal(2, at3phip_tonal_block{});
        std::vector<uint8_t> frames((size_t)2 * AT3PHIP_FRAME_BYTES, 0xA5), plain(frames);
        for (int pass = 0; pass < 2; ++pass) {
            const uint32_t flag = pass ? AT3PHIP_ALLOC_ADAPTIVE : 0u;
            const char* why = pass ? "no adaptive writer" : "the fixed table is defined for 2048-byte frames only";
            refused(c, at3phip_write_frames(c, in.data(), 2, nullptr, frames.data(), flag), why, frames);
            refused(c, at3phip_write_frames_tonal(c, in.data(), 2, nullptr, tonal.data(), frames.data(), flag), why, frames);
            refused(c, at3phip_encode_frames(c, in.data(), 2, frames.data(), flag), why, frames);
            refused(c, at3phip_encode_frames_short(c, in16.data(), 2, frames.data(), flag), why, frames);
            refused(c, at3phip_encode_frames_tonal(c, in.data(), 2, frames.data(), flag), why, frames);
            refused(c, at3phip_encode_frames_tonal_short(c, in16.data(), 2, frames.data(), flag | AT3PHIP_TONES_GATED), why, frames);
        }
        // an inadmissible size is refused and changes nothing
        for (int bad : {0, 7, 2056, (channels == 2 ? AT3PHIP_MIN_FRAME_BYTES_STEREO : AT3PHIP_MIN_FRAME_BYTES_MONO) - 8}) {
            CHECK(at3phip_set_frame_bytes(c, bad) == AT3HIP_EINVAL);
            CHECK(std::strstr(at3phip_last_error(c), "frame_bytes") != nullptr);
            CHECK(at3phip_get_frame_bytes(c, &fb) == AT3HIP_OK && fb == 376);
        }
        CHECK(at3phip_set_frame_bytes(nullptr, 376) == AT3HIP_EINVAL);
        // back at 2048 bytes the context is as usable as before
        CHECK(at3phip_set_frame_bytes(c, AT3PHIP_FRAME_BYTES) == AT3HIP_OK);
        CHECK(at3phip_reset(c) == AT3HIP_OK);
        CHECK(at3phip_write_frames(c, in.data(), 2, nullptr, plain.data(), 0) == AT3HIP_OK);
        CHECK(plain != frames);
        at3phip_destroy(c);
    }
    if (fails) return 1;
    std::printf("FRAME SIZE WITHOUT THE ADAPTIVE WRITER OK\n");
    return 0;
}
