// Builds of the ATRAC3plus engine that lack some or all of the adaptive writer's translation units: at3phip.hip reaches their
// launches through weak symbols, so such a build links, and a call whose flags need a missing unit is AT3HIP_EINVAL with an error
// that says so - never another writer's frames in the flag's place - and neither writes a byte nor moves the context's state.
// The argument, none | alloc | alloc+sparse | alloc+sparse+rd | all, names the units the program was linked with: none, at3p_alloc.hip,
// that and at3p_sparse.hip, those and at3p_rd.hip, those and at3p_psy.hip. Mono and stereo, the context's size at 2048 and at 376
// bytes, each of the sixteen combinations of the four allocation flags: all six frame-writing calls against kWriter, and
// at3phip_decode with AT3PHIP_DECODE_SPARSE against kDecoder; at3phip_host_allocate_rd and at3phip_host_allocate_psy, the symbols by
// which a host detects the two newer flags, are there exactly when their units are. The tables are data, printed by --print from the
// engine as it stood before the mode was resolved in one place, and for AT3PHIP_ALLOC_PSY before this program took the flag (DESIGN.md
// 22.2 and 24.1 have the procedure), and not derived here from the rule they test.
// Built and run by tests/simt_harness_lib.py's run_alloc_modes: the engine compiled for the host with tools/emu's runtime.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/at3phip.h"

extern "C" __attribute__((weak)) int at3phip_host_allocate_rd(const uint8_t*, const uint16_t*, const uint64_t*, int32_t, int32_t, int32_t, uint8_t*, int32_t*,
                                                              int32_t*, int32_t*, int32_t*);
extern "C" __attribute__((weak)) int at3phip_host_allocate_psy(const uint8_t*, const uint16_t*, const uint64_t*, const uint8_t*, int32_t, int32_t, int32_t,
                                                               uint8_t*, int32_t*, int32_t*, int32_t*, int32_t*, uint8_t*);

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

static const char* const kConfigs[5] = {"none", "alloc", "alloc+sparse", "alloc+sparse+rd", "all"};
static const int kSizes[2] = {AT3PHIP_FRAME_BYTES, 376};
static const char* const kCalls[6] = {"write_frames", "write_frames_tonal", "encode_frames", "encode_frames_short", "encode_frames_tonal",
                                      "encode_frames_tonal_short"};

struct Expect {
    int rc;
    const char* why;   // a fragment of the last-error text of a refused call
};
static const Expect kOk = {AT3HIP_OK, nullptr};
static const Expect kFixed = {AT3HIP_EINVAL, "the fixed table is defined for 2048-byte frames only"};
static const Expect kNoAdaptive = {AT3HIP_EINVAL, "no adaptive writer (at3p_alloc.hip)"};
static const Expect kNoSparse = {AT3HIP_EINVAL, "no sparse writer (at3p_alloc.hip, at3p_sparse.hip)"};
static const Expect kNoRd = {AT3HIP_EINVAL, "no rate-distortion writer (at3p_rd.hip)"};
static const Expect kSparseAlone = {AT3HIP_EINVAL, "AT3PHIP_ALLOC_SPARSE needs AT3PHIP_ALLOC_ADAPTIVE in the same call"};
static const Expect kRdAlone = {AT3HIP_EINVAL, "AT3PHIP_ALLOC_RD needs AT3PHIP_ALLOC_ADAPTIVE and AT3PHIP_ALLOC_SPARSE in the same call"};
static const Expect kPsyAlone = {AT3HIP_EINVAL, "AT3PHIP_ALLOC_PSY needs AT3PHIP_ALLOC_ADAPTIVE, AT3PHIP_ALLOC_SPARSE and AT3PHIP_ALLOC_RD in the same call"};
static const Expect kNoPsy = {AT3HIP_EINVAL, "AT3PHIP_ALLOC_PSY: this build has no masking-weighted writer (at3p_psy.hip)"};
static const Expect kNoUnpack = {AT3HIP_EINVAL, "no sparse unpack kernels (at3p_sparse.hip)"};

// [units][size][flags]: flags' bit 0 = AT3PHIP_ALLOC_ADAPTIVE, bit 1 = AT3PHIP_ALLOC_SPARSE, bit 2 = AT3PHIP_ALLOC_RD, bit 3 =
// AT3PHIP_ALLOC_PSY; the same for all six calls and for mono and stereo
static const Expect kWriter[5][2][16] = {
    {{kOk, kNoAdaptive, kSparseAlone, kNoSparse, kRdAlone, kRdAlone, kRdAlone, kNoRd,
      kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kNoPsy},
     {kFixed, kNoAdaptive, kFixed, kNoAdaptive, kFixed, kNoAdaptive, kFixed, kNoAdaptive,
      kFixed, kNoAdaptive, kFixed, kNoAdaptive, kFixed, kNoAdaptive, kFixed, kNoAdaptive}},
    {{kOk, kOk, kSparseAlone, kNoSparse, kRdAlone, kRdAlone, kRdAlone, kNoRd,
      kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kNoPsy},
     {kFixed, kOk, kFixed, kNoSparse, kFixed, kRdAlone, kFixed, kNoRd,
      kFixed, kPsyAlone, kFixed, kPsyAlone, kFixed, kPsyAlone, kFixed, kNoPsy}},
    {{kOk, kOk, kSparseAlone, kOk, kRdAlone, kRdAlone, kRdAlone, kNoRd,
      kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kNoPsy},
     {kFixed, kOk, kFixed, kOk, kFixed, kRdAlone, kFixed, kNoRd,
      kFixed, kPsyAlone, kFixed, kPsyAlone, kFixed, kPsyAlone, kFixed, kNoPsy}},
    {{kOk, kOk, kSparseAlone, kOk, kRdAlone, kRdAlone, kRdAlone, kOk,
      kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kNoPsy},
     {kFixed, kOk, kFixed, kOk, kFixed, kRdAlone, kFixed, kOk,
      kFixed, kPsyAlone, kFixed, kPsyAlone, kFixed, kPsyAlone, kFixed, kNoPsy}},
    {{kOk, kOk, kSparseAlone, kOk, kRdAlone, kRdAlone, kRdAlone, kOk,
      kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kPsyAlone, kOk},
     {kFixed, kOk, kFixed, kOk, kFixed, kRdAlone, kFixed, kOk,
      kFixed, kPsyAlone, kFixed, kPsyAlone, kFixed, kPsyAlone, kFixed, kOk}},
};
// [units]: at3phip_decode with AT3PHIP_DECODE_SPARSE, at both sizes
static const Expect kDecoder[5] = {kNoUnpack, kNoUnpack, kOk, kOk, kOk};

static uint32_t alloc_flags(int bits)
{
    return (bits & 1 ? AT3PHIP_ALLOC_ADAPTIVE : 0u) | (bits & 2 ? AT3PHIP_ALLOC_SPARSE : 0u) | (bits & 4 ? AT3PHIP_ALLOC_RD : 0u) |
           (bits & 8 ? AT3PHIP_ALLOC_PSY : 0u);
}

struct Input {
    std::vector<float> f;
    std::vector<int16_t> s;
    std::vector<at3phip_tonal_block> tonal;
    explicit Input(int channels) : f((size_t)2 * 2048 * channels), s(f.size()), tonal(2, at3phip_tonal_block{})
    {
        uint32_t x = 12345u;   // a fixed LCG noise
        for (size_t i = 0; i < f.size(); ++i) {
            x = x * 1664525u + 1013904223u;
            s[i] = (int16_t)((int)(x >> 18) - 8192);
            f[i] = (float)s[i] / 32768.0f;
        }
    }
};

static int call(int which, at3phip_ctx* c, const Input& in, uint8_t* frames, uint32_t flags)
{
    switch (which) {
    case 0: return at3phip_write_frames(c, in.f.data(), 2, nullptr, frames, flags);
    case 1: return at3phip_write_frames_tonal(c, in.f.data(), 2, nullptr, in.tonal.data(), frames, flags);
    case 2: return at3phip_encode_frames(c, in.f.data(), 2, frames, flags);
    case 3: return at3phip_encode_frames_short(c, in.s.data(), 2, frames, flags);
    case 4: return at3phip_encode_frames_tonal(c, in.f.data(), 2, frames, flags);
    default: return at3phip_encode_frames_tonal_short(c, in.s.data(), 2, frames, flags | AT3PHIP_TONES_GATED);
    }
}

static at3phip_ctx* create(int channels)
{
    at3phip_config cfg{};
    cfg.channels = channels, cfg.n_streams = 1, cfg.max_frames = 2;
    at3phip_ctx* c = nullptr;
    CHECK(at3phip_create(&cfg, &c) == AT3HIP_OK);
    return c;
}

int main(int argc, char** argv)
{
    int units = -1;
    for (int i = 0; i < 5 && argc > 1; ++i)
        if (!std::strcmp(argv[1], kConfigs[i])) units = i;
    const bool print = argc > 2 && !std::strcmp(argv[2], "--print");
    if (units < 0) return std::printf("usage: %s none|alloc|alloc+sparse|alloc+sparse+rd|all [--print]\n", argv[0]), 2;
    CHECK((at3phip_host_allocate_rd != nullptr) == (units >= 3));    // the symbols by which a host detects the flags
    CHECK((at3phip_host_allocate_psy != nullptr) == (units == 4));
    for (int channels = 1; channels <= 2; ++channels) {
        // `refusing` receives the calls the table refuses, and nothing else but the setter; `accepting` the others
        at3phip_ctx *refusing = create(channels), *accepting = create(channels), *fresh = create(channels);
        if (!refusing || !accepting || !fresh) return 1;
        const Input in(channels);
        const std::vector<uint8_t> untouched((size_t)2 * AT3PHIP_FRAME_BYTES, 0xA5);
        std::vector<uint8_t> frames(untouched);
        for (int size = 0; size < 2; ++size) {
            int32_t fb = 0;
            for (at3phip_ctx* c : {refusing, accepting}) {
                CHECK(at3phip_set_frame_bytes(c, kSizes[size]) == AT3HIP_OK);
                CHECK(at3phip_get_frame_bytes(c, &fb) == AT3HIP_OK && fb == kSizes[size]);
            }
            for (int bits = 0; bits < 16; ++bits)
                for (int which = 0; which < 6; ++which) {
                    const Expect& e = kWriter[units][size][bits];
                    at3phip_ctx* c = e.rc == AT3HIP_OK ? accepting : refusing;
                    frames = untouched;
                    const int rc = call(which, c, in, frames.data(), alloc_flags(bits));
                    if (print) {
                        std::printf("%s ch%d %d flags%d %s: %d %s%s\n", kConfigs[units], channels, kSizes[size], bits, kCalls[which], rc,
                                    rc ? at3phip_last_error(c) : "", rc && frames != untouched ? " WROTE" : "");
                        continue;
                    }
                    CHECK(rc == e.rc);
                    if (rc != AT3HIP_OK) {
                        CHECK(e.why && std::strstr(at3phip_last_error(c), e.why) != nullptr);
                        CHECK(frames == untouched);   // nothing was written
                    } else {
                        CHECK(frames != untouched);
                    }
                }
        }
        // an inadmissible size is refused and changes nothing
        int32_t fb = 0;
        for (int bad : {0, 7, 2056, (channels == 2 ? AT3PHIP_MIN_FRAME_BYTES_STEREO : AT3PHIP_MIN_FRAME_BYTES_MONO) - 8}) {
            CHECK(at3phip_set_frame_bytes(refusing, bad) == AT3HIP_EINVAL);
            CHECK(std::strstr(at3phip_last_error(refusing), "frame_bytes") != nullptr);
            CHECK(at3phip_get_frame_bytes(refusing, &fb) == AT3HIP_OK && fb == 376);
        }
        CHECK(at3phip_set_frame_bytes(nullptr, 376) == AT3HIP_EINVAL);
        // back at 2048 bytes, with no at3phip_reset: the refused calls moved no stream state, so the context encodes as a new one does
        CHECK(at3phip_set_frame_bytes(refusing, AT3PHIP_FRAME_BYTES) == AT3HIP_OK);
        std::vector<uint8_t> plain(untouched);
        CHECK(at3phip_encode_frames(refusing, in.f.data(), 2, frames.data(), 0) == AT3HIP_OK);
        CHECK(at3phip_encode_frames(fresh, in.f.data(), 2, plain.data(), 0) == AT3HIP_OK);
        CHECK(plain != untouched);
        if (print) std::printf("%s ch%d after the refused calls: %s\n", kConfigs[units], channels, frames == plain ? "as a new context" : "DIFFERS");
        else CHECK(frames == plain);
        for (at3phip_ctx* c : {refusing, accepting, fresh}) at3phip_destroy(c);

        at3phip_decoder_config dcfg{};
        dcfg.channels = channels, dcfg.n_streams = 1, dcfg.max_frames = 2;
        at3phip_decoder* d = nullptr;
        CHECK(at3phip_decoder_create(&dcfg, &d) == AT3HIP_OK);
        if (!d) return 1;
        const std::vector<float> silent((size_t)2 * 2048 * channels, 7.0f);
        std::vector<float> pcm(silent);
        for (int size = 0; size < 2; ++size) {
            CHECK(at3phip_decoder_set_frame_bytes(d, kSizes[size]) == AT3HIP_OK);
            const Expect& e = kDecoder[units];
            pcm = silent;
            const int rc = at3phip_decode(d, plain.data(), 2, pcm.data(), AT3PHIP_DECODE_SPARSE);
            if (print) {
                std::printf("%s ch%d %d decode: %d %s%s\n", kConfigs[units], channels, kSizes[size], rc, rc ? at3phip_decoder_last_error(d) : "",
                            rc && pcm != silent ? " WROTE" : "");
                continue;
            }
            CHECK(rc == e.rc);
            if (rc != AT3HIP_OK) {
                CHECK(e.why && std::strstr(at3phip_decoder_last_error(d), e.why) != nullptr);
                CHECK(pcm == silent);
            }
        }
        // without the flag the decoder works as before
        CHECK(at3phip_decoder_set_frame_bytes(d, AT3PHIP_FRAME_BYTES) == AT3HIP_OK);
        CHECK(at3phip_decoder_reset(d) == AT3HIP_OK);
        at3phip_decoder_counters cnt{};
        CHECK(at3phip_decoder_get_counters(d, &cnt, 1) == AT3HIP_OK);
        CHECK(at3phip_decode(d, plain.data(), 2, pcm.data(), 0) == AT3HIP_OK);
        CHECK(at3phip_decoder_get_counters(d, &cnt, 0) == AT3HIP_OK && cnt.bad_code == 0 && cnt.unsupported_syntax == 0);
        at3phip_decoder_destroy(d);
    }
    if (fails) return 1;
    std::printf("ALLOCATION MODES OK (%s)\n", kConfigs[units]);
    return 0;
}
