/* TEST INFRASTRUCTURE: a small deterministic stand-in for the tonal analysis (the reference's MakeGhaProcessor0 needs libgha,
 * which it does not vendor), shared by the schedule driver that tools/gen_golden_at3p_tonal_write.py builds around the
 * reference's TAt3PEnc and by tests/host/test_host_shim_at3p_tonal.cpp. Call k = 0, 1, 2, ... of the analysis
 *   - halves subband k % 16 of the writable previous buffers (so that the change is seen to reach the transform), and
 *   - returns a block derived from k on two calls of three (none when k % 3 == 2).
 * The block is formed in the C ABI's record (include/at3phip.h); the driver converts it to TAt3PGhaData. */
#ifndef AT3P_FAKE_GHA_H
#define AT3P_FAKE_GHA_H
#include <string.h>

#include "../../include/at3phip.h"

static inline void at3p_fake_gha_modify(int k, float* w1, float* w2)
{
    const int sb = k % 16;
    for (int i = 0; i < 128; ++i) {
        w1[sb * 128 + i] *= 0.5f;
        if (w2) w2[sb * 128 + i] *= 0.5f;
    }
}

/* 1 and *out filled when call k finds a block, else 0 */
static inline int at3p_fake_gha_block(int k, int channels, at3phip_tonal_block* out)
{
    memset(out, 0, sizeof(*out));
    if (k % 3 == 2) return 0;
    const int nb = 1 + (5 * k) % 16;
    int at = 0;
    out->num_tone_bands = (uint8_t)nb;
    if (channels == 2) {
        out->second_is_leader = (uint8_t)(k & 1);
        for (int b = 0; b < nb; ++b)
            if (((k >> 1) + b) % 3 == 0) out->tone_sharing |= (uint16_t)(1u << b);
    }
    for (int ch = 0; ch < channels; ++ch)
        for (int b = 0; b < nb; ++b) {
            at3phip_tonal_band* bd = &out->band[ch][b];
            if (ch == 1 && ((out->tone_sharing >> b) & 1)) continue;
            int n = (k + 2 * b + ch) % 4;
            if (at + n > AT3PHIP_TONAL_MAX_WAVES) n = AT3PHIP_TONAL_MAX_WAVES - at;
            bd->n_waves = (uint8_t)n;
            bd->start = (uint8_t)((k + b) % 4 == 0 ? 1 + (k + 3 * b) % 32 : 0);
            bd->stop = (uint8_t)((k + b + ch) % 5 == 0 ? 1 + (31 - (k + b) % 8) : 0);
            const int base = (k & 1) ? 520 + (k * 29 + b * 53 + ch * 7) % 300 : (k * 29 + b * 53 + ch * 7) % 400;
            for (int i = 0; i < n; ++i, ++at)
                out->wave[at] = AT3PHIP_TONAL_WAVE(base + 61 * i, (k + b + 5 * i) % 48, (3 * k + b + 7 * i) % 32);
        }
    return 1;
}
#endif
