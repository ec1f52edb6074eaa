/* TEST INFRASTRUCTURE ONLY - a C restatement of the ATRAC3plus tone analysis with shared bands, as include/at3phip.h defines it
 * (FINDING TONES, SHARING S1-S5 after the gates): one stream, frame after frame, with or without AT3PHIP_TONES_GATED. Steps 1-5
 * and G1-G4 are at3p_gha_cpu.c's and at3p_gha_gate_cpu.c's (included here) call for call; this file adds the twin decision, the
 * population of the budget, the record's sharing word and the residual of a shared band, which is generate_tones
 * (at3p_tonal_cpu.c) fed with the record after the decoder's own copy of channel 0's band. The same analysis is written out in
 * atracdenc_amd/csrc/at3p_gha.hpp (the kernels) and in TAt3PToneAnalyser (atracdenc_amd/host/at3hip_host.hpp): the three change
 * together. Compiled by the tests with gcc -O2 -fPIC -ffp-contract=off -fno-fast-math. */
#include "at3p_gha_gate_cpu.c"

/* W_c(b): the packed words of channel ch's kept waves in band sb */
static int band_words(const gwave* w, int nw, int ch, int sb, uint32_t* out)
{
    int n = 0;
    for (int i = 0; i < nw; ++i)
        if (w[i].ch == ch && w[i].sb == sb) out[n++] = AT3PHIP_TONAL_WAVE(w[i].freq, w[i].amp_sf, w[i].phase);
    return n;
}

static int words_within(const uint32_t* a, int na, const uint32_t* b, int nb)
{
    for (int i = 0; i < na; ++i) {
        int found = 0;
        for (int j = 0; j < nb; ++j) found |= a[i] == b[j];
        if (!found) return 0;
    }
    return 1;
}

/* G2's point pair of a gate byte, in the record's "+1" convention */
static void gate_points(int g, int* start, int* stop)
{
    *start = g > 0 && g < 0x80 ? g + 1 : 0;
    *stop = g >= 0x80 ? (g & 31) + 1 : 0;
}

/* S2: W_0(b) = W_1(b) as sets and E_0(b) = E_1(b) */
static int twin_band(const gwave* w, int nw, int g0, int g1, int sb)
{
    uint32_t a[AT3PHIP_TONE_MAX_BAND_WAVES], b[AT3PHIP_TONE_MAX_BAND_WAVES];
    const int na = band_words(w, nw, 0, sb, a), nb = band_words(w, nw, 1, sb, b);
    int s0, p0, s1, p1;
    gate_points(g0, &s0, &p0);
    gate_points(g1, &s1, &p1);
    return words_within(a, na, b, nb) && words_within(b, nb, a, na) && s0 == s1 && p0 == p1;
}

/* block_to_trec_points, then what the decoder does with the sharing flags (parse_tonal): a shared band of channel 1 is channel 0's */
static void block_to_trec_shared(const at3phip_tonal_block* b, trec* r)
{
    block_to_trec_points(b, r);
    for (int sb = 0; sb < b->num_tone_bands && sb < 16; ++sb)
        if ((b->tone_sharing >> sb) & 1) r->band[1][sb] = r->band[0][sb];
}

size_t at3pgs_state_bytes(void) { return sizeof(at3pg_stream); }
void at3pgs_reset(void* state) { at3pg_reset(state); }

/* at3phip_analyse_tones for one stream with `flags` (AT3PHIP_TONES_GATED, AT3PHIP_TONES_SHARED or both or none), laid out as
 * at3pg_analyse; found [n] (may be null): the waves of step 5 in each slot, before S3 */
void at3pgs_analyse(void* state, int C, const float* bands, int n, at3phip_tonal_block* blocks, float* residual, uint32_t flags, int32_t* found)
{
    at3pg_stream* st = (at3pg_stream*)state;
    const int gated = (flags & AT3PHIP_TONES_GATED) != 0, shared = (flags & AT3PHIP_TONES_SHARED) != 0 && C == 2;   /* S1 */
    init_gha_tables();
    for (int f = 0; f < n; ++f) {
        gwave w[2 * 16 * AT3PHIP_TONE_MAX_BAND_WAVES];
        int nw = 0, gate[2][16] = {{0}};
        for (int ch = 0; ch < C; ++ch)
            for (int sb = 0; sb < 16; ++sb) {
                float x[256];
                memcpy(x, st->x[ch] + sb * 128, 128 * sizeof(float));
                memcpy(x + 128, bands + (((size_t)f * C + ch) * 16 + sb) * 128, 128 * sizeof(float));
                const int g0 = gated ? gate_band(x) : 0, g1 = gated ? gate_band(x + 128) : 0;
                int lo = 0, hi = 63, got;
                gate[ch][sb] = g1;
                if (g0 | g1) {
                    gate_interval(g0, g1, &lo, &hi);
                    got = find_band_gated(x, lo, hi, w + nw);
                } else {
                    got = find_band(x, w + nw);
                }
                for (int i = 0; i < got; ++i) { w[nw + i].ch = ch; w[nw + i].sb = sb; }
                nw += got;
            }
        if (found) found[f] = nw;
        /* S2, then S3: channel 1's waves of the twin bands leave the population */
        int twin[16] = {0};
        if (shared) {
            for (int sb = 0; sb < 16; ++sb) twin[sb] = twin_band(w, nw, gate[0][sb], gate[1][sb], sb);
            int kept = 0;
            for (int i = 0; i < nw; ++i)
                if (!(w[i].ch == 1 && twin[w[i].sb])) w[kept++] = w[i];
            nw = kept;
        }
        select_waves(w, nw, &blocks[f]);
        for (int ch = 0; ch < C; ++ch)   /* G2; S4: a twin band of channel 1 stays all zero */
            for (int sb = 0; sb < 16; ++sb) {
                const int g = gate[ch][sb];
                if (!g || (ch == 1 && twin[sb])) continue;
                if (g < 0x80) blocks[f].band[ch][sb].start = (uint8_t)(g + 1);
                else blocks[f].band[ch][sb].stop = (uint8_t)((g & 31) + 1);
                if (sb + 1 > blocks[f].num_tone_bands) blocks[f].num_tone_bands = (uint8_t)(sb + 1);
            }
        for (int sb = 0; sb < blocks[f].num_tone_bands; ++sb)   /* S4 */
            if (twin[sb]) blocks[f].tone_sharing |= (uint16_t)(1u << sb);
        /* S5 */
        trec cur;
        block_to_trec_shared(&blocks[f], &cur);
        float* r = residual + (size_t)f * C * 2048;
        for (int ch = 0; ch < C; ++ch) {
            memcpy(r + ch * 2048, st->x[ch], 2048 * sizeof(float));
            if (cur.present || st->filt.present)
                for (int sb = 0; sb < 16; ++sb)
                    if (cur.band[ch][sb].nw || st->filt.band[ch][sb].nw) generate_tones(&st->filt, &cur, ch, sb, r + ch * 2048 + sb * 128, 1);
        }
        st->filt = cur;
        st->last = blocks[f];
        for (int ch = 0; ch < C; ++ch) memcpy(st->x[ch], bands + ((size_t)f * C + ch) * 2048, 2048 * sizeof(float));
    }
}
