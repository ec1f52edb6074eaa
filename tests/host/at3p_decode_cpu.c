/* TEST INFRASTRUCTURE ONLY - a from-scratch C restatement of the ATRAC3plus decoder defined in include/at3phip.h (the decoder
 * section), written for three jobs: the bit-exact anchor the GPU decoder (atracdenc_amd/csrc/at3p_decode.hpp) is fuzzed against,
 * the one-core CPU baseline of tools/at3p_decode_bench.py, and - through its steps 1-2 - the front half of the golden generator
 * (tools/gen_golden_at3p_decode.py), whose back half is the reference's own TAt3pMIDCT::Do and ff_atrac3p_ipqf. Compiled by the
 * tests with gcc -O2 -fPIC -ffp-contract=off -fno-fast-math.
 *
 * Every step is stated here once, with the frame size, AT3PHIP_DECODE_SPARSE and AT3PHIP_DECODE_TONES as arguments of the one frame
 * parser and the one frame loop. The at3pd_* entry points are the decoder without flags at 2048 bytes; at3p_tonal_cpu.c (at3pt_*:
 * tonal blocks at 2048 bytes) and at3p_writer_cpu.c (at3pw_*: every argument) include this file and add entry points only.
 *
 * Per stream and channel it keeps what the reference's synthesis keeps: the IMDCT's windowed second halves and the previous
 * frame's window flags (TAt3pMIDCT::THistBuf), and the 24-row history ring of the synthesis filter (Atrac3pIPQFChannelCtx).
 * The tables are the project's generated data (at3p_vlc.inc, at3p_mant.inc, at3p_fir.inc); the code is written from the
 * definition. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../atracdenc_amd/csrc/at3p_vlc.inc"
#include "../../atracdenc_amd/csrc/at3p_mant.inc"
#include "../../atracdenc_amd/csrc/at3p_tone_vlc.inc"

static const float kFir[384] = {
#include "../../atracdenc_amd/csrc/at3p_fir.inc"
};

typedef struct { float r, i; } cpx;

static const uint16_t kQuStart[33] = {0, 16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 224, 256, 288, 320, 352, 384,
                                      448, 512, 576, 640, 704, 768, 896, 1024, 1152, 1280, 1408, 1536, 1664, 1792, 1920, 2048};

static struct {
    int ready;
    float sine128[128], sine64[64];
    float cs256[128];
    cpx tw64[64];
    double cos16[16][16];         /* [k][n] */
    uint16_t lut[56][4096];       /* spectra tables 0..55: next 12 bits -> symbol | length << 8 */
} T;

__attribute__((noinline, optimize("O0"))) static void calc_sincos(float* dst, size_t n, float scale)
{
    const float alpha = 2.0 * M_PI / (8.0 * n);
    const float omiga = 2.0 * M_PI / n;
    scale = sqrtf(scale / n);
    for (size_t i = 0; i < (n >> 2); ++i) {
        dst[2 * i + 0] = scale * cosf(omiga * i + alpha);
        dst[2 * i + 1] = scale * sinf(omiga * i + alpha);
    }
}

__attribute__((noinline, optimize("O0"))) static void init_tables(void)
{
    if (T.ready) return;
    for (int i = 0; i < 128; ++i) T.sine128[i] = 2.0 * sinf((i + 0.5) * (M_PI / (2.0 * 128)));
    for (int i = 0; i < 64; ++i) T.sine64[i] = 2.0 * sinf((i + 0.5) * (M_PI / (2.0 * 64)));
    calc_sincos(T.cs256, 256, 128.0f);   /* TMIDCT<256>() : TMDCTBase(256, 256 / 2) */
    const double pi = 3.141592653589793238462643383279502884197169399375105820974944;
    for (int i = 0; i < 64; ++i) {
        const double ph = -2 * pi * i / 64;
        T.tw64[i].r = (float)cos(ph);
        T.tw64[i].i = (float)sin(ph);
    }
    for (int k = 0; k < 16; ++k)
        for (int n = 0; n < 16; ++n) T.cos16[k][n] = cos((M_PI / 16) * ((double)n + 0.5) * ((double)k + 0.5));
    for (int t = 0; t < 56; ++t) {
        memset(T.lut[t], 0, sizeof(T.lut[t]));
        for (int sym = 0; sym < AT3P_VLC_OFF[t + 1] - AT3P_VLC_OFF[t]; ++sym) {
            const uint16_t e = AT3P_VLC[AT3P_VLC_OFF[t] + sym];
            const int len = e >> 12, code = e & 0xfff;
            if (!len) continue;
            for (int x = 0; x < (1 << (12 - len)); ++x) T.lut[t][(code << (12 - len)) | x] = (uint16_t)(sym | (len << 8));
        }
    }
    T.ready = 1;
}

/* ---- kissfft-order FFT (64 points: factors 4, 4, 4) ---- */
static inline cpx cmul(cpx a, cpx b)
{
    cpx m;
    m.r = a.r * b.r - a.i * b.i;
    m.i = a.r * b.i + a.i * b.r;
    return m;
}
static void fft_combine4(cpx* F, int m, int fstride, const cpx* tw)
{
    for (int k = 0; k < m; ++k) {
        const cpx s0 = cmul(F[m + k], tw[k * fstride]);
        const cpx s1 = cmul(F[2 * m + k], tw[2 * k * fstride]);
        const cpx s2 = cmul(F[3 * m + k], tw[3 * k * fstride]);
        cpx s5, s3, s4;
        s5.r = F[k].r - s1.r; s5.i = F[k].i - s1.i;
        F[k].r += s1.r; F[k].i += s1.i;
        s3.r = s0.r + s2.r; s3.i = s0.i + s2.i;
        s4.r = s0.r - s2.r; s4.i = s0.i - s2.i;
        F[2 * m + k].r = F[k].r - s3.r; F[2 * m + k].i = F[k].i - s3.i;
        F[k].r += s3.r; F[k].i += s3.i;
        F[m + k].r = s5.r + s4.i; F[m + k].i = s5.i - s4.r;
        F[3 * m + k].r = s5.r - s4.i; F[3 * m + k].i = s5.i + s4.r;
    }
}
static void fft_rec(cpx* out, const cpx* in, int n, int fstride, const cpx* tw)
{
    const int m = n / 4;
    if (m == 1) {
        for (int q = 0; q < 4; ++q) out[q] = in[q * fstride];
    } else {
        for (int q = 0; q < 4; ++q) fft_rec(out + q * m, in + q * fstride, m, fstride * 4, tw);
    }
    fft_combine4(out, m, fstride, tw);
}

/* TMIDCT<256>::operator(): 128 in -> 256 out */
static void imdct256(const float* in, float* buf)
{
    const float* cs = T.cs256;
    const int N = 256, n2 = N >> 1, n4 = N >> 2, n34 = 3 * n4, n54 = 5 * n4;
    cpx fin[64], fout[64];
    int n;
    for (n = 0; n < n2; n += 2) {
        const float r0 = in[n], i0 = in[n2 - 1 - n];
        const float c = cs[n], s = cs[n + 1];
        fin[n / 2].r = -2.0 * (i0 * s + r0 * c);
        fin[n / 2].i = -2.0 * (i0 * c - r0 * s);
    }
    fft_rec(fout, fin, 64, 1, T.tw64);
    for (n = 0; n < n4; n += 2) {
        const float r0 = fout[n / 2].r, i0 = fout[n / 2].i;
        const float c = cs[n], s = cs[n + 1];
        const float r1 = r0 * c + i0 * s, i1 = r0 * s - i0 * c;
        buf[n34 - 1 - n] = r1;
        buf[n34 + n] = r1;
        buf[n4 + n] = i1;
        buf[n4 - 1 - n] = -i1;
    }
    for (; n < n2; n += 2) {
        const float r0 = fout[n / 2].r, i0 = fout[n / 2].i;
        const float c = cs[n], s = cs[n + 1];
        const float r1 = r0 * c + i0 * s, i1 = r0 * s - i0 * c;
        buf[n34 - 1 - n] = r1;
        buf[n - n4] = -r1;
        buf[n4 + n] = i1;
        buf[n54 - 1 - n] = i1;
    }
}

/* ---- step 1: the bit reader, MSB first: every read must end within the frame's `limit` bits; a look-ahead past them sees zeros ---- */
typedef struct { const uint8_t* buf; int pos, bad, limit; } bits;
static int bit_at(const bits* b, int p) { return p < b->limit ? (b->buf[p >> 3] >> (7 - (p & 7))) & 1 : 0; }
static uint32_t rd(bits* b, int n)
{
    if (b->bad || b->pos + n > b->limit) { b->bad = 1; return 0; }
    uint32_t v = 0;
    for (int k = 0; k < n; ++k, ++b->pos) v = (v << 1) | (uint32_t)bit_at(b, b->pos);
    return v;
}
/* a code of a complete prefix code given as code | length << 12 per symbol (the word-length deltas, the tone-band count), searched
 * in symbol order */
static int vlc(bits* b, const uint16_t* table, int n_sym, int* invalid)
{
    if (b->bad) return 0;
    for (int sym = 0; sym < n_sym; ++sym) {
        const int len = table[sym] >> 12, code = table[sym] & 0xfff;
        if (!len) continue;
        uint32_t v = 0;
        for (int k = 0; k < len; ++k) v = (v << 1) | (uint32_t)bit_at(b, b->pos + k);
        if ((int)v == code) {
            if (b->pos + len > b->limit) { b->bad = 1; return 0; }
            b->pos += len;
            return sym;
        }
    }
    *invalid = 1;
    return 0;
}
/* test-only: how often each spectrum code (table, symbol) was decoded since the last reset (at3pd_hits) */
static uint32_t g_hits[56][256];

/* the same for a spectrum code, through the table's 12-bit look-up */
static int spec_vlc(bits* b, int table, int* invalid)
{
    if (b->bad) return 0;
    uint32_t v = 0;
    for (int k = 0; k < 12; ++k) v = (v << 1) | (uint32_t)bit_at(b, b->pos + k);
    const uint16_t e = T.lut[table][v];
    const int len = e >> 8;
    if (!len) { *invalid = 1; return 0; }
    if (b->pos + len > b->limit) { b->bad = 1; return 0; }
    b->pos += len;
    g_hits[table][e & 0xff]++;
    return e & 0xff;
}

/* reasons (at3phip_decoder_counters order) */
enum { R_OK = 0, R_BAD_HEADER, R_UNSUPPORTED, R_TONAL, R_BAD_CODE, R_READ_PAST_END, R_NO_TERMINATOR };

/* what a frame carried, for the tests (zeros past the counts; everything zero for a frame rejected before it) */
typedef struct at3pd_fields {
    int32_t reason, n_qu, full_table;
    int32_t wl[2][32], sf[2][32], tab[2][32];
    int32_t win[2];
} at3pd_fields;

/* a frame's tonal block (include/at3phip.h, TONAL BLOCKS), with the envelope step 4b keeps per band between frames */
typedef struct { int has_start, start, has_stop, stop; } tenv;
typedef struct { int nw, start_index; tenv pend, curr; } tband;
typedef struct {
    int present;
    tband band[2][16];
    int freq[48], amp_sf[48], phase[48];
} trec;

static int first_set_bit_plus1(uint32_t x)
{
    int n = 0;
    while (x >> n) ++n;
    return n ? n : 1;
}

/* the tonal block after its flag; r is zero on entry */
static int parse_tonal(bits* b, int C, trec* r)
{
    int invalid = 0;
#define CHK() do { if (b->bad) return R_READ_PAST_END; if (invalid) return R_BAD_CODE; } while (0)
#define MUST(n, val) do { const uint32_t v_ = rd(b, n); CHK(); if (v_ != (uint32_t)(val)) return R_UNSUPPORTED; } while (0)
    MUST(1, 1);
    const int nb = vlc(b, AT3P_TONE_BANDS_VLC, 16, &invalid) + 1;
    CHK();
    int shared[16] = {0}, leader = 0;
    if (C == 2) {
        if (rd(b, 1)) {
            if (rd(b, 1) == 0) {
                for (int i = 0; i < nb; ++i) shared[i] = 1;
            } else {
                for (int i = 0; i < nb; ++i) shared[i] = (int)rd(b, 1);
            }
        }
        CHK();
        if (rd(b, 1)) {
            MUST(1, 0);
            leader = 1;
        }
        MUST(1, 0);
    }
    int idx = 0;
    for (int ch = 0; ch < C; ++ch) {
        tband* bd = r->band[ch];
        if (ch) MUST(1, 0);
        for (int i = 0; i < nb; ++i) {
            if (ch && shared[i]) continue;
            bd[i].pend.start = -1;
            bd[i].pend.stop = 32;
            if (rd(b, 1)) { bd[i].pend.has_start = 1; bd[i].pend.start = (int)rd(b, 5); }
            if (rd(b, 1)) { bd[i].pend.has_stop = 1; bd[i].pend.stop = (int)rd(b, 5); }
        }
        MUST(ch + 1, 0);
        for (int i = 0; i < nb; ++i) {
            if (ch && shared[i]) continue;
            bd[i].nw = (int)rd(b, 4);
        }
        CHK();
        for (int i = 0; i < nb; ++i) {
            if ((ch && shared[i]) || !bd[i].nw) continue;
            bd[i].start_index = idx;
            idx += bd[i].nw;
        }
        if (idx > 48) return R_BAD_CODE;
        if (ch) MUST(1, 0);
        for (int i = 0; i < nb; ++i) {
            const int n = bd[i].nw;
            if ((ch && shared[i]) || !n) continue;
            int* fq = r->freq + bd[i].start_index;
            const int desc = n > 1 ? (int)rd(b, 1) : 0;
            if (!desc) {
                fq[0] = (int)rd(b, 10);
                for (int j = 1; j < n; ++j) {
                    const int p = fq[j - 1];
                    if (p < 512) {
                        fq[j] = (int)rd(b, 10);
                    } else {
                        const int nbits = first_set_bit_plus1((uint32_t)(1023 - p));
                        fq[j] = (int)rd(b, nbits) + 1024 - (1 << nbits);
                    }
                }
            } else {
                fq[n - 1] = (int)rd(b, 10);
                for (int j = n - 2; j >= 0; --j) fq[j] = (int)rd(b, first_set_bit_plus1((uint32_t)fq[j + 1]));
            }
            CHK();
        }
        MUST(ch + 1, 0);
        for (int i = 0; i < nb; ++i)
            if (!(ch && shared[i]))
                for (int j = 0; j < bd[i].nw; ++j) r->amp_sf[bd[i].start_index + j] = (int)rd(b, 6);
        CHK();
        for (int i = 0; i < nb; ++i)
            if (!(ch && shared[i]))
                for (int j = 0; j < bd[i].nw; ++j) r->phase[bd[i].start_index + j] = (int)rd(b, 5);
        CHK();
    }
    if (C == 2)
        for (int i = 0; i < nb; ++i) {
            if (shared[i]) r->band[1][i] = r->band[0][i];
            if (leader) {
                const tband t = r->band[0][i];
                r->band[0][i] = r->band[1][i];
                r->band[1][i] = t;
            }
        }
    r->present = 1;
#undef MUST
#undef CHK
    return R_OK;
}

/* steps 1-2 of one frame of limit_bits / 8 bytes: spec [channels][2048] (zeroed here), win [channels]; sparse: the decoder with
 * AT3PHIP_DECODE_SPARSE, which takes word length 0 inside the coded range; r: the tonal record (zeroed here), or NULL for the
 * decoder without AT3PHIP_DECODE_TONES, which rejects a tonal block */
static int parse_frame(const uint8_t* frame, int limit_bits, int channels, float* spec, uint16_t* win, trec* r, at3pd_fields* f, int sparse)
{
    bits b = {frame, 0, 0, limit_bits};
    int invalid = 0;
    memset(f, 0, sizeof(*f));
    memset(spec, 0, sizeof(float) * 2048 * channels);
    if (r) memset(r, 0, sizeof(*r));
    win[0] = win[channels - 1] = 0;
#define CHK() do { if (b.bad) return R_READ_PAST_END; if (invalid) return R_BAD_CODE; } while (0)
    if (rd(&b, 1) != 0) return R_BAD_HEADER;
    if ((int)rd(&b, 2) != channels - 1) return R_BAD_HEADER;
    const int nqu = (int)rd(&b, 5) + 1;
    if (rd(&b, 1) != 0) return R_UNSUPPORTED;   /* mute */
    f->n_qu = nqu;
    /* word lengths */
    {
        if (rd(&b, 2) != 3 || rd(&b, 2) != 0 || rd(&b, 2) != 0) return R_UNSUPPORTED;
        const int idx = (int)rd(&b, 2);
        f->wl[0][0] = (int)rd(&b, 3);
        for (int i = 1; i < nqu; ++i) f->wl[0][i] = (f->wl[0][i - 1] + vlc(&b, AT3P_WL_VLC[idx], 8, &invalid)) & 7;
        CHK();
    }
    if (channels == 2) {
        if (rd(&b, 2) != 1 || rd(&b, 2) != 0) return R_UNSUPPORTED;
        const int idx = (int)rd(&b, 2);
        for (int i = 0; i < nqu; ++i) f->wl[1][i] = (f->wl[0][i] + vlc(&b, AT3P_WL_VLC[idx], 8, &invalid)) & 7;
        CHK();
    }
    if (!sparse) {
        for (int ch = 0; ch < channels; ++ch)
            for (int i = 0; i < nqu; ++i)
                if (f->wl[ch][i] == 0) return R_BAD_CODE;   /* the word-length-0 decision: out of range */
    } else if (f->wl[0][nqu - 1] == 0 && f->wl[channels - 1][nqu - 1] == 0) {
        return R_UNSUPPORTED;   /* the highest unit carries a non-zero word length in some channel */
    }
    /* scale-factor indices */
    for (int ch = 0; ch < channels; ++ch) {
        if (rd(&b, 2) != 0) return R_UNSUPPORTED;
        for (int i = 0; i < nqu; ++i) f->sf[ch][i] = (int)rd(&b, 6);
        CHK();
    }
    /* code-table indices */
    f->full_table = (int)rd(&b, 1);
    for (int ch = 0; ch < channels; ++ch) {
        if (rd(&b, 1) != 0 || rd(&b, 2) != 0 || rd(&b, 1) != 0) return R_UNSUPPORTED;
        for (int i = 0; i < nqu; ++i) {
            if (!sparse || f->wl[ch][i]) {
                f->tab[ch][i] = (int)rd(&b, f->full_table + 2);
            } else if (ch && f->wl[0][i]) {   /* the "copy from channel 0" flag: the writer emits 1, "do not copy" */
                const uint32_t keep = rd(&b, 1);
                CHK();
                if (keep != 1) return R_UNSUPPORTED;
            }
        }
        CHK();
    }
    /* spectra and power-compensation groups */
    for (int ch = 0; ch < channels; ++ch) {
        float* sp = spec + 2048 * ch;
        for (int qu = 0; qu < nqu; ++qu) {
            if (f->wl[ch][qu] == 0) continue;   /* (sparse only) the unit's lines stay +0.0f */
            const int wl = f->wl[ch][qu], t = wl - 1 + 7 * f->tab[ch][qu];
            const int group_size = AT3P_SPEC_TAB[t][0] & 15, num_coeffs = AT3P_SPEC_TAB[t][0] >> 4;
            const int cbits = AT3P_SPEC_TAB[t][1] & 15, is_signed = AT3P_SPEC_TAB[t][1] >> 4;
            const float mant = AT3P_MANT[wl], scale = AT3P_SCALE[f->sf[ch][qu]];
            const int start = kQuStart[qu], n = kQuStart[qu + 1] - start;
            for (int pos = 0; pos < n;) {
                if (group_size != 1 && rd(&b, 1) == 0) {   /* an all-zero group */
                    CHK();
                    pos += group_size * num_coeffs;
                    continue;
                }
                for (int j = 0; j < group_size; ++j) {
                    const int val = spec_vlc(&b, t, &invalid);
                    CHK();
                    for (int i = 0; i < num_coeffs; ++i, ++pos) {
                        int m = (val >> (cbits * i)) & ((1 << cbits) - 1);
                        if (is_signed) {
                            m = (int)((uint32_t)m << (32 - cbits)) >> (32 - cbits);
                        } else if (m != 0 && rd(&b, 1)) {
                            m = -m;
                        }
                        CHK();
                        sp[start + pos] = (float)m * mant * scale;
                    }
                }
            }
        }
        const int npw = AT3P_SB_POWGRPS[AT3P_QU_TO_SB[nqu - 1]];
        for (int i = 0; i < npw; ++i) {
            const uint32_t lev = rd(&b, 4);
            CHK();
            if (lev != 15) return R_UNSUPPORTED;
        }
    }
    /* the tail */
    if (channels == 2) {
        const uint32_t sn = rd(&b, 2);
        CHK();
        if (sn != 0) return R_UNSUPPORTED;
    }
    const int sb_bits = AT3P_QU_TO_SB[31] + 1;   /* the writer's count: its tonal part is formed in the pass with 32 units */
    for (int ch = 0; ch < channels; ++ch) {
        uint16_t w = 0;
        if (rd(&b, 1)) {
            if (rd(&b, 1) == 0) {
                w = 0xffff;
            } else {
                for (int i = 0; i < sb_bits; ++i) w |= (uint16_t)(rd(&b, 1) << i);
            }
        }
        CHK();
        f->win[ch] = w;
    }
    for (int ch = 0; ch < channels; ++ch) {
        const uint32_t g = rd(&b, 1);
        CHK();
        if (g) return R_UNSUPPORTED;   /* gain compensation */
    }
    {
        const uint32_t tonal = rd(&b, 1);
        CHK();
        if (tonal) {
            if (!r) return R_TONAL;
            const int why = parse_tonal(&b, channels, r);
            if (why) return why;
        }
        const uint32_t noise = rd(&b, 1);
        CHK();
        if (noise) return R_UNSUPPORTED;
        const uint32_t term = rd(&b, 2);
        CHK();
        if (term != 3) return R_NO_TERMINATOR;
    }
#undef CHK
    for (int ch = 0; ch < channels; ++ch) win[ch] = (uint16_t)f->win[ch];
    return R_OK;
}

/* ---- steps 3-6 ---- */
typedef struct {
    float tail[16][128];   /* THistBuf::Buf: the windowed second halves of the previous frame */
    uint16_t win;          /* THistBuf::Win: the previous frame's flags */
    float buf1[24][8], buf2[24][8];
    int pos;
} at3pd_channel;

typedef struct {
    at3pd_channel ch[2];
} at3pd_stream;

static int g_reverse_pairing;   /* test-only: window frame n's first half with ITS OWN flags (the wrong pairing) */
void at3pd_test_reverse_pairing(int on) { g_reverse_pairing = on; }

static const float kRescale = (float)(32768.0 / 1.122018);

/* step 3 for one channel: spec [2048] -> subband samples [16][128] */
static void midct(at3pd_channel* c, const float* spec, uint16_t win, float* sub)
{
    const uint16_t first = g_reverse_pairing ? win : c->win;
    for (int b = 0; b < 16; ++b) {
        float in[128], inv[256];
        for (int j = 0; j < 128; ++j) in[j] = (b & 1) ? spec[b * 128 + 127 - j] : spec[b * 128 + j];
        imdct256(in, inv);
        if ((first >> b) & 1) {
            for (int j = 0; j < 32; ++j) inv[j] = 0.0f;
            for (int j = 0; j < 64; ++j) inv[j + 32] *= T.sine64[j];
            for (int j = 96; j < 128; ++j) inv[j] *= 2.0f;
        } else {
            for (int j = 0; j < 128; ++j) inv[j] *= T.sine128[j];
        }
        if ((win >> b) & 1) {
            for (int j = 128; j < 160; ++j) inv[j] *= 2.0f;
            for (int j = 0; j < 64; ++j) inv[223 - j] *= T.sine64[j];
            for (int j = 224; j < 256; ++j) inv[j] = 0.0f;
        } else {
            for (int j = 0; j < 128; ++j) inv[255 - j] *= T.sine128[j];
        }
        for (int j = 0; j < 128; ++j) sub[b * 128 + j] = inv[j] + c->tail[b][j];
        memcpy(c->tail[b], inv + 128, sizeof(c->tail[b]));
    }
    c->win = win;
}

/* step 5 for one channel: rescaled subband samples [16][128] -> 2048 samples */
static void ipqf(at3pd_channel* c, const float* in, float* out)
{
    memset(out, 0, 2048 * sizeof(float));
    for (int s = 0; s < 128; ++s) {
        float x[16], y[16];
        for (int sb = 0; sb < 16; ++sb) x[sb] = in[sb * 128 + s];
        for (int k = 0; k < 16; ++k) {
            double sum = 0;
            for (int n = 0; n < 16; ++n) sum += (double)x[n] * T.cos16[k][n];
            y[15 - k] = (float)(sum * (1.0 / 1024));
        }
        for (int i = 0; i < 8; ++i) {
            c->buf1[c->pos][i] = y[i + 8];
            c->buf2[c->pos][i] = y[7 - i];
        }
        /* tap t reads the columns 2t and 2t + 1 samples back: rows pos + 2t and pos + 2t + 1 of the 24-row ring */
        for (int t = 0; t < 12; ++t) {
            const int r1 = (c->pos + 2 * t) % 24, r2 = (c->pos + 2 * t + 1) % 24;
            for (int i = 0; i < 8; ++i) {
                const float a = c->buf1[r1][i] * kFir[12 * i + t], d = c->buf2[r2][i] * kFir[192 + 12 * i + t];
                out[s * 16 + i] = out[s * 16 + i] + (a + d);
                const float e = c->buf1[r1][7 - i] * kFir[12 * (i + 8) + t], g = c->buf2[r2][7 - i] * kFir[192 + 12 * (i + 8) + t];
                out[s * 16 + i + 8] = out[s * 16 + i + 8] + (e + g);
            }
        }
        c->pos = (c->pos + 23) % 24;
    }
}

/* ---- step 4b, as ff_atrac3p_generate_tones runs it: frame after frame with tones_info / tones_info_prev and their curr_env kept
 * between frames (the GPU reconstructs those from three records) ---- */
static struct { float sine[2048], hann[256], amp_sf[64]; int init; } TT;

static void init_tone_tables(void)
{
    if (TT.init) return;
    for (int i = 0; i < 2048; ++i) TT.sine[i] = (float)sin(2 * M_PI * i / 2048);
    for (int i = 0; i < 256; ++i) TT.hann[i] = (float)((1.0f - cos(2 * M_PI * i / 256.0f)) * 0.5f);
    for (int i = 0; i < 64; ++i) TT.amp_sf[i] = exp2f((i - 3) / 4.0f);
    TT.init = 1;
}

static void waves_synth(const trec* r, const tband* t, const tenv* e, int reg, float* out)
{
    for (int wn = 0; wn < t->nw; ++wn) {
        const int k = t->start_index + wn;
        const double amp = (double)TT.amp_sf[r->amp_sf[k]];
        const int inc = r->freq[k];
        int pos = (((r->phase[k] & 31) << 6) - (reg ^ 128) * inc) & 2047;
        for (int i = 0; i < 128; ++i) {
            out[i] = (float)((double)out[i] + (double)TT.sine[pos] * amp);
            pos = (pos + inc) & 2047;
        }
    }
    if (e->has_start) {
        const int pos = (e->start << 2) - reg;
        if (pos > 0 && pos <= 128) {
            for (int i = 0; i < pos; ++i) out[i] = 0.0f;
            if (!e->has_stop || e->start != e->stop)
                for (int k = 0; k < 4; ++k) out[pos + k] = out[pos + k] * TT.hann[32 * k];
        }
    }
    if (e->has_stop) {
        const int pos = ((e->stop + 1) << 2) - reg;
        if (pos > 0 && pos <= 128) {
            for (int k = 0; k < 4; ++k) out[pos - 4 + k] = out[pos - 4 + k] * TT.hann[96 - 32 * k];
            for (int i = pos; i < 128; ++i) out[i] = 0.0f;
        }
    }
}

/* encoder = 0: the decoder's step 4b (s - g, g = 0.0f - (wavreg1 + wavreg2)); encoder = 1: ApplyFilter's out -= wavreg1 + wavreg2 */
static void generate_tones(const trec* prev, trec* cur, int ch, int sb, float* out, int encoder)
{
    const tband* now = &prev->band[ch][sb];
    tband* next = &cur->band[ch][sb];
    tenv* c = &next->curr;
    if (next->pend.has_start && next->pend.start < next->pend.stop) { c->has_start = 1; c->start = next->pend.start + 32; }
    else if (now->pend.has_start) { c->has_start = 1; c->start = now->pend.start; }
    else { c->has_start = 0; c->start = 0; }
    if (now->pend.has_stop && now->pend.stop >= c->start) { c->has_stop = 1; c->stop = now->pend.stop; }
    else if (next->pend.has_stop) { c->has_stop = 1; c->stop = next->pend.stop + 32; }
    else { c->has_stop = 0; c->stop = 64; }
    const int reg1 = now->curr.stop < 32 ? 0 : 1, reg2 = c->start >= 32 ? 0 : 1;
    float w1[128] = {0}, w2[128] = {0};
    if (now->nw && reg1) waves_synth(prev, now, &now->curr, 128, w1);
    if (next->nw && reg2) waves_synth(cur, next, c, 0, w2);
    if (now->nw && next->nw && reg1 && reg2) {
        for (int i = 0; i < 128; ++i) { w1[i] = w1[i] * TT.hann[128 + i]; w2[i] = w2[i] * TT.hann[i]; }
    } else {
        if (now->nw && !now->curr.has_stop) for (int i = 0; i < 128; ++i) w1[i] = w1[i] * TT.hann[128 + i];
        if (next->nw && !c->has_start) for (int i = 0; i < 128; ++i) w2[i] = w2[i] * TT.hann[i];
    }
    for (int i = 0; i < 128; ++i) {
        if (encoder) {
            out[i] -= w1[i] + w2[i];
        } else {
            const float g = 0.0f - (w1[i] + w2[i]);
            out[i] = out[i] - g;
        }
    }
}

/* ---- the frame loop ---- */
/* steps 1-2 of one frame of frame_bytes bytes; a rejected frame gives a zero spectrum, sine windows and no record. r as parse_frame's */
static int unpack(const uint8_t* frame, int frame_bytes, int C, float* spec, uint16_t* win, trec* r, at3pd_fields* f, int sparse)
{
    init_tables();
    const int why = parse_frame(frame, 8 * frame_bytes, C, spec, win, r, f, sparse);
    f->reason = why;
    if (why) {
        if (r) memset(r, 0, sizeof(*r));
        memset(spec, 0, sizeof(float) * 2048 * C);
        for (int ch = 0; ch < C; ++ch) win[ch] = 0;
    }
    return why;
}

/* frames [n][frame_bytes] -> pcm [n][2048][C] float32, with tonal blocks (tones = 1) or as the decoder without the flag. prev: frame
 * n - 1's record with the curr_env step 4b gave it (NULL, with tones = 0, for a stream that keeps none); rejected [6] accumulates;
 * fields [n] optional */
static void decode_frames(at3pd_stream* st, trec* prev, int C, const uint8_t* frames, int frame_bytes, int n_frames, float* pcm,
                          uint64_t* rejected, at3pd_fields* fields, int tones, int sparse)
{
    init_tone_tables();
    for (int fr = 0; fr < n_frames; ++fr) {
        float spec[2][2048];
        uint16_t win[2] = {0, 0};
        trec cur;
        at3pd_fields f;
        memset(&cur, 0, sizeof(cur));
        const int why = unpack(frames + (size_t)fr * frame_bytes, frame_bytes, C, &spec[0][0], win, tones ? &cur : NULL, &f, sparse);
        if (fields) fields[fr] = f;
        if (why) rejected[why - 1]++;
        for (int ch = 0; ch < C; ++ch) {
            float sub[2048], out[2048];
            midct(&st->ch[ch], spec[ch], win[ch], sub);
            for (int i = 0; i < 2048; ++i) sub[i] = sub[i] * kRescale;
            if (tones && (cur.present || prev->present))
                for (int sb = 0; sb < 16; ++sb)
                    if (cur.band[ch][sb].nw || prev->band[ch][sb].nw) generate_tones(prev, &cur, ch, sb, sub + sb * 128, 0);
            ipqf(&st->ch[ch], sub, out);
            for (int i = 0; i < 2048; ++i) {
                float v = out[i];
                v = v > 1.0f ? 1.0f : v;
                v = v < -1.0f ? -1.0f : v;
                pcm[((size_t)fr * 2048 + i) * C + ch] = v;
            }
        }
        if (prev) *prev = cur;
    }
}

/* ---- the decoder without AT3PHIP_DECODE_TONES at 2048 bytes ---- */
size_t at3pd_state_bytes(void) { return sizeof(at3pd_stream); }
size_t at3pd_fields_bytes(void) { return sizeof(at3pd_fields); }

void at3pd_reset(void* state)
{
    init_tables();
    memset(state, 0, sizeof(at3pd_stream));
}

/* steps 1-2 of one frame: specs [channels][2048], win [channels]; returns the reason (0 = decoded) */
int at3pd_unpack_frame(const uint8_t* frame, int channels, float* specs, uint16_t* win, void* fields_out)
{
    at3pd_fields f;
    const int why = unpack(frame, 2048, channels, specs, win, NULL, &f, 0);
    if (fields_out) memcpy(fields_out, &f, sizeof(f));
    return why;
}

/* frames [n][2048] -> pcm [n][2048][channels] float32; rejected [6] accumulates; fields [n] optional */
void at3pd_decode(void* state, int channels, const uint8_t* frames, int n_frames, float* pcm, uint64_t* rejected, void* fields)
{
    decode_frames((at3pd_stream*)state, NULL, channels, frames, 2048, n_frames, pcm, rejected, (at3pd_fields*)fields, 0, 0);
}

/* test-only: the spectrum codes decoded so far by every entry point that parses frames, counts [56][256] by (table, symbol) (NULL:
 * none copied); reset != 0 zeroes the counters afterwards */
void at3pd_hits(uint32_t* counts, int reset)
{
    if (counts) memcpy(counts, g_hits, sizeof(g_hits));
    if (reset) memset(g_hits, 0, sizeof(g_hits));
}

/* the host-built tables the decoder needs, for the tests: cos16 [16][16] ([k][n]), sine128, sine64 */
void at3pd_tables(double* cos16, float* sine128, float* sine64)
{
    init_tables();
    memcpy(cos16, T.cos16, sizeof(T.cos16));
    memcpy(sine128, T.sine128, sizeof(T.sine128));
    memcpy(sine64, T.sine64, sizeof(T.sine64));
}
