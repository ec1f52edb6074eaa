/* TEST INFRASTRUCTURE ONLY - CPU restatement of the ATRAC3plus adaptive writer and of the decoder's unpack with SPARSE WORD LENGTHS
 * (include/at3phip.h: ADAPTIVE WORD LENGTHS, FRAME SIZE, SPARSE WORD LENGTHS, and the decoder section with AT3PHIP_DECODE_SPARSE),
 * the sparse steps and the frame size as arguments. With `sparse` 0 every function here is tests/host/at3p_rate_cpu.c's, frames,
 * PCM and counters bit for bit (tests/test_at3p_sparse_cpu.py pins that); everything sparse is pinned to this file. Plain C, scalar.
 *   encoder  steps A1-A6 written out again; with sparse: A3s, A4s, A6s;
 *   decoder  steps 1-2 (and the tonal block) written out again, with sparse: word length 0 inside the coded range; steps 3-6 and
 *            4b are those of at3p_decode_cpu.c / at3p_tonal_cpu.c, included here as at3p_rate_cpu.c includes them.
 * Compiled by the tests with gcc -O2 -fPIC -ffp-contract=off -fno-fast-math. */
#include "at3p_tonal_cpu.c"

#define MAX_FRAME_SZ 2048
#define T_MIN (-21)
#define T_MAX 63
#define K_MAX 64
#define TAIL_BYTES 256

/* ================================================================ encoder ================================================= */
static const uint16_t kSpecsPerBlock[32] = {16, 16, 16, 16, 16, 16, 16, 16, 32, 32, 32, 32, 32, 32, 32, 32,
                                            64, 64, 64, 64, 64, 64, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128};

typedef struct {
    uint8_t* buf;   /* NULL: only count */
    int pos, limit; /* limit: the frame's bits; what lies past it is dropped */
} wbits;

static void wput(wbits* b, uint32_t val, int n)
{
    for (int k = n - 1; k >= 0; --k) {
        if (b->buf && b->pos < b->limit && ((val >> k) & 1u)) b->buf[b->pos >> 3] |= (uint8_t)(0x80u >> (b->pos & 7));
        b->pos++;
    }
}
static void wput_vlc(wbits* b, uint16_t e) { wput(b, e & 0xfffu, e >> 12); }

/* A1: TScaler::Scale */
static int r_scale_block(const float* in, int len, float* values)
{
    float maxAbs = 0;
    for (int i = 0; i < len; ++i) {
        const float a = fabsf(in[i]);
        if (a > maxAbs) maxAbs = a;
    }
    if (maxAbs > 1.0f) maxAbs = 1.0f;
    int idx = 0;
    while (idx < 63 && AT3P_SCALE[idx] < maxAbs) ++idx;
    const float sf = AT3P_SCALE[idx];
    for (int i = 0; i < len; ++i) {
        float v = in[i] / sf;
        if (fabsf(v) >= 1.0f) v = (v > 0) ? (float)0.99999 : (float)-0.99999;
        values[i] = v;
    }
    return idx;
}

/* EncodeQuSpectra: bits of `n` mantissas under table `idx`; written out when b->buf != NULL */
static int r_qu_spectra(const int* q, int n, int idx, wbits* b)
{
    const int group_size = AT3P_SPEC_TAB[idx][0] & 15, num_coeffs = AT3P_SPEC_TAB[idx][0] >> 4;
    const int bits = AT3P_SPEC_TAB[idx][1] & 15, is_signed = AT3P_SPEC_TAB[idx][1] >> 4;
    const uint16_t* vlc = AT3P_VLC + AT3P_VLC_OFF[idx];
    const int before = b->pos;
    for (int pos = 0; pos < n;) {
        if (group_size != 1) wput(b, 1, 1);
        for (int j = 0; j < group_size; ++j) {
            uint32_t val = 0;
            int signs[4] = {0, 0, 0, 0};
            for (int i = 0; i < num_coeffs; ++i) {
                int16_t t = (int16_t)q[pos++];
                if (!is_signed && t != 0) {
                    signs[i] = t > 0 ? 1 : -1;
                    if (t < 0) t = (int16_t)-t;
                } else {
                    t = (int16_t)(t & ((1u << bits) - 1));
                }
                t = (int16_t)(t << (bits * i));
                val |= (uint32_t)(uint16_t)t;
            }
            wput_vlc(b, vlc[val & 0xffu]);
            for (int i = 0; i < 4; ++i)
                if (signs[i] != 0) wput(b, signs[i] > 0 ? 0 : 1, 1);
        }
    }
    return b->pos - before;
}

/* (for a scaled value that is not finite see the note at quantise() in at3p_alloc_cpu.c: the same conversion) */
static void r_quantise(const float* values, int n, int wl, int* mant)
{
    const float mul = AT3P_INV_MANT[wl];
    for (int i = 0; i < n; ++i) mant[i] = (int)lrintf(values[i] * mul);
}

/* A1 + A2 for one frame (they do not depend on the frame size) */
int at3ps_cost_table(const float* specs, int channels, uint8_t* sfi, uint16_t* bits, uint8_t* tab, float* values_out)
{
    if (channels < 1 || channels > 2) return -1;
    float values[2048];
    int mant[128];
    for (int ch = 0; ch < channels; ++ch) {
        for (int qu = 0; qu < 32; ++qu) {
            const int start = kQuStart[qu], n = kSpecsPerBlock[qu];
            sfi[ch * 32 + qu] = (uint8_t)r_scale_block(specs + ch * 2048 + start, n, values + start);
            bits[(ch * 32 + qu) * 8] = 0;
            tab[(ch * 32 + qu) * 8] = 0;
            for (int w = 1; w <= 7; ++w) {
                r_quantise(values + start, n, w, mant);
                long best = -1;
                int bi = 0;
                for (int i = 0; i < 8; ++i) {
                    wbits cnt = {NULL, 0, 0};
                    const int t = r_qu_spectra(mant, n, w - 1 + 7 * i, &cnt);
                    if (best < 0 || t < best) {
                        best = t;
                        bi = i;
                    }
                }
                bits[(ch * 32 + qu) * 8 + w] = (uint16_t)best;
                tab[(ch * 32 + qu) * 8 + w] = (uint8_t)bi;
            }
        }
        if (values_out) memcpy(values_out + ch * 2048, values, sizeof(values));
    }
    return 0;
}

static int r_want(int sfi, int t)
{
    const int d = sfi - t;
    if (d <= 0) return 0;
    return d / 3 > 7 ? 7 : d / 3;
}

/* A3: the candidate allocation A(t, k); returns N, and in *took how many units took the t - 1 value */
static int r_candidate_dense(const uint8_t* sfi, int channels, int t, int k, uint8_t wl[2][32], int* took)
{
    int N = 1;
    memset(wl, 0, 64);
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu) {
            wl[ch][qu] = (uint8_t)r_want(sfi[ch * 32 + qu], t);
            if (wl[ch][qu] >= 1 && qu + 1 > N) N = qu + 1;
        }
    if (N >= 29 && N <= 31) N = 32;
    int taken = 0;
    for (int qu = 0; qu < N; ++qu)
        for (int ch = 0; ch < channels; ++ch) {
            const int up = r_want(sfi[ch * 32 + qu], t - 1);
            if (up > wl[ch][qu] && taken < k) {
                wl[ch][qu] = (uint8_t)up;
                ++taken;
            }
        }
    if (took) *took = taken;
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu) {
            if (qu < N && wl[ch][qu] == 0) wl[ch][qu] = 1;
            if (qu >= N) wl[ch][qu] = 0;
        }
    return N;
}

/* A3s: all 32 units are walked, nothing is raised from 0 to 1, N follows the k-raise */
static int r_candidate_sparse(const uint8_t* sfi, int channels, int t, int k, uint8_t wl[2][32], int* took)
{
    memset(wl, 0, 64);
    int taken = 0;
    for (int qu = 0; qu < 32; ++qu)
        for (int ch = 0; ch < channels; ++ch) {
            const int w0 = r_want(sfi[ch * 32 + qu], t), up = r_want(sfi[ch * 32 + qu], t - 1);
            wl[ch][qu] = (uint8_t)w0;
            if (up > w0 && taken < k) {
                wl[ch][qu] = (uint8_t)up;
                ++taken;
            }
        }
    if (took) *took = taken;
    int N = 0;
    for (int qu = 0; qu < 32; ++qu)
        for (int ch = 0; ch < channels; ++ch)
            if (wl[ch][qu] >= 1) N = qu + 1;
    if (N == 0) {   /* no unit wanted: unit 0 of channel 0 carries the frame */
        N = 1;
        wl[0][0] = 1;
    }
    if (N >= 29 && N <= 31) {   /* the syntax has no 29..31; the highest coded unit carries a non-zero word length */
        N = 32;
        if (wl[0][31] == 0 && wl[1][31] == 0) wl[0][31] = 1;
    }
    return N;
}

static int r_candidate(const uint8_t* sfi, int channels, int t, int k, uint8_t wl[2][32], int* took, int sparse)
{
    return sparse ? r_candidate_sparse(sfi, channels, t, k, wl, took) : r_candidate_dense(sfi, channels, t, k, wl, took);
}

/* TWordLenEncoder: channel 0 in mode 3 (deltas to the previous unit), channel 1 in mode 1 (deltas to channel 0) */
static int r_best_wl_table(const int8_t* delta, int sz, int maxDelta)
{
    const int t0 = maxDelta >= 3 ? 2 : maxDelta == 2 ? 1 : 0, t1 = maxDelta >= 3 ? 3 : t0;
    int best = 0;
    long consumed = -1;
    for (int i = t0; i <= t1; ++i) {
        long t = 0;
        for (int j = 1; j < sz; ++j) t += AT3P_WL_VLC[i][delta[j]] >> 12;
        if (consumed < 0 || t < consumed) {
            consumed = t;
            best = i;
        }
    }
    return best;
}
static void r_wordlen_section(wbits* b, const uint8_t* wl0, const uint8_t* wl1, int N, int channels)
{
    int8_t d0[32], dx[32];
    int max0 = 0, maxx = 0;
    d0[0] = (int8_t)wl0[0];
    for (int i = 0; i < N; ++i) {
        if (i) {
            const int d = (int)wl0[i] - (int)wl0[i - 1];
            max0 |= abs(d);
            d0[i] = (int8_t)(d & 7);
        }
        const int t = channels == 2 ? (int)wl1[i] - (int)wl0[i] : 0;
        maxx |= abs(t);
        dx[i] = (int8_t)(t & 7);
    }
    {
        const int idx = r_best_wl_table(d0, N, max0);
        wput(b, 3, 2);
        wput(b, 0, 2);
        wput(b, 0, 2);
        wput(b, (uint32_t)idx, 2);
        wput(b, (uint32_t)d0[0], 3);
        for (int i = 1; i < N; ++i) wput_vlc(b, AT3P_WL_VLC[idx][d0[i]]);
    }
    if (channels == 2) {
        const int idx = r_best_wl_table(dx, N, maxx);
        wput(b, 1, 2);
        wput(b, 0, 2);
        wput(b, (uint32_t)idx, 2);
        for (int i = 0; i < N; ++i) wput_vlc(b, AT3P_WL_VLC[idx][dx[i]]);
    }
}

/* the code-table section's bits: 1, then per channel 4 and, A4: 3 per unit below N; A4s: 3 per unit below N with a non-zero word
 * length and, in channel 1, 1 per unit with word length 0 whose channel-0 word length is not 0 (the "copy from channel 0" flag) */
static int r_codetab_bits(uint8_t wl[2][32], int N, int channels, int sparse)
{
    int n = 1;
    for (int ch = 0; ch < channels; ++ch) {
        n += 4;
        for (int qu = 0; qu < N; ++qu) {
            if (!sparse || wl[ch][qu]) n += 3;
            else if (ch && wl[0][qu]) n += 1;
        }
    }
    return n;
}

/* A4 / A4s: Bits(A) */
static int r_alloc_bits(const uint16_t* bits, int channels, int tail_bits, uint8_t wl[2][32], int N, int sparse)
{
    wbits b = {NULL, 0, 0};
    r_wordlen_section(&b, wl[0], wl[1], N, channels);
    long total = 5 + 1 + b.pos + channels * (2 + 6 * N) + r_codetab_bits(wl, N, channels, sparse) + channels * 4 * AT3P_SB_POWGRPS[AT3P_QU_TO_SB[N - 1]] +
                 tail_bits;
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < N; ++qu)
            if (wl[ch][qu]) total += bits[(ch * 32 + qu) * 8 + wl[ch][qu]];   /* (entry 0 is not read) */
    return total > 0x7fffffff ? 0x7fffffff : (int)total;
}

/* A3-A5 on a cost table against the budget 8 * frame_bytes - 3: wl_out [channels][32] (0 at and above N), N, t*, k*; returns
 * Bits(A(t*, k*)). Where no t fits (a caller's table only), t* = 63 and k* = 0. */
int at3ps_allocate(const uint8_t* sfi, const uint16_t* bits, int channels, int tail_bits, int frame_bytes, int sparse, uint8_t* wl_out,
                   int32_t* n_units, int32_t* t_out, int32_t* k_out)
{
    const int size_bits = 8 * frame_bytes - 3;
    uint8_t wl[2][32];
    int ts = T_MAX, ks = 0;
    for (int t = T_MIN; t <= T_MAX; ++t) {
        const int N = r_candidate(sfi, channels, t, 0, wl, NULL, sparse);
        if (r_alloc_bits(bits, channels, tail_bits, wl, N, sparse) <= size_bits) {
            ts = t;
            break;
        }
    }
    for (int k = 0; k <= K_MAX; ++k) {
        const int N = r_candidate(sfi, channels, ts, k, wl, NULL, sparse);
        if (r_alloc_bits(bits, channels, tail_bits, wl, N, sparse) <= size_bits) ks = k;
    }
    const int N = r_candidate(sfi, channels, ts, ks, wl, &ks, sparse);   /* k* as reported: the units that took the t - 1 value */
    memcpy(wl_out, wl, (size_t)channels * 32);
    *n_units = N;
    *t_out = ts;
    *k_out = ks;
    return r_alloc_bits(bits, channels, tail_bits, wl, N, sparse);
}

typedef struct {
    int32_t t, k, num_quant_units, bits;   /* bits: Bits(A(t*, k*)), without the three leading bits */
    uint8_t wl[2][32], sfi[2][32], tab[2][32];
} at3ps_frame_info;

/* A6: one frame of frame_bytes bytes; tail: tail_bits bits, most significant first */
static void r_write_frame(const float* specs, int channels, int frame_bytes, int sparse, const uint8_t* tail, int tail_bits, uint8_t* out,
                          at3ps_frame_info* info)
{
    uint8_t sfi[2][32], tab[2][32][8], wl[2][32];
    uint16_t bits[2][32][8];
    float values[2][2048];
    int mant[128];
    memset(sfi, 0, sizeof(sfi));
    memset(tab, 0, sizeof(tab));
    memset(bits, 0, sizeof(bits));
    at3ps_cost_table(specs, channels, &sfi[0][0], &bits[0][0][0], &tab[0][0][0], &values[0][0]);
    int32_t N, t, k;
    const int total = at3ps_allocate(&sfi[0][0], &bits[0][0][0], channels, tail_bits, frame_bytes, sparse, &wl[0][0], &N, &t, &k);
    if (channels == 1) memset(wl[1], 0, 32);
    memset(out, 0, (size_t)frame_bytes);
    wbits b = {out, 0, 8 * frame_bytes};
    wput(&b, 0, 1);
    wput(&b, (uint32_t)channels - 1, 2);
    wput(&b, (uint32_t)N - 1, 5);
    wput(&b, 0, 1);
    r_wordlen_section(&b, wl[0], wl[1], N, channels);
    for (int ch = 0; ch < channels; ++ch) {
        wput(&b, 0, 2);
        for (int i = 0; i < N; ++i) wput(&b, sfi[ch][i], 6);
    }
    wput(&b, 1, 1);
    for (int ch = 0; ch < channels; ++ch) {
        wput(&b, 0, 1);
        wput(&b, 0, 2);
        wput(&b, 0, 1);
        for (int i = 0; i < N; ++i) {
            if (!sparse || wl[ch][i]) wput(&b, tab[ch][i][wl[ch][i]], 3);
            else if (ch && wl[0][i]) wput(&b, 1, 1);   /* A4s: "do not copy from channel 0" */
        }
    }
    for (int ch = 0; ch < channels; ++ch) {
        for (int qu = 0; qu < N; ++qu) {
            if (wl[ch][qu] == 0) continue;   /* (A4s; A3 never leaves a 0 below N) */
            r_quantise(values[ch] + kQuStart[qu], kSpecsPerBlock[qu], wl[ch][qu], mant);
            r_qu_spectra(mant, kSpecsPerBlock[qu], wl[ch][qu] - 1 + 7 * tab[ch][qu][wl[ch][qu]], &b);
        }
        const int numPwrSpec = AT3P_SB_POWGRPS[AT3P_QU_TO_SB[N - 1]];
        for (int i = 0; i < numPwrSpec; ++i) wput(&b, 15, 4);
    }
    for (int i = 0; i < tail_bits; ++i) wput(&b, (tail[i >> 3] >> (7 - (i & 7))) & 1u, 1);
    if (info) {
        info->t = t;
        info->k = k;
        info->num_quant_units = N;
        info->bits = total;
        memcpy(info->wl, wl, sizeof(wl));
        memcpy(info->sfi, sfi, sizeof(sfi));
        for (int ch = 0; ch < 2; ++ch)
            for (int qu = 0; qu < 32; ++qu) info->tab[ch][qu] = qu < N && ch < channels && wl[ch][qu] ? tab[ch][qu][wl[ch][qu]] : 0;
    }
}

/* specs [n_frames][channels][2048], tails [n_frames][TAIL_BYTES], tail_bits [n_frames] -> out [n_frames][frame_bytes]; info optional */
int at3ps_write_frames(const float* specs, int channels, int n_frames, int frame_bytes, int sparse, const uint8_t* tails, const int32_t* tail_bits,
                       uint8_t* out, void* info)
{
    if (channels < 1 || channels > 2 || frame_bytes < 8 || frame_bytes > MAX_FRAME_SZ || frame_bytes % 8) return -1;
    for (int f = 0; f < n_frames; ++f) {
        if (tail_bits[f] < 0 || tail_bits[f] > TAIL_BYTES * 8) return -1;
        r_write_frame(specs + (size_t)f * channels * 2048, channels, frame_bytes, sparse, tails + (size_t)f * TAIL_BYTES, tail_bits[f],
                      out + (size_t)f * frame_bytes, info ? (at3ps_frame_info*)info + f : NULL);
    }
    return n_frames;
}
int at3ps_frame_info_size(void) { return (int)sizeof(at3ps_frame_info); }
int at3ps_tail_bytes(void) { return TAIL_BYTES; }

/* ================================================================ decoder ================================================= */
/* step 1's bit reader, MSB first: every read must end within the frame's `limit` bits; a look-ahead past them sees zeros */
typedef struct { const uint8_t* buf; int pos, bad, limit; } lbits;
static int lbit_at(const lbits* b, int p) { return p < b->limit ? (b->buf[p >> 3] >> (7 - (p & 7))) & 1 : 0; }
static uint32_t lrd(lbits* b, int n)
{
    if (b->bad || b->pos + n > b->limit) { b->bad = 1; return 0; }
    uint32_t v = 0;
    for (int k = 0; k < n; ++k, ++b->pos) v = (v << 1) | (uint32_t)lbit_at(b, b->pos);
    return v;
}
/* a code of a complete prefix code given as code | length << 12 per symbol, searched in symbol order */
static int lvlc(lbits* b, const uint16_t* table, int n_sym, int* invalid)
{
    if (b->bad) return 0;
    for (int sym = 0; sym < n_sym; ++sym) {
        const int len = table[sym] >> 12, code = table[sym] & 0xfff;
        if (!len) continue;
        uint32_t v = 0;
        for (int k = 0; k < len; ++k) v = (v << 1) | (uint32_t)lbit_at(b, b->pos + k);
        if ((int)v == code) {
            if (b->pos + len > b->limit) { b->bad = 1; return 0; }
            b->pos += len;
            return sym;
        }
    }
    *invalid = 1;
    return 0;
}

#define LCHK() do { if (b->bad) return R_READ_PAST_END; if (invalid) return R_BAD_CODE; } while (0)
#define LMUST(n, val) do { const uint32_t v_ = lrd(b, n); LCHK(); if (v_ != (uint32_t)(val)) return R_UNSUPPORTED; } while (0)

/* the tonal block after its flag; r is zero on entry */
static int lparse_tonal(lbits* b, int C, trec* r)
{
    int invalid = 0;
    LMUST(1, 1);
    const int nb = lvlc(b, AT3P_TONE_BANDS_VLC, 16, &invalid) + 1;
    LCHK();
    int shared[16] = {0}, leader = 0;
    if (C == 2) {
        if (lrd(b, 1)) {
            if (lrd(b, 1) == 0) {
                for (int i = 0; i < nb; ++i) shared[i] = 1;
            } else {
                for (int i = 0; i < nb; ++i) shared[i] = (int)lrd(b, 1);
            }
        }
        LCHK();
        if (lrd(b, 1)) {
            LMUST(1, 0);
            leader = 1;
        }
        LMUST(1, 0);
    }
    int idx = 0;
    for (int ch = 0; ch < C; ++ch) {
        tband* bd = r->band[ch];
        if (ch) LMUST(1, 0);
        for (int i = 0; i < nb; ++i) {
            if (ch && shared[i]) continue;
            bd[i].pend.start = -1;
            bd[i].pend.stop = 32;
            if (lrd(b, 1)) { bd[i].pend.has_start = 1; bd[i].pend.start = (int)lrd(b, 5); }
            if (lrd(b, 1)) { bd[i].pend.has_stop = 1; bd[i].pend.stop = (int)lrd(b, 5); }
        }
        LMUST(ch + 1, 0);
        for (int i = 0; i < nb; ++i) {
            if (ch && shared[i]) continue;
            bd[i].nw = (int)lrd(b, 4);
        }
        LCHK();
        for (int i = 0; i < nb; ++i) {
            if ((ch && shared[i]) || !bd[i].nw) continue;
            bd[i].start_index = idx;
            idx += bd[i].nw;
        }
        if (idx > 48) return R_BAD_CODE;
        if (ch) LMUST(1, 0);
        for (int i = 0; i < nb; ++i) {
            const int n = bd[i].nw;
            if ((ch && shared[i]) || !n) continue;
            int* fq = r->freq + bd[i].start_index;
            const int desc = n > 1 ? (int)lrd(b, 1) : 0;
            if (!desc) {
                fq[0] = (int)lrd(b, 10);
                for (int j = 1; j < n; ++j) {
                    const int p = fq[j - 1];
                    if (p < 512) {
                        fq[j] = (int)lrd(b, 10);
                    } else {
                        const int nbits = first_set_bit_plus1((uint32_t)(1023 - p));
                        fq[j] = (int)lrd(b, nbits) + 1024 - (1 << nbits);
                    }
                }
            } else {
                fq[n - 1] = (int)lrd(b, 10);
                for (int j = n - 2; j >= 0; --j) fq[j] = (int)lrd(b, first_set_bit_plus1((uint32_t)fq[j + 1]));
            }
            LCHK();
        }
        LMUST(ch + 1, 0);
        for (int i = 0; i < nb; ++i)
            if (!(ch && shared[i]))
                for (int j = 0; j < bd[i].nw; ++j) r->amp_sf[bd[i].start_index + j] = (int)lrd(b, 6);
        LCHK();
        for (int i = 0; i < nb; ++i)
            if (!(ch && shared[i]))
                for (int j = 0; j < bd[i].nw; ++j) r->phase[bd[i].start_index + j] = (int)lrd(b, 5);
        LCHK();
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
    return R_OK;
}

/* steps 1-2 of one frame of limit / 8 bytes: spec [channels][2048] (zeroed here), win [channels]; r: the tonal record (zeroed here),
 * or NULL for the decoder without AT3PHIP_DECODE_TONES, which rejects a tonal block */
static int lparse_frame(const uint8_t* frame, int limit, int channels, float* spec, uint16_t* win, trec* r, at3pd_fields* f, int sparse)
{
    lbits bb = {frame, 0, 0, limit};
    lbits* b = &bb;
    int invalid = 0;
    memset(f, 0, sizeof(*f));
    memset(spec, 0, sizeof(float) * 2048 * channels);
    if (r) memset(r, 0, sizeof(*r));
    win[0] = win[channels - 1] = 0;
    if (lrd(b, 1) != 0) return R_BAD_HEADER;
    if ((int)lrd(b, 2) != channels - 1) return R_BAD_HEADER;
    const int nqu = (int)lrd(b, 5) + 1;
    if (lrd(b, 1) != 0) return R_UNSUPPORTED;   /* mute */
    f->n_qu = nqu;
    {
        if (lrd(b, 2) != 3 || lrd(b, 2) != 0 || lrd(b, 2) != 0) return R_UNSUPPORTED;
        const int idx = (int)lrd(b, 2);
        f->wl[0][0] = (int)lrd(b, 3);
        for (int i = 1; i < nqu; ++i) f->wl[0][i] = (f->wl[0][i - 1] + lvlc(b, AT3P_WL_VLC[idx], 8, &invalid)) & 7;
        LCHK();
    }
    if (channels == 2) {
        if (lrd(b, 2) != 1 || lrd(b, 2) != 0) return R_UNSUPPORTED;
        const int idx = (int)lrd(b, 2);
        for (int i = 0; i < nqu; ++i) f->wl[1][i] = (f->wl[0][i] + lvlc(b, AT3P_WL_VLC[idx], 8, &invalid)) & 7;
        LCHK();
    }
    if (!sparse) {
        for (int ch = 0; ch < channels; ++ch)
            for (int i = 0; i < nqu; ++i)
                if (f->wl[ch][i] == 0) return R_BAD_CODE;   /* the word-length-0 decision: out of range */
    } else if (f->wl[0][nqu - 1] == 0 && f->wl[channels - 1][nqu - 1] == 0) {
        return R_UNSUPPORTED;   /* the highest unit carries a non-zero word length in some channel */
    }
    for (int ch = 0; ch < channels; ++ch) {
        if (lrd(b, 2) != 0) return R_UNSUPPORTED;
        for (int i = 0; i < nqu; ++i) f->sf[ch][i] = (int)lrd(b, 6);
        LCHK();
    }
    f->full_table = (int)lrd(b, 1);
    for (int ch = 0; ch < channels; ++ch) {
        if (lrd(b, 1) != 0 || lrd(b, 2) != 0 || lrd(b, 1) != 0) return R_UNSUPPORTED;
        for (int i = 0; i < nqu; ++i) {
            if (!sparse || f->wl[ch][i]) {
                f->tab[ch][i] = (int)lrd(b, f->full_table + 2);
            } else if (ch && f->wl[0][i]) {   /* the "copy from channel 0" flag: the writer emits 1, "do not copy" */
                const uint32_t keep = lrd(b, 1);
                LCHK();
                if (keep != 1) return R_UNSUPPORTED;
            }
        }
        LCHK();
    }
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
                if (group_size != 1 && lrd(b, 1) == 0) {   /* an all-zero group */
                    LCHK();
                    pos += group_size * num_coeffs;
                    continue;
                }
                for (int j = 0; j < group_size; ++j) {
                    const int val = lvlc(b, AT3P_VLC + AT3P_VLC_OFF[t], AT3P_VLC_OFF[t + 1] - AT3P_VLC_OFF[t], &invalid);
                    LCHK();
                    for (int i = 0; i < num_coeffs; ++i, ++pos) {
                        int m = (val >> (cbits * i)) & ((1 << cbits) - 1);
                        if (is_signed) {
                            m = (int)((uint32_t)m << (32 - cbits)) >> (32 - cbits);
                        } else if (m != 0 && lrd(b, 1)) {
                            m = -m;
                        }
                        LCHK();
                        sp[start + pos] = (float)m * mant * scale;
                    }
                }
            }
        }
        const int npw = AT3P_SB_POWGRPS[AT3P_QU_TO_SB[nqu - 1]];
        for (int i = 0; i < npw; ++i) {
            const uint32_t lev = lrd(b, 4);
            LCHK();
            if (lev != 15) return R_UNSUPPORTED;
        }
    }
    if (channels == 2) {
        const uint32_t sn = lrd(b, 2);
        LCHK();
        if (sn != 0) return R_UNSUPPORTED;
    }
    const int sb_bits = AT3P_QU_TO_SB[31] + 1;   /* the writer's count: its tonal part is formed in the pass with 32 units */
    for (int ch = 0; ch < channels; ++ch) {
        uint16_t w = 0;
        if (lrd(b, 1)) {
            if (lrd(b, 1) == 0) {
                w = 0xffff;
            } else {
                for (int i = 0; i < sb_bits; ++i) w |= (uint16_t)(lrd(b, 1) << i);
            }
        }
        LCHK();
        f->win[ch] = w;
    }
    for (int ch = 0; ch < channels; ++ch) {
        const uint32_t g = lrd(b, 1);
        LCHK();
        if (g) return R_UNSUPPORTED;   /* gain compensation */
    }
    {
        const uint32_t tonal = lrd(b, 1);
        LCHK();
        if (tonal) {
            if (!r) return R_TONAL;
            const int why = lparse_tonal(b, channels, r);
            if (why) return why;
        }
        const uint32_t noise = lrd(b, 1);
        LCHK();
        if (noise) return R_UNSUPPORTED;
        const uint32_t term = lrd(b, 2);
        LCHK();
        if (term != 3) return R_NO_TERMINATOR;
    }
    for (int ch = 0; ch < channels; ++ch) win[ch] = (uint16_t)f->win[ch];
    return R_OK;
}
#undef LMUST
#undef LCHK

/* steps 1-2 of one frame of frame_bytes bytes; a rejected frame gives a zero spectrum, sine windows and no record */
static int r_unpack(const uint8_t* frame, int frame_bytes, int C, float* spec, uint16_t* win, trec* cur, int tones, at3pd_fields* f, int sparse)
{
    const int why = lparse_frame(frame, 8 * frame_bytes, C, spec, win, tones ? cur : NULL, f, sparse);
    if (!tones) memset(cur, 0, sizeof(*cur));
    f->reason = why;
    if (why) {
        memset(cur, 0, sizeof(*cur));
        memset(spec, 0, sizeof(float) * 2048 * C);
        for (int ch = 0; ch < C; ++ch) win[ch] = 0;
    }
    return why;
}

/* for the tests: specs [C][2048], win [C], fields (at3pd_fields, optional); returns the reason */
int at3ps_unpack_frame(const uint8_t* frame, int frame_bytes, int C, float* specs, uint16_t* win, int tones, int sparse, void* fields_out)
{
    init_tables();
    trec cur;
    at3pd_fields f;
    const int why = r_unpack(frame, frame_bytes, C, specs, win, &cur, tones, &f, sparse);
    if (fields_out) memcpy(fields_out, &f, sizeof(f));
    return why;
}

size_t at3ps_state_bytes(void) { return sizeof(at3pt_stream); }
void at3ps_reset(void* state) { at3pt_reset(state); }

/* frames [n][frame_bytes] -> pcm [n][2048][C] float32, with tonal blocks (tones = 1) or as the decoder without the flag;
 * rejected [6] accumulates */
void at3ps_decode(void* state, int C, const uint8_t* frames, int frame_bytes, int n_frames, float* pcm, uint64_t* rejected, int tones, int sparse)
{
    at3pt_stream* st = (at3pt_stream*)state;
    init_tables();
    init_tone_tables();
    for (int fr = 0; fr < n_frames; ++fr) {
        float spec[2][2048];
        uint16_t win[2] = {0, 0};
        trec cur;
        at3pd_fields f;
        const int why = r_unpack(frames + (size_t)fr * frame_bytes, frame_bytes, C, &spec[0][0], win, &cur, tones, &f, sparse);
        if (why) rejected[why - 1]++;
        for (int ch = 0; ch < C; ++ch) {
            float sub[2048], out[2048];
            midct(&st->base.ch[ch], spec[ch], win[ch], sub);
            for (int i = 0; i < 2048; ++i) sub[i] = sub[i] * kRescale;
            if (tones && (cur.present || st->prev.present))
                for (int sb = 0; sb < 16; ++sb)
                    if (cur.band[ch][sb].nw || st->prev.band[ch][sb].nw) generate_tones(&st->prev, &cur, ch, sb, sub + sb * 128, 0);
            ipqf(&st->base.ch[ch], sub, out);
            for (int i = 0; i < 2048; ++i) {
                float v = out[i];
                v = v > 1.0f ? 1.0f : v;
                v = v < -1.0f ? -1.0f : v;
                pcm[((size_t)fr * 2048 + i) * C + ch] = v;
            }
        }
        st->prev = cur;
    }
}
