/* TEST INFRASTRUCTURE ONLY - CPU restatement of the ATRAC3plus adaptive writer (include/at3phip.h: ADAPTIVE WORD LENGTHS, steps A1-A6,
 * FRAME SIZE, SPARSE WORD LENGTHS), the frame size and the sparse steps as arguments, and the decoder restatement's entry points with
 * the same two arguments. Plain C, scalar. Everything about the adaptive writer is pinned to this file; tests/golden/
 * at3p_writer_fold.npz, at3p_alloc.npz and at3p_sparse.npz pin this file.
 *   encoder  the scaler and the quantiser of the fixed writer (oracle/at3p_frame_oracle.c restates them from the reference), the cost
 *            table, the candidate allocations (A3, with sparse A3s), their bit counts (A4, A4s), the two full scans and the frame in
 *            the fixed writer's layout (A6, A6s). The frame's tail (window shapes, gain-compensation bits, tonal flag and block,
 *            noise flag, terminator) is handed in as a bit string: tests/at3p_writer_lib.py forms it with the restated tonal-block
 *            writer of tests/at3p_tonal_lib.py;
 *   decoder  at3p_decode_cpu.c's frame loop, included here through at3p_tonal_cpu.c.
 * Compiled by the tests, as the last include of at3p_rd_cpu.c, with gcc -O2 -fPIC -ffp-contract=off -fno-fast-math. */
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
static int scale_block(const float* in, int len, float* values)
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
static int qu_spectra(const int* q, int n, int idx, wbits* b)
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

/* As oracle/at3p_frame_oracle.c quantises. For a scaled value that is not finite (NaN or infinite spectra: the scaler's output
 * for them) lrintf's result is unspecified by C and (int) of it implementation-defined: on x86-64 with glibc lrintf gives
 * LONG_MIN and the conversion keeps its low 32 bits, 0, which is what the kernel's v_cvt_i32_f32 gives for NaN. The non-finite
 * cases of the GPU and harness tests hold the two to one another on the hosts the suite runs on. */
static void quantise(const float* values, int n, int wl, int* mant)
{
    const float mul = AT3P_INV_MANT[wl];
    for (int i = 0; i < n; ++i) mant[i] = (int)lrintf(values[i] * mul);
}

/* A1 + A2 for one frame (they do not depend on the frame size) */
int at3pw_cost_table(const float* specs, int channels, uint8_t* sfi, uint16_t* bits, uint8_t* tab, float* values_out)
{
    if (channels < 1 || channels > 2) return -1;
    float values[2048];
    int mant[128];
    for (int ch = 0; ch < channels; ++ch) {
        for (int qu = 0; qu < 32; ++qu) {
            const int start = kQuStart[qu], n = kSpecsPerBlock[qu];
            sfi[ch * 32 + qu] = (uint8_t)scale_block(specs + ch * 2048 + start, n, values + start);
            bits[(ch * 32 + qu) * 8] = 0;
            tab[(ch * 32 + qu) * 8] = 0;
            for (int w = 1; w <= 7; ++w) {
                quantise(values + start, n, w, mant);
                long best = -1;
                int bi = 0;
                for (int i = 0; i < 8; ++i) {
                    wbits cnt = {NULL, 0, 0};
                    const int t = qu_spectra(mant, n, w - 1 + 7 * i, &cnt);
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

static int want(int sfi, int t)
{
    const int d = sfi - t;
    if (d <= 0) return 0;
    return d / 3 > 7 ? 7 : d / 3;
}

/* A3: the candidate allocation A(t, k); returns N, and in *took how many units took the t - 1 value */
static int candidate_dense(const uint8_t* sfi, int channels, int t, int k, uint8_t wl[2][32], int* took)
{
    int N = 1;
    memset(wl, 0, 64);
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu) {
            wl[ch][qu] = (uint8_t)want(sfi[ch * 32 + qu], t);
            if (wl[ch][qu] >= 1 && qu + 1 > N) N = qu + 1;
        }
    if (N >= 29 && N <= 31) N = 32;
    int taken = 0;
    for (int qu = 0; qu < N; ++qu)
        for (int ch = 0; ch < channels; ++ch) {
            const int up = want(sfi[ch * 32 + qu], t - 1);
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

/* how A3s (and R2) close an allocation over all 32 units: N from the highest non-zero word length, and the two fix-ups */
static int close_sparse(uint8_t wl[2][32], int channels)
{
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

/* A3s: all 32 units are walked, nothing is raised from 0 to 1, N follows the k-raise */
static int candidate_sparse(const uint8_t* sfi, int channels, int t, int k, uint8_t wl[2][32], int* took)
{
    memset(wl, 0, 64);
    int taken = 0;
    for (int qu = 0; qu < 32; ++qu)
        for (int ch = 0; ch < channels; ++ch) {
            const int w0 = want(sfi[ch * 32 + qu], t), up = want(sfi[ch * 32 + qu], t - 1);
            wl[ch][qu] = (uint8_t)w0;
            if (up > w0 && taken < k) {
                wl[ch][qu] = (uint8_t)up;
                ++taken;
            }
        }
    if (took) *took = taken;
    return close_sparse(wl, channels);
}

static int candidate(const uint8_t* sfi, int channels, int t, int k, uint8_t wl[2][32], int* took, int sparse)
{
    return sparse ? candidate_sparse(sfi, channels, t, k, wl, took) : candidate_dense(sfi, channels, t, k, wl, took);
}

/* TWordLenEncoder: channel 0 in mode 3 (deltas to the previous unit), channel 1 in mode 1 (deltas to channel 0) */
static int best_wl_table(const int8_t* delta, int sz, int maxDelta)
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
static void wordlen_section(wbits* b, const uint8_t* wl0, const uint8_t* wl1, int N, int channels)
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
        const int idx = best_wl_table(d0, N, max0);
        wput(b, 3, 2);
        wput(b, 0, 2);
        wput(b, 0, 2);
        wput(b, (uint32_t)idx, 2);
        wput(b, (uint32_t)d0[0], 3);
        for (int i = 1; i < N; ++i) wput_vlc(b, AT3P_WL_VLC[idx][d0[i]]);
    }
    if (channels == 2) {
        const int idx = best_wl_table(dx, N, maxx);
        wput(b, 1, 2);
        wput(b, 0, 2);
        wput(b, (uint32_t)idx, 2);
        for (int i = 0; i < N; ++i) wput_vlc(b, AT3P_WL_VLC[idx][dx[i]]);
    }
}

/* the code-table section's bits: 1, then per channel 4 and, A4: 3 per unit below N; A4s: 3 per unit below N with a non-zero word
 * length and, in channel 1, 1 per unit with word length 0 whose channel-0 word length is not 0 (the "copy from channel 0" flag) */
static int codetab_bits(uint8_t wl[2][32], int N, int channels, int sparse)
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
static int alloc_bits(const uint16_t* bits, int channels, int tail_bits, uint8_t wl[2][32], int N, int sparse)
{
    wbits b = {NULL, 0, 0};
    wordlen_section(&b, wl[0], wl[1], N, channels);
    long total = 5 + 1 + b.pos + channels * (2 + 6 * N) + codetab_bits(wl, N, channels, sparse) + channels * 4 * AT3P_SB_POWGRPS[AT3P_QU_TO_SB[N - 1]] +
                 tail_bits;
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < N; ++qu)
            if (wl[ch][qu]) total += bits[(ch * 32 + qu) * 8 + wl[ch][qu]];   /* (entry 0 is not read) */
    return total > 0x7fffffff ? 0x7fffffff : (int)total;
}

/* A3-A5 on a cost table against the budget 8 * frame_bytes - 3: wl_out [channels][32] (0 at and above N), N, t*, k*; returns
 * Bits(A(t*, k*)). Where no t fits (a caller's table only), t* = 63 and k* = 0. */
int at3pw_allocate(const uint8_t* sfi, const uint16_t* bits, int channels, int tail_bits, int frame_bytes, int sparse, uint8_t* wl_out,
                   int32_t* n_units, int32_t* t_out, int32_t* k_out)
{
    const int size_bits = 8 * frame_bytes - 3;
    uint8_t wl[2][32];
    int ts = T_MAX, ks = 0;
    for (int t = T_MIN; t <= T_MAX; ++t) {
        const int N = candidate(sfi, channels, t, 0, wl, NULL, sparse);
        if (alloc_bits(bits, channels, tail_bits, wl, N, sparse) <= size_bits) {
            ts = t;
            break;
        }
    }
    for (int k = 0; k <= K_MAX; ++k) {
        const int N = candidate(sfi, channels, ts, k, wl, NULL, sparse);
        if (alloc_bits(bits, channels, tail_bits, wl, N, sparse) <= size_bits) ks = k;
    }
    const int N = candidate(sfi, channels, ts, ks, wl, &ks, sparse);   /* k* as reported: the units that took the t - 1 value */
    memcpy(wl_out, wl, (size_t)channels * 32);
    *n_units = N;
    *t_out = ts;
    *k_out = ks;
    return alloc_bits(bits, channels, tail_bits, wl, N, sparse);
}

/* what a frame was written with: the end of both per-frame records */
typedef struct { uint8_t wl[2][32], sfi[2][32], tab[2][32]; } frame_alloc;

typedef struct {
    int32_t t, k, num_quant_units, bits;   /* bits: Bits(A(t*, k*)), without the three leading bits */
    frame_alloc used;
} at3pw_frame_info;

/* A6 / A6s: one frame of frame_bytes bytes for a given allocation: wl (0 at and above N, and for a channel not coded), the scale
 * factor indices, the cost table's code-table choices tab [ch][qu][w] and A1's scaled values; tail: tail_bits bits, most
 * significant first */
static void emit_frame(uint8_t* out, int frame_bytes, int channels, int sparse, uint8_t sfi[2][32], uint8_t tab[2][32][8], uint8_t wl[2][32], int N,
                       float values[2][2048], const uint8_t* tail, int tail_bits, frame_alloc* used)
{
    int mant[128];
    memset(out, 0, (size_t)frame_bytes);
    wbits b = {out, 0, 8 * frame_bytes};
    wput(&b, 0, 1);
    wput(&b, (uint32_t)channels - 1, 2);
    wput(&b, (uint32_t)N - 1, 5);
    wput(&b, 0, 1);
    wordlen_section(&b, wl[0], wl[1], N, channels);
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
            quantise(values[ch] + kQuStart[qu], kSpecsPerBlock[qu], wl[ch][qu], mant);
            qu_spectra(mant, kSpecsPerBlock[qu], wl[ch][qu] - 1 + 7 * tab[ch][qu][wl[ch][qu]], &b);
        }
        const int numPwrSpec = AT3P_SB_POWGRPS[AT3P_QU_TO_SB[N - 1]];
        for (int i = 0; i < numPwrSpec; ++i) wput(&b, 15, 4);
    }
    for (int i = 0; i < tail_bits; ++i) wput(&b, (tail[i >> 3] >> (7 - (i & 7))) & 1u, 1);
    if (used) {
        memcpy(used->wl, wl, sizeof(used->wl));
        memcpy(used->sfi, sfi, sizeof(used->sfi));
        for (int ch = 0; ch < 2; ++ch)
            for (int qu = 0; qu < 32; ++qu) used->tab[ch][qu] = qu < N && ch < channels && wl[ch][qu] ? tab[ch][qu][wl[ch][qu]] : 0;
    }
}

/* A1-A6 of one frame: the allocation A(t*, k*), then the frame */
static void write_frame(const float* specs, int channels, int frame_bytes, int sparse, const uint8_t* tail, int tail_bits, uint8_t* out,
                        at3pw_frame_info* info)
{
    uint8_t sfi[2][32], tab[2][32][8], wl[2][32];
    uint16_t bits[2][32][8];
    float values[2][2048];
    memset(sfi, 0, sizeof(sfi));
    memset(tab, 0, sizeof(tab));
    memset(bits, 0, sizeof(bits));
    at3pw_cost_table(specs, channels, &sfi[0][0], &bits[0][0][0], &tab[0][0][0], &values[0][0]);
    int32_t N, t, k;
    const int total = at3pw_allocate(&sfi[0][0], &bits[0][0][0], channels, tail_bits, frame_bytes, sparse, &wl[0][0], &N, &t, &k);
    if (channels == 1) memset(wl[1], 0, 32);
    emit_frame(out, frame_bytes, channels, sparse, sfi, tab, wl, N, values, tail, tail_bits, info ? &info->used : NULL);
    if (info) {
        info->t = t;
        info->k = k;
        info->num_quant_units = N;
        info->bits = total;
    }
}

/* specs [n_frames][channels][2048], tails [n_frames][TAIL_BYTES], tail_bits [n_frames] -> out [n_frames][frame_bytes]; info optional */
int at3pw_write_frames(const float* specs, int channels, int n_frames, int frame_bytes, int sparse, const uint8_t* tails, const int32_t* tail_bits,
                       uint8_t* out, void* info)
{
    if (channels < 1 || channels > 2 || frame_bytes < 8 || frame_bytes > MAX_FRAME_SZ || frame_bytes % 8) return -1;
    for (int f = 0; f < n_frames; ++f) {
        if (tail_bits[f] < 0 || tail_bits[f] > TAIL_BYTES * 8) return -1;
        write_frame(specs + (size_t)f * channels * 2048, channels, frame_bytes, sparse, tails + (size_t)f * TAIL_BYTES, tail_bits[f],
                      out + (size_t)f * frame_bytes, info ? (at3pw_frame_info*)info + f : NULL);
    }
    return n_frames;
}
int at3pw_frame_info_size(void) { return (int)sizeof(at3pw_frame_info); }
int at3pw_tail_bytes(void) { return TAIL_BYTES; }

/* ================================================================ decoder ================================================= */
/* steps 1-2 of one frame of frame_bytes bytes: specs [C][2048], win [C], fields (at3pd_fields, optional); returns the reason */
int at3pw_unpack_frame(const uint8_t* frame, int frame_bytes, int C, float* specs, uint16_t* win, int tones, int sparse, void* fields_out)
{
    trec cur;
    at3pd_fields f;
    const int why = unpack(frame, frame_bytes, C, specs, win, tones ? &cur : NULL, &f, sparse);
    if (fields_out) memcpy(fields_out, &f, sizeof(f));
    return why;
}

size_t at3pw_state_bytes(void) { return sizeof(at3pt_stream); }
void at3pw_reset(void* state) { at3pt_reset(state); }

/* frames [n][frame_bytes] -> pcm [n][2048][C] float32, with tonal blocks (tones = 1) or as the decoder without the flag;
 * rejected [6] accumulates */
void at3pw_decode(void* state, int C, const uint8_t* frames, int frame_bytes, int n_frames, float* pcm, uint64_t* rejected, int tones, int sparse)
{
    at3pt_stream* st = (at3pt_stream*)state;
    decode_frames(&st->base, &st->prev, C, frames, frame_bytes, n_frames, pcm, rejected, NULL, tones, sparse);
}

