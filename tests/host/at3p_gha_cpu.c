/* TEST INFRASTRUCTURE ONLY - a C restatement of the ATRAC3plus tone analysis defined in include/at3phip.h (FINDING TONES, steps
 * 1-8): one stream, frame after frame. The residual of step 8 is at3pt_apply_filter's generate_tones (at3p_tonal_cpu.c, included
 * here) fed with the records this file finds. The same analysis is written out in atracdenc_amd/csrc/at3p_gha.hpp (the kernels)
 * and in TAt3PToneAnalyser (atracdenc_amd/host/at3hip_host.hpp): the three change together. Compiled by the tests with gcc -O2 -fPIC -ffp-contract=off -fno-fast-math. */
#include "at3p_tonal_cpu.c"
#include "../../include/at3phip.h"

typedef struct { float r, i; } gcpx;

static struct {
    gcpx tw[256];
    double thr[64];
    double rs[1024], rc[1024];
    int init;
} GT;

static void init_gha_tables(void)
{
    init_tone_tables();
    if (GT.init) return;
    const double pi = 3.141592653589793238462643383279502884197169399375105820974944;   /* kiss_fft.c:357-363 */
    for (int i = 0; i < 256; ++i) {
        const double ph = -2 * pi * i / 256;
        GT.tw[i].r = (float)cos(ph);
        GT.tw[i].i = (float)sin(ph);
    }
    for (int i = 0; i < 64; ++i) {
        const double a = (double)TT.amp_sf[i] * exp2(-0.125);
        GT.thr[i] = a * a;
    }
    for (int f = 0; f < 1024; ++f) {   /* the projections' normalisers: sums over t = 0..255 in order */
        double ns = 0, nc = 0;
        for (int t = 0; t < 256; ++t) {
            const int pos = ((t - 128) * f) & 2047;
            const double sn = (double)TT.sine[pos], cs = (double)TT.sine[(pos + 512) & 2047];
            ns = ns + (double)TT.hann[t] * (sn * sn);
            nc = nc + (double)TT.hann[t] * (cs * cs);
        }
        GT.rs[f] = ns > 0 ? 1.0 / ns : 0.0;
        GT.rc[f] = nc > 0 ? 1.0 / nc : 0.0;
    }
    GT.init = 1;
}

/* ---- the kissfft-order FFT (kiss_fft.c:21-90, 238-302), forward, n = 4^k ---- */
static gcpx gmul(gcpx a, gcpx b)
{
    gcpx m;
    m.r = a.r * b.r - a.i * b.i;
    m.i = a.r * b.i + a.i * b.r;
    return m;
}

static void gfft(gcpx* out, const gcpx* in, int n, int fstride)
{
    const int m = n / 4;
    if (m == 1) {
        for (int q = 0; q < 4; ++q) out[q] = in[q * fstride];
    } else {
        for (int q = 0; q < 4; ++q) gfft(out + q * m, in + q * fstride, m, fstride * 4);
    }
    for (int k = 0; k < m; ++k) {   /* kf_bfly4 */
        const gcpx s0 = gmul(out[m + k], GT.tw[k * fstride]);
        const gcpx s1 = gmul(out[2 * m + k], GT.tw[2 * k * fstride]);
        const gcpx s2 = gmul(out[3 * m + k], GT.tw[3 * k * fstride]);
        gcpx s5, s3, s4;
        s5.r = out[k].r - s1.r; s5.i = out[k].i - s1.i;
        out[k].r += s1.r; out[k].i += s1.i;
        s3.r = s0.r + s2.r; s3.i = s0.i + s2.i;
        s4.r = s0.r - s2.r; s4.i = s0.i - s2.i;
        out[2 * m + k].r = out[k].r - s3.r; out[2 * m + k].i = out[k].i - s3.i;
        out[k].r += s3.r; out[k].i += s3.i;
        out[m + k].r = s5.r + s4.i; out[m + k].i = s5.i - s4.r;
        out[3 * m + k].r = s5.r - s4.i; out[3 * m + k].i = s5.i + s4.r;
    }
}

typedef struct { int valid, ch, sb, freq, amp_sf, phase; double a2; } gwave;

/* steps 1-5 for one subband: x = 256 samples; at most AT3PHIP_TONE_MAX_BAND_WAVES waves, by descending coarse power */
static int find_band(const float* x, gwave* out)
{
    float y[256], P[129];
    gcpx in[256], F[256];
    for (int t = 0; t < 256; ++t) {
        y[t] = x[t] * TT.hann[t];
        in[t].r = y[t];
        in[t].i = 0.0f;
    }
    gfft(F, in, 256, 1);
    for (int k = 0; k <= 128; ++k) P[k] = F[k].r * F[k].r + F[k].i * F[k].i;
    float sum = 0.0f;
    for (int k = 1; k <= 127; ++k) sum = sum + P[k];
    const double floor_p = (double)AT3PHIP_TONE_PEAK_RATIO * ((double)sum / 127.0);
    int ck[AT3PHIP_TONE_MAX_BAND_WAVES], nc = 0;
    for (int k = 0; k <= 128; ++k) {   /* the spectrum of a real signal is even about bins 0 and 128: P[-1] = P[1], P[129] = P[127] */
        const float left = P[k == 0 ? 1 : k - 1], right = P[k == 128 ? 127 : k + 1];
        if (!(P[k] > left && P[k] >= right && (double)P[k] >= floor_p)) continue;
        int at = nc;   /* sorted by descending power; an equal power stays behind the lower k */
        while (at > 0 && P[k] > P[ck[at - 1]]) --at;
        if (at >= AT3PHIP_TONE_MAX_BAND_WAVES) continue;
        const int last = nc < AT3PHIP_TONE_MAX_BAND_WAVES ? nc : AT3PHIP_TONE_MAX_BAND_WAVES - 1;
        for (int j = last; j > at; --j) ck[j] = ck[j - 1];
        ck[at] = k;
        if (nc < AT3PHIP_TONE_MAX_BAND_WAVES) ++nc;
    }
    int n = 0;
    for (int c = 0; c < nc; ++c) {
        const int lo = 8 * ck[c] - AT3PHIP_TONE_FINE_SPAN < 1 ? 1 : 8 * ck[c] - AT3PHIP_TONE_FINE_SPAN;
        const int hi = 8 * ck[c] + AT3PHIP_TONE_FINE_SPAN > 1023 ? 1023 : 8 * ck[c] + AT3PHIP_TONE_FINE_SPAN;
        int bf = -1;
        double bs = 0, bc = 0, bp = 0;
        for (int f = lo; f <= hi; ++f) {
            double S = 0, C = 0;
            for (int t = 0; t < 256; ++t) {
                const int pos = ((t - 128) * f) & 2047;
                S = S + (double)y[t] * (double)TT.sine[pos];
                C = C + (double)y[t] * (double)TT.sine[(pos + 512) & 2047];
            }
            const double pw = (S * S) * GT.rs[f] + (C * C) * GT.rc[f];
            if (bf < 0 || pw > bp) { bf = f; bs = S; bc = C; bp = pw; }
        }
        if (bf < 0) continue;
        const double ca = bs * GT.rs[bf], cb = bc * GT.rc[bf];   /* x[t] = ca sin + cb cos, by least squares under the window */
        const double a2 = ca * ca + cb * cb;
        if (!(a2 >= (double)AT3PHIP_TONE_MIN_AMP * (double)AT3PHIP_TONE_MIN_AMP)) continue;
        int sf = 0;
        for (int i = 0; i < 64; ++i)
            if (a2 >= GT.thr[i]) sf = i;
        int ph = 0;
        double bv = 0;
        for (int p = 0; p < 32; ++p) {
            const double v = ca * (double)TT.sine[(64 * p + 512) & 2047] + cb * (double)TT.sine[64 * p];
            if (p == 0 || v > bv) { ph = p; bv = v; }
        }
        out[n].valid = 1; out[n].freq = bf; out[n].amp_sf = sf; out[n].phase = ph; out[n].a2 = a2;
        ++n;
    }
    return n;
}

/* steps 6-7: w[nw] waves of one frame -> the record */
static int wave_before(const gwave* a, const gwave* b)   /* the record's order: channel, band, frequency index */
{
    if (a->ch != b->ch) return a->ch < b->ch;
    if (a->sb != b->sb) return a->sb < b->sb;
    return a->freq < b->freq;
}

static void select_waves(gwave* w, int nw, at3phip_tonal_block* blk)
{
    memset(blk, 0, sizeof(*blk));
    for (int i = 0; i < nw; ++i) {
        int rank = 0;
        for (int j = 0; j < nw; ++j)
            if (j != i && (w[j].a2 > w[i].a2 || (w[j].a2 == w[i].a2 && wave_before(&w[j], &w[i])))) ++rank;
        w[i].valid = rank < AT3PHIP_TONAL_MAX_WAVES;
    }
    for (int i = 0; i < nw; ++i) {
        if (!w[i].valid) continue;
        int at = 0;
        for (int j = 0; j < nw; ++j)
            if (w[j].valid && wave_before(&w[j], &w[i])) ++at;
        blk->wave[at] = AT3PHIP_TONAL_WAVE(w[i].freq, w[i].amp_sf, w[i].phase);
        blk->band[w[i].ch][w[i].sb].n_waves++;
        if (w[i].sb + 1 > blk->num_tone_bands) blk->num_tone_bands = (uint8_t)(w[i].sb + 1);
    }
}

static void block_to_trec(const at3phip_tonal_block* b, trec* r)
{
    memset(r, 0, sizeof(*r));
    r->present = b->num_tone_bands != 0;
    int at = 0;
    for (int ch = 0; ch < 2; ++ch)
        for (int sb = 0; sb < 16; ++sb) {
            tband* t = &r->band[ch][sb];
            t->nw = b->band[ch][sb].n_waves;
            t->start_index = at;
            t->pend.start = -1;
            t->pend.stop = 32;
            for (int i = 0; i < t->nw; ++i, ++at) {
                r->freq[at] = (int)(b->wave[at] & 1023u);
                r->amp_sf[at] = (int)((b->wave[at] >> 10) & 63u);
                r->phase[at] = (int)((b->wave[at] >> 16) & 31u);
            }
        }
}

typedef struct {
    float x[2][2048];            /* the last frame's subband samples */
    at3phip_tonal_block last;    /* the last block */
    trec filt;                   /* at3pt_apply_filter's state: the last block as generate_tones left it */
} at3pg_stream;

size_t at3pg_state_bytes(void) { return sizeof(at3pg_stream); }
void at3pg_reset(void* state)
{
    init_gha_tables();
    memset(state, 0, sizeof(at3pg_stream));
}

/* at3phip_analyse_tones for one stream: bands [n][C][16][128]; blocks [n]: slot f = the block of (frame f - 1, frame f);
 * residual [n][C][16][128]: slot f = the residual of frame f - 1 (frame -1 of the first call: the zero frame) */
void at3pg_analyse(void* state, int C, const float* bands, int n, at3phip_tonal_block* blocks, float* residual)
{
    at3pg_stream* st = (at3pg_stream*)state;
    init_gha_tables();
    for (int f = 0; f < n; ++f) {
        gwave w[2 * 16 * AT3PHIP_TONE_MAX_BAND_WAVES];
        int nw = 0;
        for (int ch = 0; ch < C; ++ch)
            for (int sb = 0; sb < 16; ++sb) {
                float x[256];
                memcpy(x, st->x[ch] + sb * 128, 128 * sizeof(float));
                memcpy(x + 128, bands + (((size_t)f * C + ch) * 16 + sb) * 128, 128 * sizeof(float));
                const int got = find_band(x, w + nw);
                for (int i = 0; i < got; ++i) { w[nw + i].ch = ch; w[nw + i].sb = sb; }
                nw += got;
            }
        select_waves(w, nw, &blocks[f]);
        /* step 8 on the previous frame: this block fading in, the block before fading out */
        trec cur;
        block_to_trec(&blocks[f], &cur);
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

/* the last block of the stream (what the frame writer pairs with the next call's first frame) */
void at3pg_last_block(const void* state, at3phip_tonal_block* out) { *out = ((const at3pg_stream*)state)->last; }

/* the table block of at3phip_host_tone_find_tables */
void at3pg_tables(float* sine, float* hann, float* amp_sf, float* tw, double* thr, double* rs, double* rc)
{
    init_gha_tables();
    memcpy(sine, TT.sine, sizeof(TT.sine));
    memcpy(hann, TT.hann, sizeof(TT.hann));
    memcpy(amp_sf, TT.amp_sf, sizeof(TT.amp_sf));
    memcpy(tw, GT.tw, sizeof(GT.tw));
    memcpy(thr, GT.thr, sizeof(GT.thr));
    memcpy(rs, GT.rs, sizeof(GT.rs));
    memcpy(rc, GT.rc, sizeof(GT.rc));
}
