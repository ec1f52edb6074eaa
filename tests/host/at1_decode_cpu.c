/* TEST INFRASTRUCTURE ONLY - a from-scratch C restatement of the reference's ATRAC1 decoder (TAtrac1Decoder,
 * atrac1denc.cpp:139-177), written for three jobs: the bit-exact anchor the GPU decoder (atracdenc_amd/csrc/at1_decode.hpp)
 * is fuzzed against where the reference does not exist, the one-core CPU baseline of tools/at1_decode_bench.py, and an
 * independent check of the goldens in tests/golden/at1_decode.npz. Compiled by the tests with
 * gcc -O2 -fPIC -ffp-contract=off -fno-fast-math (the reference's x86-64 arithmetic: no contraction, no reassociation).
 *
 * Per channel it keeps what the reference keeps: the three band buffers of TAtrac1MDCT::IMdct (with their 16-sample
 * overlap tails), and the two TQmf merge histories plus the high band's 39-sample delay line of
 * Atrac1SynthesisFilterBank. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { float r, i; } cpx;

static const float kTapHalf[24] = {   /* qmf/qmf.cpp:25-32 */
    -0.00001461907f,  -0.00009205479f, -0.000056157569f, 0.00030117269f, 0.0002422519f,  -0.00085293897f,
    -0.0005205574f,   0.0020340169f,   0.00078333891f,   -0.0042153862f, -0.00075614988f, 0.0078402944f,
    -0.000061169922f, -0.01344162f,    0.0024626821f,    0.021736089f,   -0.007801671f,   -0.034090221f,
    0.01880949f,      0.054326009f,    -0.043596379f,    -0.099384367f,  0.13207909f,     0.46424159f};
static const int kSpecsPerBlock[52] = {8,  8,  8,  8,  4,  4,  4,  4,  8,  8,  8,  8,  6,  6,  6,  6,  6,  6,
                                       6,  6,  6,  6,  6,  6,  7,  7,  7,  7,  9,  9,  9,  9,  10, 10, 10, 10,
                                       12, 12, 12, 12, 12, 12, 12, 12, 20, 20, 20, 20, 20, 20, 20, 20};
static const int kBlocksPerBand[4] = {0, 20, 36, 52};
static const int kSpecsStartLong[52] = {0,   8,   16,  24,  32,  36,  40,  44,  48,  56,  64,  72,  80,  86,  92,  98,  104, 110,
                                        116, 122, 128, 134, 140, 146, 152, 159, 166, 173, 180, 189, 198, 207, 216, 226, 236, 246,
                                        256, 268, 280, 292, 304, 316, 328, 340, 352, 372, 392, 412, 432, 452, 472, 492};
static const int kSpecsStartShort[52] = {0,   32,  64,  96,  8,   40,  72,  104, 12,  44,  76,  108, 20,  52,  84,  116, 26,  58,
                                         90,  122, 128, 160, 192, 224, 134, 166, 198, 230, 141, 173, 205, 237, 150, 182, 214, 246,
                                         256, 288, 320, 352, 384, 416, 448, 480, 268, 300, 332, 364, 396, 428, 460, 492};
static const int kBfuAmount[8] = {20, 28, 32, 36, 40, 44, 48, 52};

static struct {
    int ready;
    float qmf_win[48], scale[64], sine[32], maxq[17];
    float cs512[256], cs256[128], cs64[32];   /* TMIDCT<N>(2N) : TMDCTBase(N, N) -> CalcSinCos scale sqrt(N / N) = 1 */
    cpx tw128[128], tw64[64], tw16[16];
} T;

/* CalcSinCos (lib/mdct/mdct.cpp:25-36) with the float overloads; called at run time (never folded at compile time) */
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

__attribute__((noinline, optimize("O0"))) static void twiddles(cpx* tw, int n)   /* kiss_fft_alloc, forward */
{
    const double pi = 3.141592653589793238462643383279502884197169399375105820974944;
    for (int i = 0; i < n; ++i) {
        const double ph = -2 * pi * i / n;
        tw[i].r = (float)cos(ph);
        tw[i].i = (float)sin(ph);
    }
}

__attribute__((noinline, optimize("O0"))) static void init_tables(void)
{
    if (T.ready) return;
    for (int i = 0; i < 24; ++i) T.qmf_win[i] = T.qmf_win[47 - i] = kTapHalf[i] * 2.0;       /* qmf.cpp:41-44 */
    for (uint32_t i = 0; i < 64; ++i) T.scale[i] = pow(2.0, (double)(i / 3.0 - 21.0));     /* atrac1.h:124-128 */
    for (uint32_t i = 0; i < 32; ++i) T.sine[i] = sin((i + 0.5) * (M_PI / (2.0 * 32.0)));  /* atrac1.h:129-133 */
    for (int wl = 2; wl <= 16; ++wl) T.maxq[wl] = 1.0 / (float)((1 << (wl - 1)) - 1);      /* atrac1_dequantiser.cpp:55 */
    calc_sincos(T.cs512, 512, 512.0f);
    calc_sincos(T.cs256, 256, 256.0f);
    calc_sincos(T.cs64, 64, 64.0f);
    twiddles(T.tw128, 128);
    twiddles(T.tw64, 64);
    twiddles(T.tw16, 16);
    T.ready = 1;
}

/* ---- kissfft-order FFT (kiss_fft.c kf_work with factors 4 .. 4 [2]) ---- */
static inline cpx cmul(cpx a, cpx b)
{
    cpx m;
    m.r = a.r * b.r - a.i * b.i;
    m.i = a.r * b.i + a.i * b.r;
    return m;
}
static void fft_combine2(cpx* F, int m, int fstride, const cpx* tw)
{
    for (int k = 0; k < m; ++k) {
        const cpx t = cmul(F[m + k], tw[k * fstride]);
        F[m + k].r = F[k].r - t.r; F[m + k].i = F[k].i - t.i;
        F[k].r += t.r; F[k].i += t.i;
    }
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
    const int p = (n % 4 == 0) ? 4 : 2;
    const int m = n / p;
    if (m == 1) {
        for (int q = 0; q < p; ++q) out[q] = in[q * fstride];
    } else {
        for (int q = 0; q < p; ++q) fft_rec(out + q * m, in + q * fstride, m, fstride * p, tw);
    }
    if (p == 4) fft_combine4(out, m, fstride, tw);
    else fft_combine2(out, m, fstride, tw);
}

/* TMIDCT<N>::operator() (lib/mdct/mdct.h:107-180): N/2 in -> N out */
static void imdct_n(const float* in, float* buf, int N)
{
    const float* cs = N == 512 ? T.cs512 : N == 256 ? T.cs256 : T.cs64;
    const cpx* tw = N == 512 ? T.tw128 : N == 256 ? T.tw64 : T.tw16;
    const int n2 = N >> 1, n4 = N >> 2, n34 = 3 * n4, n54 = 5 * n4;
    cpx fin[128], fout[128];
    int n;
    for (n = 0; n < n2; n += 2) {
        const float r0 = in[n], i0 = in[n2 - 1 - n];
        const float c = cs[n], s = cs[n + 1];
        fin[n / 2].r = -2.0 * (i0 * s + r0 * c);
        fin[n / 2].i = -2.0 * (i0 * c - r0 * s);
    }
    fft_rec(fout, fin, n4, 1, tw);
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

/* vector_fmul_window (atrac1denc.cpp:51-68) with len 16 and the 32-point sine window */
static void fmul_window(float* dst, const float* src0, const float* src1)
{
    const float* win = T.sine + 16;
    dst += 16;
    src0 += 16;
    for (int i = -16, j = 15; i < 0; i++, j--) {
        const float s0 = src0[i], s1 = src1[j], wi = win[i], wj = win[j];
        dst[i] = s0 * wj - s1 * wi;
        dst[j] = s0 * wi + s1 * wj;
    }
}

/* ---- TBitStream::Read (lib/bitstream/bitstream.cpp:69-95) over one 212-byte sound unit ---- */
typedef struct { const uint8_t* buf; int pos; int bad; } bits;
static uint32_t rd(bits* b, int n)
{
    if (b->bad || b->pos + n > 212 * 8) { b->bad = 1; return 0; }
    uint32_t v = 0;
    for (int k = 0; k < n; ++k, ++b->pos) v = (v << 1) | ((b->buf[b->pos >> 3] >> (7 - (b->pos & 7))) & 1u);
    return v;
}

typedef struct at1d_chan {
    float low[256 + 16], mid[256 + 16], hi[512 + 16];     /* TAtrac1Decoder::PcmBufLow / Mid / Hi */
    float merge2[256 + 46], merge1[512 + 46];             /* TQmf<256> / TQmf<512>::PcmBufferMerge */
    float delay[39 + 512], midlow[512];                   /* Atrac1SynthesisFilterBank::DelayBuf / MidLowTmp */
} at1d_chan;

/* reasons a unit is rejected (the two exceptions the lambda catches): 1 = block size mode, 2 = read past the end */
static int parse_unit(const uint8_t* unit, float specs[512], int lc[3])
{
    bits b = {unit, 0, 0};
    lc[0] = 2 - (int)rd(&b, 2);   /* TBlockSizeMod::Parse, atrac/at1/atrac1.cpp:37-53 */
    lc[1] = 2 - (int)rd(&b, 2);
    lc[2] = 3 - (int)rd(&b, 2);
    rd(&b, 2);
    if (lc[0] < 0 || lc[1] < 0 || lc[2] < 0) return 1;
    /* TAtrac1Dequantiser::Dequant (atrac/at1/atrac1_dequantiser.cpp:31-72) */
    uint32_t wl[52], sf[52];
    const int nbfu = kBfuAmount[rd(&b, 3)];
    rd(&b, 2);
    rd(&b, 3);
    for (int i = 0; i < nbfu; ++i) wl[i] = rd(&b, 4);
    for (int i = 0; i < nbfu; ++i) sf[i] = rd(&b, 6);
    for (int i = nbfu; i < 52; ++i) wl[i] = sf[i] = 0;
    for (int band = 0; band < 3; ++band)
        for (int bfu = kBlocksPerBand[band]; bfu < kBlocksPerBand[band + 1]; ++bfu) {
            const int n = kSpecsPerBlock[bfu];
            const uint32_t w = !!wl[bfu] + wl[bfu];
            const float scale = T.scale[sf[bfu]];
            const int start = lc[band] ? kSpecsStartShort[bfu] : kSpecsStartLong[bfu];
            if (w) {
                const float mq = T.maxq[w];
                for (int i = 0; i < n; ++i) {
                    const uint32_t v = rd(&b, (int)w);
                    const int s = (int)(v << (32 - w)) >> (32 - w);   /* MakeSign */
                    specs[start + i] = scale * mq * s;
                }
            } else {
                memset(&specs[start], 0, n * sizeof(float));
            }
        }
    return b.bad ? 2 : 0;
}

/* TAtrac1MDCT::IMdct (atrac1denc.cpp:103-137) */
static void imdct_bands(float* specs, const int lc[3], at1d_chan* c)
{
    int pos = 0;
    for (int band = 0; band < 3; ++band) {
        const int nblk = 1 << lc[band];
        const int bufsz = band == 2 ? 256 : 128;
        const int blksz = nblk == 1 ? bufsz : 32;
        int start = 0;
        float* dst = band == 0 ? c->low : band == 1 ? c->mid : c->hi;
        float inv_buf[512] = {0};
        float inv[512];
        const float* prev = &dst[bufsz * 2 - 16];
        for (int blk = 0; blk < nblk; ++blk) {
            if (band)
                for (int i = 0, j = blksz - 1; i < blksz / 2; ++i, --j) {   /* SwapArray */
                    const float t = specs[pos + i];
                    specs[pos + i] = specs[pos + j];
                    specs[pos + j] = t;
                }
            const int N = 2 * blksz;
            imdct_n(&specs[pos], inv, N);
            for (int i = 0; i < N / 2; ++i) inv_buf[start + i] = inv[i + N / 4];
            fmul_window(dst + start, prev, &inv_buf[start]);
            prev = &inv_buf[start + 16];
            start += blksz;
            pos += blksz;
        }
        if (nblk == 1) memcpy(dst + 32, &inv_buf[16], (band == 2 ? 240 : 112) * sizeof(float));
        for (int j = 0; j < 16; ++j) dst[bufsz * 2 - 16 + j] = inv_buf[bufsz - 16 + j];
    }
}

/* TQmf<nIn>::Synthesis (qmf/qmf.h:66-89) */
static void qmf_synth(float* merge, int nin, float* out, const float* lower, const float* upper)
{
    float* np = &merge[46];
    for (int i = 0; i < nin; i += 4) {
        np[i + 0] = lower[i / 2] + upper[i / 2];
        np[i + 1] = lower[i / 2] - upper[i / 2];
        np[i + 2] = lower[i / 2 + 1] + upper[i / 2 + 1];
        np[i + 3] = lower[i / 2 + 1] - upper[i / 2 + 1];
    }
    const float* w = merge;
    for (int j = nin / 2; j != 0; j--) {
        float s1 = 0, s2 = 0;
        for (int i = 0; i < 48; i += 2) {
            s1 += w[i] * T.qmf_win[i];
            s2 += w[i + 1] * T.qmf_win[i + 1];
        }
        out[0] = s2;
        out[1] = s1;
        w += 2;
        out += 2;
    }
    memmove(&merge[0], &merge[nin], 46 * sizeof(float));
}

/* ---- C API used by the tests and the benchmark ---- */
size_t at1d_state_bytes(void) { return sizeof(at1d_chan); }

void at1d_reset(void* state, int nch)
{
    init_tables();
    memset(state, 0, sizeof(at1d_chan) * (size_t)nch);
}

/* n_frames invocations of the decoder lambda: units [n][nch][212] (TAeaInput::ReadFrame order), pcm [n][512][nch].
 * rejected[0] / [1] count the units rejected for their block size mode / for a read past the end. */
void at1d_decode(void* state, int nch, const uint8_t* units, int n_frames, float* pcm, uint64_t* rejected)
{
    init_tables();
    at1d_chan* chans = (at1d_chan*)state;
    for (int f = 0; f < n_frames; ++f)
        for (int ch = 0; ch < nch; ++ch) {
            at1d_chan* c = &chans[ch];
            float specs[512] = {0}, sum[512];
            int lc[3];
            const int why = parse_unit(units + ((size_t)f * nch + ch) * 212, specs, lc);
            if (why) {
                rejected[why - 1]++;
                memset(specs, 0, sizeof(specs));
                lc[0] = lc[1] = lc[2] = 0;
            }
            imdct_bands(specs, lc, c);
            /* Atrac1SynthesisFilterBank::Synthesis (atrac/at1/atrac1_qmf.h:46-64) */
            memcpy(&c->delay[0], &c->delay[256], 39 * sizeof(float));
            memcpy(&c->delay[39], c->hi, 256 * sizeof(float));
            qmf_synth(c->merge2, 256, c->midlow, c->low, c->mid);
            qmf_synth(c->merge1, 512, sum, c->midlow, c->delay);
            for (int i = 0; i < 512; ++i) {
                float v = sum[i];
                if (v > 1) v = 1;
                if (v < -1) v = -1;
                pcm[((size_t)f * 512 + i) * nch + ch] = v;
            }
        }
}
