// ATRAC3 decode kernels (gfx950): the decoder defined in include/at3hip.h (decoder section) for a batch of streams, every frame
// of a call in parallel.
//
// What a frame needs of its past. Output frame n is the synthesis of its four subbands, and a subband sample of frame n is
// TGainProcessor::Demodulate(gains n-1, gains n) over the first IMDCT half of frame n and the second half of frame n-1. The
// synthesis bank's histories reach back into frame n-1's subband samples [221, 256) only (46 merged samples of each TQmf<512>,
// and the TQmf<1024>'s 46 merged samples are 12 output pairs of frame n-1's TQmf<512> stages over those). Those samples in turn
// need frame n-2's IMDCT tail and gains. So nothing is scanned:
//   k_at3d_unpack   one wavefront per (frame, stream-unit): bit unpack (one lane), dequantisation, the four bands' IMDCT-512
//                   (kissfft order, fft_lds) and the 2 x DecodeWindow window; writes the windowed IMDCT and the gain points
//   k_at3d_synth    one workgroup per (frame, stream): demodulation of frame n and of frame n-1's tail, the inverse
//                   matrixing of joint stereo, the three TQmf stages per channel with frame n-1's histories rebuilt, clamp,
//                   f32 or s16 output
//   k_at3d_state    the call's last two frames become frames -2 and -1 of the next call
// Every float operation is the definition's, in its order, without contraction; no scratch.
// Shared with the other decoders: the bit reader and sign extension (at3_bits.hpp: MsbReader, sext), the TMIDCT rotations and
// unfold and the clamped output store (at3_common.hpp: midct_pre, midct_post, midct_unfold, store_pcm).
#pragma once
#include "at3_bits.hpp"
#include "at3_common.hpp"

namespace at3 {

// Constant tables of the decoder, built on the host (at3hip.hip) with the reference's libm expressions; the VLC look-up is
// expanded from the encoder's c_huff by k_at3d_vlc_lut.
struct Dec3Tables {
    float qmf_win[48];      // QmfWindow
    float scale[64];        // ScaleTable
    float dwin2[256];       // 2 * DecodeWindow (atrac3.h)
    float gain_level[16];   // GainLevel
    float gain_interp[32];  // GainInterpolation (31 used)
    float inv_maxq[8];      // (float)(1.0 / MaxQuant[wl]), wl = 1..7
    float cs512[256];       // TMIDCT<512>(): CalcSinCos(512, 256)
    cpx tw128[128];         // kissfft forward twiddles of the 128-point core
    uint16_t vlc[8][256];   // [selector][next 8 bits]: symbol | code length << 8 (selectors 1..7)
};

// Gain points of one unit, as parsed (n[band] = 0 past the unit's QMF band count and for rejected units).
struct Dec3Gains {
    uint8_t n[4];
    uint8_t level[4][8];
    uint8_t loc[4][8];
};
static_assert(sizeof(Dec3Gains) == 68, "Dec3Gains layout");

constexpr int kDec3Reasons = 6;   // at3hip_decoder_counters order
enum { kR3Ok = 0, kR3BadId, kR3UnsupportedJs, kR3ReadPastEnd, kR3TonalPastEnd, kR3BadTonalMode, kR3BadTonalQuant };

// The raw / gains records of a call are frame-major with two leading slots, so that the carried frames -2 and -1 sit at the
// same place whatever the number of frames of the call: record (slot, stream, unit) at (slot * S + s) * 2 + u.
__device__ __forceinline__ size_t dec3_rec(int slot, int s, int u, int S) { return ((size_t)slot * S + s) * 2 + u; }

__device__ static const uint8_t c_huff_size[7] = {9, 5, 7, 9, 15, 31, 63};

__global__ __launch_bounds__(256) void k_at3d_vlc_lut(Dec3Tables* T)
{
    const int v = threadIdx.x;
    T->vlc[0][v] = 0;
    for (int s = 1; s <= 7; ++s) {
        const int off = huff_off(s);
        uint16_t e = 0;
        for (int k = 0; k < c_huff_size[s - 1]; ++k) {
            const int code = c_huff[off + k] & 0xff, len = c_huff[off + k] >> 8;
            if ((v >> (8 - len)) == code) e = (uint16_t)(k | (len << 8));
        }
        T->vlc[s][v] = e;
    }
}

struct Dec3UnpackParams {
    const Dec3Tables* T;
    const uint8_t* frames;        // [S][F][frame_sz]
    int32_t n_frames, n_streams, frame_sz, js;
    float* raw;                   // records of [4][512] floats
    Dec3Gains* gains;             // records
    unsigned long long* rejected; // [6]
};

// One symbol of a selector's code through its 256-entry look-up (Dec3Tables::vlc): the next 8 bits give symbol and length.
__device__ __forceinline__ int dec3_vlc(MsbReader& b, const uint16_t* lut)
{
    if (b.bad) return 0;
    const uint32_t e = lut[b.peek(8)];
    const int len = (int)(e >> 8);
    if (b.pos + len > b.limit) {
        b.bad = 1;
        return 0;
    }
    b.advance(len);
    return (int)(e & 0xff);
}

__device__ __forceinline__ int dec3_mantissa(MsbReader& b, const uint16_t (*lut)[256], bool vlc_mode, int s)
{
    if (!vlc_mode) return sext(b.rd(clc_len(s)), clc_len(s));
    const int i = dec3_vlc(b, lut[s]);
    return (i & 1) ? (i + 1) >> 1 : -(i >> 1);
}

// the unit's syntax (include/at3hip.h, step 1) and its dequantisation (step 2) on one lane: g, base and tonal are zero on
// entry; wls / sfs are work space (LDS, like everything it writes: no scratch)
__device__ __forceinline__ int dec3_parse(MsbReader& b, const uint16_t (*lut)[256], const float* scale, const float* inv_maxq, bool js_second, Dec3Gains& g,
                                          float* base, float* tonal, uint8_t* wls, uint8_t* sfs)
{
#define DEC3_CHK()                              \
    do {                                        \
        if (b.bad) return kR3ReadPastEnd;       \
    } while (0)
    if (js_second) {
        const uint32_t w = b.rd(1), d = b.rd(3);
        bool ok = w == 0 && d == 7;
        for (int i = 0; i < 4; ++i) ok = (b.rd(2) == 3) && ok;
        DEC3_CHK();
        if (!ok) return kR3UnsupportedJs;
        const uint32_t id = b.rd(2);
        DEC3_CHK();
        if (id != 3) return kR3BadId;
    } else {
        const uint32_t id = b.rd(6);
        DEC3_CHK();
        if (id != 0x28) return kR3BadId;
    }
    const int nqmf = (int)b.rd(2) + 1;
    for (int band = 0; band < nqmf; ++band) {
        const int n = (int)b.rd(3);
        g.n[band] = (uint8_t)n;
        for (int i = 0; i < n; ++i) {
            g.level[band][i] = (uint8_t)b.rd(4);
            g.loc[band][i] = (uint8_t)b.rd(5);
        }
    }
    DEC3_CHK();
    const int ngroups = (int)b.rd(5);
    DEC3_CHK();
    if (ngroups) {
        const int mode = (int)b.rd(2);
        DEC3_CHK();
        if (mode > 1) return kR3BadTonalMode;
        for (int grp = 0; grp < ngroups; ++grp) {
            int flags = 0;
            for (int band = 0; band < nqmf; ++band) flags |= (int)b.rd(1) << band;
            const int cv = (int)b.rd(3) + 1;
            const int q = (int)b.rd(3);
            DEC3_CHK();
            if (q < 2) return kR3BadTonalQuant;
            const float mq = inv_maxq[q];
            for (int j = 0; j < 4 * nqmf; ++j) {
                if (!((flags >> (j >> 2)) & 1)) continue;
                const int cnt = (int)b.rd(3);
                for (int c = 0; c < cnt; ++c) {
                    const int sf = (int)b.rd(6);
                    const int pos = j * 64 + (int)b.rd(6);
                    DEC3_CHK();
                    if (pos + cv > 1024) return kR3TonalPastEnd;
                    const float sc = scale[sf];
                    for (int z = 0; z < cv; ++z) {
                        const int m = dec3_mantissa(b, lut, mode == 0, q);
                        tonal[pos + z] += (float)m * sc * mq;
                    }
                    DEC3_CHK();
                }
            }
        }
    }
    const int nbfu = (int)b.rd(5) + 1;
    const bool vlc_mode = b.rd(1) == 0;
    for (int i = 0; i < nbfu; ++i) wls[i] = (uint8_t)b.rd(3);
    for (int i = 0; i < nbfu; ++i) sfs[i] = wls[i] ? (uint8_t)b.rd(6) : 0;
    DEC3_CHK();
    for (int i = 0; i < nbfu; ++i) {
        const int wl = wls[i];
        if (!wl) continue;
        const float sc = scale[sfs[i]], mq = inv_maxq[wl];
        const int k1 = bfu_start(i + 1);
        if (wl == 1) {
            for (int k = bfu_start(i); k < k1; k += 2) {
                int a, c;
                if (!vlc_mode) {
                    const uint32_t code = b.rd(4);
                    a = sext(code >> 2, 2);
                    c = sext(code & 3, 2);
                } else {
                    // inverse of MantissasToVlcIndex: symbols 0..8 -> (a, b)
                    const int sym = dec3_vlc(b, lut[1]);
                    a = sym == 3 || sym == 5 || sym == 6 ? 1 : sym == 4 || sym == 7 || sym == 8 ? -1 : 0;
                    c = sym == 1 || sym == 5 || sym == 7 ? 1 : sym == 2 || sym == 6 || sym == 8 ? -1 : 0;
                }
                base[k] = (float)a * sc * mq;
                base[k + 1] = (float)c * sc * mq;
            }
        } else {
            for (int k = bfu_start(i); k < k1; ++k) base[k] = (float)dec3_mantissa(b, lut, vlc_mode, wl) * sc * mq;
        }
        DEC3_CHK();
    }
#undef DEC3_CHK
    return kR3Ok;
}

constexpr int kDec3UnpackThreads = 64;   // one wavefront per unit: the parse is one lane, so units in flight per CU count

__global__ __launch_bounds__(kDec3UnpackThreads) void k_at3d_unpack(Dec3UnpackParams p)
{
    constexpr int NT = kDec3UnpackThreads;
    __shared__ uint32_t s_w[260];                       // the unit, big-endian words, zero past its bytes (and past word 257)
    __shared__ uint16_t s_lut[8][256];
    __shared__ float s_base[1024];                      // dequantised lines, then the spectrum (+ tonal)
    __shared__ __attribute__((aligned(16))) float s_tonal[1024];   // tonal sums, then the four 128-point FFTs
    __shared__ Dec3Gains s_g;
    __shared__ uint8_t s_wl[32], s_sf[32];
    __shared__ int s_reason;
    cpx* s_f = (cpx*)s_tonal;

    const Dec3Tables* T = p.T;
    const int f = blockIdx.x, su = blockIdx.y, tid = threadIdx.x;
    const int s = su >> 1, u = su & 1;
    const int fsz = p.frame_sz;
    const int limit = p.js ? fsz : fsz >> 1;   // bytes the unit may read
    const uint8_t* frame = p.frames + ((size_t)s * p.n_frames + f) * fsz;
    for (int i = tid; i < 260; i += NT) {
        uint32_t w = 0;
        for (int k = 0; k < 4; ++k) {
            const int j = 4 * i + k;
            uint32_t byte = 0;
            if (j < limit) byte = !p.js ? frame[u * limit + j] : u ? frame[fsz - 1 - j] : frame[j];
            w = (w << 8) | byte;
        }
        s_w[i] = w;
    }
    for (int i = tid; i < 8 * 256; i += NT) (&s_lut[0][0])[i] = (&T->vlc[0][0])[i];
    for (int i = tid; i < 1024; i += NT) {
        s_base[i] = 0.0f;
        s_tonal[i] = 0.0f;
    }
    for (int i = tid; i < (int)sizeof(Dec3Gains); i += NT) ((uint8_t*)&s_g)[i] = 0;
    __syncthreads();
    if (tid == 0) {
        MsbReader b(s_w, limit * 8);
        const int why = dec3_parse(b, s_lut, T->scale, T->inv_maxq, p.js && u == 1, s_g, s_base, s_tonal, s_wl, s_sf);
        s_reason = why;
        if (why) atomicAdd(&p.rejected[why - 1], 1ull);
    }
    __syncthreads();
    const bool rejected = s_reason != kR3Ok;
    for (int i = tid; i < (int)sizeof(Dec3Gains); i += NT) {   // a rejected unit has no gain points
        const uint8_t v = rejected ? 0 : ((const uint8_t*)&s_g)[i];
        ((uint8_t*)(p.gains + dec3_rec(f + 2, s, u, p.n_streams)))[i] = v;
    }
    for (int i = tid; i < 1024; i += NT) s_base[i] = rejected ? 0.0f : s_base[i] + s_tonal[i];
    __syncthreads();
    // TMIDCT<512> pre-rotation of the four bands (odd bands: SwapArray folded into the index), into the FFT's leaf order
    const float* cs = T->cs512;
    for (int j = tid; j < 512; j += NT) {
        const int band = j >> 7, k2 = j & 127, n = 2 * k2;
        const int a = band & 1 ? 255 - n : n, bb = band & 1 ? n : 255 - n;
        const float r0 = s_base[256 * band + a];
        const float i0 = s_base[256 * band + bb];
        s_f[band * 128 + fft_leaf_pos<128>(k2)] = midct_pre(r0, i0, cs[n], cs[n + 1]);
    }
    __syncthreads();
    fft_lds<128, false>(s_f, 128, 4, T->tw128, tid, NT);
    // post-rotation (mdct.h) and the window: inv[j] *= 2 DecodeWindow[j], inv[511 - j] *= 2 DecodeWindow[j]
    float* raw = p.raw + dec3_rec(f + 2, s, u, p.n_streams) * 2048;
    const float* W = T->dwin2;
    for (int j = tid; j < 512; j += NT) {
        const int band = j >> 7, k2 = j & 127, n = 2 * k2;
        float r1, i1;
        midct_post(s_f[j], cs[n], cs[n + 1], r1, i1);
        float* o = raw + band * 512;
        midct_unfold<128>(n, r1, i1, [&](int x, float v) { o[x] = v * W[x < 256 ? x : 511 - x]; });
    }
}

}  // namespace at3

namespace at3 {

struct Dec3SynthParams {
    const Dec3Tables* T;
    const float* raw;
    const Dec3Gains* gains;
    void* out;                    // [S][F][1024][2] float or int16
    int32_t n_frames, n_streams, js, s16;
};

// TGainProcessor::Demodulate(now, next) at position p of a band: the reference's loop, with the position's level found by
// walking the gain points (the ramp's level is multiplied up in the reference's order)
__device__ __forceinline__ float dec3_demod(const Dec3Tables* T, const Dec3Gains& now, const Dec3Gains& next, int band, float cur,
                                            float prev, int p)
{
    const float scale = next.n[band] ? T->gain_level[next.level[band][0]] : 1.0f;
    const float v = cur * scale + prev;
    const int nn = now.n[band];
    int pos = 0;
    for (int i = 0; i < nn; ++i) {
        const int last = now.loc[band][i] << 3;
        float level = T->gain_level[now.level[band][i]];
        if (p >= pos && p < last) return v * level;
        pos = pos > last ? pos : last;
        const int end = last + 8;
        if (p >= pos && p < end) {
            const float inc = T->gain_interp[(i + 1 < nn ? now.level[band][i + 1] : 4) - now.level[band][i] + 15];
            for (int k = pos; k < p; ++k) level *= inc;
            return v * level;
        }
        pos = pos > end ? pos : end;
    }
    return v;
}

// one output pair of TQmf::Synthesis over the merge window w
__device__ __forceinline__ void dec3_qmf_pair(const float* w, const float* QW, float& o0, float& o1)
{
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int i = 0; i < 48; i += 2) {
        s1 += w[i] * QW[i];
        s2 += w[i + 1] * QW[i + 1];
    }
    o0 = s2;
    o1 = s1;
}

constexpr int kDec3Hist = 35;   // frame n-1's subband samples [221, 256)

__global__ __launch_bounds__(256) void k_at3d_synth(Dec3SynthParams p)
{
    __shared__ float s_sub[2][4][256];           // frame n's subbands: per unit, then (after the matrixing) per channel
    __shared__ float s_psub[2][4][kDec3Hist];    // frame n-1's subband samples [221, 256)
    __shared__ float s_m1[2][2][512 + 46];       // [channel][stage] merge buffers of the two TQmf<512>
    __shared__ float s_pm[2][2][70];             // frame n-1's merged samples newPart[442, 512) of the two TQmf<512>
    __shared__ float s_m2[2][1024 + 46];         // [channel] merge buffer of the TQmf<1024>
    __shared__ Dec3Gains s_g[3][2];              // frames n-2, n-1, n

    const Dec3Tables* T = p.T;
    const int f = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int S = p.n_streams;
    for (int i = tid; i < 6 * (int)sizeof(Dec3Gains); i += 256) {
        const int r = i / (int)sizeof(Dec3Gains), o = i % (int)sizeof(Dec3Gains);
        ((uint8_t*)&s_g[r >> 1][r & 1])[o] = ((const uint8_t*)(p.gains + dec3_rec(f + (r >> 1), s, r & 1, S)))[o];
    }
    __syncthreads();
    for (int i = tid; i < 2048; i += 256) {
        const int u = i >> 10, band = (i >> 8) & 3, q = i & 255;
        const float cur = p.raw[dec3_rec(f + 2, s, u, S) * 2048 + band * 512 + q];
        const float prev = p.raw[dec3_rec(f + 1, s, u, S) * 2048 + band * 512 + 256 + q];
        s_sub[u][band][q] = dec3_demod(T, s_g[1][u], s_g[2][u], band, cur, prev, q);
    }
    for (int i = tid; i < 8 * kDec3Hist; i += 256) {
        const int u = i / (4 * kDec3Hist), band = (i / kDec3Hist) & 3, q = i % kDec3Hist;
        const float cur = p.raw[dec3_rec(f + 1, s, u, S) * 2048 + band * 512 + 221 + q];
        const float prev = p.raw[dec3_rec(f, s, u, S) * 2048 + band * 512 + 256 + 221 + q];
        s_psub[u][band][q] = dec3_demod(T, s_g[0][u], s_g[1][u], band, cur, prev, 221 + q);
    }
    __syncthreads();
    if (p.js) {   // inverse of TAtrac3Encoder::Matrixing: L = M + S, R = M - S
        for (int i = tid; i < 1024; i += 256) {
            const float m = (&s_sub[0][0][0])[i], d = (&s_sub[1][0][0])[i];
            (&s_sub[0][0][0])[i] = m + d;
            (&s_sub[1][0][0])[i] = m - d;
        }
        for (int i = tid; i < 4 * kDec3Hist; i += 256) {
            const float m = (&s_psub[0][0][0])[i], d = (&s_psub[1][0][0])[i];
            (&s_psub[0][0][0])[i] = m + d;
            (&s_psub[1][0][0])[i] = m - d;
        }
        __syncthreads();
    }
    // TQmf<512>::Synthesis(buf1, sub0, sub1) and (buf2, sub3, sub2): merged samples; the history is frame n-1's newPart[466, 512)
    for (int i = tid; i < 1024; i += 256) {
        const int c = i >> 9, st = (i >> 8) & 1, q = i & 255;
        const float lo = s_sub[c][st ? 3 : 0][q], up = s_sub[c][st ? 2 : 1][q];
        s_m1[c][st][46 + 2 * q] = lo + up;
        s_m1[c][st][47 + 2 * q] = lo - up;
    }
    for (int i = tid; i < 4 * kDec3Hist; i += 256) {
        const int c = i / (2 * kDec3Hist), st = (i / kDec3Hist) & 1, k = i % kDec3Hist, q = 221 + k;
        const float lo = s_psub[c][st ? 3 : 0][k], up = s_psub[c][st ? 2 : 1][k];
        const float a = lo + up, b = lo - up;
        s_pm[c][st][2 * k] = a;
        s_pm[c][st][2 * k + 1] = b;
        if (q >= 233) {
            s_m1[c][st][2 * q - 466] = a;
            s_m1[c][st][2 * q - 465] = b;
        }
    }
    __syncthreads();
    // the two TQmf<512> stages' output pairs, merged for the TQmf<1024>; frame n-1's pairs 244 .. 255 give its history
    const float* QW = T->qmf_win;
    for (int i = tid; i < 512 + 24; i += 256) {
        if (i < 512) {
            const int c = i >> 8, j = i & 255;
            float a0, a1, b0, b1;
            dec3_qmf_pair(&s_m1[c][0][2 * j], QW, a0, a1);
            dec3_qmf_pair(&s_m1[c][1][2 * j], QW, b0, b1);
            s_m2[c][46 + 4 * j] = a0 + b0;
            s_m2[c][47 + 4 * j] = a0 - b0;
            s_m2[c][48 + 4 * j] = a1 + b1;
            s_m2[c][49 + 4 * j] = a1 - b1;
        } else {
            const int c = (i - 512) / 12, j = 244 + (i - 512) % 12;
            float a0, a1, b0, b1;
            dec3_qmf_pair(&s_pm[c][0][2 * (j - 244)], QW, a0, a1);
            dec3_qmf_pair(&s_pm[c][1][2 * (j - 244)], QW, b0, b1);
            if (2 * j >= 489) {
                s_m2[c][4 * j - 978] = a0 + b0;
                s_m2[c][4 * j - 977] = a0 - b0;
            }
            s_m2[c][4 * j + 2 - 978] = a1 + b1;
            s_m2[c][4 * j + 3 - 978] = a1 - b1;
        }
    }
    __syncthreads();
    // TQmf<1024>::Synthesis output pairs, clamp, interleave
    const size_t F = p.n_frames;
    for (int i = tid; i < 1024; i += 256) {
        const int c = i >> 9, j = i & 511;
        float o0, o1;
        dec3_qmf_pair(&s_m2[c][2 * j], QW, o0, o1);
        const size_t base = (((size_t)s * F + f) * 1024 + 2 * j) * 2 + c;
        auto pair = [&](bool s16) {
            store_pcm(p.out, base, o0, s16);
            store_pcm(p.out, base + 2, o1, s16);
        };
        if (p.s16) pair(true);   // one branch for the pair: two in a row cost this loop 17 VGPRs and a wave of occupancy
        else pair(false);
    }
}

// The call's last two frames (slots F, F + 1) become slots 0 and 1 of the next call.
__global__ __launch_bounds__(256) void k_at3d_state(float* raw, Dec3Gains* gains, int32_t n_frames, int32_t n_streams)
{
    __shared__ float s_raw[2][2048];
    __shared__ Dec3Gains s_g[2];
    const int su = blockIdx.x, s = su >> 1, u = su & 1, tid = threadIdx.x;
    for (int i = tid; i < 4096; i += 256) s_raw[i >> 11][i & 2047] = raw[dec3_rec(n_frames + (i >> 11), s, u, n_streams) * 2048 + (i & 2047)];
    if (tid < 2 * (int)sizeof(Dec3Gains)) {
        const int r = tid / (int)sizeof(Dec3Gains), o = tid % (int)sizeof(Dec3Gains);
        ((uint8_t*)&s_g[r])[o] = ((const uint8_t*)(gains + dec3_rec(n_frames + r, s, u, n_streams)))[o];
    }
    __syncthreads();
    for (int i = tid; i < 4096; i += 256) raw[dec3_rec(i >> 11, s, u, n_streams) * 2048 + (i & 2047)] = s_raw[i >> 11][i & 2047];
    if (tid < 2 * (int)sizeof(Dec3Gains)) {
        const int r = tid / (int)sizeof(Dec3Gains), o = tid % (int)sizeof(Dec3Gains);
        ((uint8_t*)(gains + dec3_rec(r, s, u, n_streams)))[o] = ((const uint8_t*)&s_g[r])[o];
    }
}

}  // namespace at3
