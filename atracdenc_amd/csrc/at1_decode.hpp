// ATRAC1 decode kernels (gfx950): the body of the lambda of TAtrac1Decoder::GetLambda (atrac1denc.cpp:139-177) for a
// batch of streams, every frame of a call in parallel.
//
// What a frame needs of its past. Frame n's PCM is the synthesis of its three band signals (TAtrac1MDCT::IMdct output)
// with the filter bank's histories. In the reference's layout the band buffer of frame n holds
//   [0, 32)         block 0 windowed against the 16-sample tail that frame n-1's IMDCT left
//   [32, 64)        always this frame's own IMDCT (every block-size mode writes it)
//   [64, bufSz)     this frame's own IMDCT - EXCEPT under the two- and four-block modes that a valid unit can select
//                   (LogCount 1 for the low / middle band, 1 or 2 for the high band): they write only the first 64 / 128
//                   samples and the rest of the buffer keeps what the last frame that wrote it left there.
// The histories of the synthesis (46 merged samples per TQmf stage, the high band's 39-sample delay line) reach back only
// into frame n-1's band samples [93, 128) (low, middle) and [194, 256) (high), which are frame n-1's band buffer as above.
// So three passes:
//   k_at1d_bands   one workgroup per (stream-channel, frame): bit unpack, dequantisation, block-switched IMDCT; writes the
//                  samples this frame writes, block 0's IMDCT half for the window and the 16-sample tails, and its mode
//   k_at1d_scan    one workgroup per stream-channel: for every frame and every partly-written range the index of the last
//                  frame (this call) that wrote it - a max-scan over the frames
//   k_at1d_synth   one workgroup per (stream-channel, frame): resolves frames n and n-1's band buffers from those, windows
//                  block 0, rebuilds frame n-1's part of the histories and runs the two QMF stages, clamps, writes PCM
//   k_at1d_state   carries the last frame's band buffer [64, bufSz) and tails into the next call
// Every float operation is the reference's, in its order, without contraction; no scratch.
// Shared with the other decoders: the sign extension (at3_bits.hpp: sext), the TMIDCT rotations and the clamped output store
// (at3_common.hpp: midct_pre, midct_post, store_pcm). The unit is read at computed positions by 128 lanes at once (dec_bits),
// not in sequence, so the sequential MsbReader has no place here; of Buf[N] only the middle half is kept, so neither has
// midct_unfold.
#pragma once
#include "at1_kernels.hpp"
#include "at3_bits.hpp"

namespace at1 {

// Constant tables of the decoder, built on the host (at1hip.hip) with the container's libm and uploaded.
struct DecTables {
    float qmf_win[48];     // QmfWindow (qmf.cpp:36-45)
    float sine[32];        // SineWindow
    float scale[64];       // ScaleTable
    float maxq[17];        // 1.0 / (float)((1 << (wl - 1)) - 1), atrac1_dequantiser.cpp:55 (index = word length)
    float cs512[256];      // TMIDCT<512>(1024): CalcSinCos(512, 512 / 512 -> scale 1)
    float cs256[128];      // TMIDCT<256>(512)
    float cs64[32];        // TMIDCT<64>(128)
    cpx tw128[128];        // kissfft forward twiddles of the N/4-point cores
    cpx tw64[64];
    cpx tw16[16];
};

constexpr int kDecTailLen = 48;   // 3 bands x 16
constexpr int kDecScanThreads = 256;

struct DecBandsParams {
    const DecTables* T;
    const uint8_t* units;          // [S][F][C][212]
    int32_t n_frames, nch;
    float* raw;                    // [S*C][F][512]: low [0,128), mid [128,256), high [256,512)
    float* tails;                  // [S*C][F][48]
    int32_t* modes;                // [S*C][F]: LogCount low | mid << 2 | high << 4
    unsigned long long* rejected;  // [2]: block-size mode, read past the end
};

// partly written ranges: 0 low [64,128), 1 mid [64,128), 2 high [64,128), 3 high [128,256)
__device__ __forceinline__ int dec_writes(int mode)
{
    const int l0 = mode & 3, l1 = (mode >> 2) & 3, l2 = (mode >> 4) & 3;
    return (l0 != 1 ? 1 : 0) | (l1 != 1 ? 2 : 0) | (l2 != 1 ? 4 : 0) | ((l2 == 0 || l2 == 3) ? 8 : 0);
}
__device__ __forceinline__ int dec_range(int x)   // range of a position >= 64 of the 512-float band record
{
    return x < 128 ? 0 : x < 256 ? 1 : x < 384 ? 2 : 3;
}

// TBitStream::Read (bitstream.cpp:69-95) of n <= 16 bits at bit p from the unit staged in LDS (zero padded past byte 211)
__device__ __forceinline__ uint32_t dec_bits(const uint8_t* u, int p, int n)
{
    const int b = p >> 3;
    const uint32_t w = ((uint32_t)u[b] << 24) | ((uint32_t)u[b + 1] << 16) | ((uint32_t)u[b + 2] << 8) | (uint32_t)u[b + 3];
    return (w << (p & 7)) >> (32 - n);
}

template <int N4>
__device__ __forceinline__ void dec_fft(cpx* F, int nfft, const cpx* tw, int tid)
{
    at3::fft_lds<N4, false>(F, N4, nfft, tw, tid, 128);
}

__global__ __launch_bounds__(128) void k_at1d_bands(DecBandsParams p)
{
    __shared__ uint8_t s_unit[224];
    __shared__ float s_spec[512];
    __shared__ __attribute__((aligned(16))) cpx s_f[256];   // FFT points: low [0,64), mid [64,128), high [128,256)
    __shared__ float s_inv[512];                            // invBuf of the three bands: low [0,128), mid [128,256), high [256,512)
    __shared__ int s_wl[kMaxBfus], s_sf[kMaxBfus], s_off[kMaxBfus];
    __shared__ int s_lc[3], s_bad, s_nbfu;

    const DecTables* T = p.T;
    const int f = blockIdx.x, sc = blockIdx.y, tid = threadIdx.x;
    const int s = sc / p.nch, c = sc % p.nch;
    const uint8_t* unit = p.units + (((size_t)s * p.n_frames + f) * p.nch + c) * kFrame;
    for (int i = tid; i < 224; i += 128) s_unit[i] = i < kFrame ? unit[i] : 0;
    for (int i = tid; i < 512; i += 128) {
        s_spec[i] = 0.0f;
        s_inv[i] = 0.0f;
    }
    __syncthreads();
    // TBlockSizeMod::Parse (atrac1.cpp:37-53) and the fixed-position fields of TAtrac1Dequantiser::Dequant
    const int nbfu = bfu_amount(dec_bits(s_unit, 8, 3));
    if (tid < kMaxBfus) {
        const bool have = tid < nbfu;
        s_wl[tid] = have ? (int)dec_bits(s_unit, 16 + 4 * tid, 4) : 0;
        s_sf[tid] = have ? (int)dec_bits(s_unit, 16 + 4 * nbfu + 6 * tid, 6) : 0;
    }
    __syncthreads();
    if (tid == 0) {
        const uint32_t h = s_unit[0];
        const int lc0 = 2 - (int)(h >> 6), lc1 = 2 - (int)((h >> 4) & 3), lc2 = 3 - (int)((h >> 2) & 3);
        int bad = (lc0 < 0 || lc1 < 0) ? 1 : 0;
        // mantissas follow the scale factors BFU after BFU; a read that ends past bit 1696 throws (bitstream.cpp:73-74)
        int off = 16 + 10 * nbfu;
        for (int b = 0; b < kMaxBfus; ++b) {
            s_off[b] = off;
            const int w = s_wl[b] ? s_wl[b] + 1 : 0;
            off += w * c_spb[b];
        }
        if (!bad && off > kFrame * 8) bad = 2;
        s_bad = bad;
        s_nbfu = nbfu;
        s_lc[0] = bad ? 0 : lc0;
        s_lc[1] = bad ? 0 : lc1;
        s_lc[2] = bad ? 0 : lc2;
        if (bad) atomicAdd(&p.rejected[bad - 1], 1ull);
        p.modes[(size_t)sc * p.n_frames + f] = bad ? 0 : (lc0 | lc1 << 2 | lc2 << 4);
    }
    __syncthreads();
    const int lc[3] = {s_lc[0], s_lc[1], s_lc[2]};
    if (!s_bad) {
        // TAtrac1Dequantiser::Dequant: position t of the BFU-ordered line list
        for (int t = tid; t < 512; t += 128) {
            const int b = c_bfu_of_pos[t];
            const int w = s_wl[b] ? s_wl[b] + 1 : 0;
            if (b < s_nbfu && w) {
                const int i = t - c_start_long[b];
                const uint32_t v = dec_bits(s_unit, s_off[b] + i * w, w);
                const int m = at3::sext(v, w);   // MakeSign
                const float sfq = T->scale[s_sf[b]] * T->maxq[w];
                const int lcb = b < 20 ? lc[0] : b < 36 ? lc[1] : lc[2];
                s_spec[(lcb ? c_start_short[b] : c_start_long[b]) + i] = sfq * (float)m;
            }
        }
    }
    __syncthreads();
    // TAtrac1MDCT::IMdct (atrac1denc.cpp:103-137): TMIDCT pre-rotation (mdct.h:124-137) of every block, straight into the FFT's
    // leaf order; the mirrored bands' SwapArray is folded into the read index. Specs are consumed from `pos` on, which does
    // not restart per band: a two-block low band (64 lines) leaves the middle band starting at line 64.
    int pos[3];
    pos[0] = 0;
    pos[1] = lc[0] ? (32 << lc[0]) : 128;
    pos[2] = pos[1] + (lc[1] ? (32 << lc[1]) : 128);
#pragma unroll
    for (int band = 0; band < 3; ++band) {
        const int nblk = 1 << lc[band];
        const int bsz = nblk == 1 ? (band == 2 ? 256 : 128) : 32;   // blockSz = N / 2 coefficients in, N / 4 FFT points
        const int n4 = bsz >> 1;
        const float* cs = nblk != 1 ? T->cs64 : band == 2 ? T->cs512 : T->cs256;
        cpx* F = s_f + (band == 0 ? 0 : band == 1 ? 64 : 128);
        for (int j = tid; j < nblk * n4; j += 128) {
            const int k = j / n4, k2 = j % n4, n = 2 * k2;
            const float* in = s_spec + pos[band] + k * bsz;
            const float r0 = band ? in[bsz - 1 - n] : in[n];
            const float i0 = band ? in[n] : in[bsz - 1 - n];
            const cpx v = at3::midct_pre(r0, i0, cs[n], cs[n + 1]);
            const int leaf = n4 == 128 ? at3::fft_leaf_pos<128>(k2) : n4 == 64 ? at3::fft_leaf_pos<64>(k2) : at3::fft_leaf_pos<16>(k2);
            F[k * n4 + leaf] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int band = 0; band < 3; ++band) {
        cpx* F = s_f + (band == 0 ? 0 : band == 1 ? 64 : 128);
        const int nblk = 1 << lc[band];
        if (nblk != 1) dec_fft<16>(F, nblk, T->tw16, tid);
        else if (band == 2) dec_fft<128>(F, 1, T->tw128, tid);
        else dec_fft<64>(F, 1, T->tw64, tid);
    }
    // post-rotation (mdct.h:143-178): of Buf[N] only [N/4, 3N/4) reaches invBuf (inv[i + N/4]); there it is
    // invBuf[n2 - 1 - n] = r1 and invBuf[n] = i1 for every even n < n2
#pragma unroll
    for (int band = 0; band < 3; ++band) {
        const int nblk = 1 << lc[band];
        const int bsz = nblk == 1 ? (band == 2 ? 256 : 128) : 32;
        const int n4 = bsz >> 1;
        const float* cs = nblk != 1 ? T->cs64 : band == 2 ? T->cs512 : T->cs256;
        const cpx* F = s_f + (band == 0 ? 0 : band == 1 ? 64 : 128);
        float* inv = s_inv + (band == 0 ? 0 : band == 1 ? 128 : 256);
        for (int j = tid; j < nblk * n4; j += 128) {
            const int k = j / n4, k2 = j % n4, n = 2 * k2;
            float r1, i1;
            at3::midct_post(F[j], cs[n], cs[n + 1], r1, i1);
            inv[k * bsz + bsz - 1 - n] = r1;
            inv[k * bsz + n] = i1;
        }
    }
    __syncthreads();
    // what this frame writes of its band buffers: block 0's IMDCT half (windowed in k_at1d_synth against frame n-1's tail),
    // the long block's copy (atrac1denc.cpp:132-133) or blocks 1.. windowed against their predecessors (vector_fmul_window,
    // atrac1denc.cpp:51-68); and the 16-sample tail for frame n+1
    float* raw = p.raw + ((size_t)sc * p.n_frames + f) * 512;
    const float* W = T->sine;
    for (int x = tid; x < 512; x += 128) {
        const int band = x < 128 ? 0 : x < 256 ? 1 : 2;
        const int o = band == 0 ? 0 : band == 1 ? 128 : 256;
        const int i = x - o;
        const float* inv = s_inv + o;
        const int nblk = 1 << lc[band];
        if (i < 16) {
            raw[x] = inv[i];
        } else if (i >= 32) {
            if (nblk == 1) {
                raw[x] = inv[i - 16];
            } else if (i < 32 * nblk) {
                const int k = i >> 5, a = i & 31;
                const float* prev = inv + 32 * (k - 1) + 16;
                const float* cur = inv + 32 * k;
                raw[x] = a < 16 ? prev[a] * W[31 - a] - cur[15 - a] * W[a] : prev[31 - a] * W[31 - a] + cur[a - 16] * W[a];
            }
        }
    }
    if (tid < kDecTailLen) {
        const int band = tid >> 4;
        const int bufsz = band == 2 ? 256 : 128;
        p.tails[((size_t)sc * p.n_frames + f) * kDecTailLen + tid] = s_inv[(band == 0 ? 0 : band == 1 ? 128 : 256) + bufsz - 16 + (tid & 15)];
    }
}

// For every frame and partly written range: the last frame <= it (this call) that wrote the range, -1 = none (the carried
// state's buffer holds it). A max-scan over the frames: contiguous chunks per thread, then a scan over the threads.
__global__ __launch_bounds__(kDecScanThreads) void k_at1d_scan(const int32_t* modes, int4* lw, int32_t n_frames)
{
    __shared__ int4 s_carry[kDecScanThreads];
    const int sc = blockIdx.x, tid = threadIdx.x;
    const int chunk = (n_frames + kDecScanThreads - 1) / kDecScanThreads;
    const int f0 = tid * chunk, f1 = f0 + chunk < n_frames ? f0 + chunk : n_frames;
    const int32_t* m = modes + (size_t)sc * n_frames;
    int4 last = make_int4(-1, -1, -1, -1);
    for (int f = f0; f < f1; ++f) {
        const int w = dec_writes(m[f]);
        if (w & 1) last.x = f;
        if (w & 2) last.y = f;
        if (w & 4) last.z = f;
        if (w & 8) last.w = f;
    }
    s_carry[tid] = last;
    __syncthreads();
    for (int d = 1; d < kDecScanThreads; d <<= 1) {
        const int4 a = tid >= d ? s_carry[tid - d] : make_int4(-1, -1, -1, -1);
        __syncthreads();
        int4 b = s_carry[tid];
        b.x = a.x > b.x ? a.x : b.x;
        b.y = a.y > b.y ? a.y : b.y;
        b.z = a.z > b.z ? a.z : b.z;
        b.w = a.w > b.w ? a.w : b.w;
        s_carry[tid] = b;
        __syncthreads();
    }
    int4 run = tid ? s_carry[tid - 1] : make_int4(-1, -1, -1, -1);
    int4* out = lw + (size_t)sc * n_frames;
    for (int f = f0; f < f1; ++f) {
        const int w = dec_writes(m[f]);
        if (w & 1) run.x = f;
        if (w & 2) run.y = f;
        if (w & 4) run.z = f;
        if (w & 8) run.w = f;
        out[f] = run;
    }
}

struct DecSynthParams {
    const DecTables* T;
    const float* raw;        // [S*C][F][512]
    const float* tails;      // [S*C][F][48]
    const int4* lw;          // [S*C][F]
    const float* st_band;    // [S*C][512] the previous call's last frame, positions >= 64 of each band
    const float* st_tail;    // [S*C][48]
    void* out;               // [S][F][512][C] float or int16
    int32_t n_frames, nch, s16;
};

__device__ __forceinline__ int lw_get(int4 v, int r) { return r == 0 ? v.x : r == 1 ? v.y : r == 2 ? v.z : v.w; }

__global__ __launch_bounds__(256) void k_at1d_synth(DecSynthParams p)
{
    __shared__ float s_cur[512];    // frame n's band buffers: low [0,128), mid [128,256), high [256,512)
    __shared__ float s_prev[512];   // frame n-1's, positions >= 64 of each band
    __shared__ float s_m2[256 + 46];
    __shared__ float s_pnew[70];    // frame n-1's merged low / mid samples 186 .. 255 (TQmf<256>::PcmBufferMerge[232, 302))
    __shared__ float s_midlow[256];
    __shared__ float s_pmidlow[24]; // frame n-1's MidLowTmp[232, 256)
    __shared__ float s_m1[512 + 46];

    const DecTables* T = p.T;
    const int f = blockIdx.x, sc = blockIdx.y, tid = threadIdx.x;
    const size_t F = p.n_frames;
    const float* raw_sc = p.raw + (size_t)sc * F * 512;
    const int4 lw_n = p.lw[(size_t)sc * F + f];
    const int4 lw_p = f ? p.lw[(size_t)sc * F + f - 1] : make_int4(-1, -1, -1, -1);
    const float* tail_p = f ? p.tails + ((size_t)sc * F + f - 1) * kDecTailLen : p.st_tail + (size_t)sc * kDecTailLen;
    const float* st = p.st_band + (size_t)sc * 512;
    const float* W = T->sine;
    for (int x = tid; x < 512; x += 256) {
        const int o = x < 128 ? 0 : x < 256 ? 128 : 256;
        const int i = x - o;
        float v;
        if (i < 32) {
            // block 0: vector_fmul_window(dst, prevBuf = frame n-1's tail, &invBuf[0], SineWindow, 16)
            const float* head = raw_sc + (size_t)f * 512 + o;
            const float* tail = tail_p + (o == 0 ? 0 : o == 128 ? 16 : 32);
            v = i < 16 ? tail[i] * W[31 - i] - head[15 - i] * W[i] : tail[31 - i] * W[31 - i] + head[i - 16] * W[i];
        } else if (i < 64) {
            v = raw_sc[(size_t)f * 512 + x];
        } else {
            const int r = dec_range(x);
            const int m = lw_get(lw_n, r);
            v = m >= 0 ? raw_sc[(size_t)m * 512 + x] : st[x];
            const int mp = lw_get(lw_p, r);
            s_prev[x] = mp >= 0 ? raw_sc[(size_t)mp * 512 + x] : st[x];
        }
        s_cur[x] = v;
    }
    __syncthreads();
    // TQmf<256>::Synthesis (qmf.h:66-89) of Atrac1SynthesisFilterBank (atrac1_qmf.h:58-63): merged low +- mid
    {
        const float* lo = s_cur;
        const float* mi = s_cur + 128;
        for (int q = tid; q < 128; q += 256) {
            s_m2[46 + 2 * q] = lo[q] + mi[q];
            s_m2[47 + 2 * q] = lo[q] - mi[q];
        }
        if (tid >= 128 && tid < 128 + 35) {   // frame n-1's merged samples of lines 93 .. 127
            const int q = 93 + (tid - 128);
            const float a = s_prev[q] + s_prev[128 + q], b = s_prev[q] - s_prev[128 + q];
            s_pnew[2 * q - 186] = a;
            s_pnew[2 * q - 185] = b;
            if (q >= 105) {   // the history: PcmBufferMerge[0, 46) = frame n-1's newPart[210, 256)
                s_m2[2 * q - 210] = a;
                s_m2[2 * q - 209] = b;
            }
        }
    }
    __syncthreads();
    const float* QW = T->qmf_win;
    if (tid < 128) {
        const float* w = s_m2 + 2 * tid;
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int i = 0; i < 48; i += 2) {
            s1 += w[i] * QW[i];
            s2 += w[i + 1] * QW[i + 1];
        }
        s_midlow[2 * tid] = s2;
        s_midlow[2 * tid + 1] = s1;
    } else if (tid < 140) {
        // frame n-1's MidLowTmp[232, 256): output pairs 116 .. 127, windows over its merge buffer [232, 302) = newPart[186, 256)
        const int j = tid - 128;
        const float* w = s_pnew + 2 * j;
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int i = 0; i < 48; i += 2) {
            s1 += w[i] * QW[i];
            s2 += w[i + 1] * QW[i + 1];
        }
        s_pmidlow[2 * j] = s2;
        s_pmidlow[2 * j + 1] = s1;
    }
    __syncthreads();
    // TQmf<512>::Synthesis of MidLowTmp and the delay line (DelayBuf[q] = high[q - 39], frame n-1's high band before q = 39)
    {
        const float* hi = s_cur + 256;
        const float* phi = s_prev + 256;
        const int q = tid;
        const float lo = s_midlow[q];
        const float up = q < 39 ? phi[217 + q] : hi[q - 39];
        s_m1[46 + 2 * q] = lo + up;
        s_m1[47 + 2 * q] = lo - up;
        if (q >= 233) {   // the history: frame n-1's newPart[466, 512)
            const float plo = s_pmidlow[q - 232];
            const float pup = phi[q - 39];
            s_m1[2 * q - 466] = plo + pup;
            s_m1[2 * q - 465] = plo - pup;
        }
    }
    __syncthreads();
    {
        const float* w = s_m1 + 2 * tid;
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int i = 0; i < 48; i += 2) {
            s1 += w[i] * QW[i];
            s2 += w[i + 1] * QW[i + 1];
        }
        // clamp to [PcmValueMin, PcmValueMax] and interleave (atrac1denc.cpp:166-173)
        const int s = sc / p.nch, c = sc % p.nch;
        const size_t base = (((size_t)s * F + f) * 512 + 2 * tid) * p.nch + c;
        auto pair = [&](bool s16) {
            at3::store_pcm(p.out, base, s2, s16);
            at3::store_pcm(p.out, base + p.nch, s1, s16);
        };
        if (p.s16) pair(true);   // one branch for the pair, as in k_at3d_synth
        else pair(false);
    }
}

// The last frame's band buffer (positions >= 64 of each band) and tails become the carried state.
__global__ __launch_bounds__(256) void k_at1d_state(const float* raw, const float* tails, const int4* lw, float* st_band, float* st_tail,
                                                    int32_t n_frames)
{
    const int sc = blockIdx.x, tid = threadIdx.x;
    const size_t F = n_frames;
    const int4 l = lw[(size_t)sc * F + F - 1];
    for (int x = tid; x < 512; x += 256) {
        const int o = x < 128 ? 0 : x < 256 ? 128 : 256;
        if (x - o < 64) continue;
        const int m = lw_get(l, dec_range(x));
        if (m >= 0) st_band[(size_t)sc * 512 + x] = raw[((size_t)sc * F + m) * 512 + x];
    }
    if (tid < kDecTailLen) st_tail[(size_t)sc * kDecTailLen + tid] = tails[((size_t)sc * F + F - 1) * kDecTailLen + tid];
}

}  // namespace at1
