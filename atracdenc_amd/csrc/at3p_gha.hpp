// ATRAC3plus tone analysis kernels (gfx950): include/at3phip.h, FINDING TONES, steps 1-8, between k_at3p_pqf and k_at3p_mdct.
//   k_at3p_tone_find    steps 1-5: one wavefront per (stream, frame, channel, subband), four subbands per workgroup
//   k_at3p_tone_select  steps 6-7: one workgroup per (stream, frame) ranks the frame's waves by counting and packs the record
//   k_at3p_tone_sub     step 8: one workgroup per (stream, frame, channel) subtracts this block and the one before
//   k_at3p_tone_state   the carried frame and block, and the writer's first record of the call
// Slot f of a call works on the pair (frame f-1, frame f), frame -1 being the carried one, so every slot of a call runs side by
// side. Every sum runs in the order the header states, in one lane: the restatement (tests/host/at3p_gha_cpu.c) is the same
// loop. Float operations without contraction.
// The analysis is written out three times and the three change together: here, in the C restatement tests/host/at3p_gha_cpu.c
// and in the host mirror's TAt3PToneAnalyser (atracdenc_amd/host/at3hip_host.hpp); the table builder is build_tone_find_tables.
#pragma once
#include "at3p_kernels.hpp"
#include "at3p_write.hpp"

namespace at3p {

// The analysis' tables, built on the host with its libm (build_tone_find_tables, at3phip.hip).
struct ToneFindTables {
    float sine[2048];   // sine_table of the decoder's tone synthesis
    float hann[256];    // hann_window
    float amp_sf[64];   // amp_sf_tab
    at3::cpx tw[256];   // forward twiddles of the 256-point FFT
    double thr[64];     // (amp_sf_tab[i] * 2^(-1/8))^2
    double rs[1024];    // 1 / sum over t of hann_window[t] * sin^2, the sine of step 4 at frequency index f
    double rc[1024];    // the same with the cosine
};

constexpr int kToneBandWaves = 3;                     // AT3PHIP_TONE_MAX_BAND_WAVES
constexpr int kToneSpan = 7;                          // AT3PHIP_TONE_FINE_SPAN
constexpr int kToneFine = 2 * kToneSpan + 1;          // frequency indices searched per candidate
constexpr int kToneFrameWaves = 2 * 16 * kToneBandWaves;   // waves a frame can hold before the budget

// One wave as k_at3p_tone_find leaves it for k_at3p_tone_select
struct ToneCand {
    double a2;        // A2 of step 5
    uint32_t wave;    // AT3PHIP_TONAL_WAVE(FreqIndex, AmpSf, PhaseIndex)
    uint32_t valid;   // 0: no wave in this slot
};

struct ToneParams {
    const ToneFindTables* T;
    const float* bands;     // [S][F][nch][16][128]
    const float* prev_x;    // [S][nch][16][128]: the frame before the call's first
    ToneCand* cand;         // [S][F][nch][16][3]
    TonalBlock* blocks;     // [S][F]: slot f = the block of (frame f-1, frame f)
    TonalBlock* last;       // [S]: the block of the slot before the call's first
    TonalBlock* writer;     // [S][F] or null: slot f = the record the frame writer pairs with residual slot f, the block of slot f-1
    float* resid;           // [S][F][nch][16][128]: slot f = the residual of frame f-1
    int32_t n_frames, nch;
};

__global__ __launch_bounds__(256) void k_at3p_tone_find(ToneParams p)
{
    __shared__ float s_sine[2048];
    __shared__ __attribute__((aligned(8))) at3::cpx s_tw[256];
    __shared__ __attribute__((aligned(8))) at3::cpx s_F[4][256];
    __shared__ float s_y[4][256];
    __shared__ float s_P[4][130];
    __shared__ double s_fS[4][kToneBandWaves * kToneFine], s_fC[4][kToneBandWaves * kToneFine], s_fP[4][kToneBandWaves * kToneFine];

    const ToneFindTables* T = p.T;
    // gridDim.x = (slot, group of four subbands), gridDim.y = (stream, channel) as in every other kernel of the context: whatever
    // at3phip_create admits (n_streams * channels <= 65535) can be launched
    const int f = blockIdx.x >> 2, nch = p.nch, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int sc = blockIdx.y, sb = 4 * (blockIdx.x & 3) + w;
    const int s = sc / nch, ch = sc - s * nch;
    const size_t item = ((size_t)s * p.n_frames + f) * nch + ch;

    for (int i = tid; i < 2048; i += 256) s_sine[i] = T->sine[i];
    s_tw[tid] = T->tw[tid];
    // step 1, stored for the sums of step 4 and, in the transform's leaf order, for step 2
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = lane + 64 * r;
        const float* src = t >= 128 ? p.bands + item * kFrame + 128 * sb + (t - 128)
                         : f > 0    ? p.bands + (item - nch) * kFrame + 128 * sb + t
                                    : p.prev_x + ((size_t)s * nch + ch) * kFrame + 128 * sb + t;
        const float y = *src * T->hann[t];
        s_y[w][t] = y;
        at3::cpx v;
        v.r = y;
        v.i = 0.0f;
        s_F[w][fft_leaf_pos<256>(t)] = v;
    }
    __syncthreads();
    // step 2 (from here on the four wavefronts go their own ways)
    fft_lds<256, false, false, true>(s_F[w], 256, 1, s_tw, lane, 64);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const at3::cpx v = s_F[w][lane + 64 * r];
        s_P[w][lane + 64 * r] = v.r * v.r + v.i * v.i;
    }
    if (lane == 0) {
        const at3::cpx v = s_F[w][128];
        s_P[w][128] = v.r * v.r + v.i * v.i;
    }
    at3::wave_sync();
    // step 3: the sum in every lane alike, the candidates by ballot, the three largest in wave-uniform registers
    float sum = 0.0f;
    for (int k = 1; k <= 127; ++k) sum = sum + s_P[w][k];
    const double floor_p = 16.0 * ((double)sum / 127.0);
    auto is_cand = [&](int k) {   // (the spectrum of a real signal is even about bins 0 and 128)
        const float pk = s_P[w][k];
        return pk > s_P[w][k == 0 ? 1 : k - 1] && pk >= s_P[w][k == 128 ? 127 : k + 1] && (double)pk >= floor_p;
    };
    const unsigned long long m_lo = __ballot(is_cand(lane));                         // bins 0 .. 63
    const unsigned long long m_hi = __ballot(is_cand(lane + 64));                    // bins 64 .. 127
    const unsigned long long m_top = __ballot(is_cand(128)) & 1ull;                  // bin 128
    int nc = 0, k0 = 0, k1 = 0, k2 = 0;
    float p0 = -1.0f, p1 = -1.0f, p2 = -1.0f;   // (a power is never negative)
    for (int part = 0; part < 3; ++part) {
        unsigned long long m = part == 0 ? m_lo : part == 1 ? m_hi : m_top;
        while (m) {
            const int k = __builtin_ctzll(m) + 64 * part;
            m &= m - 1;
            const float pk = s_P[w][k];
            if (pk > p0) {
                p2 = p1; k2 = k1; p1 = p0; k1 = k0; p0 = pk; k0 = k;
            } else if (pk > p1) {
                p2 = p1; k2 = k1; p1 = pk; k1 = k;
            } else if (pk > p2) {
                p2 = pk; k2 = k;
            }
            nc = nc < kToneBandWaves ? nc + 1 : nc;
        }
    }
    // step 4: one lane per (candidate, frequency index), each walking t = 0 .. 255 in order
    {
        const int c = lane / kToneFine, o = lane - c * kToneFine;
        const int kc = c == 0 ? k0 : c == 1 ? k1 : k2;
        const int fi = 8 * kc - kToneSpan + o;
        if (c < nc && fi >= 1 && fi <= 1023) {
            double S = 0.0, C = 0.0;
            int pos = (-128 * fi) & 2047;
            for (int t = 0; t < 256; ++t) {
                const double y = (double)s_y[w][t];
                S = S + y * (double)s_sine[pos];
                C = C + y * (double)s_sine[(pos + 512) & 2047];
                pos = (pos + fi) & 2047;
            }
            s_fS[w][lane] = S;
            s_fC[w][lane] = C;
            s_fP[w][lane] = (S * S) * T->rs[fi] + (C * C) * T->rc[fi];
        }
    }
    at3::wave_sync();
    // steps 4 (the choice) and 5: one lane per candidate
    if (lane < kToneBandWaves) {
        ToneCand out;
        out.a2 = 0.0;
        out.wave = 0u;
        out.valid = 0u;
        if (lane < nc) {
            const int kc = lane == 0 ? k0 : lane == 1 ? k1 : k2;
            int bf = -1;
            double bs = 0.0, bc = 0.0, bp = 0.0;
            for (int o = 0; o < kToneFine; ++o) {
                const int fi = 8 * kc - kToneSpan + o;
                if (fi < 1 || fi > 1023) continue;
                const double pw = s_fP[w][lane * kToneFine + o];
                if (bf < 0 || pw > bp) {
                    bf = fi;
                    bs = s_fS[w][lane * kToneFine + o];
                    bc = s_fC[w][lane * kToneFine + o];
                    bp = pw;
                }
            }
            const int bi = bf < 0 ? 0 : bf;
            const double ca = bs * T->rs[bi], cb = bc * T->rc[bi];   // x[t] = ca sin + cb cos, by least squares under the window
            const double a2 = ca * ca + cb * cb;
            if (bf >= 0 && a2 >= 8.0 * 8.0) {
                int sf = 0;
                for (int i = 0; i < 64; ++i)
                    if (a2 >= T->thr[i]) sf = i;
                int ph = 0;
                double bv = 0.0;
                for (int q = 0; q < 32; ++q) {
                    const double v = ca * (double)s_sine[(64 * q + 512) & 2047] + cb * (double)s_sine[64 * q];
                    if (q == 0 || v > bv) {
                        ph = q;
                        bv = v;
                    }
                }
                out.a2 = a2;
                out.wave = (uint32_t)bf | (uint32_t)sf << 10 | (uint32_t)ph << 16;
                out.valid = 1u;
            }
        }
        p.cand[(item * 16 + sb) * kToneBandWaves + lane] = out;
    }
}

__global__ __launch_bounds__(128) void k_at3p_tone_select(ToneParams p)
{
    __shared__ double s_a2[kToneFrameWaves];
    __shared__ uint32_t s_key[kToneFrameWaves], s_wave[kToneFrameWaves], s_ok[kToneFrameWaves];
    __shared__ uint32_t s_rec[kTonalBlockWords];
    __shared__ uint32_t s_top;

    const int f = blockIdx.x, s = blockIdx.y, nch = p.nch, tid = threadIdx.x;
    const size_t item = (size_t)s * p.n_frames + f;
    const int ch = tid / (16 * kToneBandWaves), rest = tid - ch * (16 * kToneBandWaves), sb = rest / kToneBandWaves;
    const bool mine = tid < kToneFrameWaves;

    if (tid < kTonalBlockWords) s_rec[tid] = 0u;
    if (tid == 0) s_top = 0u;
    if (mine) {
        ToneCand c;
        c.a2 = 0.0;
        c.wave = 0u;
        c.valid = 0u;
        if (ch < nch) c = p.cand[(item * nch + ch) * 16 * kToneBandWaves + rest];   // [ch][sb][slot]: rest = sb * 3 + slot
        s_a2[tid] = c.a2;
        s_wave[tid] = c.wave;
        s_key[tid] = (uint32_t)ch << 16 | (uint32_t)sb << 12 | (c.wave & 1023u);   // the record's order: channel, band, frequency index
        s_ok[tid] = c.valid;
    }
    __syncthreads();
    // step 6: a wave stays when fewer than 48 go before it
    bool keep = false;
    if (mine && s_ok[tid]) {
        const double a2 = s_a2[tid];
        const uint32_t key = s_key[tid];
        int rank = 0;
        for (int j = 0; j < kToneFrameWaves; ++j)
            if (j != tid && s_ok[j] && (s_a2[j] > a2 || (s_a2[j] == a2 && s_key[j] < key))) ++rank;
        keep = rank < kTonalMaxWaves;
    }
    __syncthreads();
    if (mine) s_ok[tid] = keep ? 1u : 0u;
    __syncthreads();
    // step 7: its place is the number of kept waves before it in the record's order
    if (keep) {
        const uint32_t key = s_key[tid];
        int at = 0;
        for (int j = 0; j < kToneFrameWaves; ++j)
            if (s_ok[j] && s_key[j] < key) ++at;
        s_rec[33 + (at < kTonalMaxWaves ? at : kTonalMaxWaves - 1)] = s_wave[tid];
        atomicAdd(&s_rec[1 + ch * 16 + sb], 1u);    // n_waves is the band word's low byte; a band holds at most 3
        atomicMax(&s_top, (uint32_t)sb + 1u);
    }
    __syncthreads();
    if (tid == 0) s_rec[0] = s_top;   // num_tone_bands; second_is_leader and tone_sharing stay 0
    __syncthreads();
    if (tid < kTonalBlockWords) {
        const uint32_t v = s_rec[tid];
        reinterpret_cast<uint32_t*>(p.blocks + item)[tid] = v;
        if (p.writer && f + 1 < p.n_frames) reinterpret_cast<uint32_t*>(p.writer + item + 1)[tid] = v;
    }
}

// the sum of a band's waves at sample i of a frame: the decoder's step 4b (decp_waves, at3p_decode.hpp) without an envelope
__device__ __forceinline__ float tone_waves(const ToneFindTables* T, const uint32_t* rec, int first, int n, int reg, int i)
{
    float v = 0.0f;
    for (int k = 0; k < n; ++k) {
        const int at = first + k;
        const uint32_t wv = rec[33 + (at < kTonalMaxWaves ? at : kTonalMaxWaves - 1)];
        const int inc = (int)(wv & 1023u), sf = (int)((wv >> 10) & 63u), ph = (int)((wv >> 16) & 31u);
        const double amp = (double)T->amp_sf[sf];
        const int pos = ((ph << 6) + (i - (reg ^ 128)) * inc) & 2047;
        v = (float)((double)v + (double)T->sine[pos] * amp);
    }
    return v;
}

__global__ __launch_bounds__(256) void k_at3p_tone_sub(ToneParams p)
{
    __shared__ uint32_t s_cur[kTonalBlockWords], s_old[kTonalBlockWords];
    __shared__ int s_first[2][16], s_n[2][16];   // [0]: the block before (fading out), [1]: this slot's (fading in)

    const ToneFindTables* T = p.T;
    const int f = blockIdx.x, sc = blockIdx.y, nch = p.nch, tid = threadIdx.x;
    const int s = sc / nch, ch = sc - s * nch;
    const size_t item = ((size_t)s * p.n_frames + f) * nch + ch;

    if (tid < kTonalBlockWords) {
        const TonalBlock* cur = p.blocks + (size_t)s * p.n_frames + f;
        s_cur[tid] = reinterpret_cast<const uint32_t*>(cur)[tid];
        s_old[tid] = reinterpret_cast<const uint32_t*>(f > 0 ? cur - 1 : p.last + s)[tid];
    }
    __syncthreads();
    if (tid < 32) {   // the band's first wave: the waves of every band before it, channel 0's bands first
        const uint32_t* rec = tid < 16 ? s_old : s_cur;
        const int b = tid & 15;
        int first = 0;
        for (int j = 0; j < ch * 16 + b; ++j) first += (int)(rec[1 + j] & 0xffu);
        const int n = (int)(rec[1 + ch * 16 + b] & 0xffu);
        s_first[tid >> 4][b] = first;
        s_n[tid >> 4][b] = n > kTonalMaxBandWaves ? kTonalMaxBandWaves : n;
    }
    __syncthreads();
    const float* src = f > 0 ? p.bands + (item - nch) * kFrame : p.prev_x + ((size_t)s * nch + ch) * kFrame;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int j = tid + 256 * r, b = j >> 7, i = j & 127;
        float x = src[j];
        const int n1 = s_n[0][b], n2 = s_n[1][b];
        if (n1 | n2) {   // ApplyFilter: out -= wavreg1 + wavreg2
            float w1 = tone_waves(T, s_old, s_first[0][b], n1, 128, i);
            float w2 = tone_waves(T, s_cur, s_first[1][b], n2, 0, i);
            if (n1) w1 = w1 * T->hann[128 + i];
            if (n2) w2 = w2 * T->hann[i];
            x = x - (w1 + w2);
        }
        p.resid[item * kFrame + j] = x;
    }
}

// After a call: the writer's first record is the block carried into the call; then the call's last frame and block are carried on.
__global__ __launch_bounds__(256) void k_at3p_tone_state(ToneParams p, float* prev_x)
{
    const int s = blockIdx.x, tid = threadIdx.x;
    const TonalBlock* newest = p.blocks + (size_t)s * p.n_frames + (p.n_frames - 1);
    if (tid < kTonalBlockWords) {   // (a work-item reads and writes its own word only)
        uint32_t* last = reinterpret_cast<uint32_t*>(p.last + s);
        if (p.writer) reinterpret_cast<uint32_t*>(p.writer + (size_t)s * p.n_frames)[tid] = last[tid];
        last[tid] = reinterpret_cast<const uint32_t*>(newest)[tid];
    }
    const int n = p.nch * kFrame;
    const float* src = p.bands + ((size_t)s * p.n_frames + (p.n_frames - 1)) * n;
    for (int j = tid; j < n; j += 256) prev_x[(size_t)s * n + j] = src[j];
}

}  // namespace at3p
