// ATRAC3plus tone analysis kernels (gfx950): include/at3phip.h, FINDING TONES, steps 1-8, between k_at3p_pqf and k_at3p_mdct.
//   k_at3p_tone_find    steps 1-5: one wavefront per (stream, frame, channel, subband), four subbands per workgroup
//   k_at3p_tone_select  steps 6-7: one workgroup per (stream, frame) ranks the frame's waves by counting and packs the record
//   k_at3p_tone_sub     step 8: one workgroup per (stream, frame, channel) subtracts this block and the one before
//   k_at3p_tone_state   the carried frame and block, and the writer's first record of the call
// Slot f of a call works on the pair (frame f-1, frame f), frame -1 being the carried one, so every slot of a call runs side by
// side. Every sum runs in the order the header states, in one lane: the restatement (tests/host/at3p_gha_cpu.c) is the same
// loop. Float operations without contraction.
// GATES (AT3PHIP_TONES_GATED, steps G1-G5 of the header): k_at3p_tone_find<true> gates both frames of its pair, windows and fits
// the bands that have an event and hands the second frame's gate to k_at3p_tone_select, which writes the points;
// k_at3p_tone_sub<true> applies the records' envelopes (the decoder's own functions, at3p_tone_synth.hpp), for which the block
// before the last one is carried as well. k_at3p_tone_find<false> and k_at3p_tone_sub<false> are the kernels without any of it.
// SHARING (AT3PHIP_TONES_SHARED, steps S1-S5 of the header, stereo only): k_at3p_tone_select<true> decides the twin bands, keeps
// channel 1's waves of those bands out of the budget and writes the sharing word; k_at3p_tone_sub<., true> resolves channel 1's
// band through each record's own sharing word. The <false> instances are the kernels without any of it; k_at3p_tone_find and
// k_at3p_tone_state are the same for both (the carried records hold their sharing words).
// These kernels and the host mirror's TAt3PToneAnalyser (atracdenc_amd/host/at3hip_host.hpp) are each pinned bit for bit to one C
// restatement, tests/host/at3p_gha_cpu.c: a change to the definition changes all three. The table builder is build_tone_find_tables.
#pragma once
#include "at3p_kernels.hpp"
#include "at3p_write.hpp"
#include "at3p_tone_synth.hpp"

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
constexpr int kToneGateMin = 4;                       // AT3PHIP_TONE_GATE_MIN
constexpr double kToneGateRatio = 16.0;               // AT3PHIP_TONE_GATE_RATIO

// One wave as k_at3p_tone_find leaves it for k_at3p_tone_select
struct ToneCand {
    double a2;        // A2 of step 5
    uint32_t wave;    // AT3PHIP_TONAL_WAVE(FreqIndex, AmpSf, PhaseIndex)
    uint32_t valid;   // bit 0: a wave in this slot; bits 8 .. 15 of a band's first slot: the gate of the pair's second frame (G1's byte)
};

struct ToneParams {
    const ToneFindTables* T;
    const float* bands;     // [S][F][nch][16][128]
    const float* prev_x;    // [S][nch][16][128]: the frame before the call's first
    ToneCand* cand;         // [S][F][nch][16][3]
    TonalBlock* blocks;     // [S][F]: slot f = the block of (frame f-1, frame f)
    TonalBlock* last;       // [2][S]: the block of the slot before the call's first, then the block before that one
    TonalBlock* writer;     // [S][F] or null: slot f = the record the frame writer pairs with residual slot f, the block of slot f-1
    float* resid;           // [S][F][nch][16][128]: slot f = the residual of frame f-1
    int32_t n_frames, nch, n_streams;
    int32_t gated;          // AT3PHIP_TONES_GATED
};

// G1 from what its lanes left in g: the cell energies e[j] of frame fr at g[32 fr + j], d(s), before(s), after(s) at
// g[64 + 32 fr + s], g[128 + ..], g[192 + ..]
__device__ __forceinline__ uint32_t tone_gate_pick(const double* g, int fr)
{
    int bs = kToneGateMin;
    double bd = g[64 + 32 * fr + kToneGateMin];
    for (int sp = kToneGateMin + 1; sp <= 32 - kToneGateMin; ++sp) {
        const double d = g[64 + 32 * fr + sp];
        if (d > bd) {
            bs = sp;
            bd = d;
        }
    }
    const double before = g[128 + 32 * fr + bs], after = g[192 + 32 * fr + bs];
    // the loud side holds at least MIN loud cells next to the split: each over R times the quiet side's mean, and not zero
    const double* e = g + 32 * fr;
    if (after >= kToneGateRatio * before && after > 0.0) {
        bool ok = true;
        for (int j = bs; j < bs + kToneGateMin; ++j) ok = ok && e[j] >= kToneGateRatio * before && e[j] > 0.0;
        return ok ? (uint32_t)bs : 0u;
    }
    if (before >= kToneGateRatio * after && before > 0.0) {
        bool ok = true;
        for (int j = bs - kToneGateMin; j < bs; ++j) ok = ok && e[j] >= kToneGateRatio * after && e[j] > 0.0;
        return ok ? 0x80u | (uint32_t)(bs - 1) : 0u;
    }
    return 0u;
}

// a gate byte as the band of a record that holds nothing but its point
__device__ __forceinline__ TonalBand tone_gate_band(uint32_t gate)
{
    TonalBand b;
    b.nw = 0;
    b.start_index = 0;
    b.sp = gate && gate < 0x80u ? (uint8_t)(gate + 1u) : (uint8_t)0;
    b.ep = gate >= 0x80u ? (uint8_t)((gate & 31u) + 1u) : (uint8_t)0;
    return b;
}

template <bool kGated>
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
    bool gated = false;       // wave-uniform: the band has an event in one of the two frames
    uint32_t gate1 = 0u;      // the second frame's
    int t0 = 0, t1 = 255;     // G3's interval in samples
    if constexpr (kGated) {
        // the pair's first frame and its second
        const float* x0 = (f > 0 ? p.bands + (item - nch) * kFrame : p.prev_x + ((size_t)s * nch + ch) * kFrame) + 128 * sb;
        const float* x1 = p.bands + item * kFrame + 128 * sb;
        double* g = reinterpret_cast<double*>(s_F[w]);   // 256 doubles of this wavefront's own, free until step 1
        {   // G1: one lane per cell, then one lane per (frame, split)
            const float* c = (lane < 32 ? x0 : x1) + 4 * (lane & 31);
            float e = c[0] * c[0];
            e = e + c[1] * c[1];
            e = e + c[2] * c[2];
            e = e + c[3] * c[3];
            g[lane] = (double)e;
        }
        at3::wave_sync();
        {
            const int sp = lane & 31;
            const double* e = g + (lane & 32);
            double acc = 0.0, ps = 0.0;   // P[32] and P[sp]
            for (int j = 0; j < 32; ++j) {
                acc = acc + e[j];
                if (j + 1 == sp) ps = acc;
            }
            double d = 0.0, before = 0.0, after = 0.0;
            if (sp >= kToneGateMin && sp <= 32 - kToneGateMin) {
                before = ps / (double)sp;
                after = (acc - ps) / (double)(32 - sp);
                d = fabs(after - before);
            }
            g[64 + lane] = d;
            g[128 + lane] = before;
            g[192 + lane] = after;
        }
        at3::wave_sync();
        const uint32_t gate0 = tone_gate_pick(g, 0);
        gate1 = tone_gate_pick(g, 1);
        at3::wave_sync();   // (s_F[w] is step 1's from here)
        if (gate0 | gate1) {   // G3
            const DecpEnv env = decp_curr_env(tone_gate_band(gate1), tone_gate_band(gate0));
            gated = true;
            t0 = 4 * (env.hs ? env.s : 0);
            t1 = 4 * (env.he ? env.e : 63) + 3;
        }
    }
    // step 1, stored for the sums of step 4 and, in the transform's leaf order, for step 2
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = lane + 64 * r;
        const float* src = t >= 128 ? p.bands + item * kFrame + 128 * sb + (t - 128)
                         : f > 0    ? p.bands + (item - nch) * kFrame + 128 * sb + t
                                    : p.prev_x + ((size_t)s * nch + ch) * kFrame + 128 * sb + t;
        const float y = *src * (kGated && gated && (t < t0 || t > t1) ? 0.0f : T->hann[t]);
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
    if (kGated && gated && (t1 - t0 + 1) / 4 < kToneGateMin) nc = 0;   // G3: too short an interval gets no wave
    // step 4: one lane per (candidate, frequency index), each walking t = 0 .. 255 in order
    bool fit_ok = true;   // G4: the lane's frequency index has a positive determinant
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
            if (kGated && gated) {   // G4: the 2 x 2 normal equations under the gated window; a and b take the places of S and C
                double gss = 0.0, gcc = 0.0, gsc = 0.0;
                pos = ((t0 - 128) * fi) & 2047;
                for (int t = t0; t <= t1; ++t) {
                    const double hw = (double)T->hann[t], sn = (double)s_sine[pos], cs = (double)s_sine[(pos + 512) & 2047];
                    gss = gss + hw * (sn * sn);
                    gcc = gcc + hw * (cs * cs);
                    gsc = gsc + hw * (sn * cs);
                    pos = (pos + fi) & 2047;
                }
                const double det = gss * gcc - gsc * gsc;
                fit_ok = det > 0.0;
                const double a = (S * gcc - C * gsc) / det, b = (C * gss - S * gsc) / det;
                s_fS[w][lane] = a;
                s_fC[w][lane] = b;
                s_fP[w][lane] = a * S + b * C;
            } else {
                s_fS[w][lane] = S;
                s_fC[w][lane] = C;
                s_fP[w][lane] = (S * S) * T->rs[fi] + (C * C) * T->rc[fi];
            }
        }
    }
    unsigned long long fit_mask = ~0ull;
    if constexpr (kGated) fit_mask = __ballot(fit_ok);
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
                if (fi < 1 || fi > 1023 || !((fit_mask >> (lane * kToneFine + o)) & 1ull)) continue;
                const double pw = s_fP[w][lane * kToneFine + o];
                if (bf < 0 || pw > bp) {
                    bf = fi;
                    bs = s_fS[w][lane * kToneFine + o];
                    bc = s_fC[w][lane * kToneFine + o];
                    bp = pw;
                }
            }
            const int bi = bf < 0 ? 0 : bf;
            // x[t] = ca sin + cb cos, by least squares under the window
            const double ca = kGated && gated ? bs : bs * T->rs[bi], cb = kGated && gated ? bc : bc * T->rc[bi];
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
        if (kGated && lane == 0) out.valid |= gate1 << 8;
        p.cand[(item * 16 + sb) * kToneBandWaves + lane] = out;
    }
}

// kShared: S2-S4 of a stereo context (only launched with nch = 2)
template <bool kShared>
__global__ __launch_bounds__(128) void k_at3p_tone_select(ToneParams p)
{
    __shared__ double s_a2[kToneFrameWaves];
    __shared__ uint32_t s_key[kToneFrameWaves], s_wave[kToneFrameWaves], s_ok[kToneFrameWaves];
    __shared__ uint32_t s_rec[kTonalBlockWords];
    __shared__ uint32_t s_top;
    __shared__ uint32_t s_gate[2 * 16], s_twin;   // kShared only: the bands' gate bytes, and bit b = band b is a twin

    const int f = blockIdx.x, s = blockIdx.y, nch = p.nch, tid = threadIdx.x;
    const size_t item = (size_t)s * p.n_frames + f;
    const int ch = tid / (16 * kToneBandWaves), rest = tid - ch * (16 * kToneBandWaves), sb = rest / kToneBandWaves;
    const bool mine = tid < kToneFrameWaves;
    uint32_t gate = 0u;

    if (tid < kTonalBlockWords) s_rec[tid] = 0u;
    if (tid == 0) s_top = 0u;
    if (kShared && tid == 0) s_twin = 0u;
    if (mine) {
        ToneCand c;
        c.a2 = 0.0;
        c.wave = 0u;
        c.valid = 0u;
        if (ch < nch) c = p.cand[(item * nch + ch) * 16 * kToneBandWaves + rest];   // [ch][sb][slot]: rest = sb * 3 + slot
        s_a2[tid] = c.a2;
        s_wave[tid] = c.wave;
        s_key[tid] = (uint32_t)ch << 16 | (uint32_t)sb << 12 | (c.wave & 1023u);   // the record's order: channel, band, frequency index
        s_ok[tid] = c.valid & 1u;
        gate = p.gated ? (c.valid >> 8) & 0xffu : 0u;   // (only a band's first slot carries one)
        if (kShared && rest == sb * kToneBandWaves) s_gate[ch * 16 + sb] = gate;
    }
    __syncthreads();
    if constexpr (kShared) {
        if (tid < 16) {   // S2: one lane per band; the words as sets (a band's words differ from one another), the points by their gate bytes
            const uint32_t* ok0 = s_ok + tid * kToneBandWaves;
            const uint32_t* ok1 = ok0 + 16 * kToneBandWaves;
            const uint32_t* w0 = s_wave + tid * kToneBandWaves;
            const uint32_t* w1 = w0 + 16 * kToneBandWaves;
            uint32_t n0 = 0u, n1 = 0u;
            bool same = s_gate[tid] == s_gate[16 + tid];
#pragma unroll
            for (int i = 0; i < kToneBandWaves; ++i) {
                n0 += ok0[i];
                n1 += ok1[i];
                bool found = false;
#pragma unroll
                for (int j = 0; j < kToneBandWaves; ++j) found = found || (ok1[j] && w1[j] == w0[i]);
                same = same && (!ok0[i] || found);
            }
            if (same && n0 == n1) atomicOr(&s_twin, 1u << tid);
        }
        __syncthreads();
        if (mine && ch == 1 && ((s_twin >> sb) & 1u)) {   // S3, S4: channel 1's waves of a twin band leave the population, and its point is not written
            s_ok[tid] = 0u;
            gate = 0u;
        }
        __syncthreads();
    }
    if (gate) {   // G2: the point, with or without a wave in the band: byte 1 of the band's word is start + 1, byte 2 stop + 1
        atomicAdd(&s_rec[1 + ch * 16 + sb], gate < 0x80u ? (gate + 1u) << 8 : ((gate & 31u) + 1u) << 16);
        atomicMax(&s_top, (uint32_t)sb + 1u);
    }
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
    // num_tone_bands (the highest band with a wave or a point, plus 1); second_is_leader stays 0, and so does tone_sharing without S4
    if (tid == 0) s_rec[0] = kShared ? s_top | (s_twin & ((1u << s_top) - 1u)) << 16 : s_top;
    __syncthreads();
    if (tid < kTonalBlockWords) {
        const uint32_t v = s_rec[tid];
        reinterpret_cast<uint32_t*>(p.blocks + item)[tid] = v;
        if (p.writer && f + 1 < p.n_frames) reinterpret_cast<uint32_t*>(p.writer + item + 1)[tid] = v;
    }
}

// S5: the channel whose band b a record's channel ch uses: channel 0's where the record shares the band
__device__ __forceinline__ int tone_rec_channel(uint32_t word0, int ch, int b)
{
    return ch == 1 && ((word0 >> (16 + b)) & 1u) ? 0 : ch;
}

// band b of channel ch of a record's words as the decoder's TonalBand; kShared: through the record's sharing word
template <bool kShared = false>
__device__ __forceinline__ TonalBand tone_rec_band(const uint32_t* rec, int ch, int b)
{
    if constexpr (kShared) ch = tone_rec_channel(rec[0], ch, b);
    int first = 0;   // the band's first wave: the waves of every band before it, channel 0's bands first
    for (int j = 0; j < ch * 16 + b; ++j) first += (int)(rec[1 + j] & 0xffu);
    const uint32_t word = rec[1 + ch * 16 + b];
    int n = (int)(word & 0xffu);
    n = n > kTonalMaxBandWaves ? kTonalMaxBandWaves : n;
    first = first > kTonalMaxWaves ? kTonalMaxWaves : first;
    TonalBand t;
    t.nw = (uint8_t)(n > kTonalMaxWaves - first ? kTonalMaxWaves - first : n);   // (no read past the record's waves, whatever it holds)
    t.start_index = (uint8_t)first;
    t.sp = (uint8_t)((word >> 8) & 0xffu);
    t.ep = (uint8_t)((word >> 16) & 0xffu);
    return t;
}

// kGated = false: no record of the stream holds a point, and none is looked for
// kShared = false: no record of the stream shares a band
template <bool kGated, bool kShared>
__global__ __launch_bounds__(256) void k_at3p_tone_sub(ToneParams p)
{
    __shared__ uint32_t s_cur[kTonalBlockWords], s_old[kTonalBlockWords];
    __shared__ TonalBand s_band[2][16];   // [0]: the block before (fading out), [1]: this slot's (fading in)
    __shared__ DecpToneJob s_job[16];     // region 1: the block before, region 2: this slot's

    const ToneFindTables* T = p.T;
    const int f = blockIdx.x, sc = blockIdx.y, nch = p.nch, tid = threadIdx.x;
    const int s = sc / nch, ch = sc - s * nch;
    const size_t item = ((size_t)s * p.n_frames + f) * nch + ch;
    const TonalBlock* cur = p.blocks + (size_t)s * p.n_frames + f;

    if (tid < kTonalBlockWords) {
        s_cur[tid] = reinterpret_cast<const uint32_t*>(cur)[tid];
        s_old[tid] = reinterpret_cast<const uint32_t*>(f > 0 ? cur - 1 : p.last + s)[tid];
    }
    __syncthreads();
    if (tid < 32) s_band[tid >> 4][tid & 15] = tone_rec_band<kShared>(tid < 16 ? s_old : s_cur, ch, tid & 15);
    __syncthreads();
    if (tid < 16) {   // step 8 / G5: what the decoder's step 4b does with these records
        // the block before the old one: its points decide the old block's envelope
        const TonalBlock* older = f > 1 ? cur - 2 : f == 1 ? p.last + s : p.last + p.n_streams + s;
        const uint32_t* ow = reinterpret_cast<const uint32_t*>(older);
        const uint32_t word = kGated ? ow[1 + (kShared ? tone_rec_channel(ow[0], ch, tid) : ch) * 16 + tid] : 0u;
        TonalBand pv;
        pv.nw = 0;
        pv.start_index = 0;
        pv.sp = (uint8_t)((word >> 8) & 0xffu);
        pv.ep = (uint8_t)((word >> 16) & 0xffu);
        s_job[tid] = decp_tone_job(s_band[1][tid], s_band[0][tid], pv, true);
    }
    __syncthreads();
    const float* src = f > 0 ? p.bands + (item - nch) * kFrame : p.prev_x + ((size_t)s * nch + ch) * kFrame;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int j = tid + 256 * r, b = j >> 7, i = j & 127;
        float x = src[j];
        const DecpToneJob& J = s_job[b];
        if constexpr (kGated) {
            if (J.active) {   // ApplyFilter: out -= wavreg1 + wavreg2
                float w1 = J.n1 ? decp_waves(T, &s_old[33 + J.i1], J.n1, J.e1, 128, i) : 0.0f;
                float w2 = J.n2 ? decp_waves(T, &s_cur[33 + J.i2], J.n2, J.e2, 0, i) : 0.0f;
                if (J.h1) w1 = w1 * T->hann[128 + i];
                if (J.h2) w2 = w2 * T->hann[i];
                x = x - (w1 + w2);
            }
        } else {   // without points every region is synthesised and Hann-windowed: the job is its four counts and indices
            const int n1 = J.n1, n2 = J.n2;
            if (n1 | n2) {
                float w1 = decp_waves<false>(T, &s_old[33 + J.i1], n1, J.e1, 128, i);
                float w2 = decp_waves<false>(T, &s_cur[33 + J.i2], n2, J.e2, 0, i);
                if (n1) w1 = w1 * T->hann[128 + i];
                if (n2) w2 = w2 * T->hann[i];
                x = x - (w1 + w2);
            }
        }
        p.resid[item * kFrame + j] = x;
    }
}

// After a call: the writer's first record is the block carried into the call; then the call's last frame and last two blocks are
// carried on.
__global__ __launch_bounds__(256) void k_at3p_tone_state(ToneParams p, float* prev_x)
{
    const int s = blockIdx.x, tid = threadIdx.x;
    const TonalBlock* newest = p.blocks + (size_t)s * p.n_frames + (p.n_frames - 1);
    if (tid < kTonalBlockWords) {   // (a work-item reads and writes its own word only)
        uint32_t* last = reinterpret_cast<uint32_t*>(p.last + s);
        const uint32_t was = last[tid];
        if (p.writer) reinterpret_cast<uint32_t*>(p.writer + (size_t)s * p.n_frames)[tid] = was;
        if (p.gated)   // (an ungated stream's records hold no point: the block before the last one is never looked at)
            reinterpret_cast<uint32_t*>(p.last + p.n_streams + s)[tid] = p.n_frames > 1 ? reinterpret_cast<const uint32_t*>(newest - 1)[tid] : was;
        last[tid] = reinterpret_cast<const uint32_t*>(newest)[tid];
    }
    const int n = p.nch * kFrame;
    const float* src = p.bands + ((size_t)s * p.n_frames + (p.n_frames - 1)) * n;
    for (int j = tid; j < n; j += 256) prev_x[(size_t)s * n + j] = src[j];
}

}  // namespace at3p
