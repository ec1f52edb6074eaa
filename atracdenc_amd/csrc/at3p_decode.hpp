// ATRAC3plus decode kernels (gfx950): the decoder defined in include/at3phip.h (decoder section) for a batch of streams, every
// frame of a call in parallel.
//
// What a frame needs of its past. Frame n's subband samples are its IMDCT's first half windowed with frame n-1's flags plus
// frame n-1's second half windowed with the same flags (TAt3pMIDCT::Do). Its PCM is the synthesis filter over those samples and
// the ring of the last 23 DCT-IV columns of frame n-1, which need frame n-1's samples [105, 128), and so frame n-2's IMDCT tail
// and flags. So a frame needs the IMDCT outputs of frames n, n-1, n-2 and nothing is scanned:
//   k_at3pd_unpack  one wavefront per (frame, stream): bit unpack of both channels (one lane), dequantisation, then the 16 x C
//                   TMIDCT<256> (kissfft order, fft_lds) of the frame; writes the unwindowed IMDCT outputs and the window flags
//   k_at3pd_synth   one workgroup per (frame, stream, channel): the windows with the (n-1, n) pairing and the overlap-add for
//                   frame n and for frame n-1's last 23 columns, the rescale, the 151 DCT-IVs in f64, the 12-tap FIR, clamp,
//                   f32 or s16 output
//   k_at3pd_state   the call's last two frames become frames -2 and -1 of the next call, its last three tonal records
//                   records -3 .. -1
// Tonal blocks (AT3PHIP_DECODE_TONES): the unpack lane also parses the tonal block into a TonalRec per (frame, stream); step 4b
// runs in k_at3pd_synth. Frame n's samples need the records of frames n, n-1 (waves) and n-2 (frame n-1's envelope); frame n-1's
// last 23 samples need those of frames n-1 .. n-3, so four records are read and three are carried.
// Every float and double operation is the definition's, in its order, without contraction; no scratch.
// Shared with the other decoders: the bit reader, the linear code scan and the sign extension (at3_bits.hpp: MsbReader,
// prefix_scan, sext), the TMIDCT rotations and unfold and the clamped output store (at3_common.hpp: midct_pre, midct_post,
// midct_unfold, store_pcm).
#pragma once
#include "at3_bits.hpp"
#include "at3_common.hpp"
#include "at3p_tone_synth.hpp"

namespace at3p {

constexpr int kDecLut2Blocks = 1024;   // second-level VLC blocks (16 entries each); the tables need 887

// Constant tables of the decoder, built on the host (at3phip.hip) with the container's libm.
struct DecTables {
    double cos16[16][16];                // [k][n] = cos((M_PI / 16) * ((double)n + 0.5) * ((double)k + 0.5)), the "dct4" of the synthesis
    float fir[384];                      // at3p_fir.inc: ff_ipqf_coeffs1[t][i] = fir[12 i + t], ff_ipqf_coeffs2[t][i] = fir[192 + 12 i + t]
    float cs256[128];                    // TMIDCT<256>(): CalcSinCos(256, 128)
    cpx tw64[64];                        // kissfft forward twiddles of the 64-point core
    float sine128[128], sine64[64];      // SineWin128, SineWin64
    float mant[8];                       // atrac3p_mant_tab
    float scale[64];                     // NAt3p::TScaleTable::ScaleTable
    uint8_t spec_tab[56][2];             // group_size | num_coeffs << 4, bits | is_signed << 4 of spectra tables 0..55
    uint16_t wl_vlc[4][8];               // code | length << 12
    uint8_t qu_to_sb[32], sb_powgrps[16];
    // spectra tables 0..55: lut1[t][next 8 bits] = symbol | length << 8 (length 1..8), or 0x8000 | block for longer codes, whose
    // entry is lut2[block][the 4 bits after those 8] = symbol | length << 8; length 0 = no code
    uint16_t lut1[56][256];
    uint16_t lut2[kDecLut2Blocks][16];
};

// The tone synthesis' tables (ff_atrac3p_init_dsp_static), built on the host with its libm.
struct DecToneTables {
    float sine[2048];   // sine_table: (float)sin(2 pi i / 2048)
    float hann[256];    // hann_window: (float)((1.0 - cos(2 pi i / 256)) * 0.5)
    float amp_sf[64];   // amp_sf_tab: exp2f((i - 3) / 4.0f)
    uint16_t vlc[16];   // AT3P_TONE_BANDS_VLC: the code of NumToneBands - 1
};

// One frame's tonal block after ApplyFilter's bookkeeping (include/at3phip.h, step 1 with AT3PHIP_DECODE_TONES); TonalBand:
// at3p_tone_synth.hpp.
constexpr int kMaxWaves = 48;
struct TonalRec {
    uint32_t present;
    TonalBand band[2][16];
    uint32_t wave[kMaxWaves];   // freq | amp_sf << 10 | phase << 16
};
constexpr int kTonalWords = sizeof(TonalRec) / 4;
static_assert(sizeof(TonalRec) % 4 == 0, "TonalRec is copied as words");
constexpr int kTonalCarry = 3;   // records -3 .. -1 lead a call's records

// record of frame f (f = -3 .. -1: the carried ones) of stream s
template <typename Rec>
__device__ __forceinline__ Rec* decp_tonal_rec(Rec* t, int f, int s, int S) { return t + (size_t)(f + kTonalCarry) * S + s; }

constexpr int kDecReasons = 6;   // at3phip_decoder_counters order
enum { kRpOk = 0, kRpBadHeader, kRpUnsupported, kRpTonal, kRpBadCode, kRpReadPastEnd, kRpNoTerminator };

// The raw / flags records of a call are frame-major with two leading slots, so that the carried frames -2 and -1 sit at the
// same place whatever the number of frames of the call: record (slot, stream, channel) at (slot * S + s) * C + ch.
__device__ __forceinline__ size_t decp_rec(int slot, int s, int ch, int S, int C) { return ((size_t)slot * S + s) * C + ch; }

struct DecUnpackParams {
    const DecTables* T;
    const uint8_t* frames;        // [S][F][frame_bytes]
    int32_t n_frames, n_streams, nch;
    float* raw;                   // records of [16][256] floats: the TMIDCT<256> output per subband
    uint16_t* flags;              // records: steep-window bits
    unsigned long long* rejected; // [6]
    TonalRec* tonal;              // [F + 3][S]: record f + 3 = frame f
    const uint16_t* tone_vlc;     // AT3P_TONE_BANDS_VLC
    int32_t tones;                // AT3PHIP_DECODE_TONES
    int32_t frame_bytes;          // k_at3pd_unpack_sized only: a multiple of 8 up to 2048 (at3phip_decoder_set_frame_bytes)
};

using at3::MsbReader;   // over the frame staged in LDS as big-endian words; constructed with the frame's 8 * frame_bytes bits

// One symbol of spectra table t through the two-level look-up (DecTables::lut1, lut2) over the next 12 bits.
__device__ __forceinline__ int decp_spec_vlc(MsbReader& b, const DecTables* T, int t, int& invalid)
{
    if (b.bad) return 0;
    const uint32_t v = b.peek(12);
    uint32_t e = T->lut1[t][v >> 4];
    if (e & 0x8000u) e = T->lut2[e & 0x7fffu][v & 15u];
    const int len = (int)(e >> 8);
    if (!len) {
        invalid = 1;
        return 0;
    }
    if (b.pos + len > b.limit) {
        b.bad = 1;
        return 0;
    }
    b.advance(len);
    return (int)(e & 0xffu);
}

__device__ __forceinline__ int decp_bits_for(uint32_t x) { return x ? 32 - __builtin_clz(x) : 1; }   // GetFirstSetBit(x) + 1

// The tonal block (include/at3phip.h, step 1 with AT3PHIP_DECODE_TONES) into r, which is zero on entry; r holds
// the block after ApplyFilter's bookkeeping (start indices, shared bands, the leader swap) when kRpOk is returned.
__device__ __forceinline__ int decp_tonal(MsbReader& b, const uint16_t* tone_vlc, int C, TonalRec* r)
{
    int invalid = 0;
#define DECP_CHK()                              \
    do {                                        \
        if (b.bad) return kRpReadPastEnd;       \
        if (invalid) return kRpBadCode;         \
    } while (0)
#define DECP_MUST(n, val)                                   \
    do {                                                    \
        const uint32_t v_ = b.rd(n);                        \
        DECP_CHK();                                         \
        if (v_ != (uint32_t)(val)) return kRpUnsupported;   \
    } while (0)
    DECP_MUST(1, 1);   // amplitude mode 1
    const int nb = at3::prefix_scan<16>(b, tone_vlc, invalid) + 1;   // AT3P_TONE_BANDS_VLC: at most 6 bits, a complete code
    DECP_CHK();
    uint32_t shared = 0;
    int leader = 0;
    if (C == 2) {
        if (b.rd(1)) {
            if (b.rd(1) == 0) {
                shared = (1u << nb) - 1u;
            } else {
                for (int i = 0; i < nb; ++i) shared |= b.rd(1) << i;
            }
        }
        DECP_CHK();
        if (b.rd(1)) {
            DECP_MUST(1, 0);   // '1 1 x': never written
            leader = 1;
        }
        DECP_MUST(1, 0);       // invert-phase flags
    }
    int nwav = 0;
    for (int ch = 0; ch < C; ++ch) {
        TonalBand* bd = r->band[ch];
        const uint32_t skip = ch ? shared : 0u;
        if (ch) DECP_MUST(1, 0);   // envelope copy
        for (int i = 0; i < nb; ++i) {
            if ((skip >> i) & 1u) continue;
            if (b.rd(1)) bd[i].sp = (uint8_t)(b.rd(5) + 1);
            if (b.rd(1)) bd[i].ep = (uint8_t)(b.rd(5) + 1);
        }
        DECP_MUST(ch + 1, 0);      // num-waves mode
        for (int i = 0; i < nb; ++i) {
            if ((skip >> i) & 1u) continue;
            const int n = (int)b.rd(4);
            bd[i].nw = (uint8_t)n;
            bd[i].start_index = (uint8_t)(nwav < kMaxWaves ? nwav : kMaxWaves);
            nwav += n;
        }
        DECP_CHK();
        if (nwav > kMaxWaves) return kRpBadCode;
        if (ch) DECP_MUST(1, 0);   // delta to the leader
        for (int i = 0; i < nb; ++i) {
            const int n = bd[i].nw;
            if (((skip >> i) & 1u) || !n) continue;
            uint32_t* w = r->wave + bd[i].start_index;
            const int desc = n > 1 ? (int)b.rd(1) : 0;
            if (!desc) {
                uint32_t prev = b.rd(10);
                w[0] = prev;
                for (int j = 1; j < n; ++j) {
                    uint32_t cur;
                    if (prev < 512) {
                        cur = b.rd(10);
                    } else {
                        const int nbits = decp_bits_for(1023u - prev);
                        cur = b.rd(nbits) + 1024u - (1u << nbits);
                    }
                    w[j] = cur;
                    prev = cur;
                }
            } else {
                uint32_t prev = b.rd(10);
                w[n - 1] = prev;
                for (int j = n - 2; j >= 0; --j) {
                    const uint32_t cur = b.rd(decp_bits_for(prev));
                    w[j] = cur;
                    prev = cur;
                }
            }
            DECP_CHK();
        }
        DECP_MUST(ch + 1, 0);      // amplitude mode
        for (int i = 0; i < nb; ++i) {
            const int n = bd[i].nw;
            if ((skip >> i) & 1u) continue;
            for (int j = 0; j < n; ++j) r->wave[bd[i].start_index + j] |= b.rd(6) << 10;
        }
        DECP_CHK();
        for (int i = 0; i < nb; ++i) {
            const int n = bd[i].nw;
            if ((skip >> i) & 1u) continue;
            for (int j = 0; j < n; ++j) r->wave[bd[i].start_index + j] |= b.rd(5) << 16;
        }
        DECP_CHK();
    }
    if (C == 2)
        for (int i = 0; i < nb; ++i) {
            if ((shared >> i) & 1u) r->band[1][i] = r->band[0][i];
            if (leader) {
                const TonalBand t = r->band[0][i];
                r->band[0][i] = r->band[1][i];
                r->band[1][i] = t;
            }
        }
    r->present = 1;
#undef DECP_MUST
#undef DECP_CHK
    return kRpOk;
}

// The frame's syntax (include/at3phip.h, step 1) and its dequantisation (step 2) on one lane; spec (LDS) is zero on entry.
// With tonal_rec (AT3PHIP_DECODE_TONES) a tonal block is parsed into it, else it rejects the frame.
// kSparse (AT3PHIP_DECODE_SPARSE): a word length of 0 is a unit without a code-table index and without a spectrum; in channel 1 it
// carries the "copy from channel 0" flag where channel 0's unit is coded, which must be 1; the highest unit must be coded in some
// channel. A compile-time parameter: the parse is one lane's serial code and the unflagged one stays what it was.
template <bool kSparse>
__device__ __forceinline__ int decp_parse(MsbReader& b, const DecTables* T, int C, float* spec, uint8_t (*wl)[32], uint8_t (*sf)[32],
                                       uint8_t (*tab)[32], uint16_t* winf, const uint16_t* tone_vlc, TonalRec* tonal_rec)
{
    int invalid = 0;
#define DECP_CHK()                              \
    do {                                        \
        if (b.bad) return kRpReadPastEnd;       \
        if (invalid) return kRpBadCode;         \
    } while (0)
    if (b.rd(1) != 0) return kRpBadHeader;
    if ((int)b.rd(2) != C - 1) return kRpBadHeader;
    const int nqu = (int)b.rd(5) + 1;
    if (b.rd(1) != 0) return kRpUnsupported;
    {
        if (b.rd(2) != 3 || b.rd(2) != 0 || b.rd(2) != 0) return kRpUnsupported;
        const int idx = (int)b.rd(2);
        int w = (int)b.rd(3);
        wl[0][0] = (uint8_t)w;
        for (int i = 1; i < nqu; ++i) {
            w = (w + at3::prefix_scan<8>(b, T->wl_vlc[idx], invalid)) & 7;
            wl[0][i] = (uint8_t)w;
        }
        DECP_CHK();
    }
    if (C == 2) {
        if (b.rd(2) != 1 || b.rd(2) != 0) return kRpUnsupported;
        const int idx = (int)b.rd(2);
        for (int i = 0; i < nqu; ++i) wl[1][i] = (uint8_t)((wl[0][i] + at3::prefix_scan<8>(b, T->wl_vlc[idx], invalid)) & 7);
        DECP_CHK();
    }
    if constexpr (kSparse) {
        if (wl[0][nqu - 1] == 0 && wl[C - 1][nqu - 1] == 0) return kRpUnsupported;
    } else {
        for (int ch = 0; ch < C; ++ch)
            for (int i = 0; i < nqu; ++i)
                if (wl[ch][i] == 0) return kRpBadCode;
    }
    for (int ch = 0; ch < C; ++ch) {
        if (b.rd(2) != 0) return kRpUnsupported;
        for (int i = 0; i < nqu; ++i) sf[ch][i] = (uint8_t)b.rd(6);
        DECP_CHK();
    }
    const int full = (int)b.rd(1);
    for (int ch = 0; ch < C; ++ch) {
        if (b.rd(1) != 0 || b.rd(2) != 0 || b.rd(1) != 0) return kRpUnsupported;
        if constexpr (kSparse) {
            for (int i = 0; i < nqu; ++i) {
                if (wl[ch][i]) {
                    tab[ch][i] = (uint8_t)b.rd(full + 2);
                } else if (ch && wl[0][i]) {
                    const uint32_t keep = b.rd(1);
                    DECP_CHK();
                    if (keep != 1) return kRpUnsupported;
                }
            }
        } else {
            for (int i = 0; i < nqu; ++i) tab[ch][i] = (uint8_t)b.rd(full + 2);
        }
        DECP_CHK();
    }
    for (int ch = 0; ch < C; ++ch) {
        float* sp = spec + 2048 * ch;
        for (int qu = 0; qu < nqu; ++qu) {
            if constexpr (kSparse) {
                if (wl[ch][qu] == 0) continue;   // the unit's lines stay +0.0f
            }
            const int w = wl[ch][qu], t = w - 1 + 7 * tab[ch][qu];
            const int gsz = T->spec_tab[t][0] & 15, nc = T->spec_tab[t][0] >> 4;
            const int cbits = T->spec_tab[t][1] & 15, is_signed = T->spec_tab[t][1] >> 4;
            const float mant = T->mant[w], scale = T->scale[sf[ch][qu]];
            const int start = at3p_qu_start(qu), n = at3p_qu_start(qu + 1) - start;
            for (int pos = 0; pos < n;) {
                if (gsz != 1 && b.rd(1) == 0) {
                    DECP_CHK();
                    pos += gsz * nc;
                    continue;
                }
                for (int j = 0; j < gsz; ++j) {
                    const int val = decp_spec_vlc(b, T, t, invalid);
                    DECP_CHK();
                    for (int i = 0; i < nc; ++i, ++pos) {
                        int m = (val >> (cbits * i)) & ((1 << cbits) - 1);
                        if (is_signed) {
                            m = at3::sext((uint32_t)m, cbits);
                        } else if (m != 0 && b.rd(1)) {
                            m = -m;
                        }
                        DECP_CHK();
                        sp[start + pos] = (float)m * mant * scale;
                    }
                }
            }
        }
        const int npw = T->sb_powgrps[T->qu_to_sb[nqu - 1]];
        for (int i = 0; i < npw; ++i) {
            const uint32_t lev = b.rd(4);
            DECP_CHK();
            if (lev != 15) return kRpUnsupported;
        }
    }
    if (C == 2) {
        const uint32_t sn = b.rd(2);
        DECP_CHK();
        if (sn != 0) return kRpUnsupported;
    }
    const int sb_bits = T->qu_to_sb[31] + 1;
    for (int ch = 0; ch < C; ++ch) {
        uint32_t w = 0;
        if (b.rd(1)) {
            if (b.rd(1) == 0) {
                w = 0xffffu;
            } else {
                for (int i = 0; i < sb_bits; ++i) w |= b.rd(1) << i;
            }
        }
        DECP_CHK();
        winf[ch] = (uint16_t)w;
    }
    for (int ch = 0; ch < C; ++ch) {
        const uint32_t g = b.rd(1);
        DECP_CHK();
        if (g) return kRpUnsupported;
    }
    const uint32_t tonal = b.rd(1);
    DECP_CHK();
    if (tonal) {
        if (!tonal_rec) return kRpTonal;
        const int why = decp_tonal(b, tone_vlc, C, tonal_rec);
        if (why) return why;
    }
    const uint32_t noise = b.rd(1);
    DECP_CHK();
    if (noise) return kRpUnsupported;
    const uint32_t term = b.rd(2);
    DECP_CHK();
    if (term != 3) return kRpNoTerminator;
#undef DECP_CHK
    return kRpOk;
}

constexpr int kDecUnpackThreads = 64;   // one wavefront per frame: the parse is one lane, so frames in flight per CU count

// k_at3pd_unpack_with<kSized> and, for AT3PHIP_DECODE_SPARSE, k_at3pd_unpack_sparse_with<kSized>: one body, two parses
#define DECP_UNPACK_KERNEL k_at3pd_unpack_with
#define DECP_UNPACK_SPARSE false
#include "at3p_decode_unpack.inc"
#undef DECP_UNPACK_KERNEL
#undef DECP_UNPACK_SPARSE
#define DECP_UNPACK_KERNEL k_at3pd_unpack_sparse_with
#define DECP_UNPACK_SPARSE true
#include "at3p_decode_unpack.inc"
#undef DECP_UNPACK_KERNEL
#undef DECP_UNPACK_SPARSE

// (the instantiations are named where they are launched, at3phip.hip and at3p_sparse.hip: naming one instantiates it, and a
// translation unit must hold only its own)

// at3p_sparse.hip needs the unpack kernel alone: what follows are kernels that are no templates and belong to one translation unit.
#ifndef AT3P_DECODE_UNPACK_ONLY

struct DecSynthParams {
    const DecTables* T;
    const float* raw;
    const uint16_t* flags;
    void* out;                    // [S][F][2048][C] float or int16
    int32_t n_frames, n_streams, nch, s16;
    const TonalRec* tonal;        // as DecUnpackParams::tonal
    const DecToneTables* TT;
    int32_t tones;                // step 4b
};

// ---- step 4b: ff_atrac3p_generate_tones for the band of frame k, tones_info = record k, tones_info_prev = record k-1 ----------
// What generate_tones does for the band of frame k (DecpToneJob, decp_curr_env and decp_waves: at3p_tone_synth.hpp)
__device__ __forceinline__ DecpToneJob decp_tone_job(const TonalRec* rk, const TonalRec* rk1, const TonalRec* rk2, int ch, int b)
{
    return decp_tone_job(rk->band[ch][b], rk1->band[ch][b], rk2->band[ch][b], rk->present || rk1->present);
}

constexpr int kDecHist = 23;              // frame n-1's DCT-IV columns the FIR reaches
constexpr int kDecCols = 128 + kDecHist;

// the windowed first half (x = inv[j]) and second half (y = inv[128 + j]) of TAt3pMIDCT::Do, flags `fl` of subband b
__device__ __forceinline__ float decp_win_first(const DecTables* T, float x, uint32_t fl, int b, int j)
{
    if ((fl >> b) & 1u) return j < 32 ? 0.0f : j < 96 ? x * T->sine64[j - 32] : x * 2.0f;
    return x * T->sine128[j];
}
__device__ __forceinline__ float decp_win_second(const DecTables* T, float y, uint32_t fl, int b, int j)
{
    if ((fl >> b) & 1u) return j < 32 ? y * 2.0f : j < 96 ? y * T->sine64[95 - j] : 0.0f;
    return y * T->sine128[127 - j];
}

__global__ __launch_bounds__(256) void k_at3pd_synth(DecSynthParams p)
{
    __shared__ float s_x[16][kDecCols + 1];   // rescaled subband samples: column c = frame n-1's sample 105 + c (c < 23), else frame n's c - 23
    __shared__ float s_d[kDecCols][16];       // the DCT-IV outputs per column (idct_out)
    __shared__ float s_fir[384];

    const DecTables* T = p.T;
    const int f = blockIdx.x, sc = blockIdx.y, tid = threadIdx.x, C = p.nch, S = p.n_streams;
    const int s = sc / C, ch = sc - s * C;
    const uint32_t fl2 = p.flags[decp_rec(f, s, ch, S, C)];       // frame n-2
    const uint32_t fl1 = p.flags[decp_rec(f + 1, s, ch, S, C)];   // frame n-1
    const float* r0 = p.raw + decp_rec(f, s, ch, S, C) * 4096;
    const float* r1 = p.raw + decp_rec(f + 1, s, ch, S, C) * 4096;
    const float* r2 = p.raw + decp_rec(f + 2, s, ch, S, C) * 4096;
    for (int i = tid; i < 384; i += 256) s_fir[i] = T->fir[i];
    const float rescale = (float)(32768.0 / 1.122018);
    for (int i = tid; i < 16 * kDecCols; i += 256) {
        const int b = i / kDecCols, c = i - b * kDecCols;
        float v;
        if (c < kDecHist) {
            const int j = 128 - kDecHist + c;
            v = decp_win_first(T, r1[b * 256 + j], fl2, b, j) + decp_win_second(T, r0[b * 256 + 128 + j], fl2, b, j);
        } else {
            const int j = c - kDecHist;
            v = decp_win_first(T, r2[b * 256 + j], fl1, b, j) + decp_win_second(T, r1[b * 256 + 128 + j], fl1, b, j);
        }
        s_x[b][c] = v * rescale;
    }
    if (p.tones) {   // step 4b for frame n (role 0) and for frame n-1's last 23 samples (role 1)
        __shared__ DecpToneJob s_job[2][16];
        __shared__ uint32_t s_wave[3][kMaxWaves];   // the waves of records n, n-1, n-2
        const DecToneTables* TT = p.TT;
        if (tid < 32) {
            const int role = tid >> 4, b = tid & 15;
            s_job[role][b] = decp_tone_job(decp_tonal_rec(p.tonal, f - role, s, S), decp_tonal_rec(p.tonal, f - 1 - role, s, S),
                                           decp_tonal_rec(p.tonal, f - 2 - role, s, S), ch, b);
        }
        for (int i = tid; i < 3 * kMaxWaves; i += 256) {
            const int d = i / kMaxWaves;
            s_wave[d][i - d * kMaxWaves] = decp_tonal_rec(p.tonal, f - d, s, S)->wave[i - d * kMaxWaves];
        }
        __syncthreads();
        for (int i = tid; i < 16 * kDecCols; i += 256) {
            const int b = i / kDecCols, c = i - b * kDecCols;
            const int role = c < kDecHist ? 1 : 0, j = c < kDecHist ? 128 - kDecHist + c : c - kDecHist;
            const DecpToneJob& J = s_job[role][b];
            if (!J.active) continue;
            float w1 = J.n1 ? decp_waves(TT, &s_wave[role + 1][J.i1], J.n1, J.e1, 128, j) : 0.0f;
            float w2 = J.n2 ? decp_waves(TT, &s_wave[role][J.i2], J.n2, J.e2, 0, j) : 0.0f;
            if (J.h1) w1 = w1 * TT->hann[128 + j];
            if (J.h2) w2 = w2 * TT->hann[j];
            const float g = 0.0f - (w1 + w2);
            s_x[b][c] = s_x[b][c] - g;
        }
    }
    __syncthreads();
    // dct4: out[15 - k] = (float)(sum_n (double)x[n] * cos16[k][n] * (1.0 / 1024)), the sum in order, each step rounded
    {
        const int k = tid & 15;
        double cr[16];
#pragma unroll
        for (int n = 0; n < 16; ++n) cr[n] = T->cos16[k][n];
        for (int c = tid >> 4; c < kDecCols; c += 16) {
            double sum = 0.0;
#pragma unroll
            for (int n = 0; n < 16; ++n) sum += (double)s_x[n][c] * cr[n];
            s_d[c][15 - k] = (float)(sum * (1.0 / 1024));
        }
    }
    __syncthreads();
    // the FIR: output o = 16 s + i sums 12 taps over the columns 2t and 2t + 1 back, from +0.0f, in tap order
    const size_t F = p.n_frames;
    for (int o = tid; o < 2048; o += 256) {
        const int sm = o >> 4, i = o & 15, cs = sm + kDecHist;
        float acc = 0.0f;
        if (i < 8) {
#pragma unroll
            for (int t = 0; t < 12; ++t) {
                const float a = s_d[cs - 2 * t][i + 8] * s_fir[12 * i + t];
                const float d = s_d[cs - 2 * t - 1][7 - i] * s_fir[192 + 12 * i + t];
                acc = acc + (a + d);
            }
        } else {
            const int ii = i - 8;
#pragma unroll
            for (int t = 0; t < 12; ++t) {
                const float e = s_d[cs - 2 * t][15 - ii] * s_fir[12 * i + t];
                const float g = s_d[cs - 2 * t - 1][ii] * s_fir[192 + 12 * i + t];
                acc = acc + (e + g);
            }
        }
        at3::store_pcm(p.out, (((size_t)s * F + f) * 2048 + o) * C + ch, acc, p.s16);
    }
}

// The call's last two frames (slots F, F + 1) become slots 0 and 1 of the next call, and its last three tonal records (slots F ..
// F + 2) slots 0 .. 2.
__global__ __launch_bounds__(256) void k_at3pd_state(float* raw, uint16_t* flags, TonalRec* tonal, int32_t n_frames, int32_t n_streams,
                                                     int32_t nch)
{
    __shared__ float s_raw[2][4096];
    __shared__ uint16_t s_fl[2];
    __shared__ uint32_t s_tone[kTonalCarry][kTonalWords];
    const int sc = blockIdx.x, s = sc / nch, ch = sc - s * nch, tid = threadIdx.x;
    for (int i = tid; i < 8192; i += 256) s_raw[i >> 12][i & 4095] = raw[decp_rec(n_frames + (i >> 12), s, ch, n_streams, nch) * 4096 + (i & 4095)];
    if (tid < 2) s_fl[tid] = flags[decp_rec(n_frames + tid, s, ch, n_streams, nch)];
    if (ch == 0)
        for (int i = tid; i < kTonalCarry * kTonalWords; i += 256) {
            const int k = i / kTonalWords;
            s_tone[k][i - k * kTonalWords] = ((const uint32_t*)decp_tonal_rec(tonal, n_frames - kTonalCarry + k, s, n_streams))[i - k * kTonalWords];
        }
    __syncthreads();
    for (int i = tid; i < 8192; i += 256) raw[decp_rec(i >> 12, s, ch, n_streams, nch) * 4096 + (i & 4095)] = s_raw[i >> 12][i & 4095];
    if (tid < 2) flags[decp_rec(tid, s, ch, n_streams, nch)] = s_fl[tid];
    if (ch == 0)
        for (int i = tid; i < kTonalCarry * kTonalWords; i += 256) {
            const int k = i / kTonalWords;
            ((uint32_t*)decp_tonal_rec(tonal, k - kTonalCarry, s, n_streams))[i - k * kTonalWords] = s_tone[k][i - k * kTonalWords];
        }
}

#endif  // AT3P_DECODE_UNPACK_ONLY

}  // namespace at3p
