// ATRAC3plus frame writer with adaptive word lengths (gfx950): include/at3phip.h, ADAPTIVE WORD LENGTHS, steps A1-A6.
//   k_at3p_write_adaptive        the fixed writer's scaler and quantiser (at3p_write.hpp), then per frame the cost table of
//                                every (channel, unit, word length), the two full scans over the candidate allocations and the
//                                frame in the fixed writer's layout, one (stream, frame) per workgroup;
//   k_at3p_write_adaptive_tonal  the same with a record per frame, whose block counts in every candidate's bits.
// The word lengths are no longer the reference's table, so the word-length section (TWordLenEncoder, at3p_bitstream.cpp:
// 170-252) is priced and written here and WriteTables::head is not used. Spectra, tail and tonal block go through the fixed
// writer's emit_chunk, tonal_price and tonal_emit. host_allocate is steps A3-A5 on the host (at3phip_host_allocate), host_allocate_rd
// R2-R4 and, with offsets, M4-M6 (at3phip_host_allocate_rd, at3phip_host_allocate_psy).
//   k_at3p_write_adaptive_sparse, k_at3p_write_adaptive_tonal_sparse  the same two with SPARSE WORD LENGTHS (A3s, A4s, A6s): a unit
//                                inside the coded range may keep word length 0, and then has no code-table index and no spectrum.
//                                Instantiations of their own in a translation unit of their own, at3p_sparse.hip: next to the two
//                                above they change how the compiler inlines the device functions all four share, and with that
//                                the code of the two above.
//   k_at3p_write_adaptive_with<WriteParamsRd>, <WriteParamsTonalRd>  the sparse two with RATE-DISTORTION WORD LENGTHS (R1-R5): a distortion
//                                table beside the cost table, every unit's pick per lambda, the scans over j and k beside those over
//                                t and k, and the guard that keeps the sparse allocation where it has less distortion. at3p_rd.hpp
//                                holds their arithmetic, at3p_rd.hip instantiates them, for the same reason.
//   k_at3p_write_adaptive_with<WriteParamsPsy>, <WriteParamsTonalPsy>  the rate-distortion two with MASKING-WEIGHTED WORD LENGTHS (M1-M7):
//                                a masking threshold per unit from the distortion table's first column, its offset to the frame's
//                                lowest as a shift of lambda in the unit's picks, up to 32 more values of j, and the guard's sums
//                                weighted. at3p_psy.hpp holds their arithmetic and tables, at3p_psy.hip instantiates them.
#pragma once
#include <cstring>
#include <type_traits>

#include "at3p_write.hpp"
#include "at3p_rd.hpp"
#include "at3p_psy.hpp"

namespace at3p {

constexpr int kAllocTMin = -21, kAllocTMax = 63, kAllocKMax = 64;

// A3: clamp(floor((sfi - t) / 3), 0, 7)
__host__ __device__ inline int alloc_want(int sfi, int t)
{
    const int d = sfi - t;
    return d <= 0 ? 0 : d >= 21 ? 7 : d / 3;
}
// FindBestWlDeltaEncode's range for an OR-accumulated largest delta: first table | last table << 2
__host__ __device__ inline int alloc_wl_range(int max_delta) { return max_delta >= 3 ? (2 | 3 << 2) : max_delta == 2 ? (1 | 1 << 2) : 0; }

// ---- host: Bits(A) of A4 / A4s for word lengths wl (0 at and above N), and A3s's closing rules --------------------------------
inline int host_alloc_bits(const int (&wl)[2][32], int N, const uint16_t* bits, int channels, int tail_bits)
{
    long total = 6 + tail_bits + channels * (2 + 6 * N) + 1 + channels * (4 + 3 * N) + channels * 4 * AT3P_SB_POWGRPS[AT3P_QU_TO_SB[N - 1]];
    for (int ch = 0; ch < channels; ++ch) {
        // (FindBestWlDeltaEncode sums from the list's second entry in both modes: channel 1's first code counts in the
        // largest delta and in the bits, not in the choice of the table)
        int len[4] = {0, 0, 0, 0}, mx = 0;
        for (int qu = ch ? 0 : 1; qu < N; ++qu) {
            const int d = wl[ch][qu] - (ch ? wl[0][qu] : wl[0][qu - 1]);
            mx |= d < 0 ? -d : d;
            if (qu)
                for (int i = 0; i < 4; ++i) len[i] += AT3P_WL_VLC[i][d & 7] >> 12;
        }
        const int r = alloc_wl_range(mx), a = r & 3, b = r >> 2, idx = len[b] < len[a] ? b : a;
        total += (ch ? 6 + (AT3P_WL_VLC[idx][(wl[1][0] - wl[0][0]) & 7] >> 12) : 11) + len[idx];
        for (int qu = 0; qu < N; ++qu) {
            if (wl[ch][qu]) total += bits[(ch * 32 + qu) * 8 + wl[ch][qu]];
            else total -= (ch && wl[0][qu]) ? 2 : 3;   // A4s (A3 leaves no 0 below N): no index; channel 1's clone flag
        }
    }
    return total > 0x7fffffffl ? 0x7fffffff : (int)total;
}
// A3s: N after the raise, the empty frame, the step from 29..31 to 32; top: the highest unit with a non-zero word length, or -1
inline int host_sparse_close(int (&wl)[2][32], int top)
{
    int N = top + 1;
    if (N == 0) {
        N = 1;
        wl[0][0] = 1;
    }
    if (N >= 29 && N <= 31) {   // (unit 31 then has 0 in every channel)
        N = 32;
        wl[0][31] = 1;
    }
    return N;
}

// A3s's walk, which R2 and M4 share: every unit has a pair (w0, up), given by pair(ch, qu, &w0, &up); the first k units whose up exceeds
// their w0 take it; then A3s's closing rules. Returns N; took: the units that took their up.
template <typename Pair>
inline int host_sparse_walk(int (&wl)[2][32], int channels, int k, int* took, Pair pair)
{
    int top = -1;
    *took = 0;
    for (int qu = 0, left = k; qu < 32; ++qu)
        for (int ch = 0; ch < channels; ++ch) {
            int w0 = 0, up = 0;
            pair(ch, qu, &w0, &up);
            wl[ch][qu] = w0;
            if (left > 0 && up > w0) {
                wl[ch][qu] = up;
                --left;
                ++*took;
            }
            if (wl[ch][qu]) top = qu;
        }
    return host_sparse_close(wl, top);
}
// The two scans of A4 and A5 (R3, M5): the smallest first parameter in lo..hi whose candidate fits with k = 0 (hi where none does: a
// caller's table only), then the largest k that fits. fits(p, k) forms the candidate and tells; (p*, k*) is left formed.
template <typename Fits>
inline void host_scan(int lo, int hi, int* p_star, Fits fits)
{
    int ps = hi, ks = 0;
    for (int p = hi; p >= lo; --p)
        if (fits(p, 0)) ps = p;
    for (int k = 0; k <= kAllocKMax; ++k)
        if (fits(ps, k)) ks = k;
    fits(ps, ks);
    *p_star = ps;
}

// ---- host: steps A3-A5 on a cost table ---------------------------------------------------------------------------------
// sfi [channels][32], bits [channels][32][8] (entry w = the unit's bits at word length w, entry 0 unused) -> wl [channels][32]
// (0 at and above N), N, t*, k*; returns Bits(A(t*, k*)). size_bits: the budget of A4, 8 * frame_bytes - 3. sparse: A3s and A4s.
inline int host_allocate(const uint8_t* sfi, const uint16_t* bits, int channels, int tail_bits, int size_bits, uint8_t* wl_out, int* n_units, int* t_out,
                         int* k_out, bool sparse = false)
{
    int wl[2][32] = {};
    int N = 1, took = 0;
    auto form_dense = [&](int t, int k) {   // A(t, k) into wl and N; took: the units that took the t - 1 value
        int top = -1;
        for (int qu = 0; qu < 32; ++qu)
            for (int ch = 0; ch < channels; ++ch) {
                wl[ch][qu] = alloc_want(sfi[ch * 32 + qu], t);
                if (wl[ch][qu]) top = qu;
            }
        N = top < 0 ? 1 : top + 1;
        if (N >= 29 && N <= 31) N = 32;
        took = 0;
        for (int qu = 0, left = k; qu < 32; ++qu)
            for (int ch = 0; ch < channels; ++ch) {
                if (qu >= N) {
                    wl[ch][qu] = 0;
                    continue;
                }
                const int up = alloc_want(sfi[ch * 32 + qu], t - 1);
                if (left > 0 && up > wl[ch][qu]) {
                    wl[ch][qu] = up;
                    --left;
                    ++took;
                }
                if (wl[ch][qu] == 0) wl[ch][qu] = 1;
            }
    };
    auto count = [&]() { return host_alloc_bits(wl, N, bits, channels, tail_bits); };   // Bits(A)
    int ts = 0;
    host_scan(kAllocTMin, kAllocTMax, &ts, [&](int t, int k) {
        if (!sparse) form_dense(t, k);
        else   // A3s: every unit is walked, nothing is raised from 0 to 1, N follows the raise
            N = host_sparse_walk(wl, channels, k, &took, [&](int ch, int qu, int* w0, int* up) {
                *w0 = alloc_want(sfi[ch * 32 + qu], t);
                *up = alloc_want(sfi[ch * 32 + qu], t - 1);
            });
        return count() <= size_bits;
    });
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu) wl_out[ch * 32 + qu] = (uint8_t)wl[ch][qu];
    *n_units = N;
    *t_out = ts;
    *k_out = took;   // k* as reported: a k beyond the units that can take the t - 1 value gives the same allocation
    return count();
}

// ---- host: R2-R4 and, with offsets, M4-M6 on a cost table and a distortion table ------------------------------------------------
// dist: S [channels][32][8]. o: null for RATE-DISTORTION WORD LENGTHS, or M3's offsets for MASKING-WEIGHTED WORD LENGTHS, which are
// the same with lambda shifted per unit, the scan reaching down by the largest offset and the guard's sums weighted. Returns Bits of
// the allocation written; chose: 1 = R(j*, k*) or P(j*, k*), 0 = the sparse allocation A(t*, k*).
inline int host_allocate_rd(const uint8_t* sfi, const uint16_t* bits, const uint64_t* dist, const int (*o)[32], int channels, int tail_bits,
                            int size_bits, uint8_t* wl_out, int* n_units, int* j_out, int* k_out, int* chose)
{
    double D[2][32][8] = {};
    uint16_t B[2][32][8] = {};
    int O = 0;
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu) {
            for (int w = 0; w < 8; ++w) {
                D[ch][qu][w] = rd_d(dist[(ch * 32 + qu) * 8 + w], rd_g(AT3P_SCALE[sfi[ch * 32 + qu]]));
                B[ch][qu][w] = w ? bits[(ch * 32 + qu) * 8 + w] : 0;   // (entry 0 is not read)
            }
            if (o && o[ch][qu] > O) O = o[ch][qu];
        }
    int wl[2][32] = {};
    int N = 1, took = 0, js = 0;
    auto count = [&]() { return host_alloc_bits(wl, N, bits, channels, tail_bits); };
    host_scan(kRdJMin - O, kRdJMax, &js, [&](int j, int k) {   // R3, M5; R(j, k) or P(j, k) into wl and N
        N = host_sparse_walk(wl, channels, k, &took, [&](int ch, int qu, int* w0, int* up) {
            const int shift = o ? o[ch][qu] : 0;
            *w0 = rd_pick(D[ch][qu], B[ch][qu], rd_lambda(j + shift, AT3P_SCALE));
            *up = rd_pick(D[ch][qu], B[ch][qu], rd_lambda(j - 1 + shift, AT3P_SCALE));
        });
        return count() <= size_bits;
    });
    // R4, M6: against the sparse allocation A(t*, k*)
    uint8_t wl_a[64] = {};
    int n_a = 0, t_a = 0, k_a = 0;
    const int bits_a = host_allocate(sfi, bits, channels, tail_bits, size_bits, wl_a, &n_a, &t_a, &k_a, true);
    double sum_r = 0.0, sum_a = 0.0;
    for (int qu = 0; qu < 32; ++qu)
        for (int ch = 0; ch < channels; ++ch) {
            double d_r = D[ch][qu][wl[ch][qu]], d_a = D[ch][qu][wl_a[ch * 32 + qu]];
            if (o) {   // M6's weight G[63 - o]. Without offsets it would be G[63], exactly 1.0 (ScaleTable[63] is 2^0): R4's sums as written
                const double g = rd_g(AT3P_SCALE[63 - o[ch][qu]]);
                d_r *= g;
                d_a *= g;
            }
            sum_r += d_r;
            sum_a += d_a;
        }
    *j_out = js;
    *k_out = took;   // k* as reported (A5)
    *chose = sum_r <= sum_a;
    if (*chose) {
        for (int ch = 0; ch < channels; ++ch)
            for (int qu = 0; qu < 32; ++qu) wl_out[ch * 32 + qu] = (uint8_t)wl[ch][qu];
        *n_units = N;
        return count();
    }
    memcpy(wl_out, wl_a, (size_t)channels * 32);
    *n_units = n_a;
    return bits_a;
}

// The argument checks every host allocator of include/at3phip.h makes (t: the scan's first result, t* or j*)
inline int host_allocate_args(const uint8_t* sfi, const uint16_t* bits, int32_t channels, int32_t tail_bits, int32_t frame_bytes, const uint8_t* wl_out,
                              const int32_t* n_units, const int32_t* t, const int32_t* k)
{
    if (!sfi || !bits || !wl_out || !n_units || !t || !k || channels < 1 || channels > 2) return AT3HIP_EINVAL;
    if (!admissible_frame_bytes(frame_bytes, channels)) return AT3HIP_EINVAL;
    if (tail_bits < 0 || tail_bits > 8 * frame_bytes - 3) return AT3HIP_EINVAL;
    for (int i = 0; i < 32 * channels; ++i)
        if (sfi[i] > 63) return AT3HIP_EINVAL;
    return AT3HIP_OK;
}
// and those of the two that take a distortion table: the above, dist, the guard's outcome, and S's bound
inline int host_allocate_rd_args(const uint8_t* sfi, const uint16_t* bits, const uint64_t* dist, int32_t channels, int32_t tail_bits, int32_t frame_bytes,
                                 const uint8_t* wl_out, const int32_t* n_units, const int32_t* j, const int32_t* k, const int32_t* chose)
{
    if (!dist || !chose) return AT3HIP_EINVAL;
    if (const int rc = host_allocate_args(sfi, bits, channels, tail_bits, frame_bytes, wl_out, n_units, j, k)) return rc;
    for (int i = 0; i < 256 * channels; ++i)
        if (dist[i] > (1ull << 47)) return AT3HIP_EINVAL;   // 128 lines of at most 2^40 each
    return AT3HIP_OK;
}

// at3phip_host_allocate_sized and at3phip_host_allocate_sparse: the arguments' checks, then host_allocate
inline int host_allocate_checked(const uint8_t* sfi, const uint16_t* bits, int32_t channels, int32_t tail_bits, int32_t frame_bytes, uint8_t* wl_out,
                                 int32_t* n_units, int32_t* t, int32_t* k, bool sparse)
{
    if (const int rc = host_allocate_args(sfi, bits, channels, tail_bits, frame_bytes, wl_out, n_units, t, k)) return rc;
    int n = 0, ts = 0, ks = 0;
    host_allocate(sfi, bits, channels, tail_bits, 8 * frame_bytes - 3, wl_out, &n, &ts, &ks, sparse);
    *n_units = n;
    *t = ts;
    *k = ks;
    return AT3HIP_OK;
}

// ---- device ----------------------------------------------------------------------------------------------------------
// The fixed writer's parameters and the word-length code tables (code | length << 12 per delta & 7), which the fixed writer
// only needs on the host: nothing is allocated or uploaded for the adaptive path.
template <typename P>
struct AdaptiveParams : P {
    uint16_t wl_vlc[4][8];
    int32_t frame_bytes;   // a multiple of 8 in AT3PHIP_MIN_FRAME_BYTES_* .. 2048: P::out is [items][frame_bytes]
};

// TUnit::GetOrCompute's pricing of one 16-line chunk under one code table, as k_at3p_write_with has it: the symbols are formed
// once per packing and only looked up per table.
struct ChunkPricer {
    uint32_t vals[16];
    uint32_t prev_packing;
    int n_signs;
    __device__ __forceinline__ void reset()
    {
        prev_packing = 0xffffffffu;
        n_signs = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) vals[k] = 0u;
    }
    __device__ __forceinline__ int price(const int (&q)[16], uint32_t d, const uint32_t* len4)
    {
        const int off = (int)(d & 0xffffu), group_size = (int)((d >> 16) & 15u), num_coeffs = (int)((d >> 20) & 15u);
        if ((d >> 20) != prev_packing) {   // num_coeffs, bits, is_signed
            prev_packing = d >> 20;
            const int cbits = (int)((d >> 24) & 15u), is_signed = (int)(d >> 28);
            if (num_coeffs == 1) n_signs = pack_symbols<1>(q, cbits, is_signed, vals);
            else if (num_coeffs == 2) n_signs = pack_symbols<2>(q, cbits, is_signed, vals);
            else n_signs = pack_symbols<4>(q, cbits, is_signed, vals);
        }
        const int n_sym = 16 / num_coeffs;
        int bits = n_signs + (group_size != 1 ? n_sym / group_size : 0);   // one flag bit per group
        auto len_of = [&](int sidx) {
            const int e = off + (int)vals[sidx];
            return (int)((len4[e >> 3] >> (4 * (e & 7))) & 15u);
        };
#pragma unroll
        for (int sidx = 0; sidx < 4; ++sidx) bits += len_of(sidx);
        if (num_coeffs <= 2) {
#pragma unroll
            for (int sidx = 4; sidx < 8; ++sidx) bits += len_of(sidx);
            if (num_coeffs == 1) {
#pragma unroll
                for (int sidx = 8; sidx < 16; ++sidx) bits += len_of(sidx);
            }
        }
        return bits;
    }
};

// QuantMantisas without the energy pass (atrac_scale.cpp:46-54): the multiplication and the rounding of the fixed writer
__device__ __forceinline__ void alloc_quantise(const float (&v)[16], float mul, int (&q)[16])
{
#pragma unroll
    for (int k = 0; k < 16; ++k) q[k] = __float2int_rn(v[k] * mul);
}

__device__ __forceinline__ int alloc_wave_sum(int v, int lane) { return __builtin_amdgcn_readlane(at3::wave_inclusive_scan(v, lane), 63); }

// One candidate A(t, k) on a wavefront, lane = 2 * unit + channel (the order of A3's walk). Wave-uniform: N, the two code
// tables, the section's VLC bits per channel and Bits(A); per lane: the word length and its VLC under its channel's table.
struct AllocEval {
    int wl, N, idx0, idx1, sum0, sum1, total;
    int delta, len;       // the lane's delta & 7 and its code's length (0: the lane writes no code)
};
// kSparse: A3s and A4s (SPARSE WORD LENGTHS). The "up" ballot is over all active lanes, N is the highest lane whose word length is
// non-zero after the raise, lane 0 (unit 0 of channel 0) carries the empty frame and lane 62 (unit 31 of channel 0) the step from
// 29..31 to 32; the code-table section counts 3 bits per non-zero unit and a clone flag per odd lane with 0 whose even neighbour is
// non-zero. s_B[..][0] must read as 0.
// alloc_eval_from: the candidate from the lane's two word lengths, w0 the one every unit takes and w1 the one the first k units take
// whose w1 exceeds their w0 (A3's wants at t and t - 1; RATE-DISTORTION WORD LENGTHS' picks at j and j - 1, at3p_rd.hpp).
template <bool kSparse>
__device__ __forceinline__ AllocEval alloc_eval_from(int w0, int w1, int k, bool act, int lane, int nch, const uint16_t* s_B, const uint16_t* s_wlv,
                                                     const uint8_t* s_pw, int tail_bits)
{
    AllocEval r;
    const int qu = lane >> 1, ch = lane & 1;
    int N, wl, ct_less = 0;   // ct_less: what the code-table section has less than 3 bits per unit below N
    bool below;
    if constexpr (kSparse) {
        const bool up = act && w1 > w0;
        const unsigned long long upm = __ballot(up);
        const int rank = __builtin_popcountll(upm & ((1ull << lane) - 1ull));
        wl = !act ? 0 : (up && rank < k) ? w1 : w0;
        const unsigned long long has = __ballot(wl >= 1);
        N = has ? ((63 - __builtin_clzll(has)) >> 1) + 1 : 1;
        if (!has && lane == 0) wl = 1;
        if (N >= 29 && N <= 31) {   // the syntax has no 29..31; unit 31 then has 0 in every channel
            N = 32;
            if (lane == 62) wl = 1;
        }
        below = act && qu < N;
        const unsigned long long nz = __ballot(wl >= 1), zero = __ballot(below && wl == 0);
        const unsigned long long clone = zero & (nz << 1) & 0xaaaaaaaaaaaaaaaaull;
        ct_less = 3 * __builtin_popcountll(zero) - __builtin_popcountll(clone);
    } else {
        const unsigned long long has = __ballot(act && w0 >= 1);
        N = has ? ((63 - __builtin_clzll(has)) >> 1) + 1 : 1;
        if (N >= 29 && N <= 31) N = 32;   // the syntax has no 29..31
        below = act && qu < N;
        const bool up = below && w1 > w0;
        const unsigned long long upm = __ballot(up);
        const int rank = __builtin_popcountll(upm & ((1ull << lane) - 1ull));
        wl = (up && rank < k) ? w1 : w0;
        if (wl == 0) wl = 1;
        if (!below) wl = 0;
    }
    // TWordLenEncoder: channel 0 against the previous unit (two lanes down), channel 1 against channel 0 (one lane down)
    const int src = lane - (ch ? 1 : 2);
    const int ref = __builtin_amdgcn_ds_bpermute(4 * (src < 0 ? 0 : src), wl);
    const bool coded = below && (ch == 1 || qu >= 1);
    const int d = coded ? wl - ref : 0, ad = d < 0 ? -d : d;
    int m0 = 0, m1 = 0;   // the OR-accumulated largest deltas
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const unsigned long long bm = __ballot(coded && ((ad >> b) & 1));
        if (bm & 0x5555555555555555ull) m0 |= 1 << b;
        if (bm & 0xaaaaaaaaaaaaaaaaull) m1 |= 1 << b;
    }
    const int r0 = alloc_wl_range(m0), r1 = alloc_wl_range(m1);
    const int ta = ch ? (r1 & 3) : (r0 & 3), tb = ch ? (r1 >> 2) : (r0 >> 2);
    const int la = coded ? (int)(s_wlv[ta * 8 + (d & 7)] >> 12) : 0, lb = coded ? (int)(s_wlv[tb * 8 + (d & 7)] >> 12) : 0;
    // one sum for the four lists: a code has at most 5 bits and a list at most 32 codes, so 8 bits each
    // (FindBestWlDeltaEncode sums from the list's second entry in both modes: channel 1's first code, lane 1's, counts in the
    // largest delta and in the bits, not in the choice of the table)
    const uint32_t sums = (uint32_t)alloc_wave_sum(qu >= 1 ? (la | (lb << 8)) << (16 * ch) : 0, lane);
    const int s0a = (int)(sums & 0xffu), s0b = (int)((sums >> 8) & 0xffu), s1a = (int)((sums >> 16) & 0xffu), s1b = (int)(sums >> 24);
    r.idx0 = s0b < s0a ? (r0 >> 2) : (r0 & 3);   // the first table with the fewest bits
    r.idx1 = s1b < s1a ? (r1 >> 2) : (r1 & 3);
    r.sum0 = s0b < s0a ? s0b : s0a;
    r.len = ch ? (s1b < s1a ? lb : la) : (s0b < s0a ? lb : la);
    r.sum1 = (s1b < s1a ? s1b : s1a) + __builtin_amdgcn_readlane(r.len, 1);
    const int bsum = alloc_wave_sum(below ? (int)s_B[(ch * 32 + qu) * 8 + wl] : 0, lane);
    r.total = 6 + 11 + r.sum0 + (nch == 2 ? 6 + r.sum1 : 0) + nch * (2 + 6 * N) + 1 + nch * (4 + 3 * N) + bsum + nch * (int)s_pw[N - 1] + tail_bits;
    if constexpr (kSparse) r.total -= ct_less;
    r.wl = wl;
    r.N = N;
    r.delta = d & 7;
    return r;
}
template <bool kSparse>
__device__ __forceinline__ AllocEval alloc_eval(int t, int k, int sfi, bool act, int lane, int nch, const uint16_t* s_B, const uint16_t* s_wlv,
                                                const uint8_t* s_pw, int tail_bits)
{
    return alloc_eval_from<kSparse>(alloc_want(sfi, t), alloc_want(sfi, t - 1), k, act, lane, nch, s_B, s_wlv, s_pw, tail_bits);
}

// the parameter types of the sparse instantiations: the fixed writer's, marked
struct WriteParamsSparse : WriteParams {};
struct WriteParamsTonalSparse : WriteParamsTonal {};
template <typename P> struct alloc_is_sparse { static constexpr bool value = false; };
template <> struct alloc_is_sparse<WriteParamsSparse> { static constexpr bool value = true; };
template <> struct alloc_is_sparse<WriteParamsTonalSparse> { static constexpr bool value = true; };

// A6s: the scale-factor indices and the code-table section of a sparse frame. Every wavefront forms the section's two ballots for its
// length, lane = 32 * channel + unit; wavefront 0 writes, a lane's position being the bits of the lanes below it: 3 per non-zero
// unit, 1 per clone flag. Returns what the section has less than 3 bits per unit below N.
__device__ __forceinline__ int alloc_sparse_head(uint32_t* s_out, const uint8_t* s_wl, const uint8_t* s_sfi, const uint8_t* s_tabw, int N, int nch,
                                                 int lane, int wave, int pos_sf, int pos_ct, int limit_bits)
{
    const int k = lane >> 5, q = lane & 31;
    const bool present = k < nch && q < N;
    const int w = present ? (int)s_wl[lane] : 0;
    const unsigned long long nz = __ballot(w > 0), cl = __ballot(present && k == 1 && w == 0 && s_wl[q] > 0);
    if (wave == 0 && present) {
        frame_put(s_out, pos_sf + k * (2 + 6 * N) + 2 + 6 * q, s_sfi[lane], 6, limit_bits);
        const unsigned long long lower = (1ull << lane) - 1ull;
        const int at = pos_ct + 1 + 4 * (k + 1) + 3 * __builtin_popcountll(nz & lower) + __builtin_popcountll(cl & lower);
        if (w > 0) frame_put(s_out, at, s_tabw[lane * 8 + w], 3, limit_bits);
        else if ((cl >> lane) & 1ull) frame_put(s_out, at, 1u, 1, limit_bits);   // "do not copy from channel 0"
    }
    return 3 * (nch * N - __builtin_popcountll(nz)) - __builtin_popcountll(cl);
}

template <typename P>
__global__ __launch_bounds__(256) void k_at3p_write_adaptive_with(AdaptiveParams<P> p)
{
    // kRd: RATE-DISTORTION WORD LENGTHS (at3p_rd.hpp), which are sparse frames
    // kPsy: MASKING-WEIGHTED WORD LENGTHS (at3p_psy.hpp), which are rate-distortion frames with lambda shifted per unit
    constexpr bool kTonal = P::kTonal, kRd = alloc_is_rd<P>::value, kSparse = alloc_is_sparse<P>::value || kRd, kPsy = alloc_is_psy<P>::value;
    __shared__ uint32_t s_out[kFrameBytes / 4];
    __shared__ uint32_t s_qbits[2][32][7][8];  // A2: the bits of each unit at each word length under each of its eight tables
    __shared__ uint16_t s_B[2][32][8];         // B[ch][qu][w], entry 0 unused
    __shared__ uint8_t s_tabw[2][32][8];       // tab[ch][qu][w]
    __shared__ uint32_t s_max[2][32];
    __shared__ float s_scale[64], s_inv[8];
    __shared__ uint8_t s_sfi[2][32], s_wl[2][32], s_pw[32];
    __shared__ uint16_t s_wlv[32];
    __shared__ uint32_t s_wsum[4];
    __shared__ int s_tfit[4], s_kfit[4];       // per wavefront: the smallest t and the largest k of its share that fit
    __shared__ int s_n, s_pos_sf;
    __shared__ uint16_t s_cb[256];             // the chosen table's bits per chunk, in stream order (channel, chunk)
    __shared__ uint32_t s_off[256];            // and their exclusive prefix sums per channel
    __shared__ uint32_t s_info[56];
    __shared__ uint32_t s_len4[(kLenEntries + 7) / 8];
    __shared__ uint32_t s_rec[kTonal ? kTonalBlockWords : 1];
    // kRd only (the others never name them): R1's S and D, every unit's pick at j = kRdJMin - 1 .. kRdJMax, R3's scan results
    __shared__ unsigned long long s_S[kRd ? 2 * 32 * 8 : 1];
    __shared__ double s_D[kRd ? 2 * 32 * 8 : 1];
    __shared__ uint8_t s_pick[kRd && !kPsy ? (kRdJCount + 1) * 64 : 1];
    __shared__ int s_jfit[4], s_krfit[4];
    // kPsy only: M2's two tables
    __shared__ uint32_t s_spread[kPsy ? 256 : 1];
    __shared__ uint8_t s_ath[kPsy ? 32 : 1];

    const WriteTables* W = p.W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = p.nch;
    const size_t item = blockIdx.x;
    // The frame's size: its budget (A4), its bits and its 32-bit words. s_out holds the largest frame; the words past this frame's
    // are neither zeroed, written nor stored.
    const int size_bits = 8 * p.frame_bytes - 3, limit_bits = 8 * p.frame_bytes, n_words = p.frame_bytes >> 2;
    // The thread's chunk in stream order: every thread walks all seven word lengths, so nothing is gained by dealing the
    // threads by word length as the fixed writer does.
    const int ch = tid >> 7, c = tid & 127;
    const bool active = ch < nch;
    const int qu = at3p_qu_of_line(16 * c);

    if (tid < n_words) s_out[tid] = 0u;
    if (256 + tid < n_words) s_out[256 + tid] = 0u;
#pragma unroll
    for (int i = 0; i < 14; ++i) (&s_qbits[0][0][0][0])[tid + 256 * i] = 0u;
    if constexpr (kRd) s_S[tid] = s_S[256 + tid] = 0ull;
    constexpr int kLenWords = (kLenEntries + 7) / 8, kLenIt = (kLenWords + 255) / 256;
    float x[16];
    {
        const float4* src = reinterpret_cast<const float4*>(p.specs + (item * nch + (active ? ch : 0)) * 2048 + 16 * c);
        float4 xv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) xv[k] = src[k];
        const float scale_v = W->scale[tid & 63];
        const uint32_t info_v = W->info56[(tid >= 64 && tid < 120) ? tid - 64 : 0];
        const float inv_v = W->inv_mant[tid & 7];
        const uint32_t pw_v = 4u * W->sb_powgrps[W->qu_to_sb[tid & 31]];
        const uint16_t wlv_v = (&p.wl_vlc[0][0])[tid & 31];
        uint32_t len_v[kLenIt];
#pragma unroll
        for (int i = 0; i < kLenIt; ++i) len_v[i] = W->len4[tid + 256 * i < kLenWords ? tid + 256 * i : kLenWords - 1];
        if (tid < 64) {
            (&s_max[0][0])[tid] = 0u;
            s_scale[tid] = scale_v;
        }
        if (tid >= 64 && tid < 120) s_info[tid - 64] = info_v;
        if (tid >= 120 && tid < 128) s_inv[tid - 120] = inv_v;
        if (tid >= 192 && tid < 224) s_pw[tid - 192] = (uint8_t)pw_v;
        if (tid >= 224) s_wlv[tid - 224] = wlv_v;
        if constexpr (kTonal) {
            if (tid >= 128 && tid < 128 + kTonalBlockWords) s_rec[tid - 128] = reinterpret_cast<const uint32_t*>(p.tonal + item)[tid - 128];
        }
        if constexpr (kPsy) {
            s_spread[tid] = reinterpret_cast<const uint32_t*>(&p.psy.spread[0][0])[tid];
            if (tid < 32) s_ath[tid] = p.psy.ath[tid];
        }
#pragma unroll
        for (int i = 0; i < kLenIt; ++i)
            if (tid + 256 * i < kLenWords) s_len4[tid + 256 * i] = len_v[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 v = active ? xv[k] : float4{0.0f, 0.0f, 0.0f, 0.0f};
            x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
        }
    }
    __syncthreads();
    // ---- A1, TScaler::Scale: the unit's largest magnitude (order-free), its scale factor, the scaled values ----
    {
        float m = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) m = fmaxf(m, fabsf(x[k]));
        if (active) atomicMax(&s_max[ch][qu], __float_as_uint(m));
    }
    __syncthreads();
    if (tid < 64) {
        float maxAbs = __uint_as_float((&s_max[0][0])[tid]);
        if (maxAbs > 1.0f) maxAbs = 1.0f;
        int lo = 0, hi = 63;   // map::lower_bound: the first entry >= maxAbs
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_scale[mid] < maxAbs) lo = mid + 1;
            else hi = mid;
        }
        (&s_sfi[0][0])[tid] = (uint8_t)lo;
    }
    __syncthreads();
    {
        const float sf = s_scale[s_sfi[active ? ch : 0][qu]];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float v = x[k] / sf;
            if (fabsf(v) >= 1.0f) v = (v > 0) ? 0.99999f : -0.99999f;
            x[k] = v;
        }
    }
    // ---- A2: every word length's mantissas and their bits under its eight code tables ----
    int qv[16];
    ChunkPricer pricer;
    if (active) {
        if constexpr (kRd) {   // R1 at w = 0: no mantissa, e = v
            unsigned long long acc = 0ull;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const float e = x[k] - 0.0f * p.mant[0];
                acc += rd_dist_u(e * e);
            }
            atomicAdd(&s_S[(ch * 32 + qu) * 8], acc);
        }
#pragma unroll 1
        for (int w = 1; w <= 7; ++w) {
            alloc_quantise(x, s_inv[w], qv);
            if constexpr (kRd) {   // R1: the chunk's share of S[ch][qu][w], an integer and so free of the order
                const float mant = p.mant[w];
                unsigned long long acc = 0ull;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const float e = x[k] - (float)qv[k] * mant;
                    acc += rd_dist_u(e * e);
                }
                atomicAdd(&s_S[(ch * 32 + qu) * 8 + w], acc);
            }
            pricer.reset();
            for (int i = 0; i < 8; ++i) atomicAdd(&s_qbits[ch][qu][w - 1][i], (uint32_t)pricer.price(qv, s_info[w - 1 + 7 * i], s_len4));
        }
    }
    __syncthreads();
    for (int e = tid; e < 2 * 32 * 7; e += 256) {   // the first table with the fewest bits
        const uint32_t* b = &s_qbits[0][0][0][0] + 8 * e;
        uint32_t best = b[0];
        int bi = 0;
        for (int i = 1; i < 8; ++i)
            if (b[i] < best) {
                best = b[i];
                bi = i;
            }
        const int u = e / 7, w = e % 7 + 1;
        (&s_B[0][0][0])[u * 8 + w] = (uint16_t)best;
        (&s_tabw[0][0][0])[u * 8 + w] = (uint8_t)bi;
    }
    if constexpr (kSparse) {   // a unit at word length 0 has no bits and no table
        if (tid < 64) {
            (&s_B[0][0][0])[tid * 8] = 0;
            (&s_tabw[0][0][0])[tid * 8] = 0;
        }
    }
    if constexpr (kRd) {   // R1: D = (double)S * G[sfi]
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + 256 * i;
            s_D[e] = rd_d(s_S[e], rd_g(s_scale[(&s_sfi[0][0])[e >> 3]]));
        }
    }
    __syncthreads();
    // ---- the tail's bits (formed once, as in the fixed writer), then A3-A5: every wavefront evaluates its share of the
    //      candidates, lanes are units ----
    uint32_t fl[2] = {0u, 0u};
    int win_bits[2] = {0, 0};
    for (int k = 0; k < nch; ++k) {
        fl[k] = p.flags ? p.flags[item * nch + k] : 0u;
        win_bits[k] = fl[k] == 0u ? 1 : ((fl[k] & 0xffu) == 0xffu ? 2 : 18);   // IsAllSteep keeps its mask in a uint8_t
    }
    int tail_bits = (nch == 2 ? 2 : 0) + win_bits[0] + win_bits[1] + nch + 1 + 1 + 2;
    [[maybe_unused]] TonalPlan plan;
    if constexpr (kTonal) {   // (priced by every wavefront: each needs the block's bits, wavefront 0 writes it)
        tonal_price(s_rec, nch, lane, p.tone_vlc, &plan);
        tail_bits += plan.bits;
    }
    const bool u_act = (lane & 1) < nch;
    const int u_sfi = s_sfi[lane & 1][lane >> 1];
    // M3: the lane's unit's offset o and the frame's largest, O; both 0 without kPsy, and the code below is then R2-R4 as written
    [[maybe_unused]] int psy_o = 0, psy_O = 0;
    if constexpr (kPsy) {   // every wavefront forms them: each fills its rows of the pick table with its lanes' own shifts
        const int pq = lane >> 1, pc = lane & 1;
        const uint8_t* spread = reinterpret_cast<const uint8_t*>(s_spread);
        double th = rd_lambda(s_ath[pq], s_scale);   // M2: the threshold in quiet, then the 32 maskers of the lane's channel
        for (int m = 0; m < 32; ++m) {
            const int s = spread[m * 32 + pq];
            const double cast = s_D[(pc * 32 + m) * 8] * rd_g(s_scale[63 - (s & 63)]);
            if (s <= 63 && cast > th) th = cast;
        }
        const int mu = psy_mu(th, s_scale);
        const bool live = u_act && s_S[(pc * 32 + pq) * 8] > 0ull;
        // mu_min over the live lanes and O over all, bit by bit from the top with ballots: wave-uniform, no cross-lane data moves
        unsigned long long cand = __ballot(live);
        int mu_min = 0;
        for (int b = 6; b >= 0; --b) {
            const unsigned long long z = __ballot(live && !((mu >> b) & 1)) & cand;
            if (z) cand = z;
            else mu_min |= 1 << b;
        }
        psy_o = live ? (mu - mu_min < kPsyMaxOffset ? mu - mu_min : kPsyMaxOffset) : 0;
        cand = ~0ull;
        for (int b = 5; b >= 0; --b) {
            const unsigned long long o = __ballot((psy_o >> b) & 1) & cand;
            if (o) {
                cand = o;
                psy_O |= 1 << b;
            }
        }
    }
    // kPsy: up to kPsyMaxOffset more rows, in s_qbits, which nothing reads after B and tab were formed from it
    static_assert(sizeof(s_qbits) >= (kRdJCount + 1 + kPsyMaxOffset) * 64, "the masking-weighted pick table fits in s_qbits");
    [[maybe_unused]] uint8_t* const pick = kPsy ? reinterpret_cast<uint8_t*>(&s_qbits[0][0][0][0]) : s_pick;
    [[maybe_unused]] const int j_lo = kPsy ? kRdJMin - psy_O : kRdJMin;   // M5: the scan's lower end; row i of s_pick holds the picks at j_lo - 1 + i
    if constexpr (kRd) {   // R2: the lane's unit's pick at every j the scans ask for, the rows dealt to the wavefronts
        double D[8];
        uint16_t B[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            D[w] = s_D[((lane & 1) * 32 + (lane >> 1)) * 8 + w];
            B[w] = s_B[lane & 1][lane >> 1][w];
        }
        for (int i = wave; i <= kRdJMax - j_lo + 1; i += 4)
            pick[i * 64 + lane] = (uint8_t)(u_act ? rd_pick(D, B, rd_lambda(j_lo - 1 + i + psy_o, s_scale)) : 0);
        __syncthreads();
        int jfit = kRdJMax + 1;
        for (int j = kRdJMax - wave; j >= j_lo; j -= 4) {   // R3, as the scan over t below
            const int row = (j - j_lo) * 64 + lane;
            const AllocEval e = alloc_eval_from<true>(pick[row + 64], pick[row], 0, u_act, lane, nch, &s_B[0][0][0], s_wlv, s_pw, tail_bits);
            if (e.total <= size_bits) jfit = j;
        }
        if (lane == 0) s_jfit[wave] = jfit;
    }
    {
        int tfit = kAllocTMax + 1;
        for (int t = kAllocTMax - wave; t >= kAllocTMin; t -= 4) {   // descending: the last one that fits is the smallest
            const AllocEval e = alloc_eval<kSparse>(t, 0, u_sfi, u_act, lane, nch, &s_B[0][0][0], s_wlv, s_pw, tail_bits);
            if (e.total <= size_bits) tfit = t;
        }
        if (lane == 0) s_tfit[wave] = tfit;
    }
    __syncthreads();
    int t_star = kAllocTMax;   // (nothing fits: a caller's table only, see host_allocate)
    for (int w = 0; w < 4; ++w)
        if (s_tfit[w] < t_star) t_star = s_tfit[w];
    {
        int kfit = 0;
        for (int k = wave; k <= kAllocKMax; k += 4) {
            const AllocEval e = alloc_eval<kSparse>(t_star, k, u_sfi, u_act, lane, nch, &s_B[0][0][0], s_wlv, s_pw, tail_bits);
            if (e.total <= size_bits) kfit = k;
        }
        if (lane == 0) s_kfit[wave] = kfit;
    }
    [[maybe_unused]] int j_row = 0;   // j* as the row of its picks at j* - 1
    if constexpr (kRd) {
        int j_star = kRdJMax;   // (nothing fits: a caller's table only)
        for (int w = 0; w < 4; ++w)
            if (s_jfit[w] < j_star) j_star = s_jfit[w];
        j_row = (j_star - j_lo) * 64 + lane;
        int kfit = 0;
        for (int k = wave; k <= kAllocKMax; k += 4) {
            const AllocEval e = alloc_eval_from<true>(pick[j_row + 64], pick[j_row], k, u_act, lane, nch, &s_B[0][0][0], s_wlv, s_pw, tail_bits);
            if (e.total <= size_bits) kfit = k;
        }
        if (lane == 0) s_krfit[wave] = kfit;
    }
    __syncthreads();
    // ---- A6: the frame's first bits, the unit count and the word-length section, by wavefront 0 ----
    if (wave == 0) {
        int k_star = 0;
        for (int w = 0; w < 4; ++w)
            if (s_kfit[w] > k_star) k_star = s_kfit[w];
        AllocEval e = alloc_eval<kSparse>(t_star, k_star, u_sfi, u_act, lane, nch, &s_B[0][0][0], s_wlv, s_pw, tail_bits);
        if constexpr (kRd) {   // R4: R(j*, k*) unless its distortion exceeds that of A(t*, k*), the sparse frame in e
            int kr_star = 0;
            for (int w = 0; w < 4; ++w)
                if (s_krfit[w] > kr_star) kr_star = s_krfit[w];
            const AllocEval r = alloc_eval_from<true>(pick[j_row + 64], pick[j_row], kr_star, u_act, lane, nch, &s_B[0][0][0], s_wlv, s_pw, tail_bits);
            double t_a = 0.0, t_r = 0.0;   // T: the serial sums in the order of the walk, the same in every lane
#pragma unroll
            for (int u = 0; u < 64; ++u) {
                const int wa = __builtin_amdgcn_readlane(e.wl, u), wr = __builtin_amdgcn_readlane(r.wl, u);
                if ((u & 1) < nch) {
                    if constexpr (kPsy) {   // M6: each term weighted by G[63 - o]
                        const double g = rd_g(s_scale[63 - __builtin_amdgcn_readlane(psy_o, u)]);
                        t_a += s_D[((u & 1) * 32 + (u >> 1)) * 8 + wa] * g;
                        t_r += s_D[((u & 1) * 32 + (u >> 1)) * 8 + wr] * g;
                    } else {
                        t_a += s_D[((u & 1) * 32 + (u >> 1)) * 8 + wa];
                        t_r += s_D[((u & 1) * 32 + (u >> 1)) * 8 + wr];
                    }
                }
            }
            if (t_r <= t_a) e = r;
        }
        s_wl[lane & 1][lane >> 1] = (uint8_t)e.wl;
        const int incl = at3::wave_inclusive_scan(e.len << (16 * (lane & 1)), lane);
        const int before = ((incl >> (16 * (lane & 1))) & 0xffff) - e.len;
        const int pos1 = 20 + e.sum0;   // channel 1's list
        if (e.len) {
            const int idx = (lane & 1) ? e.idx1 : e.idx0;
            frame_put(s_out, ((lane & 1) ? pos1 + 6 : 20) + before, s_wlv[idx * 8 + e.delta] & 0xfffu, e.len, limit_bits);
        }
        if (lane == 0) {
            frame_put(s_out, 1, (uint32_t)nch - 1u, 2, limit_bits);
            frame_put(s_out, 3, (uint32_t)e.N - 1u, 5, limit_bits);     // (then the mute bit, 0)
            frame_put(s_out, 9, 3u, 2, limit_bits);                     // channel 0: mode 3, no flags, no position
            frame_put(s_out, 15, (uint32_t)e.idx0, 2, limit_bits);
            frame_put(s_out, 17, (uint32_t)e.wl, 3, limit_bits);
            if (nch == 2) {
                frame_put(s_out, pos1, 1u, 2, limit_bits);              // channel 1: mode 1, no flags
                frame_put(s_out, pos1 + 4, (uint32_t)e.idx1, 2, limit_bits);
            }
            s_n = e.N;
            s_pos_sf = pos1 + (nch == 2 ? 6 + e.sum1 : 0);
        }
    }
    __syncthreads();
    const int N = s_n;
    // ---- scale factor indices, code table indices, spectra and power groups per channel, tail: the fixed writer's layout ----
    const int pos_sf = s_pos_sf;
    const int pos_ct = pos_sf + nch * (2 + 6 * N);
    int pos_data = pos_ct + 1 + nch * (4 + 3 * N);
    if constexpr (kSparse) pos_data -= alloc_sparse_head(s_out, &s_wl[0][0], &s_sfi[0][0], &s_tabw[0][0][0], N, nch, lane, wave, pos_sf, pos_ct, limit_bits);
    else if (tid < 64) {
        const int k = tid >> 5, q = tid & 31;
        if (k < nch && q < N) {
            frame_put(s_out, pos_sf + k * (2 + 6 * N) + 2 + 6 * q, s_sfi[k][q], 6, limit_bits);
            frame_put(s_out, pos_ct + 1 + k * (4 + 3 * N) + 4 + 3 * q, s_tabw[k][q][s_wl[k][q]], 3, limit_bits);
        }
    }
    if (tid == 64) frame_put(s_out, pos_ct, 1u, 1, limit_bits);   // "use full table"
    bool coded = active && qu < N;
    if constexpr (kSparse) coded = coded && s_wl[ch][qu] > 0;   // a unit at word length 0 prices and emits nothing
    const int wl = coded ? s_wl[ch][qu] : 1;
    const uint32_t d = s_info[wl - 1 + 7 * s_tabw[active ? ch : 0][qu][wl]];
    alloc_quantise(x, s_inv[wl], qv);
    pricer.reset();
    s_cb[tid] = (uint16_t)(coded ? pricer.price(qv, d, s_len4) : 0);
    __syncthreads();
    {   // prefix sums in stream order: entry u = channel u / 128, chunk u % 128
        const int v = (int)s_cb[tid];
        const int incl = at3::wave_inclusive_scan(v, lane);
        if (lane == 63) s_wsum[wave] = (uint32_t)incl;
        __syncthreads();
        s_off[tid] = (uint32_t)(incl - v) + ((wave & 1) ? s_wsum[wave - 1] : 0u);
    }
    __syncthreads();
    const int ch_total[2] = {(int)(s_wsum[0] + s_wsum[1]), (int)(s_wsum[2] + s_wsum[3])};
    const int pw = s_pw[N - 1];
    const int ch_base[2] = {pos_data, pos_data + ch_total[0] + pw};
    if (coded) {
        BitRun run;
        run.start(s_out, ch_base[ch] + (int)s_off[tid], n_words);
        const int num_coeffs = (int)((d >> 20) & 15u);
        if (num_coeffs == 1) emit_chunk<1>(W, qv, d, &run);
        else if (num_coeffs == 2) emit_chunk<2>(W, qv, d, &run);
        else emit_chunk<4>(W, qv, d, &run);
        run.finish();
    }
    if (c == 0 && active) frame_put(s_out, ch_base[ch] + ch_total[ch], (1u << pw) - 1u, pw, limit_bits);   // (15, 4) per power group
    if (kTonal ? tid == 50 : tid == 65) {
        int pos = ch_base[nch - 1] + ch_total[nch - 1] + pw;
        if (nch == 2) pos += 2;   // swap_channels, negate_coeffs
        for (int k = 0; k < nch; ++k) {
            if (win_bits[k] == 2) {
                frame_put(s_out, pos, 2u, 2, limit_bits);
            } else if (win_bits[k] == 18) {
                frame_put(s_out, pos, 3u, 2, limit_bits);
                for (int i = 0; i < 16; ++i) frame_put(s_out, pos + 2 + i, (fl[k] >> i) & 1u, 1, limit_bits);
            }
            pos += win_bits[k];
        }
        if constexpr (kTonal) {
            pos += nch;           // gain compensation per channel
            if (plan.bits) frame_put(s_out, pos, 1u, 1, limit_bits);
            pos += 1 + plan.bits + 1;   // the tonal flag and block, no noise info
        } else {
            pos += nch + 1 + 1;   // gain compensation per channel, no tonal block, no noise info
        }
        frame_put(s_out, pos, 3u, 2, limit_bits);
    }
    if constexpr (kTonal) {
        if (wave == 0)
            tonal_emit(s_out, ch_base[nch - 1] + ch_total[nch - 1] + pw + (nch == 2 ? 2 : 0) + win_bits[0] + win_bits[1] + nch + 1, s_rec, nch,
                       lane, p.tone_vlc, plan, limit_bits);
    }
    __syncthreads();
    // (word stores: frame_bytes is a multiple of 8, so every frame of a 4-byte aligned [items][frame_bytes] buffer is word-aligned)
    uint32_t* dst = reinterpret_cast<uint32_t*>(p.out + item * (size_t)p.frame_bytes);
    if (tid < n_words) dst[tid] = __builtin_bswap32(s_out[tid]);
    if (256 + tid < n_words) dst[256 + tid] = __builtin_bswap32(s_out[256 + tid]);
}
// (the instantiations are named where they are launched, at3p_alloc.hip, at3p_sparse.hip, at3p_rd.hip and at3p_psy.hip: naming one instantiates it, and a
// translation unit must hold only its own)

// ---- host: the launch of a unit's two instantiations, P without records and PT with them ------------------------------------------
// wp: the fixed writer's parameters as at3phip.hip's launch_write fills them, tone_vlc included; wp.tonal null: the writer without
// records. The word-length code tables, the mantissa steps of a rate-distortion type and the frame size travel in the kernel's
// arguments: nothing is allocated or uploaded for the adaptive path. wp.out is [n_items][frame_bytes].
template <typename P>
void launch_write_adaptive_kernel(const WriteParamsTonal& wp, int32_t frame_bytes, hipStream_t on)
{
    using Fixed = std::conditional_t<P::kTonal, WriteParamsTonal, WriteParams>;
    AdaptiveParams<P> ap;
    static_cast<Fixed&>(ap) = wp;
    if constexpr (alloc_is_rd<P>::value) memcpy(ap.mant, AT3P_MANT, sizeof(ap.mant));
    if constexpr (alloc_is_psy<P>::value) {
        memcpy(ap.psy.spread, AT3P_PSY_SPREAD, sizeof(ap.psy.spread));
        memcpy(ap.psy.ath, AT3P_PSY_ATH, sizeof(ap.psy.ath));
    }
    memcpy(ap.wl_vlc, AT3P_WL_VLC, sizeof(ap.wl_vlc));
    ap.frame_bytes = frame_bytes;
    hipLaunchKernelGGL(k_at3p_write_adaptive_with<P>, dim3((unsigned)wp.n_items), dim3(256), 0, on, ap);
}
template <typename P, typename PT>
void launch_write_adaptive_as(const WriteParamsTonal& wp, int32_t frame_bytes, hipStream_t on)
{
    if (wp.tonal) launch_write_adaptive_kernel<PT>(wp, frame_bytes, on);
    else launch_write_adaptive_kernel<P>(wp, frame_bytes, on);
}

}  // namespace at3p
