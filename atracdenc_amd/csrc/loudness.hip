// The batched loudness and true-peak meter (include/at3hip_loudness.h): the k_hops, k_carry, k_true_peak and k_scale kernels,
// the host gating and the C ABI. The look-ahead limiter on the same context is loudness_limit.hpp, included at the end.
//
// Kernel layout.
//   k_hops       one lane per (stream, hop, channel) runs the definition's chain: 13 230 steps of two f64 biquads over the
//                window [4410 (j - 2), 4410 (j + 1)) of hop j (samples before the stream's start are +0.0f, which leaves a
//                zero filter state at exactly +0.0: the restart at max(0, j - 2) needs no branch), and sums y2 * y2 over the last
//                4410. The lanes of a wavefront sit 4410 samples apart, so the samples come through LDS: wavefront 0 of a
//                workgroup computes, wavefronts 1 - 3 stage the next tile of 63 samples per lane with coalesced loads (a row of
//                63 C consecutive floats per (stream, hop)) into the other of two buffers, one barrier per tile. 63 divides
//                4410, so the sum starts on a tile boundary. A lane's samples are 65 floats apart in LDS (a row of 65 C floats
//                per (stream, hop)), a stride of C mod 32: a ds_read_b32 of the computing wavefront touches every bank once
//                per half-wave. The sample peak of
//                the hop's own samples rides along (integer max of the float's bits without the sign).
//   k_carry      copies what the next call needs, the samples [4410 max(0, H - 2), T) of every stream, into the other of two
//                carry buffers, and takes the sample peak of the new samples past the last complete hop.
//   k_true_peak  k_resample's tiling for L = 4, M = 1, K = 144: a workgroup stages 256 + 143 samples of one stream, wavefront r
//                computes phase r for 4 x 64 consecutive q with wave-uniform taps, nothing of the 4x signal is written: |u| is
//                reduced over the lane's outputs and across the wavefront, then one atomic max per wavefront and channel on
//                the float's bits (valid: non-negative floats order like their bits).
//   k_scale      out = in * gain[stream].
// Every index that scales with the batch is 64-bit. The f64 path holds no FMA (-ffp-contract=off) and no kernel uses scratch.
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/at3hip_loudness.h"
#include "../../include/at3hip_resample.h"
#include "at3_host_util.hpp"
#include "at3_pcm_in.hpp"

using at3host::dev_alloc;
using at3host::fail;

namespace {

constexpr int kHop = AT3HIP_LOUDNESS_HOP;
constexpr int kWindow = 3 * kHop;          // samples of one lane's chain
constexpr int kTile = 63;                  // samples per lane and tile: divides kHop and kWindow
constexpr int kTiles = kWindow / kTile;    // 210
constexpr int kSumTile = 2 * kHop / kTile; // 140: the first tile of the hop itself
constexpr int kHopThreads = 256;           // wavefront 0 computes, 1 - 3 stage
constexpr int kRowFloats = 65;             // LDS floats per lane: a row of a (stream, hop) is C of them, stride = C mod 32
constexpr int kTaps = 144, kPhases = 4;    // the 44100 -> 176400 converter: K, L (M = 1)
constexpr int kPeakThreads = 256;          // one wavefront per phase
constexpr int kPeakQ = 256;                // q per tile: 4 per lane
constexpr int kCarryThreads = 256;
constexpr int kCarryBlocks = 8;            // workgroups per stream of k_carry
constexpr int kScaleThreads = 256;
static_assert(kTile * kTiles == kWindow && kTile * kSumTile == 2 * kHop, "tiles must align with the hops");

struct MeterParams {
    const float* carry;      // [S][kWindow][C]: samples base .. t_old - 1 of each stream (read)
    float* carry_next;       // [S][kWindow][C]: samples base_next .. t_old + n_in - 1 (written by k_carry)
    const void* in;          // [S][n_in][C], float or int16_t: the kernels' template parameter T
    double* z;               // [max_hops][S][C]
    unsigned* peaks;         // [S][2][2]: bits of the sample peak and of the largest |u|, per channel
    const float* hp;         // [4][144]
    long long t_old;         // samples of each stream before this call
    long long base;          // absolute index of carry's first sample
    long long base_next;     // the same for carry_next
    long long q_lo, q_hi;    // k_true_peak: the q of this call
    int n_in;
    int h_old, h_new;        // complete hops before and after this call
    int n_streams;
};

// Element idx = sample * C + channel of stream s (absolute sample index) is +0.0f before the stream's start and from the end
// of the samples received (element_is_zero); the carry buffer holds it behind t_old, the call's input from there. element_ptr
// clamps idx into what the stream holds (every launch has at least one such element), so that the load is unconditional and a
// run of loads stays in flight together; the caller selects the zero afterwards.
template <int C>
__device__ __forceinline__ const float* element_ptr(const MeterParams& p, size_t s, long long idx)
{
    const long long told = p.t_old * C, lo = p.base * C, hi = told + (long long)p.n_in * C - 1;
    const long long at = idx < lo ? lo : (idx > hi ? hi : idx);
    return at >= told ? static_cast<const float*>(p.in) + s * (size_t)p.n_in * C + (size_t)(at - told) : p.carry + s * (size_t)kWindow * C + (size_t)(at - lo);
}

// What element_ptr's address holds, in two steps so that a run of loads stays in flight before the first value is used:
// element_bits is the load, element_value makes the float of it. For floats the bits are the value. 16-bit input (T = int16_t)
// is widened in element_value; the carry buffer is float for both kinds of call. A row of 16-bit samples that starts 4-byte
// aligned and has an even number of samples is read as 32-bit sample pairs (PAIRS): the address is selected first - the pair's
// dword in the row, or the float in the carry buffer - and ONE dword load follows, as for floats. Otherwise a fetch is two
// 16-bit loads, again from addresses selected first (the sample itself, or the two halves of the carried float). Which form a call takes is decided once per kernel from its arguments (all_pairs: with the call's pointer
// 4-byte aligned and n_in * C even, every stream's row is aligned and even - every stereo call behind an aligned pointer, and
// mono calls of even length), so no branch sits between the loads, no lane diverges and no load reaches outside its row.
template <typename T>
struct ElementBits { using type = uint32_t; };
template <>
struct ElementBits<float> { using type = float; };

template <typename T>
__device__ __forceinline__ bool all_pairs(const MeterParams& p, int C)
{
    return sizeof(T) == sizeof(int16_t) && ((uintptr_t)p.in & 3u) == 0 && ((long long)p.n_in * C) % 2 == 0;
}

template <int C, typename T, bool PAIRS>
__device__ __forceinline__ typename ElementBits<T>::type element_bits(const MeterParams& p, size_t s, long long idx)
{
    if constexpr (std::is_same<T, float>::value) {
        return *element_ptr<C>(p, s, idx);
    } else {
        const long long told = p.t_old * C, lo = p.base * C, hi = told + (long long)p.n_in * C - 1;
        const long long at = idx < lo ? lo : (idx > hi ? hi : idx);
        const size_t n = (size_t)p.n_in * C;
        const T* const row = static_cast<const T*>(p.in) + s * n;
        const uint32_t* const carry = reinterpret_cast<const uint32_t*>(p.carry) + s * (size_t)kWindow * C;
        if constexpr (PAIRS) {
            const uint32_t* const src = at >= told ? reinterpret_cast<const uint32_t*>(row) + ((size_t)(at - told) >> 1) : carry + (size_t)(at - lo);
            return *src;
        } else {
            // two 16-bit loads from addresses selected first: the sample twice (element_value takes either half), or the halves
            // of the carried float
            const uint16_t* const a = at >= told ? reinterpret_cast<const uint16_t*>(row) + (size_t)(at - told)
                                                 : reinterpret_cast<const uint16_t*>(carry + (size_t)(at - lo));
            const uint16_t* const b = at >= told ? a : a + 1;
            return (uint32_t)*a | ((uint32_t)*b << 16);
        }
    }
}

template <int C, typename T>
__device__ __forceinline__ float element_value(const MeterParams& p, long long idx, typename ElementBits<T>::type bits)
{
    if constexpr (std::is_same<T, float>::value) {
        return bits;
    } else {
        const long long told = p.t_old * C, lo = p.base * C, hi = told + (long long)p.n_in * C - 1;
        const long long at = idx < lo ? lo : (idx > hi ? hi : idx);
        const int v = (int16_t)(((at - told) & 1) ? (bits >> 16) : (bits & 0xffffu));
        return at >= told ? (float)v * 0x1p-15f : __uint_as_float(bits);
    }
}

// pairs: all_pairs<T>(p, C), computed once by the kernel
template <int C, typename T>
__device__ __forceinline__ float element_raw(const MeterParams& p, size_t s, long long idx, bool pairs)
{
    if constexpr (std::is_same<T, float>::value) return element_value<C, T>(p, idx, element_bits<C, T, false>(p, s, idx));
    else return element_value<C, T>(p, idx, pairs ? element_bits<C, T, true>(p, s, idx) : element_bits<C, T, false>(p, s, idx));
}

template <int C>
__device__ __forceinline__ bool element_is_zero(const MeterParams& p, long long idx)
{
    return idx < 0 || idx >= (p.t_old + p.n_in) * C;
}

template <int C, typename T>
__device__ __forceinline__ float element(const MeterParams& p, size_t s, long long idx, bool pairs)
{
    const float v = element_raw<C, T>(p, s, idx, pairs);
    return element_is_zero<C>(p, idx) ? 0.0f : v;
}

__device__ __forceinline__ unsigned magnitude_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// One step of both biquads (transposed direct form II, every product and sum on its own); returns stage 2's y.
struct Chain {
    double s1a = 0.0, s2a = 0.0, s1b = 0.0, s2b = 0.0;
    __device__ __forceinline__ double step(float sample)
    {
        constexpr double kStage1[5] = AT3HIP_KW_STAGE1;
        constexpr double kStage2[5] = AT3HIP_KW_STAGE2;
        const double x = (double)sample;
        const double y1 = kStage1[0] * x + s1a;
        s1a = (kStage1[1] * x - kStage1[3] * y1) + s2a;
        s2a = kStage1[2] * x - kStage1[4] * y1;
        const double y2 = kStage2[0] * y1 + s1b;
        s1b = (kStage2[1] * y1 - kStage2[3] * y2) + s2b;
        s2b = kStage2[2] * y1 - kStage2[4] * y2;
        return y2;
    }
};

template <int C, typename T>
__global__ __launch_bounds__(kHopThreads) void k_hops(MeterParams p)
{
    __shared__ float sx[2][64 * kRowFloats];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const bool pairs = all_pairs<T>(p, C);
    const int n_new = p.h_new - p.h_old;                         // new hops per stream
    const long long n_rows = (long long)p.n_streams * n_new;     // (stream, hop) pairs of this call
    const long long row0 = (long long)blockIdx.x * (64 / C);     // this workgroup's first pair
    constexpr int kRows = 64 / C;
    constexpr int kRow = kRowFloats * C;                         // LDS floats between rows
    constexpr int kElems = kTile * C;                            // floats per row and tile
    constexpr int kPerWave = (kRows + 2) / 3;                    // rows per staging wavefront and tile
    constexpr int kLoads = (kElems + 63) / 64;                   // loads per row and lane

    // the staging wavefronts' rows: stream and element index of the window's first float (rows past the end repeat row 0's)
    unsigned row_s[kPerWave];
    long long row_first[kPerWave];
#pragma unroll
    for (int i = 0; i < kPerWave; ++i) {
        const int r = wave > 0 ? wave - 1 + 3 * i : 0;
        const unsigned row = (r < kRows && row0 + r < n_rows) ? (unsigned)(row0 + r) : (unsigned)row0;
        row_s[i] = row / (unsigned)n_new;
        row_first[i] = ((long long)(p.h_old + row % (unsigned)n_new) - 2) * kHop * C;
    }

    // the computing lane's item
    const long long my_row = row0 + lane / C;
    const int my_c = lane % C;
    const bool mine = my_row < n_rows;
    Chain f;
    double acc = 0.0;
    unsigned peak = 0;

    for (int t = 0; t <= kTiles; ++t) {
        if (wave > 0 && t < kTiles) {   // stage tile t: every load of this wavefront first, then the selects and the LDS stores
            float* dst = sx[t & 1];
            typename ElementBits<T>::type v[kPerWave][kLoads];
            if (pairs) {   // (never for floats)
#pragma unroll
                for (int i = 0; i < kPerWave; ++i)
#pragma unroll
                    for (int k = 0; k < kLoads; ++k) v[i][k] = element_bits<C, T, true>(p, row_s[i], row_first[i] + (long long)t * kElems + lane + 64 * k);
            } else {
#pragma unroll
                for (int i = 0; i < kPerWave; ++i)
#pragma unroll
                    for (int k = 0; k < kLoads; ++k) v[i][k] = element_bits<C, T, false>(p, row_s[i], row_first[i] + (long long)t * kElems + lane + 64 * k);
            }
#pragma unroll
            for (int i = 0; i < kPerWave; ++i) {
                const int r = wave - 1 + 3 * i;
                if (r < kRows && row0 + r < n_rows) {
#pragma unroll
                    for (int k = 0; k < kLoads; ++k)
                        if (lane + 64 * k < kElems) {
                            const long long idx = row_first[i] + (long long)t * kElems + lane + 64 * k;
                            dst[r * kRow + lane + 64 * k] = element_is_zero<C>(p, idx) ? 0.0f : element_value<C, T>(p, idx, v[i][k]);
                        }
                }
            }
        }
        if (wave == 0 && t > 0 && mine) {   // compute tile t - 1
            const float* x = sx[(t - 1) & 1] + (lane / C) * kRow + my_c;
            if (t - 1 < kSumTile) {
#pragma unroll 9
                for (int i = 0; i < kTile; ++i) (void)f.step(x[i * C]);
            } else {
#pragma unroll 9
                for (int i = 0; i < kTile; ++i) {
                    const float v = x[i * C];
                    const double y = f.step(v);
                    acc = acc + y * y;
                    const unsigned m = magnitude_bits(v);
                    peak = m > peak ? m : peak;
                }
            }
        }
        __syncthreads();
    }
    if (wave == 0 && mine) {
        const size_t s = (unsigned)my_row / (unsigned)n_new;
        const size_t hop = (size_t)p.h_old + (unsigned)my_row % (unsigned)n_new;
        p.z[(hop * p.n_streams + s) * C + my_c] = acc;
        atomicMax(&p.peaks[(s * 2 + 0) * 2 + my_c], peak);
    }
}

template <int C, typename T>
__global__ __launch_bounds__(kCarryThreads) void k_carry(MeterParams p)
{
    __shared__ unsigned red[2];
    const size_t s = blockIdx.y;
    const int tid = threadIdx.x;
    if (tid < 2) red[tid] = 0;
    __syncthreads();
    const bool pairs = all_pairs<T>(p, C);
    const long long t_new = p.t_old + p.n_in;
    const long long keep = (t_new - p.base_next) * C;   // floats the next call may read
    long long tail = (long long)p.h_new * kHop;         // the new samples that no complete hop holds start here
    if (tail < p.t_old) tail = p.t_old;
    float* dst = p.carry_next + s * (size_t)kWindow * C;
    unsigned peak = 0;   // (the stride is even: a thread stays on one channel)
    for (long long i = (long long)blockIdx.x * kCarryThreads + tid; i < keep; i += (long long)kCarryBlocks * kCarryThreads) {
        const long long idx = p.base_next * C + i;
        const float v = element<C, T>(p, s, idx, pairs);
        dst[i] = v;
        if (idx >= tail * C) {
            const unsigned m = magnitude_bits(v);
            peak = m > peak ? m : peak;
        }
    }
    if (peak) atomicMax(&red[tid % C], peak);
    __syncthreads();
    if (tid < C && red[tid]) atomicMax(&p.peaks[(s * 2 + 0) * 2 + tid], red[tid]);
}

template <int C, typename T>
__global__ __launch_bounds__(kPeakThreads) void k_true_peak(MeterParams p)
{
    using V = typename std::conditional<C == 2, float2, float>::type;
    __shared__ V sx[kPeakQ + kTaps];
    const size_t s = blockIdx.y;
    const int tid = threadIdx.x;
    const bool pairs = all_pairs<T>(p, C);
    const long long q0 = p.q_lo + (long long)blockIdx.x * kPeakQ;
    // samples q0 - 71 .. q0 + 255 + 72 (output q reads x[q + k - 71], k < 144)
    const long long first = q0 - (kTaps / 2 - 1);
    for (int j = tid; j < kPeakQ + kTaps - 1; j += kPeakThreads) {
        V w;
        if constexpr (C == 2) w = make_float2(element<C, T>(p, s, (first + j) * 2, pairs), element<C, T>(p, s, (first + j) * 2 + 1, pairs));
        else w = element<C, T>(p, s, first + j, pairs);
        sx[j] = w;
    }
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // the phase
    const int lane = tid & 63;
    const float* h = p.hp + wave * kTaps;
    float acc[4][C];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int c = 0; c < C; ++c) acc[m][c] = 0.0f;
    for (int k = 0; k < kTaps; k += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float hk = h[k + u];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const V xv = sx[lane + 64 * m + k + u];
                if constexpr (C == 2) {
                    acc[m][0] = __builtin_fmaf(hk, xv.x, acc[m][0]);
                    acc[m][1] = __builtin_fmaf(hk, xv.y, acc[m][1]);
                } else {
                    acc[m][0] = __builtin_fmaf(hk, xv, acc[m][0]);
                }
            }
        }
    }
    unsigned peak[C];
#pragma unroll
    for (int c = 0; c < C; ++c) peak[c] = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const bool valid = q0 + lane + 64 * m < p.q_hi;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const unsigned b = valid ? magnitude_bits(acc[m][c]) : 0u;
            peak[c] = b > peak[c] ? b : peak[c];
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned o = __float_as_uint(__shfl_xor(__uint_as_float(peak[c]), d));
            peak[c] = o > peak[c] ? o : peak[c];
        }
        if (lane == 0 && peak[c]) atomicMax(&p.peaks[(s * 2 + 1) * 2 + c], peak[c]);
    }
}

// out[s][i] = in[s][i] * gain[s] for i < n (samples per stream); vec: n % 4 == 0 and every stream's four-sample groups are
// aligned (16 bytes of floats, 8 bytes of 16-bit samples; the output 16 bytes). A 16-bit sample is widened first:
// out = ((float)s * 0x1p-15f) * gain.
template <typename T>
__global__ __launch_bounds__(kScaleThreads) void k_scale(const T* in, float* out, const float* gain, long long n, int vec)
{
    const size_t s = blockIdx.y;
    const float g = gain[s];
    const T* src = in + s * (size_t)n;
    float* dst = out + s * (size_t)n;
    const long long stride = (long long)gridDim.x * kScaleThreads;
    const long long i0 = (long long)blockIdx.x * kScaleThreads + threadIdx.x;
    if constexpr (!std::is_same<T, float>::value) {
        if (vec) {
            const uint2* src4 = (const uint2*)src;
            float4* dst4 = (float4*)dst;
            for (long long i = i0; i < n / 4; i += stride) {
                const uint2 w = src4[i];
                float4 v;
                v.x = ((float)(int16_t)(w.x & 0xffffu) * 0x1p-15f) * g;
                v.y = ((float)(int16_t)(w.x >> 16) * 0x1p-15f) * g;
                v.z = ((float)(int16_t)(w.y & 0xffffu) * 0x1p-15f) * g;
                v.w = ((float)(int16_t)(w.y >> 16) * 0x1p-15f) * g;
                dst4[i] = v;
            }
        } else {
            const bool pairs = at3::pcm_pairs(src);
            for (long long i = i0; i < n; i += stride) dst[i] = at3::pcm_at(src, (size_t)i, (size_t)n, pairs) * g;
        }
    } else if (vec) {
        const float4* src4 = (const float4*)src;
        float4* dst4 = (float4*)dst;
        for (long long i = i0; i < n / 4; i += stride) {
            float4 v = src4[i];
            v.x = v.x * g;
            v.y = v.y * g;
            v.z = v.z * g;
            v.w = v.w * g;
            dst4[i] = v;
        }
    } else {
        for (long long i = i0; i < n; i += stride) dst[i] = src[i] * g;
    }
}

// -0.691 + 10 log10(p) (optnone: as the restatement computes it, step by step)
__attribute__((optnone, noinline)) double lufs(double p) { return -0.691 + 10.0 * log10(p); }

// The gating of the definition; z [n_hops][channels].
__attribute__((optnone, noinline)) void gate(const double* z, int H, int C, at3hip_loudness_result* r)
{
    r->n_hops = H;
    r->n_blocks_kept = 0;
    r->integrated = r->momentary_max = r->short_term_max = -HUGE_VAL;
    const int nb = H - 3;
    if (nb > 0) {
        std::vector<double> P((size_t)nb), l((size_t)nb);
        for (int b = 0; b < nb; ++b) {
            double sum = 0.0;
            for (int c = 0; c < C; ++c) {
                const double t = ((z[(size_t)b * C + c] + z[(size_t)(b + 1) * C + c]) + z[(size_t)(b + 2) * C + c]) + z[(size_t)(b + 3) * C + c];
                sum = c == 0 ? t : sum + t;
            }
            P[b] = sum / 17640.0;
            l[b] = lufs(P[b]);
            if (l[b] > r->momentary_max) r->momentary_max = l[b];
        }
        double sum = 0.0;
        int n = 0;
        for (int b = 0; b < nb; ++b)
            if (l[b] > -70.0) {
                sum = sum + P[b];
                ++n;
            }
        if (n > 0) {
            const double rel = lufs(sum / (double)n) - 10.0;
            sum = 0.0;
            n = 0;
            for (int b = 0; b < nb; ++b)
                if (l[b] > -70.0 && l[b] > rel) {
                    sum = sum + P[b];
                    ++n;
                }
            if (n > 0) {
                r->integrated = lufs(sum / (double)n);
                r->n_blocks_kept = n;
            }
        }
    }
    for (int b = 0; b + 30 <= H; ++b) {
        double sum = 0.0;
        for (int c = 0; c < C; ++c) {
            double t = z[(size_t)b * C + c];
            for (int k = 1; k < 30; ++k) t = t + z[(size_t)(b + k) * C + c];
            sum = c == 0 ? t : sum + t;
        }
        const double v = lufs(sum / 132300.0);
        if (v > r->short_term_max) r->short_term_max = v;
    }
}

__attribute__((optnone, noinline)) float gain_of(const at3hip_loudness_result* r, double target, double ceiling_db)
{
    const bool measured = r->true_peak[0] != 0.0f || r->true_peak[1] != 0.0f;
    const float* pk = measured ? r->true_peak : r->sample_peak;
    const double peak = (double)(pk[0] > pk[1] ? pk[0] : pk[1]);
    if (r->integrated == -HUGE_VAL || peak == 0.0) return 1.0f;
    const double a = pow(10.0, (target - r->integrated) / 20.0);
    const double b = pow(10.0, ceiling_db / 20.0) / peak;
    return (float)(a < b ? a : b);
}

}  // namespace

struct at3hip_loudness : at3host::EngineBase {
    at3hip_loudness_config cfg;
    float* d_carry[2] = {nullptr, nullptr};  // [S][kWindow][C], read / written alternately
    int cur = 0;
    double* d_z = nullptr;                   // [max_hops][S][C]
    unsigned* d_peaks = nullptr;             // [S][2][2]
    float* d_hp = nullptr;                   // [4][144], only with true_peak
    float* d_gain = nullptr;                 // [S]
    float* d_in = nullptr;                   // staging for host input [S][max_in][C], allocated by the first call that needs it
    int16_t* d_in_s16 = nullptr;             // the same as 16-bit samples, allocated by the first *_s16 call that takes host memory
    float* d_out = nullptr;                  // staging for at3hip_loudness_apply's host output, likewise
    long long t = 0;                         // samples received per stream since the start
    long long q_done = 0;                    // q below this have had their four outputs taken (true_peak)
    // the limiter (loudness_limit.hpp); its buffers are allocated by the first at3hip_loudness_limit_start
    uint32_t* d_lim_q[2] = {nullptr, nullptr};       // [S][2645 + max_in]: carried and new q, read / written alternately
    float* d_lim_x[2] = {nullptr, nullptr};          // [S][292][C]: carried samples, likewise
    float* d_lim_gain = nullptr;                     // [S]
    unsigned long long* d_lim_stats = nullptr;       // [S][2]
    float* d_lim_out = nullptr;                      // staging for host output, allocated by the first call that needs it
    int lim_cur = 0;
    bool lim_on = false;                             // between a start and its flush (or a reset)
    uint32_t lim_flags = 0;
    float lim_ceiling = 0.0f;
    long long lim_t = 0, lim_qd = 0, lim_em = 0;     // samples received, q computed, outputs emitted per stream
};

namespace {

long long carry_base(long long t) { const long long h = t / kHop; return kHop * (h > 2 ? h - 2 : 0); }

int clear_state(at3hip_loudness* l)
{
    HIPCHK(l, hipMemsetAsync(l->d_peaks, 0, (size_t)l->cfg.n_streams * 4 * sizeof(unsigned), l->stream));
    l->t = 0;
    l->q_done = 0;
    return AT3HIP_OK;
}

// Queues the kernels of one call: n_in new samples per stream (device memory); flush: the converter's outputs up to the end.
template <typename T>
int launch(at3hip_loudness* l, const T* in, int n_in, bool flush)
{
    const int C = l->cfg.channels, S = l->cfg.n_streams;
    MeterParams p;
    p.carry = l->d_carry[l->cur];
    p.carry_next = l->d_carry[l->cur ^ 1];
    p.in = in;
    p.z = l->d_z;
    p.peaks = l->d_peaks;
    p.hp = l->d_hp;
    p.t_old = l->t;
    p.base = carry_base(l->t);
    p.base_next = carry_base(l->t + n_in);
    p.n_in = n_in;
    p.h_old = (int)(l->t / kHop);
    p.h_new = (int)((l->t + n_in) / kHop);
    p.n_streams = S;
    const long long t_new = l->t + n_in;
    p.q_lo = l->q_done;
    p.q_hi = flush ? t_new : (t_new - kTaps / 2 > l->q_done ? t_new - kTaps / 2 : l->q_done);   // i + K/2 <= T - 1
    if (p.h_new > p.h_old) {
        const long long rows = (long long)S * (p.h_new - p.h_old);
        const long long blocks = (rows + 64 / C - 1) / (64 / C);
        if (rows > INT32_MAX) return fail(l, AT3HIP_EINVAL, "too many hops in one call");   // (k_hops divides rows in 32 bits)
        if (C == 2) hipLaunchKernelGGL((k_hops<2, T>), dim3((unsigned)blocks), dim3(kHopThreads), 0, l->stream, p);
        else hipLaunchKernelGGL((k_hops<1, T>), dim3((unsigned)blocks), dim3(kHopThreads), 0, l->stream, p);
        HIPCHK(l, hipGetLastError());
    }
    if (l->cfg.true_peak && p.q_hi > p.q_lo) {
        const long long tiles = (p.q_hi - p.q_lo + kPeakQ - 1) / kPeakQ;
        const dim3 grid((unsigned)tiles, (unsigned)S);
        if (C == 2) hipLaunchKernelGGL((k_true_peak<2, T>), grid, dim3(kPeakThreads), 0, l->stream, p);
        else hipLaunchKernelGGL((k_true_peak<1, T>), grid, dim3(kPeakThreads), 0, l->stream, p);
        HIPCHK(l, hipGetLastError());
        l->q_done = p.q_hi;
    }
    if (n_in > 0) {
        const dim3 grid(kCarryBlocks, (unsigned)S);
        if (C == 2) hipLaunchKernelGGL((k_carry<2, T>), grid, dim3(kCarryThreads), 0, l->stream, p);
        else hipLaunchKernelGGL((k_carry<1, T>), grid, dim3(kCarryThreads), 0, l->stream, p);
        HIPCHK(l, hipGetLastError());
        l->cur ^= 1;
        l->t = t_new;
    }
    return AT3HIP_OK;
}

// The samples of a call in device memory: the caller's, or the staging of its sample type, allocated by the first call that
// takes host memory of that type.
template <typename T>
int stage_in(at3hip_loudness* l, const T* in, int n_in, uint32_t flags, const T** d_in)
{
    const size_t S = l->cfg.n_streams, C = l->cfg.channels;
    *d_in = reinterpret_cast<const T*>(l->d_carry[l->cur]);   // (no input: never read)
    if (n_in == 0) return AT3HIP_OK;
    return at3host::stage_in(l, at3host::pick<T>(l->d_in, l->d_in_s16), S * (size_t)l->cfg.max_in * C, in, S * n_in * C, flags, d_in);
}

// at3hip_loudness_process (T = float) and at3hip_loudness_process_s16 (T = int16_t)
template <typename T>
int process_impl(at3hip_loudness* l, const T* in, int32_t n_in, uint32_t flags)
{
    const uint32_t known = AT3HIP_PCM_ON_DEVICE | AT3HIP_ASYNC;
    if (!l) return AT3HIP_EINVAL;
    if ((n_in > 0 && !in) || n_in < 0 || n_in > l->cfg.max_in || (flags & ~known)) return fail(l, AT3HIP_EINVAL, "bad argument");
    if ((l->t + n_in) / kHop > l->cfg.max_hops) return fail(l, AT3HIP_EINVAL, "more hops than max_hops");
    at3host::DeviceGuard guard(l->device);
    HIPCHK(l, guard.error());
    const T* d_in = nullptr;
    int rc = stage_in(l, in, n_in, flags, &d_in);
    if (rc != AT3HIP_OK) return rc;
    if ((rc = launch(l, d_in, n_in, false)) != AT3HIP_OK) return rc;
    if (flags & AT3HIP_ASYNC) return AT3HIP_OK;
    HIPCHK(l, hipStreamSynchronize(l->stream));
    return AT3HIP_OK;
}

// at3hip_loudness_apply (T = float) and at3hip_loudness_apply_s16 (T = int16_t)
template <typename T>
int apply_impl(at3hip_loudness* l, const T* in, int32_t n_in, const float* gains, float* out, uint32_t flags)
{
    const uint32_t known = AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE | AT3HIP_ASYNC;
    if (!l) return AT3HIP_EINVAL;
    if (!gains || (n_in > 0 && (!in || !out)) || n_in < 0 || n_in > l->cfg.max_in || (flags & ~known))
        return fail(l, AT3HIP_EINVAL, "bad argument");
    if (n_in == 0) return AT3HIP_OK;
    at3host::DeviceGuard guard(l->device);
    HIPCHK(l, guard.error());
    const size_t S = l->cfg.n_streams, C = l->cfg.channels;
    const T* d_in = nullptr;
    float* d_out = nullptr;
    int rc = stage_in(l, in, n_in, flags, &d_in);
    if (rc == AT3HIP_OK) rc = at3host::stage_out(l, l->d_out, S * (size_t)l->cfg.max_in * C, out, flags, &d_out);
    if (rc != AT3HIP_OK) return rc;
    HIPCHK(l, hipMemcpyAsync(l->d_gain, gains, S * sizeof(float), hipMemcpyHostToDevice, l->stream));
    const long long n = (long long)n_in * C;
    const int vec = n % 4 == 0 && (uintptr_t)d_in % (4 * sizeof(T)) == 0 && (uintptr_t)d_out % 16 == 0;
    long long blocks = ((vec ? n / 4 : n) + kScaleThreads - 1) / kScaleThreads;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_scale<T>, dim3((unsigned)blocks, (unsigned)S), dim3(kScaleThreads), 0, l->stream, d_in, d_out, l->d_gain, n, vec);
    HIPCHK(l, hipGetLastError());
    return at3host::copy_out_and_wait(l, out, l->d_out, S * n * sizeof(float), flags);
}

}  // namespace

extern "C" {

int at3hip_loudness_gate(const double* z, int32_t n_hops, int32_t channels, at3hip_loudness_result* result)
{
    if (!result || n_hops < 0 || (n_hops > 0 && !z) || (channels != 1 && channels != 2)) return AT3HIP_EINVAL;
    gate(z, n_hops, channels, result);
    return AT3HIP_OK;
}

int at3hip_loudness_gain(const at3hip_loudness_result* result, double target_lufs, double ceiling_db, float* g)
{
    if (!result || !g) return AT3HIP_EINVAL;
    *g = gain_of(result, target_lufs, ceiling_db);
    return AT3HIP_OK;
}

int at3hip_loudness_create(const at3hip_loudness_config* cfg, at3hip_loudness** out)
{
    if (!cfg || !out) return AT3HIP_EINVAL;
    *out = nullptr;
    if ((cfg->channels != 1 && cfg->channels != 2) || cfg->n_streams < 1 || cfg->max_in < 1 || cfg->max_hops < 1 ||
        (cfg->true_peak != 0 && cfg->true_peak != 1))
        return AT3HIP_EINVAL;
    if (cfg->n_streams > at3host::kMaxGridY) return AT3HIP_EINVAL;   // the stream is gridDim.y
    return at3host::create_engine(cfg->device_id, out, at3hip_loudness_destroy, [&](at3hip_loudness* l) {
        l->cfg = *cfg;
        const size_t S = cfg->n_streams, C = cfg->channels;
        int rc;
        for (int b = 0; b < 2; ++b)
            if ((rc = dev_alloc(l, &l->d_carry[b], S * kWindow * C)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(l, &l->d_z, (size_t)cfg->max_hops * S * C)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(l, &l->d_peaks, S * 4)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(l, &l->d_gain, S)) != AT3HIP_OK) return rc;
        if (cfg->true_peak) {
            float host[kPhases * kTaps];
            if (at3hip_resampler_host_tables(44100, 176400, host, sizeof(host)) != AT3HIP_OK) return AT3HIP_EINVAL;
            if ((rc = dev_alloc(l, &l->d_hp, (size_t)kPhases * kTaps)) != AT3HIP_OK) return rc;
            if ((rc = at3host::upload_table(l->d_hp, host, sizeof(host))) != AT3HIP_OK) return rc;
        }
        return clear_state(l) != AT3HIP_OK || hipStreamSynchronize(l->stream) != hipSuccess ? AT3HIP_EDEVICE : AT3HIP_OK;
    });
}

void at3hip_loudness_destroy(at3hip_loudness* l)
{
    if (l) at3host::destroy_engine(l);
}

const char* at3hip_loudness_last_error(const at3hip_loudness* l) { return at3host::engine_last_error(l); }

int at3hip_loudness_reset(at3hip_loudness* l)
{
    return at3host::guarded(l, [](at3hip_loudness* l) {
        // the carry is read only for samples the counters say were received: the counters and the peaks are the state
        l->lim_on = false;   // (a limiter run ends here; its statistics stay readable)
        return clear_state(l);
    });
}

int at3hip_loudness_process(at3hip_loudness* l, const float* in, int32_t n_in, uint32_t flags) { return process_impl(l, in, n_in, flags); }

int at3hip_loudness_process_s16(at3hip_loudness* l, const int16_t* in, int32_t n_in, uint32_t flags) { return process_impl(l, in, n_in, flags); }

int at3hip_loudness_read_hops(at3hip_loudness* l, int32_t stream, void* dst, size_t bytes)
{
    if (!l) return AT3HIP_EINVAL;
    const size_t S = l->cfg.n_streams, C = l->cfg.channels, H = (size_t)(l->t / kHop);
    if (stream < 0 || (size_t)stream >= S || bytes != H * C * sizeof(double) || (bytes && !dst))
        return fail(l, AT3HIP_EINVAL, "bad argument");
    at3host::DeviceGuard guard(l->device);
    HIPCHK(l, guard.error());
    HIPCHK(l, hipStreamSynchronize(l->stream));
    for (size_t h = 0; h < H; ++h)
        HIPCHK(l, hipMemcpy((double*)dst + h * C, l->d_z + (h * S + (size_t)stream) * C, C * sizeof(double), hipMemcpyDeviceToHost));
    return AT3HIP_OK;
}

int at3hip_loudness_finish(at3hip_loudness* l, at3hip_loudness_result* results)
{
    if (!l) return AT3HIP_EINVAL;
    if (!results) return fail(l, AT3HIP_EINVAL, "bad argument");
    at3host::DeviceGuard guard(l->device);
    HIPCHK(l, guard.error());
    const size_t S = l->cfg.n_streams, C = l->cfg.channels, H = (size_t)(l->t / kHop);
    if (l->cfg.true_peak) {   // the converter's last outputs, zeros past the end
        const int rc = launch(l, (const float*)l->d_carry[l->cur], 0, true);
        if (rc != AT3HIP_OK) return rc;
    }
    std::vector<double> z(H * S * C), zs(H * C);
    std::vector<unsigned> peaks(S * 4);
    HIPCHK(l, hipStreamSynchronize(l->stream));
    if (H) HIPCHK(l, hipMemcpy(z.data(), l->d_z, z.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(l, hipMemcpy(peaks.data(), l->d_peaks, peaks.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < S; ++s) {
        at3hip_loudness_result& r = results[s];
        for (size_t h = 0; h < H; ++h)
            for (size_t c = 0; c < C; ++c) zs[h * C + c] = z[(h * S + s) * C + c];
        gate(zs.data(), (int)H, (int)C, &r);
        r.n_samples = l->t;
        for (int c = 0; c < 2; ++c) {
            const unsigned sp = peaks[(s * 2 + 0) * 2 + c], tp = peaks[(s * 2 + 1) * 2 + c];
            const unsigned both = tp > sp ? tp : sp;
            memcpy(&r.sample_peak[c], &sp, 4);
            r.true_peak[c] = 0.0f;
            if (l->cfg.true_peak) memcpy(&r.true_peak[c], &both, 4);
        }
    }
    return clear_state(l);
}

int at3hip_loudness_apply(at3hip_loudness* l, const float* in, int32_t n_in, const float* gains, float* out, uint32_t flags)
{
    return apply_impl(l, in, n_in, gains, out, flags);
}

int at3hip_loudness_apply_s16(at3hip_loudness* l, const int16_t* in, int32_t n_in, const float* gains, float* out, uint32_t flags)
{
    return apply_impl(l, in, n_in, gains, out, flags);
}

int at3hip_loudness_sync(at3hip_loudness* l) { return at3host::engine_sync(l); }

int at3hip_loudness_set_stream(at3hip_loudness* l, void* hip_stream) { return at3host::engine_set_stream(l, hip_stream); }

}  // extern "C"

#include "loudness_limit.hpp"
