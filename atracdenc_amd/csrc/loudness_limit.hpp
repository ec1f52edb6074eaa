// The look-ahead limiter of include/at3hip_loudness.h ("The look-ahead limiter"): kernels, host state and C entry points.
// Included by loudness.hip behind the meter's own code: it uses the meter's context, magnitude_bits and stage_in.
//
// Kernel layout. The stream is gridDim.y in every kernel; nothing in LDS is sized by the batch; every
// index that scales with the batch or the call is 64-bit.
//   k_limit_detect  step 1 and 2 for 256 consecutive n of one stream: q[n] as uint32 into the stream's q row. In true-peak mode
//                   the workgroup stages 256 + 143 samples and wavefront p computes phase p for 4 x 64 consecutive n with
//                   wave-uniform taps, as k_true_peak does (the same ascending fmaf chain); the four phases and the sample itself
//                   meet in an LDS word per n (integer max of magnitude bits). The sample mode stages nothing.
//   k_limit_gain    steps 3 - 5 and 7 for kLimTile consecutive outputs of one stream. Reads q with its H + 2A halo into LDS, takes
//                   the minimum over 2048 by doubling (11 passes, in place through registers), w[n] = min of two such windows
//                   (2426 = H + A + 1 <= 2 * 2048), then an int64 prefix sum over w (9 values per lane, Hillis-Steele across
//                   the lanes' totals) and S[n] as the difference of two prefix values; x * g * s and the clamp with one
//                   8-byte load and store per stereo sample where the buffers are 8-byte aligned; the statistics go through
//                   two 64-bit LDS words into two global atomics per workgroup (max of FULL - S, count).
//   k_limit_carry   what the next call needs: the last H + 2A values of q and the last A + 72 samples, into the other of two
//                   buffers each (a call reads one and writes the other).
//   k_limit_init    the start state: q = 2^30 and samples +0.0f before the stream's start.
#pragma once

namespace {

constexpr int kLimA = AT3HIP_LIMIT_LOOKAHEAD, kLimH = AT3HIP_LIMIT_HOLD;
constexpr int kLimQCarry = kLimH + 2 * kLimA;     // q[qd - 2645 .. qd) is what outputs from qd - A on can still read
constexpr int kLimXCarry = kLimA + kTaps / 2;     // samples [t - 292, t): outputs lag by at most A + 72
constexpr int kLimThreads = 256;
constexpr int kLimDetect = 256;                   // n per workgroup of k_limit_detect
constexpr int kLimTile = 2048;                    // outputs per workgroup of k_limit_gain
constexpr int kLimSpan = 2048;                    // the doubling's window
constexpr int kLimNQ = kLimTile + kLimQCarry;     // q values a tile reads
constexpr int kLimNW = kLimTile + kLimA;          // w values a tile sums
constexpr int kLimPerLaneQ = (kLimNQ + kLimThreads - 1) / kLimThreads;   // 19
constexpr int kLimPerLaneW = (kLimNW + kLimThreads - 1) / kLimThreads;   // 9
constexpr unsigned kLimOne = 1u << 30;
constexpr unsigned long long kLimFull = (unsigned long long)AT3HIP_LIMIT_FULL;
static_assert(kLimH + kLimA + 1 <= 2 * kLimSpan && kLimH + kLimA + 1 >= kLimSpan, "two windows of the doubling must cover H + A + 1");
static_assert(kLimFull == (unsigned long long)(kLimA + 1) << 30, "AT3HIP_LIMIT_FULL");

struct LimitParams {
    const float* xc;             // [S][kLimXCarry][C]: samples t_old - 292 .. t_old - 1 (+0.0f before the start)
    float* xc_next;              // the same for t_old + n_in
    const uint32_t* qb;          // [S][q_stride]: q[qd_old - 2645 .. qd_old), then this call's q[qd_old .. qd_new)
    uint32_t* qb_next;           // [S][q_stride]: its first 2645 words are written by k_limit_carry
    uint32_t* qb_w;              // qb, for k_limit_detect's stores
    const void* in;              // [S][n_in][C] float or int16_t
    float* out;                  // [S][em_new - em_old][C]
    const float* gain;           // [S]
    const float* hp;             // [4][144]
    unsigned long long* stats;   // [S][2]: max of FULL - S, count of S < FULL
    size_t q_stride;
    long long t_old;             // samples received before this call
    long long qd_old, qd_new;    // q computed before and after this call
    long long em_old, em_new;    // outputs emitted before and after this call
    float ceiling;
    int n_in;
    int vec;                     // stereo float input and output behind 8-byte aligned pointers
};

// Sample n of channel c of stream s: +0.0f from the end of what was received, the carry below t_old, else this call's input.
template <int C, typename T>
__device__ __forceinline__ float lim_x(const LimitParams& p, size_t s, long long n, int c)
{
    if (n >= p.t_old + p.n_in) return 0.0f;
    if (n < p.t_old) return p.xc[(s * kLimXCarry + (size_t)(n - (p.t_old - kLimXCarry))) * C + c];
    const size_t i = (s * (size_t)p.n_in + (size_t)(n - p.t_old)) * C + c;
    if constexpr (std::is_same<T, float>::value) return static_cast<const float*>(p.in)[i];
    else return (float)static_cast<const int16_t*>(p.in)[i] * 0x1p-15f;
}

template <int C, typename T, bool TP>
__global__ __launch_bounds__(kLimThreads) void k_limit_detect(LimitParams p)
{
    using V = typename std::conditional<C == 2, float2, float>::type;
    __shared__ unsigned sm[kLimDetect];
    const size_t s = blockIdx.y;
    const int tid = threadIdx.x;
    const long long n0 = p.qd_old + (long long)blockIdx.x * kLimDetect;
    if constexpr (TP) {
        __shared__ V sx[kLimDetect + kTaps];
        // samples n0 - 71 .. n0 + 255 + 72 (n reads x[n + k - 71], k < 144)
        const long long first = n0 - (kTaps / 2 - 1);
        for (int j = tid; j < kLimDetect + kTaps - 1; j += kLimThreads) {
            V w;
            if constexpr (C == 2) w = make_float2(lim_x<C, T>(p, s, first + j, 0), lim_x<C, T>(p, s, first + j, 1));
            else w = lim_x<C, T>(p, s, first + j, 0);
            sx[j] = w;
        }
        __syncthreads();
        {
            const V own = sx[tid + kTaps / 2 - 1];
            unsigned m;
            if constexpr (C == 2) {
                const unsigned a = magnitude_bits(own.x), b = magnitude_bits(own.y);
                m = a > b ? a : b;
            } else {
                m = magnitude_bits(own);
            }
            sm[tid] = m;
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
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            unsigned b = magnitude_bits(acc[m][0]);
            if constexpr (C == 2) {
                const unsigned b1 = magnitude_bits(acc[m][1]);
                b = b1 > b ? b1 : b;
            }
            atomicMax(&sm[lane + 64 * m], b);
        }
        __syncthreads();
    } else {
        unsigned m = magnitude_bits(lim_x<C, T>(p, s, n0 + tid, 0));
        if constexpr (C == 2) {
            const unsigned b = magnitude_bits(lim_x<C, T>(p, s, n0 + tid, 1));
            m = b > m ? b : m;
        }
        sm[tid] = m;
    }
    const long long n = n0 + tid;
    if (n < p.qd_new) {
        const double e = (double)p.gain[s] * (double)__uint_as_float(sm[tid]);
        const double r = e > (double)p.ceiling ? (double)p.ceiling / e : 1.0;
        p.qb_w[s * p.q_stride + (size_t)kLimQCarry + (size_t)(n - p.qd_old)] = (uint32_t)(r * 1073741824.0);
    }
}

// (double) -> float toward zero, d >= 0
__device__ __forceinline__ float lim_float_rz(double d)
{
    float f = (float)d;
    if ((double)f > d) f = __uint_as_float(__float_as_uint(f) - 1u);
    return f;
}

template <int C, typename T>
__global__ __launch_bounds__(kLimThreads) void k_limit_gain(LimitParams p)
{
    __shared__ unsigned sq[kLimNQ];                    // q[n0 - A - H + i], then the doubling's minima
    __shared__ unsigned long long sp[kLimNW + 1];      // prefix sums of w[n0 - A + i]
    __shared__ unsigned long long ts[kLimThreads];
    __shared__ unsigned long long red[2];
    const size_t s = blockIdx.y;
    const int tid = threadIdx.x;
    const long long n0 = p.em_old + (long long)blockIdx.x * kLimTile;
    if (tid < 2) red[tid] = 0;
    {
        const uint32_t* qrow = p.qb + s * p.q_stride;
        const long long first = n0 - kLimA - kLimH;    // >= qd_old - kLimQCarry: em_old >= qd_old - A
        for (int i = tid; i < kLimNQ; i += kLimThreads) {
            const long long n = first + i;
            sq[i] = n < p.qd_new ? qrow[(size_t)((long long)kLimQCarry + (n - p.qd_old))] : kLimOne;   // (2^30 past the flush)
        }
    }
    __syncthreads();
    // sq[i] = min(q[i .. i + 2047]) wherever that window lies inside the tile's q
    for (int d = 1; d < kLimSpan; d <<= 1) {
        unsigned v[kLimPerLaneQ];
#pragma unroll
        for (int j = 0; j < kLimPerLaneQ; ++j) {
            const int i = tid + kLimThreads * j;
            unsigned a = i < kLimNQ ? sq[i] : 0u;
            if (i + d < kLimNQ) {
                const unsigned b = sq[i + d];
                a = b < a ? b : a;
            }
            v[j] = a;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kLimPerLaneQ; ++j) {
            const int i = tid + kLimThreads * j;
            if (i < kLimNQ) sq[i] = v[j];
        }
        __syncthreads();
    }
    // w[n0 - A + i] = min(q[i .. i + H + A]) of the tile's q = the two windows of 2048 at i and at i + H + A + 1 - 2048; lane tid
    // sums its 9 consecutive w
    constexpr int kSecond = kLimH + kLimA + 1 - kLimSpan;
    unsigned w[kLimPerLaneW];
    unsigned long long total = 0;
#pragma unroll
    for (int j = 0; j < kLimPerLaneW; ++j) {
        const int i = tid * kLimPerLaneW + j;
        unsigned a = 0;
        if (i < kLimNW) {
            a = sq[i];
            const unsigned b = sq[i + kSecond];
            a = b < a ? b : a;
        }
        w[j] = a;
        total += a;
    }
    for (int d = 1; d < kLimThreads; d <<= 1) {
        ts[tid] = total;
        __syncthreads();
        if (tid >= d) total += ts[tid - d];
        __syncthreads();
    }
    {
        unsigned long long run = total;   // inclusive over the lanes: walk back through the lane's own values
#pragma unroll
        for (int j = kLimPerLaneW - 1; j >= 0; --j) {
            const int i = tid * kLimPerLaneW + j;
            if (i < kLimNW) sp[i + 1] = run;
            run -= w[j];
        }
        if (tid == 0) sp[0] = 0;
    }
    __syncthreads();
    const float g = p.gain[s], c = p.ceiling;
    const long long n_out = p.em_new - p.em_old;
    float* orow = p.out + s * (size_t)n_out * C;
    unsigned long long deficit = 0, count = 0;
#pragma unroll 2
    for (int k = 0; k < kLimTile / kLimThreads; ++k) {
        const int i = tid + kLimThreads * k;
        const long long n = n0 + i;
        if (n >= p.em_new) break;
        const unsigned long long S = sp[i + kLimA + 1] - sp[i];
        if (S < kLimFull) {
            ++count;
            deficit = kLimFull - S > deficit ? kLimFull - S : deficit;
        }
        const float sm = lim_float_rz((double)(long long)S / (double)AT3HIP_LIMIT_FULL);
        float x[C];
        if constexpr (C == 2 && std::is_same<T, float>::value) {
            if (p.vec && n >= p.t_old) {
                const float2 v = *reinterpret_cast<const float2*>(static_cast<const float*>(p.in) + (s * (size_t)p.n_in + (size_t)(n - p.t_old)) * 2);
                x[0] = v.x;
                x[1] = v.y;
            } else {
                x[0] = lim_x<C, T>(p, s, n, 0);
                x[1] = lim_x<C, T>(p, s, n, 1);
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) x[ch] = lim_x<C, T>(p, s, n, ch);
        }
        float y[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const float t = (x[ch] * g) * sm;
            y[ch] = t > c ? c : (t < -c ? -c : t);
        }
        const size_t o = (size_t)(n - p.em_old) * C;
        if constexpr (C == 2) {
            if (p.vec) {
                *reinterpret_cast<float2*>(orow + o) = make_float2(y[0], y[1]);
            } else {
                orow[o] = y[0];
                orow[o + 1] = y[1];
            }
        } else {
            orow[o] = y[0];
        }
    }
    if (count) {
        atomicMax(&red[0], deficit);
        atomicAdd(&red[1], count);
    }
    __syncthreads();
    if (tid == 0 && red[1]) {
        atomicMax(&p.stats[s * 2 + 0], red[0]);
        atomicAdd(&p.stats[s * 2 + 1], red[1]);
    }
}

template <int C, typename T>
__global__ __launch_bounds__(kLimThreads) void k_limit_carry(LimitParams p)
{
    const size_t s = blockIdx.y;
    const int at = blockIdx.x * kLimThreads + threadIdx.x, stride = gridDim.x * kLimThreads;
    const size_t n_q = (size_t)(p.qd_new - p.qd_old);
    for (int i = at; i < kLimQCarry; i += stride) p.qb_next[s * p.q_stride + i] = p.qb[s * p.q_stride + n_q + i];
    const long long first = p.t_old + p.n_in - kLimXCarry;   // >= t_old - kLimXCarry
    for (int i = at; i < kLimXCarry * C; i += stride) p.xc_next[s * (size_t)kLimXCarry * C + i] = lim_x<C, T>(p, s, first + i / C, i % C);
}

__global__ __launch_bounds__(kLimThreads) void k_limit_init(uint32_t* qb, size_t q_stride, float* xc, int C)
{
    const size_t s = blockIdx.y;
    const int at = blockIdx.x * kLimThreads + threadIdx.x, stride = gridDim.x * kLimThreads;
    for (int i = at; i < kLimQCarry; i += stride) qb[s * q_stride + i] = kLimOne;
    for (int i = at; i < kLimXCarry * C; i += stride) xc[s * (size_t)kLimXCarry * C + i] = 0.0f;
}

constexpr int kLimCarryBlocks = 4;

size_t limit_q_stride(const at3hip_loudness* l) { return (size_t)kLimQCarry + (size_t)(l->cfg.max_in > kTaps / 2 ? l->cfg.max_in : kTaps / 2); }

int limit_delay(uint32_t flags) { return kLimA + ((flags & AT3HIP_LIMIT_TRUE_PEAK) ? kTaps / 2 : 0); }

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// at3hip_loudness_limit (T = float), at3hip_loudness_limit_s16 (T = int16_t) and, with flush, at3hip_loudness_limit_flush
template <typename T>
int limit_impl(at3hip_loudness* l, const T* in, int32_t n_in, float* out, int32_t* n_out, uint32_t flags, bool flush)
{
    const uint32_t known = (flush ? 0u : AT3HIP_PCM_ON_DEVICE) | AT3HIP_OUT_ON_DEVICE | AT3HIP_ASYNC;
    if (!l) return AT3HIP_EINVAL;
    if (!n_out || (n_in > 0 && !in) || n_in < 0 || (flags & ~known)) return fail(l, AT3HIP_EINVAL, "bad argument");
    if (n_in > l->cfg.max_in) return fail(l, AT3HIP_EINVAL, "n_in above max_in");
    if (!l->lim_on) return fail(l, AT3HIP_EINVAL, "no limiter run is open: call at3hip_loudness_limit_start first");
    const int C = l->cfg.channels;
    const size_t S = l->cfg.n_streams;
    const bool tp = (l->lim_flags & AT3HIP_LIMIT_TRUE_PEAK) != 0;
    const long long t_new = l->lim_t + n_in;
    long long qd_new = flush ? t_new : t_new - (tp ? kTaps / 2 : 0);
    if (qd_new < l->lim_qd) qd_new = l->lim_qd;
    long long em_new = flush ? t_new : qd_new - kLimA;
    if (em_new < l->lim_em) em_new = l->lim_em;
    const long long n_new = em_new - l->lim_em, n_q = qd_new - l->lim_qd;
    if (n_new > 0 && !out) return fail(l, AT3HIP_EINVAL, "bad argument");
    if ((flags & AT3HIP_PCM_ON_DEVICE) && (flags & AT3HIP_OUT_ON_DEVICE) &&
        ranges_overlap(in, S * (size_t)n_in * C * sizeof(T), out, S * (size_t)n_new * C * sizeof(float)))
        return fail(l, AT3HIP_EINVAL, "the limiter's output cannot overlap its input");
    *n_out = (int32_t)n_new;
    if (n_in == 0 && !flush) return AT3HIP_OK;
    at3host::DeviceGuard guard(l->device);
    HIPCHK(l, guard.error());
    const T* d_in = nullptr;
    if (n_in > 0) {
        const int rc = stage_in(l, in, n_in, flags, &d_in);
        if (rc != AT3HIP_OK) return rc;
    }
    float* d_out = nullptr;
    const size_t most = (size_t)(l->cfg.max_in > kLimXCarry ? l->cfg.max_in : kLimXCarry);
    if (const int rc = at3host::stage_out(l, l->d_lim_out, S * most * C, out, flags, &d_out)) return rc;
    LimitParams p;
    p.xc = l->d_lim_x[l->lim_cur];
    p.xc_next = l->d_lim_x[l->lim_cur ^ 1];
    p.qb = p.qb_w = l->d_lim_q[l->lim_cur];
    p.qb_next = l->d_lim_q[l->lim_cur ^ 1];
    p.in = d_in;
    p.out = d_out;
    p.gain = l->d_lim_gain;
    p.hp = l->d_hp;
    p.stats = l->d_lim_stats;
    p.q_stride = limit_q_stride(l);
    p.t_old = l->lim_t;
    p.qd_old = l->lim_qd;
    p.qd_new = qd_new;
    p.em_old = l->lim_em;
    p.em_new = em_new;
    p.ceiling = l->lim_ceiling;
    p.n_in = n_in;
    p.vec = C == 2 && sizeof(T) == sizeof(float) && (uintptr_t)d_in % 8 == 0 && (uintptr_t)d_out % 8 == 0;
    const dim3 block(kLimThreads);
    if (n_q > 0) {
        const dim3 grid((unsigned)((n_q + kLimDetect - 1) / kLimDetect), (unsigned)S);
        if (tp) {
            if (C == 2) hipLaunchKernelGGL((k_limit_detect<2, T, true>), grid, block, 0, l->stream, p);
            else hipLaunchKernelGGL((k_limit_detect<1, T, true>), grid, block, 0, l->stream, p);
        } else {
            if (C == 2) hipLaunchKernelGGL((k_limit_detect<2, T, false>), grid, block, 0, l->stream, p);
            else hipLaunchKernelGGL((k_limit_detect<1, T, false>), grid, block, 0, l->stream, p);
        }
        HIPCHK(l, hipGetLastError());
    }
    if (n_new > 0) {
        const dim3 grid((unsigned)((n_new + kLimTile - 1) / kLimTile), (unsigned)S);
        if (C == 2) hipLaunchKernelGGL((k_limit_gain<2, T>), grid, block, 0, l->stream, p);
        else hipLaunchKernelGGL((k_limit_gain<1, T>), grid, block, 0, l->stream, p);
        HIPCHK(l, hipGetLastError());
    }
    if (!flush) {
        const dim3 grid(kLimCarryBlocks, (unsigned)S);
        if (C == 2) hipLaunchKernelGGL((k_limit_carry<2, T>), grid, block, 0, l->stream, p);
        else hipLaunchKernelGGL((k_limit_carry<1, T>), grid, block, 0, l->stream, p);
        HIPCHK(l, hipGetLastError());
        l->lim_cur ^= 1;
    }
    l->lim_t = t_new;
    l->lim_qd = qd_new;
    l->lim_em = em_new;
    if (flush) l->lim_on = false;
    return at3host::copy_out_and_wait(l, out, l->d_lim_out, S * (size_t)n_new * C * sizeof(float), flags);
}

}  // namespace

extern "C" {

int32_t at3hip_loudness_limit_delay(uint32_t flags) { return limit_delay(flags); }

int at3hip_loudness_limit_start(at3hip_loudness* l, const float* gains, float ceiling, uint32_t flags)
{
    if (!l) return AT3HIP_EINVAL;
    if (!gains || (flags & ~AT3HIP_LIMIT_TRUE_PEAK)) return fail(l, AT3HIP_EINVAL, "bad argument");
    if (!(ceiling > 0.0f) || !std::isfinite(ceiling)) return fail(l, AT3HIP_EINVAL, "the ceiling must be finite and above 0");
    for (int s = 0; s < l->cfg.n_streams; ++s)
        if (!(gains[s] >= 0.0f) || !std::isfinite(gains[s])) return fail(l, AT3HIP_EINVAL, "a gain must be finite and at least 0");
    if (l->lim_on) return fail(l, AT3HIP_EINVAL, "a limiter run is open: flush or reset it first");
    at3host::DeviceGuard guard(l->device);
    HIPCHK(l, guard.error());
    const size_t S = l->cfg.n_streams, C = l->cfg.channels, stride = limit_q_stride(l);
    int rc;
    if (!l->d_lim_stats) {   // the first start
        for (int b = 0; b < 2; ++b) {
            if ((rc = dev_alloc(l, &l->d_lim_q[b], S * stride)) != AT3HIP_OK) return rc;
            if ((rc = dev_alloc(l, &l->d_lim_x[b], S * kLimXCarry * C)) != AT3HIP_OK) return rc;
        }
        if ((rc = dev_alloc(l, &l->d_lim_gain, S)) != AT3HIP_OK) return rc;
        if ((rc = dev_alloc(l, &l->d_lim_stats, S * 2)) != AT3HIP_OK) return rc;
    }
    if ((flags & AT3HIP_LIMIT_TRUE_PEAK) && !l->d_hp) {   // (a meter created with true_peak has the table already)
        float host[kPhases * kTaps];
        if (at3hip_resampler_host_tables(44100, 176400, host, sizeof(host)) != AT3HIP_OK) return fail(l, AT3HIP_EINVAL, "converter table");
        if ((rc = dev_alloc(l, &l->d_hp, (size_t)kPhases * kTaps)) != AT3HIP_OK) return rc;
        if ((rc = at3host::upload_table(l->d_hp, host, sizeof(host))) != AT3HIP_OK) return fail(l, rc, "table upload");
    }
    HIPCHK(l, hipMemcpyAsync(l->d_lim_gain, gains, S * sizeof(float), hipMemcpyHostToDevice, l->stream));
    HIPCHK(l, hipMemsetAsync(l->d_lim_stats, 0, S * 2 * sizeof(unsigned long long), l->stream));
    l->lim_cur = 0;
    hipLaunchKernelGGL(k_limit_init, dim3(kLimCarryBlocks, (unsigned)S), dim3(kLimThreads), 0, l->stream, l->d_lim_q[0], stride, l->d_lim_x[0], (int)C);
    HIPCHK(l, hipGetLastError());
    l->lim_flags = flags;
    l->lim_ceiling = ceiling;
    l->lim_t = l->lim_qd = l->lim_em = 0;
    l->lim_on = true;
    return AT3HIP_OK;
}

int at3hip_loudness_limit(at3hip_loudness* l, const float* in, int32_t n_in, float* out, int32_t* n_out, uint32_t flags)
{
    return limit_impl(l, in, n_in, out, n_out, flags, false);
}

int at3hip_loudness_limit_s16(at3hip_loudness* l, const int16_t* in, int32_t n_in, float* out, int32_t* n_out, uint32_t flags)
{
    return limit_impl(l, in, n_in, out, n_out, flags, false);
}

int at3hip_loudness_limit_flush(at3hip_loudness* l, float* out, int32_t* n_out, uint32_t flags)
{
    return limit_impl<float>(l, nullptr, 0, out, n_out, flags, true);
}

int at3hip_loudness_limit_stats(at3hip_loudness* l, at3hip_limit_stats* stats)
{
    if (!l) return AT3HIP_EINVAL;
    if (!stats) return fail(l, AT3HIP_EINVAL, "bad argument");
    if (!l->d_lim_stats) return fail(l, AT3HIP_EINVAL, "no limiter run was started");
    at3host::DeviceGuard guard(l->device);
    HIPCHK(l, guard.error());
    const size_t S = l->cfg.n_streams;
    std::vector<unsigned long long> raw(S * 2);
    HIPCHK(l, hipStreamSynchronize(l->stream));
    HIPCHK(l, hipMemcpy(raw.data(), l->d_lim_stats, raw.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < S; ++s) {
        stats[s].min_sum = (int64_t)(kLimFull - raw[s * 2]);
        stats[s].n_limited = (int64_t)raw[s * 2 + 1];
        stats[s].n_out = l->lim_em;
    }
    return AT3HIP_OK;
}

}  // extern "C"
