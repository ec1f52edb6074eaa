// The batched sample-rate converter (include/at3hip_resample.h): table builder, the k_resample kernel and the C ABI.
//
// Kernel layout. Output n = q L + r has i = q M + floor(r M / L) and phase (r M) mod L, so the outputs
// of one residue r share their phase and their input windows lie exactly M samples apart. A workgroup takes a tile of Q
// consecutive q (Q <= 64) of one stream: it stages the tile's input span (Q M + K - 1 samples, every channel) in LDS once,
// then each wavefront takes residues r = w, w + 8, ... with lane j on q = q0 + j. The taps are then wave-uniform (vector
// loads of one address per wavefront, global_load_dwordx4 through the caches, tables of every size alike) and every lane runs
// the definition's fmaf chain over its own window in LDS. Lane j's window starts at j M + u: with M even the span is stored with one pad sample after every M samples,
// so that consecutive lanes sit M + 1 (odd) samples apart and a ds_read_b64 / ds_read_b32 of a wavefront touches every bank
// once per half-wave.
#include <cmath>
#include <cstring>
#include <new>
#include <type_traits>

#include <hip/hip_runtime.h>

#include "../../include/at3hip_resample.h"
#include "at3_host_util.hpp"
#include "at3_pcm_in.hpp"

using at3host::dev_alloc;
using at3host::fail;

namespace {

constexpr int kThreads = 512;              // 8 wavefronts per workgroup
constexpr int kLdsBytes = 80 * 1024;       // two workgroups per CU
constexpr int kMaxQ = 64;                  // q per tile: one per lane

struct Shape {
    int L, M, K;
};

bool rate_ok(int hz)
{
    static const int kRates[] = {8000, 11025, 16000, 22050, 24000, 32000, 48000, 88200, 96000, 176400, 192000};
    for (int r : kRates)
        if (hz == r) return true;
    return false;
}

int gcd_int(int a, int b)
{
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

bool shape_of(int in, int out, Shape* s)
{
    if (!((in == 44100 && rate_ok(out)) || (out == 44100 && rate_ok(in)))) return false;
    const int g = gcd_int(in, out);
    const int f_lo = in < out ? in : out;
    s->L = out / g;
    s->M = in / g;
    s->K = 2 * (int)((72ll * in + f_lo - 1) / f_lo);
    return true;
}

double bessel_i0(double x)
{
    const double q = (x / 2) * (x / 2);
    double t = 1.0, sum = 0.0;
    sum += t;
    for (int m = 1; m < 40; ++m) {
        t = t * q / ((double)m * m);
        sum += t;
    }
    return sum;
}

// hp[L][K] of the definition (at3hip_resample.h), in double, rounded once. optnone: the host compiler must not fold or
// reassociate what the restatement computes step by step.
__attribute__((optnone, noinline)) void build_table(int in, int out, const Shape& s, float* hp)
{
    const int f_lo = in < out ? in : out;
    const double fc = 0.47675 * f_lo / in;
    const double beta = 0.1102 * (100.0 - 8.7);
    const double i0_beta = bessel_i0(beta);
    const int half = s.K / 2;
    for (int p = 0; p < s.L; ++p)
        for (int k = 0; k < s.K; ++k) {
            const double d = (double)(k - (half - 1)) - (double)p / s.L;
            const double x = 2 * fc * d;
            const double sinc = x == 0.0 ? 1.0 : sin(M_PI * x) / (M_PI * x);
            const double r = d / half;
            double w = 1 - r * r;
            if (w < 0) w = 0;
            hp[(size_t)p * s.K + k] = (float)(2 * fc * sinc * bessel_i0(beta * sqrt(w)) / i0_beta);
        }
}

struct ResampleParams {
    const float* hist;    // [S][K][C]: input samples T_old - K .. T_old - 1 of each stream (read)
    float* hist_next;     // [S][K][C]: samples T_new - K .. T_new - 1 (written by the first workgroup of each stream)
    const void* in;       // [S][n_in][C], float or int16_t: the kernel's template parameter TI
    void* out;            // [S][n_out][C], float or int16_t: TO
    const float* hp;      // [L][K]
    long long t_old;      // input samples of each stream before this call
    long long n0;         // first output of this call
    int n_in, n_out;
    int L, M, K;
    int Q, pad;           // q per tile; pad samples after every M in LDS (0 or 1)
};

// Input sample a of a stream (absolute index): zeros before the start and from T_new on; unneeded samples older than the
// history also read as zeros (only outputs this call does not emit reach them).
// in: the stream's row of this call, float or 16-bit (at3_pcm_in.hpp: a stereo sample is then one 32-bit load where the row is
// 4-byte aligned); the history is float for both.
template <int C, typename TI>
__device__ __forceinline__ void sample(const ResampleParams& p, const float* hist, const TI* in, bool pairs, long long a, float* v)
{
    const long long t_new = p.t_old + p.n_in;
    if (a < 0 || a >= t_new || a < p.t_old - p.K) {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = 0.0f;
    } else if (a < p.t_old) {
        const float* s = hist + (a - (p.t_old - p.K)) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = s[c];
    } else if constexpr (std::is_same<TI, float>::value) {
        const float* s = in + (a - p.t_old) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = s[c];
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = at3::pcm_at(in, (size_t)(a - p.t_old) * C + c, (size_t)p.n_in * C, pairs);
    }
}

// The output's 16-bit form is the decoders' (AT3HIP_RESAMPLE_OUT_S16): lrintf(clamp(x, -1, 1) * 32767.0f).
__device__ __forceinline__ void store_out(float* o, float x) { *o = x; }
__device__ __forceinline__ void store_out(int16_t* o, float x)
{
    const float y = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
    *o = (int16_t)__float2int_rn(y * 32767.0f);
}

template <int C, typename TI, typename TO>
__global__ __launch_bounds__(kThreads) void k_resample(ResampleParams p)
{
    using V = typename std::conditional<C == 2, float2, float>::type;
    __shared__ V sx[kLdsBytes / sizeof(V)];
    const size_t s = blockIdx.y;
    const float* hist = p.hist + s * (size_t)p.K * C;
    const TI* in = static_cast<const TI*>(p.in) + s * (size_t)p.n_in * C;
    const bool pairs = at3::pcm_pairs(in);
    const int tid = threadIdx.x;

    if (blockIdx.x == 0) {   // the history the next call reads
        float* hn = p.hist_next + s * (size_t)p.K * C;
        for (int j = tid; j < p.K; j += kThreads) {
            float v[C];
            sample<C>(p, hist, in, pairs, p.t_old + p.n_in - p.K + j, v);
#pragma unroll
            for (int c = 0; c < C; ++c) hn[(size_t)j * C + c] = v[c];
        }
    }
    if (p.n_out == 0) return;

    const long long q_lo = p.n0 / p.L;
    const long long q0 = q_lo + (long long)blockIdx.x * p.Q;
    const long long n_end = p.n0 + p.n_out;
    if (q0 * p.L >= n_end) return;
    const int half = p.K / 2;
    const long long s0 = q0 * p.M - (half - 1);   // absolute index of the span's first sample
    const int span = p.Q * p.M + p.K - 1;
    for (int j = tid; j < span; j += kThreads) {
        float v[C];
        sample<C>(p, hist, in, pairs, s0 + j, v);
        V w;
        if constexpr (C == 2) w = make_float2(v[0], v[1]);
        else w = v[0];
        sx[j + p.pad * (j / p.M)] = w;
    }
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const long long q = q0 + lane;
    TO* out = static_cast<TO*>(p.out) + s * (size_t)p.n_out * C;
    const V* xl = sx + lane * (p.M + p.pad);
    for (int r = wave; r < p.L; r += kThreads / 64) {
        const long long n = q * p.L + r;
        if (lane >= p.Q || n < p.n0 || n >= n_end) continue;
        const int rm = r * p.M;
        const int u0 = rm / p.L;             // floor(r M / L): the window's offset in the lane's span
        const float* h = p.hp + (size_t)(rm % p.L) * p.K;
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0f;
        int k = 0, u = u0;
        while (k < p.K) {   // segments between the pad samples (one segment when pad = 0)
            const int seg = p.pad ? (u / p.M + 1) * p.M - u : p.K;
            const int k_end = min(p.K, k + seg);
            const V* x = xl + u + p.pad * (u / p.M);
            u += k_end - k;
            for (; k + 4 <= k_end; k += 4, x += 4) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float hk = h[k + t];
                    const V xv = x[t];
                    if constexpr (C == 2) {
                        acc[0] = __builtin_fmaf(hk, xv.x, acc[0]);
                        acc[1] = __builtin_fmaf(hk, xv.y, acc[1]);
                    } else {
                        acc[0] = __builtin_fmaf(hk, xv, acc[0]);
                    }
                }
            }
            for (; k < k_end; ++k, ++x) {
                const float hk = h[k];
                const V xv = x[0];
                if constexpr (C == 2) {
                    acc[0] = __builtin_fmaf(hk, xv.x, acc[0]);
                    acc[1] = __builtin_fmaf(hk, xv.y, acc[1]);
                } else {
                    acc[0] = __builtin_fmaf(hk, xv, acc[0]);
                }
            }
        }
        TO* o = out + (size_t)(n - p.n0) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) store_out(o + c, acc[c]);
    }
}

}  // namespace

struct at3hip_resampler : at3host::EngineBase {
    at3hip_resampler_config cfg;
    Shape sh;
    int Q = 0, pad = 0, max_out = 0;
    float* d_hp = nullptr;          // [L][K]
    float* d_hist[2] = {nullptr, nullptr};   // [S][K][C], read / written alternately
    int cur = 0;
    float* d_in = nullptr;          // staging for host input  [S][max_in][C], allocated by the first call that needs it
    int16_t* d_in_s16 = nullptr;    // the same as 16-bit samples, allocated by the first at3hip_resampler_process_s16 that needs it
    float* d_out = nullptr;         // staging for host output [S][max_out][C], likewise (16-bit output uses its first half)
    long long t_in = 0;             // input samples received per stream since the start
    long long t_out = 0;            // outputs emitted per stream since the start
};

namespace {

// ceil(a L / M) for a > 0, else 0: the outputs whose i is below a
long long outputs_below(long long a, const Shape& s) { return a <= 0 ? 0 : (a * s.L + s.M - 1) / s.M; }

template <int C, typename TI>
void launch_kernel(const at3hip_resampler* r, const dim3& grid, const ResampleParams& p, bool out_s16)
{
    if (out_s16) hipLaunchKernelGGL((k_resample<C, TI, int16_t>), grid, dim3(kThreads), 0, r->stream, p);
    else hipLaunchKernelGGL((k_resample<C, TI, float>), grid, dim3(kThreads), 0, r->stream, p);
}

// Queues one call: n_in new samples (device memory), outputs [t_out, n_end) into out (device memory; int16_t with out_s16).
template <typename TI>
int launch(at3hip_resampler* r, const TI* in, int n_in, long long n_end, void* out, bool out_s16)
{
    const int C = r->cfg.channels;
    const Shape& sh = r->sh;
    ResampleParams p;
    p.hist = r->d_hist[r->cur];
    p.hist_next = r->d_hist[r->cur ^ 1];
    p.in = in;
    p.out = out;
    p.hp = r->d_hp;
    p.t_old = r->t_in;
    p.n0 = r->t_out;
    p.n_in = n_in;
    p.n_out = (int)(n_end - r->t_out);
    p.L = sh.L;
    p.M = sh.M;
    p.K = sh.K;
    p.Q = r->Q;
    p.pad = r->pad;
    long long tiles = 1;
    if (p.n_out > 0) tiles = ((n_end - 1) / sh.L - r->t_out / sh.L) / r->Q + 1;
    const dim3 grid((unsigned)tiles, (unsigned)r->cfg.n_streams);
    if (C == 2) launch_kernel<2, TI>(r, grid, p, out_s16);
    else launch_kernel<1, TI>(r, grid, p, out_s16);
    HIPCHK(r, hipGetLastError());
    r->cur ^= 1;
    r->t_in += n_in;
    r->t_out = n_end;
    return AT3HIP_OK;
}

int finish(at3hip_resampler* r, void* out, int n_out, uint32_t flags)
{
    const size_t elem = (flags & AT3HIP_RESAMPLE_OUT_S16) ? sizeof(int16_t) : sizeof(float);
    return at3host::copy_out_and_wait(r, out, r->d_out, (size_t)r->cfg.n_streams * n_out * r->cfg.channels * elem, flags);
}

// at3hip_resampler_process (TI = float) and at3hip_resampler_process_s16 (TI = int16_t)
template <typename TI>
int process_impl(at3hip_resampler* r, const TI* in, int32_t n_in, void* out, int32_t* n_out, uint32_t flags)
{
    const uint32_t known = AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE | AT3HIP_ASYNC | AT3HIP_RESAMPLE_OUT_S16;
    if (!r) return AT3HIP_EINVAL;
    if (!out || !n_out || (n_in > 0 && !in) || n_in < 0 || n_in > r->cfg.max_in || (flags & ~known))
        return fail(r, AT3HIP_EINVAL, "bad argument");
    at3host::DeviceGuard guard(r->device);
    HIPCHK(r, guard.error());
    const int C = r->cfg.channels;
    const size_t S = r->cfg.n_streams;
    // staging for host memory, allocated by the first call that takes or gives host memory: device buffers never need it
    const TI* d_in = reinterpret_cast<const TI*>(r->d_hist[r->cur]);   // (no input: never read)
    float* d_out = nullptr;
    int rc = AT3HIP_OK;
    if (n_in > 0) rc = at3host::stage_in(r, at3host::pick<TI>(r->d_in, r->d_in_s16), S * (size_t)r->cfg.max_in * C, in, S * n_in * C, flags, &d_in);
    if (rc == AT3HIP_OK) rc = at3host::stage_out(r, r->d_out, S * (size_t)r->max_out * C, (float*)out, flags, &d_out);
    if (rc != AT3HIP_OK) return rc;
    const long long n_end_new = outputs_below(r->t_in + n_in - r->sh.K / 2, r->sh);
    const long long n_end = n_end_new > r->t_out ? n_end_new : r->t_out;
    const int count = (int)(n_end - r->t_out);
    if ((rc = launch(r, d_in, n_in, n_end, d_out, (flags & AT3HIP_RESAMPLE_OUT_S16) != 0)) != AT3HIP_OK) return rc;
    *n_out = count;
    return finish(r, out, count, flags);
}

}  // namespace

extern "C" {

int at3hip_resampler_shape(int32_t in_rate, int32_t out_rate, int32_t* phases, int32_t* step, int32_t* taps)
{
    Shape s;
    if (!shape_of(in_rate, out_rate, &s)) return AT3HIP_EINVAL;
    if (phases) *phases = s.L;
    if (step) *step = s.M;
    if (taps) *taps = s.K;
    return AT3HIP_OK;
}

int at3hip_resampler_host_tables(int32_t in_rate, int32_t out_rate, void* dst, size_t bytes)
{
    Shape s;
    if (!dst || !shape_of(in_rate, out_rate, &s) || bytes != (size_t)s.L * s.K * sizeof(float)) return AT3HIP_EINVAL;
    build_table(in_rate, out_rate, s, (float*)dst);
    return AT3HIP_OK;
}

int at3hip_resampler_create(const at3hip_resampler_config* cfg, at3hip_resampler** out)
{
    if (!cfg || !out) return AT3HIP_EINVAL;
    *out = nullptr;
    Shape sh;
    if (!shape_of(cfg->in_rate, cfg->out_rate, &sh)) return AT3HIP_EINVAL;
    if ((cfg->channels != 1 && cfg->channels != 2) || cfg->n_streams < 1 || cfg->max_in < 1) return AT3HIP_EINVAL;
    if (cfg->n_streams > at3host::kMaxGridY) return AT3HIP_EINVAL;   // the stream is gridDim.y
    // LDS: the largest tile whose span (plus pads) fits; at least one q per tile
    const int C = cfg->channels, pad = (sh.M % 2 == 0) ? 1 : 0;
    int Q = kMaxQ;
    while (Q > 1) {
        const long long span = (long long)Q * sh.M + sh.K - 1;
        if ((span + pad * (span / sh.M) + 1) * C * (long long)sizeof(float) <= kLdsBytes) break;
        --Q;
    }
    {
        const long long span = (long long)Q * sh.M + sh.K - 1;
        if ((span + pad * (span / sh.M) + 1) * C * (long long)sizeof(float) > kLdsBytes) return AT3HIP_EINVAL;
    }
    const long long cap_process = ((long long)cfg->max_in * sh.L + sh.M - 1) / sh.M;
    const long long cap_flush = ((long long)(sh.K / 2) * sh.L + sh.M - 1) / sh.M;
    const long long max_out = cap_process > cap_flush ? cap_process : cap_flush;
    if (max_out > INT32_MAX) return AT3HIP_EINVAL;
    return at3host::create_engine(cfg->device_id, out, at3hip_resampler_destroy, [&](at3hip_resampler* r) {
        r->cfg = *cfg;
        r->sh = sh;
        r->Q = Q;
        r->pad = pad;
        r->max_out = (int)max_out;
        const size_t S = cfg->n_streams, table = (size_t)sh.L * sh.K;
        float* host = new (std::nothrow) float[table];
        if (!host) return AT3HIP_ENOMEM;
        build_table(cfg->in_rate, cfg->out_rate, sh, host);
        int rc = dev_alloc(r, &r->d_hp, table);
        if (rc == AT3HIP_OK) rc = at3host::upload_table(r->d_hp, host, table * sizeof(float));
        delete[] host;
        if (rc != AT3HIP_OK) return rc;
        for (int b = 0; b < 2; ++b)
            if ((rc = dev_alloc(r, &r->d_hist[b], S * sh.K * C)) != AT3HIP_OK) return rc;
        for (int b = 0; b < 2; ++b)
            if (hipMemsetAsync(r->d_hist[b], 0, S * sh.K * C * sizeof(float), r->stream) != hipSuccess) return AT3HIP_EDEVICE;
        return hipStreamSynchronize(r->stream) != hipSuccess ? AT3HIP_EDEVICE : AT3HIP_OK;
    });
}

void at3hip_resampler_destroy(at3hip_resampler* r)
{
    if (r) at3host::destroy_engine(r);
}

const char* at3hip_resampler_last_error(const at3hip_resampler* r) { return at3host::engine_last_error(r); }

int at3hip_resampler_reset(at3hip_resampler* r)
{
    if (!r) return AT3HIP_EINVAL;
    // the history is read only for samples T_old - K .. T_old - 1 of a stream: at T = 0 nothing of it, so the counters are the state
    r->t_in = 0;
    r->t_out = 0;
    return AT3HIP_OK;
}

int32_t at3hip_resampler_max_out(const at3hip_resampler* r) { return r ? r->max_out : AT3HIP_EINVAL; }

int at3hip_resampler_process(at3hip_resampler* r, const float* in, int32_t n_in, float* out, int32_t* n_out, uint32_t flags)
{
    return process_impl(r, in, n_in, out, n_out, flags);
}

int at3hip_resampler_process_s16(at3hip_resampler* r, const int16_t* in, int32_t n_in, void* out, int32_t* n_out, uint32_t flags)
{
    return process_impl(r, in, n_in, out, n_out, flags);
}

int at3hip_resampler_flush(at3hip_resampler* r, float* out, int32_t* n_out, uint32_t flags)
{
    const uint32_t known = AT3HIP_OUT_ON_DEVICE | AT3HIP_ASYNC | AT3HIP_PCM_ON_DEVICE | AT3HIP_RESAMPLE_OUT_S16;
    if (!r) return AT3HIP_EINVAL;
    if (!out || !n_out || (flags & ~known)) return fail(r, AT3HIP_EINVAL, "bad argument");
    at3host::DeviceGuard guard(r->device);
    HIPCHK(r, guard.error());
    const long long n_end = outputs_below(r->t_in, r->sh);
    const int count = (int)(n_end - r->t_out);
    float* d_out = nullptr;
    int rc = at3host::stage_out(r, r->d_out, (size_t)r->cfg.n_streams * r->max_out * r->cfg.channels, out, flags, &d_out);
    if (rc == AT3HIP_OK) rc = launch(r, (const float*)r->d_hist[r->cur], 0, n_end, d_out, (flags & AT3HIP_RESAMPLE_OUT_S16) != 0);   // (no input: never read)
    if (rc != AT3HIP_OK) return rc;
    *n_out = count;
    r->t_in = 0;
    r->t_out = 0;
    return finish(r, out, count, flags);
}

int at3hip_resampler_sync(at3hip_resampler* r) { return at3host::engine_sync(r); }

int at3hip_resampler_set_stream(at3hip_resampler* r, void* hip_stream) { return at3host::engine_set_stream(r, hip_stream); }

}  // extern "C"
