/* at3hip_resample.h - C ABI of the batched sample-rate converter: PCM at 8 .. 192 kHz to 44.1 kHz for the encoders, and the
 * decoders' 44.1 kHz output to another rate. Same library (libat3hip.so), prefix and error codes as at3hip.h. The reference
 * refuses every rate but 44100 (main.cpp:281, "unsupported sample rate"); this converter is this project's own definition,
 * written out below, restated in C by the test suite (tests/host/resample_cpu.c) and pinned to the GPU bit for bit.
 *
 * Definition.
 *   Rates. One side of the pair is 44100; the other is one of 8000, 11025, 16000, 22050, 24000, 32000, 48000, 88200, 96000,
 *   176400 or 192000. Any other pair, 44100 -> 44100 included, is AT3HIP_EINVAL.
 *   Constants. g = gcd(in, out); L = out / g phases; M = in / g, the input step; f_lo = min(in, out);
 *   K = 2 * ceil(72 * in / f_lo) taps per phase (integer arithmetic); in double: fc = 0.47675 * f_lo / in (cycles per input
 *   sample), beta = 0.1102 * (100.0 - 8.7).
 *   Table. hp[p][k] = (float)G(d) for p = 0 .. L-1, k = 0 .. K-1, d = (double)(k - (K/2 - 1)) - (double)p / L, all in double:
 *     G(d)    = 2 fc * sinc(2 fc * d) * I0(beta * sqrt(max(0, 1 - (d / (K/2))^2))) / I0(beta), evaluated left to right;
 *     sinc(x) = sin(M_PI * x) / (M_PI * x), sinc(0) = 1, with the host libm's sin and sqrt;
 *     I0(x)   = the sum of 40 terms m = 0 .. 39 added in ascending order from 0: t0 = 1, tm = t(m-1) * q / ((double)m * m)
 *               with q = (x / 2) * (x / 2).
 *   Output sample n of a stream (n from the stream's start, int64): i = floor(n M / L), p = (n M) mod L;
 *     acc = +0.0f; for k = 0 .. K-1 ascending: acc = fmaf(hp[p][k], x[i + k - (K/2 - 1)], acc); the output is acc.
 *   Samples before the stream's start are +0.0f. Each channel is filtered on its own. The filter is centred: output n sits at
 *   time n / out, no delay to trim, and a stream of T input samples gives exactly ceil(T L / M) outputs.
 *   Streaming. With T samples received so far a call emits every output whose last tap is available (i + K/2 <= T - 1);
 *   at3hip_resampler_flush emits the rest with zeros past the input's end and returns the stream to its start state. Every
 *   stream of a call takes the same n_in, so every stream gets the same number of outputs, which the host can compute alone
 *   (at3hip_resampler_max_out bounds it). Any split of the input into calls gives the same samples as one call.
 *
 * Expected properties of the float table (tests/test_resample_cpu.py): passband flat within +-0.001 dB up to 0.4535 f_lo,
 * stopband <= -99 dB from 0.5 f_lo, every phase's DC gain within 1e-5 of 1.
 *
 * The resampler is part of ABI 1.6 (see at3hip.h): a host that needs it looks for the symbol at3hip_resampler_create.
 */
#ifndef AT3HIP_RESAMPLE_H
#define AT3HIP_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#include "at3hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef struct at3hip_resampler at3hip_resampler;

typedef struct at3hip_resampler_config {
    int32_t in_rate;    /* Hz, see the rate list above */
    int32_t out_rate;   /* Hz; one of in_rate / out_rate is 44100 */
    int32_t channels;   /* 1 or 2 */
    int32_t n_streams;  /* independent streams converted side by side */
    int32_t max_in;     /* most input samples per stream (and channel) in one at3hip_resampler_process call */
    int32_t device_id;
} at3hip_resampler_config;

/* The context's stream is non-blocking; see DEVICE BUFFERS AND STREAMS (at3hip.h) and at3hip_resampler_set_stream. */
int at3hip_resampler_create(const at3hip_resampler_config* cfg, at3hip_resampler** out);
void at3hip_resampler_destroy(at3hip_resampler* r);
const char* at3hip_resampler_last_error(const at3hip_resampler* r);
/* Back to start-of-stream state for every stream (what flush leaves). */
int at3hip_resampler_reset(at3hip_resampler* r);
/* Output capacity per stream of one process or flush call: max(ceil(max_in L / M), ceil((K/2) L / M)). */
int32_t at3hip_resampler_max_out(const at3hip_resampler* r);

/* SAMPLES OUTSIDE THE FLOAT DOMAIN. Any float is accepted. An output is the definition's sum over K input samples in float32, so a NaN
 * or a sum that passes through inf - inf makes NaN the outputs whose K taps reach it (of unspecified sign and payload), an infinity
 * or an overflowing sum gives infinities, and the first output whose taps lie past the sample is exact again; every other output,
 * and every other stream of the call, has the definition's bits (tests/test_float_domain_gpu.py; no exception known). With
 * AT3HIP_RESAMPLE_OUT_S16 a NaN output is written as 0 and an infinite one as +-32767. */
/*   in  [n_streams][n_in][channels] float32, 0 <= n_in <= max_in
 *   out [n_streams][*n_out][channels] float32 (room for at3hip_resampler_max_out samples per stream)
 * flags: AT3HIP_PCM_ON_DEVICE (in is device memory), AT3HIP_OUT_ON_DEVICE, AT3HIP_ASYNC (only queue the call: in stays valid
 * and out is not read until at3hip_resampler_sync). *n_out is set before the call returns, also with AT3HIP_ASYNC. */
int at3hip_resampler_process(at3hip_resampler* r, const float* in, int32_t n_in, float* out, int32_t* n_out, uint32_t flags);
/* 16-bit output, the same bit as the decoders' *_DECODE_S16 flags: accepted by at3hip_resampler_process, at3hip_resampler_process_s16
 * and at3hip_resampler_flush. out is then int16 [n_streams][*n_out][channels], every sample lrintf(clamp(x, -1, 1) * 32767.0f) of
 * the float output x (the decoders' rule, behind a clamp). at3hip_resampler_process and at3hip_resampler_flush keep their
 * float* out prototypes: a caller casts its int16_t pointer. A library that predates at3hip_resampler_process_s16 rejects the bit
 * with AT3HIP_EINVAL in both: look for that symbol before setting it. */
#define AT3HIP_RESAMPLE_OUT_S16 8u
/* at3hip_resampler_process for 16-bit input: in [n_streams][n_in][channels] int16; layout, flags, limits and error codes as
 * above, out float32, or int16 with AT3HIP_RESAMPLE_OUT_S16. A sample s is taken as the float (float)s * 0x1p-15f (exact,
 * = s / 32768.0f: the rule of at3hip_encode_s16), so the outputs are, bit for bit, those of the float call on these floats. The
 * samples are widened by the kernel's loads: host memory crosses the bus as 16-bit (half the bytes; its staging buffer is
 * allocated by the first such call) and no float copy is written on the device. Calls of both kinds may alternate on one
 * resampler: the carried history is float. A device pointer needs only int16_t alignment (a mono stream's row starts at
 * s * n_in * 2 bytes). Added under ABI 1.6: a host looks for this symbol. */
int at3hip_resampler_process_s16(at3hip_resampler* r, const int16_t* in, int32_t n_in, void* out, int32_t* n_out, uint32_t flags);
/* The remaining outputs of every stream (zeros past the end of the input); then the start state. flags as above. */
int at3hip_resampler_flush(at3hip_resampler* r, float* out, int32_t* n_out, uint32_t flags);
/* Waits for everything queued on the resampler. */
int at3hip_resampler_sync(at3hip_resampler* r);
/* Queue this resampler's work on a caller-provided hipStream_t (NULL = its own stream), as at3hip_decoder_set_stream. */
int at3hip_resampler_set_stream(at3hip_resampler* r, void* hip_stream);

/* The shape of a pair's table, (L, M, K), on the host (no GPU needed); AT3HIP_EINVAL for an unsupported pair. */
int at3hip_resampler_shape(int32_t in_rate, int32_t out_rate, int32_t* phases, int32_t* step, int32_t* taps);
/* The table hp[L][K] float32 as at3hip_resampler_create builds it, on the host (no GPU needed); bytes = L * K * 4. */
int at3hip_resampler_host_tables(int32_t in_rate, int32_t out_rate, void* dst, size_t bytes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* AT3HIP_RESAMPLE_H */
