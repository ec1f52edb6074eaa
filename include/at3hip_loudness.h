/* at3hip_loudness.h - C ABI of the batched loudness and true-peak meter: programme loudness after ITU-R BS.1770-4 / EBU R 128
 * and the peak of 44.1 kHz PCM, for a batch of independent streams, plus the one-constant gain that brings a stream to a target
 * loudness under a peak ceiling. Same library (libat3hip.so), prefix and error codes as at3hip.h. The reference has no level
 * control: TScaler::Scale clamps what exceeds full scale (at3hip_get_counters counts it afterwards). This meter is this project's
 * own definition, written out below, restated in C by the test suite (tests/host/loudness_cpu.c) and pinned to the GPU bit for
 * bit; its outside anchors are the ITU coefficient table and the EBU Tech 3341 test signals (tests/test_loudness_cpu.py).
 *
 * Definition. 44.1 kHz only, 1 or 2 channels. Every stream of a call takes the same n_in; state carries across calls and any
 * split of a stream into calls gives the same results as one call.
 *   K-weighting. Two biquads in double, coefficients as decimal literals (no libm in their bits):
 *     stage 1 (shelf)     b = {1.5308412300503478, -2.6509799951547297, 1.169079079921587},
 *                         a1 = -1.6636551132560204, a2 = 0.7125954280732254
 *     stage 2 (high-pass) b = {1.0, -2.0, 1.0}, a1 = -1.989169673629796, a2 = 0.9891990357870393
 *     They are the usual analogue prototype of the ITU filter evaluated at fs = 44100 (K = tan(pi f0 / fs)):
 *       stage 1: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G/20),
 *                Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2,
 *                b = {(Vh + Vb K/Q + K^2)/a0, 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0}, a1 = 2 (K^2 - 1)/a0, a2 = (1 - K/Q + K^2)/a0
 *       stage 2: f0 = 38.13547087602444, Q = 0.5003270373238773, d = 1 + K/Q + K^2,
 *                b = {1, -2, 1}, a1 = 2 (K^2 - 1)/d, a2 = (1 - K/Q + K^2)/d
 *     At fs = 48000 the same formulas give the table of BS.1770 to about 1e-15.
 *   One filter step, transposed direct form II, every multiply and add rounded on its own (no contraction into FMA):
 *       y = b0*x + s1;  s1 = (b1*x - a1*y) + s2;  s2 = b2*x - a2*y
 *     Stage 2 takes stage 1's y; stage 1's x is (double) of the float sample.
 *   Hop sums. Hop j of a channel is samples [4410 j, 4410 j + 4410). z_c[j] is computed from ZERO filter state at sample
 *     4410 max(0, j - 2): both stages run from there to the end of hop j, and over hop j's samples, ascending, acc = acc + y2*y2
 *     from +0.0 (y2 = stage 2's y). Only complete hops give a z. The restart makes every hop independent of every other, so the
 *     definition is parallel by construction; stage 2's pole radius is 0.99458, and after the 8820 warm-up samples z differs
 *     from that of a never-restarted filter by about 6e-15 relative (noise plus tone plus DC; a warm-up of one hop gives 1.1e-11).
 *   Peaks. sample_peak_c is the largest |x| of every sample received, the partial last hop included; true_peak_c (only with
 *     true_peak = 1 in the config) is the larger of sample_peak_c and the largest |u|, u being EVERY output of the
 *     44100 -> 176400 converter of at3hip_resample.h for that channel, bit for bit (the same table, the same ascending fmaf chain;
 *     all 4T outputs of a stream of T samples, those at3hip_resampler_flush emits with zeros past the end included). Magnitudes
 *     are compared as the float's bits with the sign cleared, which is the float order for everything but NaNs.
 *   Gating (host, double), with H complete hops and blocks b = 0 .. H - 4:
 *     t_c = ((z_c[b] + z_c[b+1]) + z_c[b+2]) + z_c[b+3];  P_b = (t_0 [+ t_1]) / 17640.0;  l_b = -0.691 + 10 log10(P_b).
 *     Absolute gate: keep l_b > -70.0. Relative gate: -0.691 + 10 log10(mean P of the kept) - 10.0; keep l_b above both.
 *     integrated = -0.691 + 10 log10(mean P of the twice-kept); means are sums in ascending b divided by the count.
 *     integrated = -HUGE_VAL if nothing is kept or H < 4. momentary_max = the largest l_b. short_term_max: the same over windows
 *     of 30 hops (summed ascending from the first), divided by 132300.0; -HUGE_VAL for H < 4 and H < 30 respectively. A mono stream is its
 *     one channel with weight 1. log10 is the host libm's.
 *   Gain. g = (float)min(10^((target - integrated) / 20), 10^(ceiling_db / 20) / peak) in double (the host libm's pow(10.0, .)),
 *     peak = the larger channel's true peak if it was measured, else the larger sample peak; g = 1.0f when integrated is
 *     -HUGE_VAL or peak is 0. Applying it is one float multiply per sample.
 *
 * The look-ahead limiter (at3hip_loudness_limit_*). A second definition of this project's own, restated by tests/host/limiter_cpu.c
 * and pinned to the GPU bit for bit. It stands between the gain and the encoder: the gain alone (at3hip_loudness_apply) leaves
 * peaks above the ceiling, one constant gain under the ceiling lets one click set the level of a whole file. 44.1 kHz, 1 or 2
 * channels, every stream of a call takes the same n_in. A stream has a gain g (finite, >= 0) and all streams one ceiling c
 * (finite, > 0), floats, fixed from at3hip_loudness_limit_start until at3hip_loudness_limit_flush. Every output sample depends on
 * a bounded window of the input and everything that depends on an order of evaluation is integer arithmetic, so the result does
 * not depend on how the work is cut into tiles or calls. x_c[n] is sample n of channel c of the T samples between start and
 * flush; x_c[n] = +0.0f for n < 0 and n >= T.
 *   1 Detector. m[n] = the largest magnitude over the channels' |x_c[n]| and, in true-peak mode (AT3HIP_LIMIT_TRUE_PEAK), also
 *     over the four converter outputs u_c[4n + p], p = 0 .. 3, of the 44100 -> 176400 converter of at3hip_resample.h:
 *     acc = +0.0f; for k = 0 .. 143 ascending: acc = fmaf(h[p][k], x_c[n + k - 71], acc) (the table and chain of the meter's true
 *     peak). Magnitudes are compared as the float's bits with the sign cleared, so a NaN is the largest.
 *   2 Required gain. e = (double)g * (double)m[n] (exact); r[n] = e > (double)c ? (double)c / e : 1.0 (an IEEE double division);
 *     q[n] = (uint32)(r[n] * 2^30) truncated, 0 <= q <= 2^30. q[n] = 2^30 for n < 0 and for n >= T (decided here: past the flush
 *     the detector is not evaluated, although the converter's ringing of the last samples reaches there).
 *   3 Look-ahead and hold. w[n] = min(q[n - H .. n + A]), A = AT3HIP_LIMIT_LOOKAHEAD = 220 samples (5 ms), H = AT3HIP_LIMIT_HOLD =
 *     2205 samples (50 ms); w is defined for every integer n through the extension of q.
 *   4 Smoothing. S[n] = w[n - A] + ... + w[n], an exact 64-bit integer sum of A + 1 = 221 terms. Each w[j] of it covers q[n], so
 *     S[n] / AT3HIP_LIMIT_FULL <= r[n], AT3HIP_LIMIT_FULL = 221 * 2^30.
 *   5 Output. s = (double)S[n] / (double)AT3HIP_LIMIT_FULL (an IEEE double division) converted to float rounding toward zero;
 *     t = (x_c[n] * g) * s, two float multiplies, the first one at3hip_loudness_apply's; y_c[n] = t > c ? c : (t < -c ? -c : t)
 *     (a NaN t passes). Where S[n] = AT3HIP_LIMIT_FULL, s is 1.0f and y is apply's output bit for bit unless that exceeds c.
 *   6 Streaming. Latency D = A samples, in true-peak mode A + 72 (at3hip_loudness_limit_delay): after T' samples were received a
 *     stream has emitted max(0, T' - D) outputs; at3hip_loudness_limit_flush emits the rest, to T in all, and ends the run. Any
 *     split of the input into calls, calls shorter than the filter and empty calls included, gives the same samples.
 *   7 Statistics per stream since the start: min S[n] over the outputs emitted (AT3HIP_LIMIT_FULL when there is none) and the
 *     number of outputs with S[n] < AT3HIP_LIMIT_FULL. 20 log10(min S / AT3HIP_LIMIT_FULL) is the largest reduction in dB.
 *   8 Outside the float domain. Any float sample is accepted. A NaN sample is m[n] for its n (in true-peak mode for the 144 n
 *     whose filter reads it), e is NaN, the comparison fails and r = 1: the NaN does not limit and passes through step 5 as
 *     NaN. An infinite sample (with g > 0) gives e = inf and q = 0 with the sample detector: S reaches 0 around it, t = inf * 0 =
 *     NaN at the sample itself and +-0 around it. In true-peak mode the filter turns an infinity into infinities or (inf - inf)
 *     NaNs at the 144 n around it: q = 0 where the largest magnitude is an infinity, r = 1 where it is a NaN. With g = 0,
 *     e = 0 * inf = NaN and r = 1. Finite samples whose product with g overflows give e's exact double, q = 0 or close to it,
 *     and t = +-inf * s, clamped to +-c unless s is 0 (then NaN). No stream affects another. Samples (floats as bit patterns; where
 *     they are NaN, a NaN of unspecified sign and payload) and statistics are the restatement's for each stream alone
 *     (tests/test_float_domain_gpu.py, tests/test_float_domain_cpu.py; no exception known).
 *
 * The meter is part of ABI 1.6 (see at3hip.h): a host that needs it looks for the symbol at3hip_loudness_create.
 */
#ifndef AT3HIP_LOUDNESS_H
#define AT3HIP_LOUDNESS_H

#include <stddef.h>
#include <stdint.h>

#include "at3hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define AT3HIP_LOUDNESS_HOP 4410   /* samples per hop (100 ms) */

/* The K-weighting coefficients of the definition: {b0, b1, b2, a1, a2} per stage. */
#define AT3HIP_KW_STAGE1 {1.5308412300503478, -2.6509799951547297, 1.169079079921587, -1.6636551132560204, 0.7125954280732254}
#define AT3HIP_KW_STAGE2 {1.0, -2.0, 1.0, -1.989169673629796, 0.9891990357870393}

typedef struct at3hip_loudness at3hip_loudness;

typedef struct at3hip_loudness_config {
    int32_t channels;    /* 1 or 2 */
    int32_t n_streams;   /* independent streams metered side by side */
    int32_t max_in;      /* most samples per stream (and channel) in one at3hip_loudness_process / _apply call */
    int32_t max_hops;    /* most complete hops per stream between two resets / finishes */
    int32_t true_peak;   /* 1: also measure the 4x oversampled peak */
    int32_t device_id;
} at3hip_loudness_config;

typedef struct at3hip_loudness_result {
    double integrated;       /* LUFS; -HUGE_VAL when nothing passes the gates */
    double momentary_max;    /* LUFS, largest 400 ms block */
    double short_term_max;   /* LUFS, largest 3 s window */
    float sample_peak[2];    /* per channel, linear (the second is 0 for a mono stream) */
    float true_peak[2];      /* per channel, linear; 0 when it was not measured */
    int64_t n_samples;       /* samples received per channel */
    int32_t n_hops;          /* complete hops */
    int32_t n_blocks_kept;   /* 400 ms blocks that passed both gates */
} at3hip_loudness_result;

/* The context's stream is non-blocking; see DEVICE BUFFERS AND STREAMS (at3hip.h) and at3hip_loudness_set_stream. */
int at3hip_loudness_create(const at3hip_loudness_config* cfg, at3hip_loudness** out);
void at3hip_loudness_destroy(at3hip_loudness* l);
const char* at3hip_loudness_last_error(const at3hip_loudness* l);
/* Back to start-of-stream state for every stream (what at3hip_loudness_finish leaves). */
int at3hip_loudness_reset(at3hip_loudness* l);
/* Waits for everything queued on the meter. */
int at3hip_loudness_sync(at3hip_loudness* l);
/* Queue this meter's work on a caller-provided hipStream_t (NULL = its own stream), as at3hip_decoder_set_stream. */
int at3hip_loudness_set_stream(at3hip_loudness* l, void* hip_stream);

/* SAMPLES OUTSIDE THE FLOAT DOMAIN. Any float is accepted, and every field of the result is the definition's (doubles and floats as
 * bit patterns; a NaN where the definition gives a NaN, sign and payload unspecified): tests/test_float_domain_gpu.py, no exception
 * known. A NaN or an infinity makes NaN the hop sums of the hop that holds it and of the two hops that warm up on it; blocks with a
 * NaN sum fail the gates and are left out, later hops are exact. sample_peak and true_peak compare magnitudes as bit patterns, so
 * a NaN in a channel IS that channel's peak (at3hip_loudness_gain then returns what the definition computes from it: check the
 * peaks with isfinite before trusting a gain). Finite samples whose squares pass DBL_MAX cannot occur; those that are merely huge
 * give a huge, finite loudness. at3hip_loudness_apply is one float multiply per sample. No stream affects another. */
/*   in [n_streams][n_in][channels] float32, 0 <= n_in <= max_in
 * flags: AT3HIP_PCM_ON_DEVICE (in is device memory), AT3HIP_ASYNC (only queue the call: in stays valid until
 * at3hip_loudness_sync or at3hip_loudness_finish). A call that would complete more than max_hops hops is AT3HIP_EINVAL. */
int at3hip_loudness_process(at3hip_loudness* l, const float* in, int32_t n_in, uint32_t flags);
/* Waits for the queued calls, gates every stream, fills results[n_streams], then returns every stream to its start state. */
int at3hip_loudness_finish(at3hip_loudness* l, at3hip_loudness_result* results);
/* The hop sums of one stream so far, z as double [n_hops][channels] (bytes = n_hops * channels * 8, n_hops = samples received
 * / 4410); waits for queued work. The tap the parity tests compare. */
int at3hip_loudness_read_hops(at3hip_loudness* l, int32_t stream, void* dst, size_t bytes);
/* out = in * gains[stream], one float multiply per sample; in and out [n_streams][n_in][channels], gains host memory (read before
 * the call returns). flags: AT3HIP_PCM_ON_DEVICE, AT3HIP_OUT_ON_DEVICE, AT3HIP_ASYNC; queued behind earlier calls like
 * at3hip_loudness_process. out may be in. Touches no meter state. */
int at3hip_loudness_apply(at3hip_loudness* l, const float* in, int32_t n_in, const float* gains, float* out, uint32_t flags);

/* at3hip_loudness_process and at3hip_loudness_apply for 16-bit PCM: in [n_streams][n_in][channels] int16; layout, flags, limits
 * and error codes as for the float calls. A sample s is taken as the float (float)s * 0x1p-15f (exact, = s / 32768.0f: the rule
 * of at3hip_encode_s16), so hop sums, peaks and results are, bit for bit, those of the float call on these floats, and
 * at3hip_loudness_apply_s16 gives out = ((float)s * 0x1p-15f) * gains[stream] as float32 (out cannot be in). The samples are
 * widened by the kernels' loads: host memory crosses the bus as 16-bit (half the bytes; its staging buffer is allocated by the
 * first such call) and no float copy is written on the device. Calls of both kinds may alternate on one meter: the carried
 * samples are float. A device pointer needs only int16_t alignment (a mono stream's row starts at s * n_in * 2 bytes). Added
 * under ABI 1.6: a host looks for these symbols.
 * What it gains (measured): at3hip_loudness_process is compute-bound, and its hop kernel takes 1.5 times as
 * long on 16-bit samples as on floats; from host memory the 16-bit call is 1.1 times as fast as the float call, on samples that
 * are in device memory as floats already the float call is the faster one. at3hip_loudness_apply_s16 is twice as fast as
 * at3hip_loudness_apply from host memory. */
int at3hip_loudness_process_s16(at3hip_loudness* l, const int16_t* in, int32_t n_in, uint32_t flags);
int at3hip_loudness_apply_s16(at3hip_loudness* l, const int16_t* in, int32_t n_in, const float* gains, float* out, uint32_t flags);

/* THE LIMITER (the definition above, "The look-ahead limiter"). New calls on the meter's context; they touch no meter state and
 * the meter's calls touch no limiter state, except that at3hip_loudness_reset also ends a limiter run. Their tables and buffers
 * are allocated by the first at3hip_loudness_limit_start. Added under ABI 1.6: a host looks for the symbol
 * at3hip_loudness_limit_start. Calls are queued behind earlier calls on the meter's stream and honour at3hip_loudness_set_stream. */
#define AT3HIP_LIMIT_LOOKAHEAD 220              /* A */
#define AT3HIP_LIMIT_HOLD 2205                  /* H */
#define AT3HIP_LIMIT_FULL 237296943104LL        /* (A + 1) * 2^30: S of an unlimited sample */
#define AT3HIP_LIMIT_TRUE_PEAK 1u               /* flag of at3hip_loudness_limit_start / _limit_delay: the 4x oversampled detector */

typedef struct at3hip_limit_stats {
    int64_t min_sum;     /* min S[n] over the outputs emitted; AT3HIP_LIMIT_FULL when nothing was limited */
    int64_t n_limited;   /* outputs with S[n] < AT3HIP_LIMIT_FULL */
    int64_t n_out;       /* outputs emitted */
} at3hip_limit_stats;

/* The latency D in samples for these start flags (host only, no context). */
int32_t at3hip_loudness_limit_delay(uint32_t flags);
/* Begins a run for every stream: gains[n_streams] (host memory, read before the call returns; each finite and >= 0), ceiling
 * finite and > 0, flags 0 or AT3HIP_LIMIT_TRUE_PEAK. AT3HIP_EINVAL for anything else and while a run is open (between a start
 * and its flush or at3hip_loudness_reset). Clears the statistics. */
int at3hip_loudness_limit_start(at3hip_loudness* l, const float* gains, float ceiling, uint32_t flags);
/* in [n_streams][n_in][channels] float32, 0 <= n_in <= max_in; out [n_streams][*n_out][channels] float32, where *n_out =
 * max(0, T' - D) - max(0, T' - n_in - D) <= n_in is set before the call returns (T' = samples received with this call): an out of
 * n_in samples per stream always suffices. flags: AT3HIP_PCM_ON_DEVICE, AT3HIP_OUT_ON_DEVICE, AT3HIP_ASYNC as for
 * at3hip_loudness_apply. out cannot be in: an output sample lies D samples behind its input sample, so the kernels would
 * overwrite input other workgroups still read; device buffers of one call that overlap are AT3HIP_EINVAL. */
int at3hip_loudness_limit(at3hip_loudness* l, const float* in, int32_t n_in, float* out, int32_t* n_out, uint32_t flags);
/* The same for 16-bit PCM, a sample s taken as (float)s * 0x1p-15f in the kernels' loads (the rule of at3hip_encode_s16); the
 * output is float32. Calls of both kinds may alternate in one run. */
int at3hip_loudness_limit_s16(at3hip_loudness* l, const int16_t* in, int32_t n_in, float* out, int32_t* n_out, uint32_t flags);
/* Emits the last *n_out = min(T, D) outputs of every stream, out [n_streams][*n_out][channels] (room for D samples per stream
 * suffices), and ends the run; the statistics stay readable until the next start. flags: AT3HIP_OUT_ON_DEVICE, AT3HIP_ASYNC. */
int at3hip_loudness_limit_flush(at3hip_loudness* l, float* out, int32_t* n_out, uint32_t flags);
/* Waits for the queued calls and fills stats[n_streams] for the run begun by the last start. */
int at3hip_loudness_limit_stats(at3hip_loudness* l, at3hip_limit_stats* stats);

/* The gating of the definition on the host (no GPU needed): z [n_hops][channels] double -> integrated, momentary_max,
 * short_term_max, n_hops and n_blocks_kept of *result; its other fields are left as they are. */
int at3hip_loudness_gate(const double* z, int32_t n_hops, int32_t channels, at3hip_loudness_result* result);
/* The gain of the definition on the host (no GPU needed) from result's integrated loudness and peaks. */
int at3hip_loudness_gain(const at3hip_loudness_result* result, double target_lufs, double ceiling_db, float* g);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* AT3HIP_LOUDNESS_H */
