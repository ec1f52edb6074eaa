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
