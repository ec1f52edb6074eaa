/* at1hip.h - C ABI of the MI355X-native ATRAC1 encode path and of its decoder (below).
 *
 * Drop-in boundary: what a host shim inside the reference binds in place of the body of the lambda returned by
 * TAtrac1Encoder::GetLambda (atrac1denc.cpp:180-255) - per 512-sample block and channel: analysis filter bank,
 * transient detection, block-switched MDCT, loudness tracking, scale factors, bit allocation and the 212-byte sound
 * unit - for a batch of independent streams. The container (AEA header, frame writing: aea.cpp) stays on the host.
 * Plain pointers and sizes only; same library (libat3hip.so) and error codes as at3hip.h.
 */
#ifndef AT1HIP_H
#define AT1HIP_H

#include <stddef.h>
#include <stdint.h>

#include "at3hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: these declarations are its whole exported surface */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define AT1HIP_FRAME_SIZE 212   /* TAtrac1Data::SoundUnitSize, atrac/at1/atrac1.h:110 */
#define AT1HIP_BLOCK 512        /* TAtrac1Data::NumSamples, atrac/at1/atrac1.h:121 */

typedef struct at1hip_ctx at1hip_ctx;

/* Mirrors NAtrac1::TAtrac1EncodeSettings (atrac/at1/atrac1.h:33-54) plus batch geometry. */
typedef struct at1hip_config {
    int32_t channels;       /* 1 or 2 (Aea->GetChannelNum()) */
    int32_t window_auto;    /* 1 = EWM_AUTO (transient detection), 0 = EWM_NOTRANSIENT with window_mask */
    int32_t window_mask;    /* bit 0 low, bit 1 mid, bit 2 high band use short windows (atrac1denc.cpp:227) */
    int32_t bfu_idx_const;  /* BfuIdxConst: 0 = automatic, else 1..8 */
    int32_t n_streams;      /* independent audio streams encoded side by side */
    int32_t max_blocks;     /* upper bound of 512-sample blocks per stream per at1hip_encode call */
    int32_t device_id;
} at1hip_config;

typedef struct at1hip_timings {
    float total_ms;
    float front_ms;   /* QMF tree + transient detection + MDCT + scale factors */
    float scan_ms;    /* loudness tracking */
    float pack_ms;    /* bit allocation + sound-unit packing */
} at1hip_timings;

/* Replaces: TAtrac1Encoder::TAtrac1Encoder(TCompressedOutputPtr&&, TAtrac1EncodeSettings&&) (atrac1denc.cpp:36-44)
 * for n_streams encoders at once. */
int at1hip_create(const at1hip_config* cfg, at1hip_ctx** out);
void at1hip_destroy(at1hip_ctx* ctx);
const char* at1hip_last_error(const at1hip_ctx* ctx);

/* Replaces: n_blocks invocations of the lambda of TAtrac1Encoder::GetLambda per stream.
 *   pcm        [n_streams][n_blocks][512][channels] float32, interleaved, +-1.0 (pcmengin.h:173-184)
 *              Any float is accepted (NaN, +-infinity, +-FLT_MAX, overflowing or subnormal samples): the call succeeds, the sound
 *              units and the loudness tap of every stream are bit for bit the reference's for that stream alone (no exception
 *              known: tests/test_float_domain_gpu.py), and no other stream of the call is touched. A NaN or an infinity changes
 *              the 2 or 3 sound units whose QMF history and MDCT overlap hold it; a block of finite samples of 1e15 and more also
 *              raises the carried loudness, and with window_auto every later sound unit of that stream differs from the clean
 *              encode until at1hip_reset.
 *   out_frames [n_streams][n_blocks][channels][212] bytes: the buffers handed to ICompressedOutput::WriteFrame, in the
 *              reference's order (channel 0 then channel 1 of each block, atrac1denc.cpp:249-251)
 * flags: AT3HIP_PCM_ON_DEVICE / AT3HIP_OUT_ON_DEVICE as for at3hip_encode; AT3HIP_ASYNC only queues the call (buffers must stay
 * valid until at1hip_sync; host buffers then have to be page-locked for the copies to be asynchronous): consecutive calls follow
 * each other on the device without the host in between. Stream state (filter histories, the high band's delay line, MDCT
 * overlap, detector energies, loudness) is carried between calls. */
int at1hip_encode(at1hip_ctx* ctx, const float* pcm, int32_t n_blocks, uint8_t* out_frames, uint32_t flags);

/* at1hip_encode for 16-bit PCM: pcm [n_streams][n_blocks][512][channels] int16, layout, flags, limits and error codes as
 * above. A sample s is taken as the float (float)s * 0x1p-15f (exact, = s / 32768.0f: the rule of at3hip_encode_s16 and of the
 * reference's WAV reader), so the frames are, bit for bit, those of at1hip_encode on these floats. The samples are widened by
 * the first kernel's loads: host memory crosses the bus as 16-bit (half the bytes; its staging buffer is allocated by the
 * first such call) and no float copy is written on the device. Calls of both kinds may alternate on one context: the carried
 * state is float. A device pointer needs only int16_t alignment. Added under ABI 1.6: a host looks for this symbol. */
int at1hip_encode_short(at1hip_ctx* ctx, const int16_t* pcm, int32_t n_blocks, uint8_t* out_frames, uint32_t flags);

/* Waits for everything queued on the ctx. (A queued call records no stage-timing events - they are not free between the kernels -: the
 * timings then read zero; a synchronous call is timed.) */
int at1hip_sync(at1hip_ctx* ctx);

/* Back to start-of-stream state for every stream (a fresh TAtrac1Encoder). */
int at1hip_reset(at1hip_ctx* ctx);

int at1hip_get_timings(const at1hip_ctx* ctx, at1hip_timings* out);

/* Intermediate results of the last at1hip_encode call, copied to host memory `dst` (test / debugging interface):
 *   AT1HIP_TAP_SPECTRA  float32 [n_streams][n_blocks][channels][512]  TAtrac1MDCT::Mdct output
 *   AT1HIP_TAP_MASKS    int32   [n_streams][n_blocks][channels]       window masks
 *   AT1HIP_TAP_LOUDNESS float32 [n_streams][n_blocks]                 Loudness after each block's TrackLoudness
 *   AT1HIP_TAP_TABLES   the constant tables as uploaded (at1_tables.hpp layout) */
#define AT1HIP_TAP_SPECTRA 1
#define AT1HIP_TAP_MASKS 2
#define AT1HIP_TAP_LOUDNESS 3
#define AT1HIP_TAP_TABLES 4
int at1hip_read_tap(at1hip_ctx* ctx, int32_t kind, void* dst, size_t bytes);

/* The constant tables as at1hip_create builds them, on the host (no GPU needed): `bytes` must be the size of the
 * at1_tables.hpp layout (AT1HIP_TABLES_BYTES). */
#define AT1HIP_TABLES_BYTES 6904
int at1hip_host_tables(void* dst, size_t bytes);

/* ---- decoder ---------------------------------------------------------------------------------------------------------------
 * Drop-in boundary of the reference's `-d` path (main.cpp:343-365): TAtrac1Decoder (atrac1denc.cpp:46-49, 139-177) - per 512-sample
 * block and channel: bit unpack and dequantisation (TBlockSizeMod::Parse, atrac1.cpp:37-53; TAtrac1Dequantiser::Dequant,
 * atrac1_dequantiser.cpp:31-72), block-switched IMDCT (TAtrac1MDCT::IMdct, atrac1denc.cpp:103-137), the synthesis filter bank
 * (Atrac1SynthesisFilterBank::Synthesis, atrac1_qmf.h:46-64) and the clamp to [-1, 1] - for a batch of independent streams, every
 * frame of a call in parallel. Reading the AEA container (aea.cpp) stays on the host. Bit-identical to the reference. */
typedef struct at1hip_decoder at1hip_decoder;

typedef struct at1hip_decoder_config {
    int32_t channels;    /* 1 or 2 (Aea->GetChannelNum()) */
    int32_t n_streams;   /* independent audio streams decoded side by side */
    int32_t max_frames;  /* upper bound of frames (one sound unit per channel each) per stream per at1hip_decode call */
    int32_t device_id;
} at1hip_decoder_config;

/* Replaces: TAtrac1Decoder::TAtrac1Decoder(TCompressedInputPtr&&) (atrac1denc.cpp:46-49) for n_streams decoders at once.
 * The context's stream is non-blocking; see DEVICE BUFFERS AND STREAMS in at3hip.h and at1hip_decoder_set_stream. */
int at1hip_decoder_create(const at1hip_decoder_config* cfg, at1hip_decoder** out);
void at1hip_decoder_destroy(at1hip_decoder* dec);
const char* at1hip_decoder_last_error(const at1hip_decoder* dec);

/* 16-bit output: lrintf(x * 32767.0f) of each clamped sample, the float -> PCM_16 conversion with normalisation the reference's
 * writer leaves to libsndfile (pcm_io_sndfile.cpp:56,114) - a restatement that is not pinned against libsndfile here. */
#define AT1HIP_DECODE_S16 8u

/* Replaces: n_frames invocations of the lambda of TAtrac1Decoder::GetLambda per stream.
 *   units [n_streams][n_frames][channels][212] bytes: the frames TAeaInput::ReadFrame delivers, in its order (channel 0 then
 *         channel 1 of each frame, atrac1denc.cpp:143-145)
 *   pcm   [n_streams][n_frames][512][channels]: float32 (the lambda's `data`, atrac1denc.cpp:166-173), or int16 with
 *         AT1HIP_DECODE_S16
 * flags: AT3HIP_PCM_ON_DEVICE (units are device memory), AT3HIP_OUT_ON_DEVICE (pcm is device memory), AT3HIP_ASYNC (only queue
 * the call: buffers stay valid until at1hip_decoder_sync), AT1HIP_DECODE_S16. Stream state (the IMDCT overlap, the band buffers,
 * the filter bank's histories and delay line) carries across calls. A malformed unit - a block-size field that makes a LogCount
 * negative, or an allocation that reads past the unit's 1696 bits - decodes as a zero spectrum with all bands long, as the
 * reference's catch does; it is counted (at1hip_decoder_get_counters). */
int at1hip_decode(at1hip_decoder* dec, const uint8_t* units, int32_t n_frames, void* pcm, uint32_t flags);

/* Waits for everything queued on the decoder. */
int at1hip_decoder_sync(at1hip_decoder* dec);

/* Back to start-of-stream state for every stream (a fresh TAtrac1Decoder); zeroes the counters. */
int at1hip_decoder_reset(at1hip_decoder* dec);

/* Units the reference would have rejected with one "Skipping invalid ATRAC1 frame: <what>" line on stderr
 * (atrac1denc.cpp:154-162), summed over streams and channels since create / reset / the last call with reset = 1. Waits for
 * queued work. */
typedef struct at1hip_decoder_counters {
    uint64_t bad_block_size;   /* "invalid ATRAC1 block size mode" */
    uint64_t read_past_end;    /* "read past the end of the bitstream" */
} at1hip_decoder_counters;
int at1hip_decoder_get_counters(at1hip_decoder* dec, at1hip_decoder_counters* out, int32_t reset);

/* Queue this decoder's work on a caller-provided hipStream_t (NULL = the decoder's own stream): every call is then ordered
 * behind whatever the caller queued there before it (e.g. the kernel that fills `units`), and work the caller queues there
 * afterwards follows it. Waits for the decoder's queued work first. The stream must outlive its last call's completion. */
int at1hip_decoder_set_stream(at1hip_decoder* dec, void* hip_stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
