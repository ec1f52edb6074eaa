/* at3phip.h - C ABI of the MI355X-native ATRAC3plus path: the 16-band polyphase analysis
 * filter and the windowed MDCT-256 x 16 that turn PCM into the 2048-line spectrum (at3p.cpp:93-99, 139-159), and the
 * frame writer that scales and packs it, with or without a tonal block (at3p.cpp:159-163: ScaleFrame, then
 * TAt3PBitStream::WriteFrame(channels, p, sces)). The tonal (GHA) analysis between them needs libgha, an
 * un-vendored submodule of the reference: its result comes from the caller (at3phip_write_frames_tonal) or from this project's
 * own analysis (FINDING TONES below: at3phip_encode_frames_tonal), and at3phip_encode_frames is the encoder with that analysis
 * finding nothing. Same library (libat3hip.so) and error codes as at3hip.h.
 */
#ifndef AT3PHIP_H
#define AT3PHIP_H

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

#define AT3PHIP_FRAME 2048            /* TAt3PEnc::NumSamples, samples per channel and frame */
#define AT3PHIP_RESIDUAL_SCALE 16u    /* at3phip_mdct / at3phip_pqf_mdct: divide the subband samples by 32768 / 1.122018 first,
                                       * as EncodeFrame does for the residual spectrum (at3p.cpp:143-147) */

typedef struct at3phip_ctx at3phip_ctx;

typedef struct at3phip_config {
    int32_t channels;    /* 1 or 2 */
    int32_t n_streams;   /* independent streams side by side */
    int32_t max_frames;  /* upper bound of 2048-sample frames per stream per call */
    int32_t device_id;
} at3phip_config;

int at3phip_create(const at3phip_config* cfg, at3phip_ctx** out);
void at3phip_destroy(at3phip_ctx* ctx);
const char* at3phip_last_error(const at3phip_ctx* ctx);
/* Start-of-stream state: zeroed filter history (at3plus_pqf_create_a_ctx) and MDCT work buffers (TChannelCtx::MdctBuf). */
int at3phip_reset(at3phip_ctx* ctx);

/* Replaces: at3plus_pqf_do_analyse(ctx, in, out) (atrac/atrac3plus_pqf/atrac3plus_pqf.c:130-147) per channel and frame.
 *   pcm   [n_streams][n_frames][2048][channels] float32 interleaved (the `data` of EncodeFrame, at3p.cpp:93-97)
 *         Any float is accepted (NaN, +-infinity, +-FLT_MAX, overflowing or subnormal samples): subbands, spectra and the frames
 *         of at3phip_encode_frames are those of the reference's PQF, MDCT and writer for that stream alone (floats as bit patterns;
 *         where they are NaN, a NaN of unspecified sign and payload), no other stream of the call is touched, and the stream is
 *         itself again with the first frame whose PQF history (one frame) and MDCT overlap no longer hold the sample: 2 or 3
 *         frames in all. No exception is known (tests/test_float_domain_gpu.py).
 *   bands [n_streams][n_frames][channels][16][128] float32: 16 subbands x 128 samples
 * flags: AT3HIP_PCM_ON_DEVICE / AT3HIP_OUT_ON_DEVICE. The 368-sample filter history is carried between calls. */
int at3phip_pqf_analyse(at3phip_ctx* ctx, const float* pcm, int32_t n_frames, float* bands, uint32_t flags);

/* Replaces: TAt3pMDCT::Do(specs, bands, work, winType) (atrac/at3p/at3p_mdct.cpp:52-96) per channel and frame.
 *   bands     as above
 *   win_flags [n_streams][n_frames][channels] uint16, bit b = TAt3pMDCTWin::STEEP for subband b; NULL = all sine
 *   specs     [n_streams][n_frames][channels][2048] float32
 * The work buffer's first halves (THistBuf) are carried between calls. win_flags is always host memory. */
int at3phip_mdct(at3phip_ctx* ctx, const float* bands, int32_t n_frames, const uint16_t* win_flags, float* specs, uint32_t flags);

/* Both steps back to back, the subband samples staying in HBM (optionally returned through `bands`, may be NULL). */
int at3phip_pqf_mdct(at3phip_ctx* ctx, const float* pcm, int32_t n_frames, const uint16_t* win_flags, float* bands, float* specs,
                     uint32_t flags);

/* Replaces: per frame, sces[ch].ScaledBlocks = TScaler<NAt3p::TScaleTable>::ScaleFrame(specs) for each channel
 * (at3p.cpp:159, atrac/atrac_scale.cpp:141-191) and TAt3PBitStream::WriteFrame(channels, nullptr, sces)
 * (atrac/at3p/at3p_bitstream.cpp:694-726): fixed word lengths per quant unit, the cheapest of eight code tables per unit,
 * the number of quant units lowered from 32 to 28, 27, ... until the frame fits.
 *   specs     [n_streams][n_frames][channels][2048] float32 (flags & AT3HIP_PCM_ON_DEVICE: device memory)
 *   win_flags [n_streams][n_frames][channels] uint16 as in at3phip_mdct (TSubbandInfos::Win); NULL = all sine. Host memory.
 *   frames    [n_streams][n_frames][2048] bytes, each what ICompressedOutput::WriteFrame receives
 *             (flags & AT3HIP_OUT_ON_DEVICE: device memory); [n_streams][n_frames][frame_bytes] after at3phip_set_frame_bytes
 * Frames do not depend on one another. */
#define AT3PHIP_FRAME_BYTES 2048
int at3phip_write_frames(at3phip_ctx* ctx, const float* specs, int32_t n_frames, const uint16_t* win_flags, uint8_t* frames,
                         uint32_t flags);

/* TONAL BLOCKS IN THE WRITER. One frame's tonal block: the fields of TAt3PGhaData (atrac/at3p/at3p_gha.h:30-67) that
 * TTonalComponentEncoder::WriteTonalBlock reads, as a fixed-size record of 324 bytes. An all-zero record means "no tonal block";
 * so does any record with num_tone_bands = 0, whose other fields are not read. Layout:
 *   num_tone_bands    NumToneBands, 0..16
 *   second_is_leader  SecondIsLeader, 0 or 1
 *   tone_sharing      bit b = ToneSharing[b]; bits at or above num_tone_bands are not read
 *   band[ch][b]       band b < num_tone_bands of channel ch (WaveSbInfos[b]): n_waves = WaveNums, 0..15; start / stop = the
 *                     envelope's point + 1, so 1..32 for the points 0..31 and 0 for EMPTY_POINT; reserved is not read. Bands at
 *                     or above num_tone_bands, channel 1 of a mono context and the envelope of a shared band are not read.
 *   wave[i]           WaveParams as AT3PHIP_TONAL_WAVE packs them (FreqIndex 0..1023 | AmpSf 0..63 << 10 | PhaseIndex 0..31 << 16;
 *                     AmpIndex is not written by the reference): channel 0's bands in order, then channel 1's, each band's
 *                     n_waves entries side by side (WaveIndex is the running sum); at most 48 in all.
 * The contract, checked on the host before anything is queued (AT3HIP_EINVAL, the last error naming stream, frame and field):
 * the ranges above; FreqIndex non-decreasing within a band, which CreateFreqBitPack assumes (its codes are differences to
 * 1024 - 2^b); a shared band of channel 1 has no waves of its own; tone_sharing and second_is_leader are 0 in a mono context. */
#define AT3PHIP_TONAL_MAX_WAVES 48
#define AT3PHIP_TONAL_MAX_BAND_WAVES 15
#define AT3PHIP_TONAL_WAVE(freq, amp_sf, phase) ((uint32_t)(freq) | (uint32_t)(amp_sf) << 10 | (uint32_t)(phase) << 16)
typedef struct at3phip_tonal_band {
    uint8_t n_waves, start, stop, reserved;
} at3phip_tonal_band;
typedef struct at3phip_tonal_block {
    uint8_t num_tone_bands, second_is_leader;
    uint16_t tone_sharing;
    at3phip_tonal_band band[2][16];
    uint32_t wave[AT3PHIP_TONAL_MAX_WAVES];
} at3phip_tonal_block;

/* Replaces: ScaleFrame as above and TAt3PBitStream::WriteFrame(channels, &block, sces) per frame, or WriteFrame(channels,
 * nullptr, sces) for a record without a block: byte for byte the reference's frame, with the block written by
 * WriteTonalBlock and CreateFreqBitPack (at3p_bitstream.cpp:41-93, 487-629).
 *   specs, win_flags, frames, flags  exactly as in at3phip_write_frames
 *   tonal  [n_streams][n_frames] records in host memory, like win_flags; NULL = no frame has a block (at3phip_write_frames)
 * What the reference does and this call keeps: the frame's tail (window shapes, gain-compensation bits, tonal flag and block,
 * noise flag, terminator) is formed once, in the pass with 32 quant units, and its bits count in CheckFrameDone, so a block
 * lowers the number of quant units a loud frame keeps; ascending frequency order is chosen only when strictly cheaper; the
 * num-waves and amplitude mode fields are 0 in ch + 1 bits. The block is the analysis of the frame BEFORE the spectrum's
 * (TAt3PEnc::EncodeFrame writes the previous call's block, at3p.cpp:128-176): pairing records with spectra is the host's.
 * The reference aborts when, on a repeated pass, NumToneBands exceeds the quant unit count (at3p_bitstream.cpp:652-656), that is
 * when 16 units and the tail do not fit the frame. That branch cannot be reached: in stereo the first 16 units cost at most
 * 6639 bits with everything in front of the tail (a unit's cheapest table is never dearer than any one of its eight), the
 * largest tail at most 1624 bits, and a frame holds 16381; mono needs less (tests/test_at3p_tonal_write_cpu.py works the
 * figures out from at3p_vlc.inc and the word-length table).
 * Added under ABI 1.6: a host looks for this symbol. */
int at3phip_write_frames_tonal(at3phip_ctx* ctx, const float* specs, int32_t n_frames, const uint16_t* win_flags,
                               const at3phip_tonal_block* tonal, uint8_t* frames, uint32_t flags);

/* PCM to frames: at3phip_pqf_mdct with AT3PHIP_RESIDUAL_SCALE and sine windows, then at3phip_write_frames, everything in
 * between staying in HBM. This is TAt3PEnc::EncodeFrame (at3p.cpp:89-170) with GHA_PASS_INPUT | GHA_WRITE_RESIUDAL and a
 * tonal analysis that finds nothing; frame f holds input frame f (the reference's two-frame look-ahead delay is the
 * host's to add, see atracdenc_amd/host/at3hip_host.hpp). pcm as in at3phip_pqf_analyse, frames as above. */
int at3phip_encode_frames(at3phip_ctx* ctx, const float* pcm, int32_t n_frames, uint8_t* frames, uint32_t flags);
/* The same for 16-bit PCM: pcm [n_streams][n_frames][2048][channels] int16, layout, flags, limits and error codes as above. A
 * sample s is taken as the float (float)s * 0x1p-15f (exact, = s / 32768.0f: the rule of at3hip_encode_s16), so the frames are,
 * bit for bit, those of the float call on these floats. The samples are widened by the filter bank's loads: host memory crosses
 * the bus as 16-bit (half the bytes; its staging buffer is allocated by the first such call) and no float copy is written on
 * the device. Calls of both kinds may alternate on one context: the carried state is float. A device pointer needs only int16_t
 * alignment. Added under ABI 1.6: a host looks for this symbol. */
int at3phip_encode_frames_short(at3phip_ctx* ctx, const int16_t* pcm, int32_t n_frames, uint8_t* frames, uint32_t flags);
/* FINDING TONES. The analysis between the filter bank and the transform that TAt3PEnc::EncodeFrame leaves to libgha (at3p.cpp:
 * 118-170), an un-vendored submodule of the reference: there is nothing to restate, so steps 1-8 are this project's definition,
 * pinned bit for bit to tests/host/at3p_gha_cpu.c and anchored to the round trip of tests/test_at3p_gha_cpu.py.
 *
 * Definition. Input: the subband samples at3phip_pqf_analyse writes, [16][128] per channel and frame, in the scale they have
 * there. Tables: sine_table[2048], hann_window[256], amp_sf_tab[64] of the decoder (at3phip_decoder_host_tone_tables), the
 * forward twiddles tw[i] = ((float)cos(ph), (float)sin(ph)), ph = -2 pi i / 256 in double (kiss_fft.c:357-363), and
 * thr[i] = a * a, a = (double)amp_sf_tab[i] * exp2(-0.125), in double, and the projections' normalisers of steps 4 and 5,
 * rs[f] = 1.0 / sum over t of (double)hann_window[t] * (s * s), s = (double)sine_table[((t - 128) f) & 2047], and rc[f] the same with
 * sine_table[((t - 128) f + 512) & 2047], summed from 0.0 for t = 0..255 in order; all built on the host
 * (at3phip_host_tone_find_tables). Away from the ends rs and rc are 1 / 64 to a few parts in a thousand; within a bin or two of
 * frequency index 0 or 1024 the sine's mirror image falls into the window's main lobe and they are what keeps the amplitude right.
 * Block T_m of frame m describes Hann-windowed sines over the 256 samples x[0..255] = subband b of frame m, then subband b of
 * frame m+1: what the decoder synthesises for it (block m fades in over frame m, out over frame m+1, phases refer to sample 128).
 * Per channel and subband, all 16; float and double operations as written, each rounded, no FMA:
 *   1. y[t] = x[t] * hann_window[t] (float).
 *   2. Coarse spectrum: the 256-point forward FFT of (y[t], 0.0f) in float, in kissfft's order for 256 = 4 x 4 x 4 x 4
 *      (kf_work and kf_bfly4, kiss_fft.c:42-90, 238-302, with the twiddles above); P[k] = re * re + im * im (float), k = 0..128.
 *      Bin k is frequency index 8 k.
 *   3. Candidates: sum = P[1] + P[2] + ... + P[127] in float, in this order; floor = 16.0 * ((double)sum / 127.0) in double. A bin
 *      k in 0..128 is a candidate when P[k] > P[k-1], P[k] >= P[k+1] and (double)P[k] >= floor, with P[-1] = P[1] and
 *      P[129] = P[127] (the spectrum of a real signal is even about bins 0 and 128; without the two end bins no sine within half
 *      a bin of either end, and no frequency index above 1015, could be found). The AT3PHIP_TONE_MAX_BAND_WAVES (3) candidates
 *      of largest P are kept, the lower k on equal P; they go on in descending order of P.
 *   4. Fine search per candidate, for every frequency index f in max(1, 8 k - 7) .. min(1023, 8 k + 7):
 *      S(f) = sum over t of (double)y[t] * (double)sine_table[((t - 128) f) & 2047],
 *      C(f) = the same with sine_table[((t - 128) f + 512) & 2047], both from 0.0 for t = 0..255 in order. The f of largest
 *      (S * S) * rs[f] + (C * C) * rc[f] (double: the energy the fit of step 5 explains) is taken, the lowest on a tie.
 *   5. a = S * rs[f], b = C * rc[f]: the least-squares fit x[t] = a sin + b cos under the window (the window and the phases are
 *      symmetric about sample 128, so sine and cosine are orthogonal under it). A2 = a * a + b * b. The wave is kept when
 *      A2 >= 8.0 * 8.0. AmpSf = the largest i with A2 >= thr[i] (0 when there is none). PhaseIndex = the p in 0..31 of largest
 *      a * (double)sine_table[(64 p + 512) & 2047] + b * (double)sine_table[64 p], the lowest on a tie.
 *   6. Frame budget: the kept waves of the frame, both channels together, ranked by A2 descending, equal A2 by channel, then
 *      band, then frequency index; the first AT3PHIP_TONAL_MAX_WAVES (48) stay.
 *   7. The at3phip_tonal_block: a band's waves by ascending FreqIndex (two candidates are at least 2 bins apart, so their
 *      refined indices differ); num_tone_bands = the highest band holding a wave in either channel, plus 1; no envelope point
 *      (start = stop = 0), no sharing, no leader. A frame without waves gives the all-zero record.
 *   8. Residual: r_m = x_m - (T_m fading in + T_{m-1} fading out): ff_atrac3p_generate_tones as TGhaProcessorBase::ApplyFilter
 *      uses it, out -= wavreg1 + wavreg2, with the numerics of the decoder's step 4b (tests/host/at3p_tonal_cpu.c,
 *      at3pt_apply_filter). A band without waves in both blocks is left as it is.
 *   9. The frame that carries r_m's spectrum carries block T_{m-1} (the transform delays by one frame: the decoder's frame n
 *      gives input frame n-1). State at reset: a zero frame before the stream and no block before T_{-1}, which is found from
 *      (zeros, frame 0) like any other.
 * The constants are those of the prototype whose round-trip figures DESIGN.md section 17 lists; changing one changes the
 * definition. Against that prototype the definition admits the end bins in step 3 and normalises by rs and rc instead of 1 / 64
 * in steps 4 and 5: both only matter next to frequency index 0 or 1024, and the round-trip figures stay within 0.5 dB of it. Out of steps 1-9: envelope points (GATES below add them), sharing (SHARING below adds it), the leader flag, any psychoacoustic veto.
 *
 * GATES (AT3PHIP_TONES_GATED in `flags`; without the flag steps 1-9 stand as written and no output changes a byte). A block
 * describes its sines over two whole frames; a sine that starts or stops inside one of them is gated with the block's envelope
 * points, which the writer and the decoder already carry. A cell is 4 subband samples: a frame has 32, a block 64, cell j of a
 * block covering x[4 j .. 4 j + 3]. Float and double operations as written, each rounded, no FMA:
 *  G1. The gate of a frame, per channel and subband, from that frame's 128 samples x alone. e[j] = ((x[4j] * x[4j] + x[4j+1] *
 *      x[4j+1]) + x[4j+2] * x[4j+2]) + x[4j+3] * x[4j+3] in float, j = 0..31. P[0] = 0.0, P[j+1] = P[j] + (double)e[j] in double.
 *      For each split s in MIN .. 32 - MIN (MIN = AT3PHIP_TONE_GATE_MIN = 4 cells, the reference's "do not encode too short
 *      frame" rule, at3p_gha.cpp, len < 4): before(s) = P[s] / (double)s, after(s) = (P[32] - P[s]) / (double)(32 - s),
 *      d(s) = fabs(after - before). The candidate is s = MIN, replaced in ascending order by every s whose d is greater than the
 *      candidate's (so the largest d, the lowest s on a tie). With R = AT3PHIP_TONE_GATE_RATIO the candidate is an onset at s when
 *      after >= R * before and after > 0.0; else an offset with last active cell s - 1 when before >= R * after and before > 0.0;
 *      else the frame has no event (so never with a NaN energy). Added to make MIN hold for the loud side itself (a burst shorter
 *      than MIN cells is no event, and a gate never opens over cells that hold nothing): an onset also needs (double)e[j] >=
 *      R * before and e[j] > 0 for each of j = s .. s + MIN - 1, an offset (double)e[j] >= R * after and e[j] > 0 for each of
 *      j = s - MIN .. s - 1; failing that the frame has no event. At most one event per frame, channel and subband; a sine that
 *      starts and stops inside one frame is out of scope. As a byte: 0 = none, 1..31 = onset at s, 0x80 | p = offset with last
 *      active cell p.
 *  G2. What is written. The event of frame m+1 is the band's point pair in block T_m (start = s + 1 or stop = p + 1, the record's
 *      "+1" convention; the other point 0): the decoder adds 32 to the pend_env of the block it belongs to, which puts the point
 *      into that block's second half. Points are written whenever the gate fires, with or without a wave in the band, and
 *      num_tone_bands = the highest band holding a wave or a point in either channel, plus 1: every block's envelope then follows
 *      from the gates of its own two frames, and the slots of a call stay independent of one another.
 *  G3. A block's active interval [lo, hi] in cells is the curr_env that ff_atrac3p_generate_tones reconstructs for the block from
 *      its own points and those of the block before (decoder section, step 4b; decp_curr_env in the kernels): lo = start_pos with
 *      a start point, else 0; hi = stop_pos with a stop point, else 63. So an onset at s in the second frame gives [32 + s, 63];
 *      an offset at p in the first frame gives [0, p] when the second frame has no onset; an onset at s in the first frame and an
 *      offset at p in the second give [s, 32 + p]. An offset at p in the first frame FOLLOWED by an onset at s in the second gives
 *      [32 + s, 63]: the syntax holds one interval per block and the decoder keeps the later one; the analysis follows it. A
 *      block whose interval has fewer than MIN cells (hi - lo + 1 < MIN) gets no wave in that band.
 *  G4. The gated fit. A band without an event in either of its block's two frames runs steps 1-5 as written, rs and rc included.
 *      Otherwise: step 1 is y[t] = x[t] * w[t], w[t] = hann_window[t] for 4 lo <= t <= 4 hi + 3 and +0.0f elsewhere; steps 2 and
 *      3 run on that y; in step 4 S(f) and C(f) are summed as written and, beside them, from 0.0 for t = 4 lo .. 4 hi + 3 in
 *      order, Gss = sum of (double)w[t] * (sn * sn), Gcc = sum of (double)w[t] * (cs * cs), Gsc = sum of (double)w[t] * (sn * cs),
 *      sn = (double)sine_table[((t - 128) f) & 2047], cs = (double)sine_table[((t - 128) f + 512) & 2047]; det = Gss * Gcc -
 *      Gsc * Gsc; a = (S * Gcc - C * Gsc) / det, b = (C * Gss - S * Gsc) / det (the 2 x 2 normal equations of the least-squares
 *      fit under w: sine and cosine are no longer orthogonal under a one-sided window). An f whose det is not greater than 0.0 is
 *      passed over; the f of largest a * S + b * C is taken, the lowest on a tie; a candidate left without an f gives no wave.
 *      Step 5 takes that f's a and b; A2, the amplitude floor, AmpSf, PhaseIndex and steps 6-7 stay as they are (step 7 with the
 *      points of G2). The decoder does not Hann-window a gated region whose neighbour block has no wave there, and fades a gate
 *      over 4 samples; the analysis weighs with Hann times gate regardless. The mismatch costs efficiency, never correctness:
 *  G5. Step 8 subtracts exactly what the decoder's step 4b adds for these records, envelopes included (one device function,
 *      decp_waves, serves both).
 * The state carried per stream gains the block before the last one (its points decide the last block's envelope).
 *
 * SHARING (AT3PHIP_TONES_SHARED in `flags`, alone or with AT3PHIP_TONES_GATED; without the flag everything above stands as written
 * and no output changes a byte). A frame holds at most 48 waves for both channels together, and a wave that both channels hold
 * identically counts against that budget twice and is written twice; the syntax lets channel 1 take a band from channel 0
 * (tone_sharing), which the writer and the decoder already carry. The reference's analysis shares as well (at3p_gha.cpp,
 * FillFolowerRes), by frequency alone, which changes what the follower decodes; here a band is shared only when nothing changes:
 *  S1. Scope: stereo contexts. In a mono context the flag is accepted and changes nothing.
 *  S2. Twin bands, decided on the output of step 5 (with gates: of G1-G4), before the frame budget. For channel c and band b let
 *      W_c(b) be the set of the band's kept waves as their packed words, AT3PHIP_TONAL_WAVE(FreqIndex, AmpSf, PhaseIndex), and
 *      E_c(b) the band's point pair (start, stop) as G2 writes it, (0, 0) without gates. Band b is a twin when W_0(b) = W_1(b) as
 *      sets (the candidates of step 3 are ordered by power, which may differ between the channels where the words do not) and
 *      E_0(b) = E_1(b). Two bands without a wave and with equal points are twins.
 *  S3. Budget: step 6 ranks channel 0's kept waves of every band and channel 1's kept waves of the bands that are not twins, in
 *      the order it has (A2 descending, then channel, band, frequency index); the first 48 stay. A twin band of channel 1 has
 *      whatever channel 0's band keeps after the cut.
 *  S4. Record: tone_sharing bit b = twin(b) for b < num_tone_bands and 0 above; band[1][b] of a twin band is all zero (no count,
 *      no point) and contributes no entry to wave[]; second_is_leader stays 0; num_tone_bands is the highest band holding a wave
 *      or a point, plus 1, as before. Whether a band is a twin is not looked at again after the cut.
 *  S5. Residual (step 8 / G5): in a twin band channel 1 subtracts channel 0's waves under channel 0's envelope, which is what the
 *      decoder adds after copying the band. Each of the three records a slot touches - this slot's, the one before, and the one
 *      before that, whose points decide the older envelope - is resolved through its own tone_sharing. The carried state is the
 *      same records as before, so any split into calls gives the same bytes.
 * Consequence: twin bands hold equal words and equal points, so where the budget does not bind (the frame's waves, counted as in
 * step 6, are at most 48) the records with and without the flag describe the same synthesis in both channels and the residuals
 * are equal bit for bit; the flag then changes nothing but the tonal block's bits (and, through them, the quant units a loud
 * frame keeps). Where the budget binds, the waves it no longer counts twice go to the next strongest.
 * Out of this definition: the leader flag (with equal twins it buys nothing), phase-inverted and near-match sharing. */
#define AT3PHIP_TONE_PEAK_RATIO 16.0      /* step 3: a candidate's power over the mean power */
#define AT3PHIP_TONE_MAX_BAND_WAVES 3     /* step 3: candidates per channel and subband */
#define AT3PHIP_TONE_FINE_SPAN 7          /* step 4: frequency indices searched on either side of 8 k */
#define AT3PHIP_TONE_MIN_AMP 8.0          /* step 5: the smallest amplitude kept, in subband sample units */
#define AT3PHIP_TONE_GATE_MIN 4           /* G1, G3: the fewest cells on either side of a split, and in an interval that gets a wave */
#define AT3PHIP_TONE_GATE_RATIO 16.0      /* G1: the mean cell energy after an onset (before an offset) over the other side's */
/* flag of at3phip_analyse_tones, at3phip_encode_frames_tonal and at3phip_encode_frames_tonal_short: the analysis with GATES. A
 * stream stays with one mode between resets. Still ABI 1.6: a host that needs it looks for the symbol at3phip_host_tone_gates. */
#define AT3PHIP_TONES_GATED 32u
/* flag of the same three calls: the analysis with SHARING; may be combined with AT3PHIP_TONES_GATED. A stream stays with one mode
 * between resets. Still ABI 1.6: a host that needs it asks at3phip_host_tone_flags. */
#define AT3PHIP_TONES_SHARED 64u

/* Steps 1-8 on caller-supplied subband samples: the stage tap of at3phip_encode_frames_tonal.
 *   bands     [n_streams][n_frames][channels][16][128] float32 as at3phip_pqf_analyse writes them (flags & AT3HIP_PCM_ON_DEVICE:
 *             device memory)
 *   blocks    [n_streams][n_frames] records, host memory: slot f = the block of (the frame before frame f, frame f), the record
 *             the writer pairs with the NEXT residual; may be NULL
 *   residual  [n_streams][n_frames][channels][16][128] float32: slot f = the residual of the frame before frame f (a frame's
 *             block needs its successor, so the engine lags one frame); not divided by 32768 / 1.122018; may be NULL
 *             (flags & AT3HIP_OUT_ON_DEVICE: device memory)
 * State carried per stream between calls, of this function and of at3phip_encode_frames_tonal alike: the last frame's subband
 * samples and the last block; at3phip_reset clears it. Its buffers and tables are set up by the first call that needs them, not
 * by at3phip_create. Any float is accepted: every table index is masked, comparisons with a NaN are false (no candidate, no
 * wave); records, residuals (floats as bit patterns; a NaN where the definition gives one) and the frames of
 * at3phip_encode_frames_tonal are the definition's for each stream alone under every flag combination, and the analysis is
 * itself again two slots after the last non-finite sample (tests/test_float_domain_gpu.py, tests/test_float_domain_cpu.py; no
 * exception known). Added under ABI 1.6: a host looks for this symbol. */
int at3phip_analyse_tones(at3phip_ctx* ctx, const float* bands, int32_t n_frames, at3phip_tonal_block* blocks, float* residual,
                          uint32_t flags);

/* PCM to frames with the analysis: at3phip_pqf_analyse, steps 1-8, at3phip_mdct with AT3PHIP_RESIDUAL_SCALE and sine windows on
 * the residual, and the writer of at3phip_write_frames_tonal taking its records from device memory (valid by construction: no
 * host check); everything in between stays in HBM. Counted over the stream's life, output frame f holds the spectrum of residual
 * f-1 and block T_{f-2}: one frame later than at3phip_encode_frames, so ONE TRAILING FRAME OF SILENCE flushes the stream. Byte
 * for byte the frames of the host mirror's TAt3PEncoder with TAt3PToneAnalyser plugged in (atracdenc_amd/host/at3hip_host.hpp).
 * Where no wave is found and the carried state holds none, the frames are at3phip_encode_frames', one frame later. pcm, frames,
 * flags, AT3HIP_ASYNC / at3phip_sync and at3phip_reset as for at3phip_encode_frames; calls of the two kinds share the filter
 * bank's and the transform's state but not the lag, so a stream stays with one of them between resets.
 * Added under ABI 1.6: a host looks for this symbol. */
int at3phip_encode_frames_tonal(at3phip_ctx* ctx, const float* pcm, int32_t n_frames, uint8_t* frames, uint32_t flags);
/* The same for 16-bit PCM, widened in the filter bank's loads by the rule of at3phip_encode_frames_short. */
int at3phip_encode_frames_tonal_short(at3phip_ctx* ctx, const int16_t* pcm, int32_t n_frames, uint8_t* frames, uint32_t flags);

/* The analysis' tables as the first tonal call builds them, on the host (no GPU needed): float sine_table[2048],
 * float hann_window[256], float amp_sf_tab[64], float tw[256][2], double thr[64], double rs[1024], double rc[1024].
 * bytes = AT3PHIP_TONE_FIND_TABLES_BYTES. */
#define AT3PHIP_TONE_FIND_TABLES_BYTES 28416
int at3phip_host_tone_find_tables(void* dst, size_t bytes);

/* G1 on the host (no GPU needed): bands [n_frames][channels][16][128] float32 of one stream, out [n_frames][channels][16] bytes,
 * each frame's gate as G1 codes it (0 = none, 1..31 = onset at s, 0x80 | p = offset with last active cell p). A library that has
 * this symbol takes AT3PHIP_TONES_GATED. The host mirror's TAt3PToneAnalyser (atracdenc_amd/host/at3hip_host.hpp) gates through
 * this function, as it takes its tables from the one above; it is pinned to the restatement tests/host/at3p_gha_cpu.c. */
int at3phip_host_tone_gates(const float* bands, int32_t n_frames, int32_t channels, uint8_t* out);

/* The analysis flags this library understands, as a mask (no GPU needed): AT3PHIP_TONES_GATED | AT3PHIP_TONES_SHARED. A library
 * without this symbol predates AT3PHIP_TONES_SHARED. */
uint32_t at3phip_host_tone_flags(void);

/* ADAPTIVE WORD LENGTHS (AT3PHIP_ALLOC_ADAPTIVE in `flags` of at3phip_write_frames, at3phip_write_frames_tonal,
 * at3phip_encode_frames, at3phip_encode_frames_short, at3phip_encode_frames_tonal and at3phip_encode_frames_tonal_short, alone or
 * with the flags each of them takes; without the flag no output changes by a byte). The reference gives every quant unit a fixed
 * word length (TConfigure's allocTable: 7 bits for units 0-16, falling to 1 bit for unit 31) and searches only the number of
 * units, so a 2048-byte frame codes the top of the spectrum with 1-4 bits whatever the signal is, a loud stereo frame loses units
 * 28-31 and a quiet frame leaves thousands of bits unused. With the flag the word lengths are chosen per frame to fill it. The
 * syntax is unchanged (TWordLenEncoder codes arbitrary word lengths as deltas) and the decoder below decodes the frames as they
 * are. The reference has no such allocation: this is the project's definition, stated here and nowhere else, pinned bit for bit
 * to the C restatement tests/host/at3p_writer_cpu.c, and, for everything but the choice of the allocation, to the reference's own
 * coders: given the spectra and the word lengths A5 chose, the reference's TWordLenEncoder, TSfIdxEncoder, TQuantUnitsEncoder and
 * TTonalComponentEncoder under TBitStreamEncoder write the frame of A6 byte for byte and count Bits(A) + 3 bits
 * (tests/at3p_ref_parts_lib.py puts a configure part of its own, which holds the word lengths, in front of them;
 * tests/test_at3p_ref_parts_cpu.py compares where the reference is built, tests/golden/at3p_ref_parts.npz keeps frames it wrote
 * and tests/test_at3p_ref_parts_gpu.py holds the kernels to them). So A1, A2's quantiser and table choice, A4's word-length
 * section and A6's layout are the reference's; A3 and A5, which word lengths to ask for, are this text's alone. Not pinned to
 * anything outside the project: what FFmpeg's decoder makes of these frames (no such decoder was at hand). A1 is the fixed
 * writer's float code, every decision after it is integer arithmetic, so any float is accepted exactly as by the fixed writer.
 * Frames do not depend on one another: any split of a stream into calls gives the same bytes. Per frame:
 *  A1. Scale exactly as the fixed writer does (TScaler::Scale): sfi[ch][qu] in 0..63 and the scaled values. One step of sfi is a
 *      factor 2^(1/3), so three steps are one mantissa bit.
 *  A2. Cost table. For every channel, unit and word length w = 1..7 the mantissas are rint(v * inv_mant[w]) (the fixed writer's
 *      operation; no energy-adaptive pass); tab[ch][qu][w] is the cheapest of the eight code tables w - 1 + 7 i, i = 0..7, the
 *      first one on a tie, and B[ch][qu][w] that table's bits (EncodeQuSpectra's: codes, group flags, sign bits).
 *  A3. Candidate allocation A(t, k) for t in -21..63 and k in 0..64. want(ch, qu; t) = clamp(floor((sfi - t) / 3), 0, 7). N is
 *      1 plus the highest qu with want >= 1 in any channel, or 1 if there is none; an N of 29, 30 or 31 becomes 32 (the syntax
 *      has no 29..31, which is why the reference steps from 32 to 28). Then the units below N are walked with qu ascending,
 *      channel 0 before channel 1 within a qu: the first k units whose want at t - 1 exceeds their want at t take the t - 1
 *      value. Then every unit below N that still has 0 takes 1: a word length of 0 is never written, and the decoder's rule about
 *      it stands. A mono frame has one channel.
 *  A4. Bits(A): everything in the frame but its three leading bits: the unit count (5) and the mute bit (1); the word-length
 *      section exactly as TWordLenEncoder codes these word lengths - channel 0 in mode 3 as deltas to the previous unit
 *      (2 + 2 + 2 + 2 + 3 bits, then a code per unit from the second on), channel 1 in mode 1 as deltas to channel 0 (2 + 2 + 2
 *      bits, then a code per unit), each list under the table FindBestWlDeltaEncode picks (the first with the fewest bits) from
 *      the range its OR-accumulated largest delta m allows (m >= 3: tables 2 and 3; m = 2: table 1; else table 0); the scale
 *      factor indices (2 + 6 N per channel) and the code-table indices (1, then 4 + 3 N per channel); the sum of B over the coded
 *      units; the power groups for N (4 bits each, per channel); and the tail, formed once as in the fixed writer: two bits in
 *      stereo, window shapes, a gain-compensation bit per channel, tonal flag and block, noise flag, terminator. A frame is
 *      frame_bytes bytes (FRAME SIZE below; 2048 unless at3phip_set_frame_bytes was called) and A fits when
 *      Bits(A) <= 8 * frame_bytes - 3 (16381 at 2048 bytes).
 *  A5. Choice. t* is the smallest t in -21..63 whose A(t, 0) fits; t = 63 always fits at every admissible frame size: A(63, 0) is
 *      one unit per channel at word length 1, at most 77 bits in mono and 147 in stereo in front of the tail, and the tail is at
 *      most 1320 bits in mono and 1624 in stereo (FRAME SIZE below derives the smallest sizes from these). k* is the largest k
 *      in 0..64 whose A(t*, k) fits.
 *      Both are defined by the full scan and not by bisection: code lengths are not provably monotone in the word length, and
 *      the scan is the definition whether they are or not. A k beyond the number of units that can take the t - 1 value gives
 *      the allocation of that number, so k* is reported as that number: 0 for a frame that fits at t = -21.
 *  A6. The frame is A(t*, k*) in the fixed writer's layout, with tab[ch][qu][wl] as the unit's code-table index.
 * FRAME SIZE. frame_bytes is a property of the context: 2048 (352.8 kbit/s at 44.1 kHz, the one size the reference writes) until
 * at3phip_set_frame_bytes changes it. Admissible are the multiples of 8 from AT3PHIP_MIN_FRAME_BYTES_MONO (mono contexts) or
 * AT3PHIP_MIN_FRAME_BYTES_STEREO (stereo contexts) to 2048. The minimum is the smallest multiple of 8 at which A(63, 0) fits
 * whatever the spectrum and the tonal record are. Upper bounds from the tables, formed as tests/test_at3p_tonal_write_cpu.py forms
 * the 16-unit bound: in front of the tail 5 + 1 bits, the word-length section with every code at AT3P_WL_VLC's longest length,
 * scale factor and code-table indices and one power group per channel for N = 1, and unit 0's 16 lines at word length 1 under the
 * cheapest-in-the-worst-case of its eight tables (40 bits) - 77 bits in mono, 147 in stereo; the tail with 18 bits per window
 * shape, the long sharing form, every band with both envelope points, 48 waves of 10 + 6 + 5 bits and 24 order bits - 1320 bits
 * in mono, 1624 in stereo. 77 + 1320 = 1397 <= 8 * 176 - 3 and > 8 * 168 - 3; 147 + 1624 = 1771 <= 8 * 224 - 3 and > 8 * 216 - 3.
 * Everything else in A1-A6 stands at every size, "a word length of 0 is never written" included. Only 2048 bytes has a fixed
 * table: at any other size a frame-writing call without AT3PHIP_ALLOC_ADAPTIVE is refused, never served by another path.
 * Out of this definition: a word length of 0 inside the coded range, psychoacoustic weighting.
 * The tone analysis is unaffected by the flag; a stream may change it from call to call. Still ABI 1.6: a library that has the
 * symbol at3phip_host_allocate takes the flag. */
#define AT3PHIP_ALLOC_ADAPTIVE 128u

/* SPARSE WORD LENGTHS (AT3PHIP_ALLOC_SPARSE in `flags` of the same six calls, only together with AT3PHIP_ALLOC_ADAPTIVE; given alone
 * the call returns AT3HIP_EINVAL with a last-error text before anything is queued: no output byte is written and no stream state
 * moves. Without the flag nothing above changes: no byte, no PCM sample, no runtime call). A3's last step gives every unit below N at
 * least one bit, so one step of t that gives any high unit a bit raises N to that unit and pays for every unit below it at once; a
 * small frame cannot afford the step and leaves its bits unused. With the flag a unit inside the coded range may keep word length
 * 0. A1, A2, the budget 8 * frame_bytes - 3 and A5's two full scans stand; these steps replace A3, A4 and A6:
 *  A3s. Candidate A(t, k). want(ch, qu; t) as in A3. All 32 units are walked, qu ascending, channel 0 before channel 1: every unit
 *      takes its want at t, and the first k units whose want at t - 1 exceeds their want at t take the t - 1 value. No unit is
 *      raised from 0 to 1 afterwards. N is then 1 plus the highest qu whose word length is >= 1 in any channel: it is computed
 *      after the k-raise, so k extends the coded range one unit at a time (a flat spectrum, whose wants all step at the same t,
 *      needs that). If no unit has a word length >= 1, N = 1 and unit 0 of channel 0 takes 1. If N is 29, 30 or 31 it becomes 32
 *      and, unit 31 then having 0 in every channel, unit 31 of channel 0 takes 1. So the highest coded unit always carries a
 *      non-zero word length in some channel: "number of units" and "number of units with coded spectrum" never differ, and every
 *      later section's length is a function of N alone. Units at and above N have 0. k* is reported as in A5: the number of units
 *      that took the t - 1 value.
 *  A4s. Bits(A) as A4, except: the code-table section per channel is its 4 header bits plus 3 bits per unit below N whose word
 *      length is non-zero; in channel 1, one more bit for each unit below N with word length 0 whose channel-0 word length is
 *      non-zero: the syntax's "copy from channel 0" flag, written as 1 ("do not copy"; 0, copy, is never written). A unit with word
 *      length 0 contributes no mantissa bits; it still contributes its word-length code and its 6 scale-factor bits (the
 *      scale-factor mode stays 0, the index written is A1's). Word-length section, power groups and tail as in A4.
 *  A6s. The frame is A(t*, k*) in the fixed writer's layout with the code-table section as in A4s - per channel the 4 header bits,
 *      then unit by unit below N either the 3-bit index, or channel 1's flag, or nothing - and no spectrum for a unit at 0.
 * Where this syntax comes from: it is the layout FFmpeg's ATRAC3plus decoder reads (libavcodec/atrac3plus.c: the code-table index
 * is read only for units with a non-zero word length, and for a channel-1 unit at 0 under a coded channel-0 unit one bit says
 * whether channel 0's spectrum is copied), taken from that decoder AS RECALLED: the file was not at hand, the reference carries
 * only the trace of it (the fields qu_tab_idx / used_quant_units in its atrac3plus.h). This text, not FFmpeg, is what the tests pin.
 * What the reference's code does pin (tests/at3p_ref_parts_lib.py, as under ADAPTIVE WORD LENGTHS): the word-length section with
 * zeros in it (TWordLenEncoder), the scale factor indices, every unit's mantissas, code-table choice and codes
 * (TQuantUnitsEncoder::TUnit, which cannot be asked for word length 0 and is not), the power groups and the tail; frames put
 * together from these are the sparse writer's byte for byte and Bits(A) + 3 bits long. What it cannot pin is the code-table section
 * of A4s / A6s, the one part the reference has no code for: there the comparison's driver writes this text, and a difference would
 * be settled by this text. And no decoder other than this project's has read these frames: FFmpeg's was not at hand.
 * FFmpeg's other differences from the reference writer (power levels at N <= 2, the window-shape bit count) are left alone.
 * Smallest sizes: A(63, 0) under A3s is unit 0 of channel 0 at word length 1 and nothing else, which costs no more than A3's one
 * unit per channel (at most 77 bits in mono and 147 in stereo in front of the tail; tests/test_at3p_sparse_cpu.py re-derives the
 * bound), so AT3PHIP_MIN_FRAME_BYTES_* and the admissible sizes are unchanged.
 * Property: at t = -21 every want is 7, so a frame that fits at t = -21 is byte for byte the frame AT3PHIP_ALLOC_ADAPTIVE alone
 * writes.
 * Decoding: any decoder of the full syntax; this project's with AT3PHIP_DECODE_SPARSE (decoder section). Out of this definition:
 * the copy value of the clone flag, scale-factor modes other than 0, noise filling and power compensation in the decoder.
 * Still ABI 1.6: a library that has the symbol at3phip_host_allocate_sparse takes the flag; a build without the adaptive writer
 * refuses it as it refuses AT3PHIP_ALLOC_ADAPTIVE. */
#define AT3PHIP_ALLOC_SPARSE 256u

/* RATE-DISTORTION WORD LENGTHS (AT3PHIP_ALLOC_RD in `flags` of the same six calls, only together with AT3PHIP_ALLOC_ADAPTIVE and
 * AT3PHIP_ALLOC_SPARSE, because it needs word length 0; given without either the call returns AT3HIP_EINVAL with a last-error text
 * before anything is queued: no output byte is written and no stream state moves. Without the flag nothing above changes: no byte, no
 * PCM sample, no runtime call). A3 asks for a word length from the unit's scale factor, its peak, alone: a unit with one loud line
 * among quiet ones gets the word length of a flat unit, and the cost table B is used to check a candidate, never to choose one.
 * With the flag every unit takes the word length that minimises distortion + lambda * bits, lambda is scanned as t is, and the frame is
 * filled as k fills it. The frames are sparse frames: no syntax changes, and they decode with AT3PHIP_DECODE_SPARSE. This project's
 * definition, stated here and nowhere else, pinned bit for bit to the C restatement tests/host/at3p_rd_cpu.c. A1, A2, A4s, A6s, the
 * budget 8 * frame_bytes - 3 and the tail stand; these steps replace A3s and A5:
 *  R1. Distortion table, integer, order-free. For every channel, unit, word length w = 0..7 and line of the unit, with v A1's scaled
 *      and clamped value and m A2's mantissa at w (m = 0 at w = 0): e = v - (float)m * atrac3p_mant_tab[w] (a float multiply, then a
 *      float subtract, each rounded on its own), d = e * e in float, u = (uint64)(d * 0x1p40f) truncated, u = 0 when d is NaN.
 *      S[ch][qu][w] is the sum of u over the unit's lines: integer addition is exact, so the order of the lines is free (d < 1, so
 *      S < 2^47). D[ch][qu][w] = (double)S * G[sfi] with G[i] = (double)ScaleTable[i] * (double)ScaleTable[i]: that product of two
 *      floats is exact in double and S converts exactly, so D is one rounded double multiply. No libm enters.
 *  R2. Candidate R(j, k). lambda_j = 0x1p40 * G[j mod 3] * 4^floor(j / 3), floor division and a non-negative remainder;
 *      ScaleTable[i + 3] is exactly 2 ScaleTable[i], so lambda_j = 2^40 G[j] inside 0..63 and continues by exact factors of 4 outside.
 *      pick(ch, qu; j) is the w in 0..7 with the smallest D[w] + lambda_j * (double)(B[w] + (w > 0 ? 3 : 0)), B[0] = 0, multiply and
 *      add rounded separately; w is walked ascending and a tie keeps the smaller w. The 3 is the code-table index a non-zero unit pays
 *      in A4s. All 32 units are walked, qu ascending, channel 0 before channel 1: every unit takes pick(.; j), and the first k units
 *      whose pick at j - 1 exceeds their pick at j take the j - 1 value. Then A3s's closing rules apply unchanged: N follows the
 *      raise, an empty frame gives unit 0 of channel 0 word length 1, an N of 29..31 becomes 32 and unit 31 of channel 0 takes 1.
 *      Bits(R) is A4s. (The raise list is walked by unit, not ordered by distortion gained per bit: the walk by unit is A3s's.)
 *  R3. Choice, by full scans as in A5. j* is the smallest j in J_MIN..J_MAX = -30..69 whose R(j, 0) fits (J_MAX where none does: a
 *      caller's table only); k* the largest k in 0..64 whose R(j*, k) fits, reported as the number of units that took the j - 1 value.
 *      J_MAX makes every unit pick 0 whatever the spectrum: D[0] <= lines * 2^40 * G[sfi] <= lines * 2^40 (G[63] = 1), and a unit of
 *      `lines` lines costs at least lines / 16 bits at any w > 0 (every one of its 16-line chunks costs at least one bit under every
 *      code table; tests/test_at3p_rd_cpu.py re-derives that from at3p_vlc.inc), so w > 0 costs at least lambda * (lines / 16 + 3)
 *      more than w = 0 saves when lambda_j / 2^40 >= lines / (lines / 16 + 3), at most 128 / 11 < 16 = lambda_69 / 2^40
 *      (lambda_68 / 2^40 is 10.08: 69 is the smallest). So R(69, 0) is A3s's smallest frame, unit 0 of channel 0 at word length 1,
 *      and fits at every admissible size. (The tables give more: no chunk costs less than 4 bits, which makes 66 the smallest such
 *      j; 69 follows from the weaker premise and makes the count of j a multiple of 4.) J_MIN = -30: lambda_-30 = 2^-22, a bit then
 *      costs the squared error of one line that is 2^-11 off at the highest scale factor. It only has to lie below every j* of a
 *      frame with less room than its spectrum can use: on the project's signals (noise, mix, stress, tones, burst and full-scale
 *      noise, mono and stereo, 376 to 2048 bytes) the lowest j* of a frame that does not fit at -30 is -10. A frame that fits at
 *      -30 is written with the picks at -30 - word length 7 wherever a shorter one has 2^-22 more distortion per bit saved, nothing
 *      for a silent unit - and R4 puts A(t*, k*) in its place where that has less distortion. 100 values of j: the four wavefronts
 *      of the kernel share the scan evenly.
 *  R4. Guard. A(t*, k*) of A3s / A5, the frame AT3PHIP_ALLOC_SPARSE alone writes, is formed as well. T(X) is the sum of
 *      D[ch][qu][wl_X[ch][qu]] over all 32 units of every channel present in the order of the walk, a serial double sum from +0.0
 *      (units at and above N have word length 0 and count with D[0]). The frame is R(j*, k*) if T(R) <= T(A), else A(t*, k*), byte for
 *      byte today's sparse frame. Property, exact: the written allocation's T never exceeds the sparse allocation's. T is squared
 *      error on the spectrum, per frame: it bounds nothing about the time-domain signal after the decoder's overlap.
 *  R5. Floats outside the domain. A1 is the fixed writer's: an infinite line is clamped to +-0.99999, a NaN line stays NaN. A NaN
 *      scaled value gives a NaN d at every w and so u = 0: it adds no distortion and never asks for bits. The mantissa of a NaN is
 *      the conversion tests/host/at3p_writer_cpu.c documents at quantise(). Every decision after R1's float operations is integer or
 *      double arithmetic on finite numbers, so any float is accepted, frames do not depend on one another, and no stream affects
 *      another.
 * Out of this definition: psychoacoustic weighting, which MASKING-WEIGHTED WORD LENGTHS below adds under a flag of its own. Still ABI
 * 1.6: a library that has the symbol at3phip_host_allocate_rd takes the flag; a build without the rate-distortion writer (at3p_rd.hip)
 * has neither. */
#define AT3PHIP_ALLOC_RD 512u

/* MASKING-WEIGHTED WORD LENGTHS (AT3PHIP_ALLOC_PSY in `flags` of the same six calls, only together with AT3PHIP_ALLOC_ADAPTIVE,
 * AT3PHIP_ALLOC_SPARSE and AT3PHIP_ALLOC_RD; given without any of the three the call returns AT3HIP_EINVAL with a last-error text before
 * anything is queued: no output byte is written and no stream state moves. Without the flag nothing above changes: no byte, no PCM
 * sample, no runtime call). R2 minimises plain squared error, so it spends bits on noise nobody would hear: in units under the
 * threshold in quiet and in units next to a loud one. With the flag every unit sees lambda shifted by how far its masking threshold
 * lies above the frame's lowest: a unit masked 2 dB more pays for a bit what the others pay one step of j later. The frames are sparse
 * frames: no syntax changes, the decoder flag is AT3PHIP_DECODE_SPARSE. This project's definition, stated here and nowhere else, pinned
 * bit for bit to the C restatement tests/host/at3p_rd_cpu.c. A1, A2, A4s, A6s, R1, the budget and the tail stand; lambda_i is R2's
 * for any integer i, G is R1's table; one step of either index is a factor 2^(2/3) of energy, 2.007 dB.
 *  M1. Energy. E[ch][qu] = D[ch][qu][0] of R1: the unit's energy on D's scale (2^40 times the sum of its squared lines), exact and
 *      order-free already. A unit is live when S[ch][qu][0] > 0.
 *  M2. Threshold index. Th[ch][qu] = max(lambda_{ath[qu]}, max over q' in 0..31 with spread[q'][qu] <= 63 of E[ch][q'] *
 *      G[63 - spread[q'][qu]]): each product one rounded double multiply, the maxima exact. Maskers come from the same channel only
 *      (cross-channel masking is unsafe under binaural unmasking). mu[ch][qu] is the largest i in 0..MU_HI with lambda_i <= Th; it
 *      exists because Th >= lambda_{ath[qu]}. MU_HI = 73, the larger of 73 and the largest ath entry: lambda_73 is the largest lambda_i
 *      not above 2^47, and D[0] cannot exceed 2^47.
 *  M3. Offsets. mu_min is the minimum of mu over the live units of every channel in the frame. o[ch][qu] = min(mu - mu_min, 32) for a
 *      live unit and 0 for a unit that is not live (it picks 0 at every lambda); 0 everywhere when no unit is live. O is the largest
 *      o of the frame. 32 steps are 64 dB: the range over which the weighting tells units apart.
 *  M4. Candidate P(j, k): R2 with one change. pick(ch, qu; j) minimises D[w] + lambda_{j + o[ch][qu]} * (double)(B[w] + (w > 0 ? 3 : 0)),
 *      the j - 1 value likewise with lambda_{j - 1 + o[ch][qu]}. No new multiply enters the pick. The walk, the raise list, the closing
 *      rules and Bits are R2's.
 *  M5. Choice. j* is the smallest j in -30 - O .. 69 whose P(j, 0) fits (69 where none does: a caller's table only); k* as in R3. At
 *      j = 69 every unit sees an index of at least 69 and picks 0 by R3's bound, which holds for every larger lambda, so the smallest
 *      frame fits at every admissible size. The lower end moves with O so that the most-masked unit can still reach lambda_-30 before
 *      the scan gives up; a frame with room would otherwise be left underfilled.
 *  M6. Guard. Tw(X) is the serial double sum from +0.0, in the walk's order, of D[ch][qu][wl_X[ch][qu]] * G[63 - o[ch][qu]]: one rounded
 *      multiply per term. The frame is P(j*, k*) if Tw(P) <= Tw(A), else A(t*, k*), the sparse frame byte for byte. Property, exact:
 *      the written allocation's Tw never exceeds the sparse allocation's.
 *  M7. Floats outside the domain. R5 stands: a NaN line adds nothing to S. Everything in M1-M6 is integer or double arithmetic on
 *      finite numbers (E <= 2^47, G <= 1); no stream affects another.
 * Consequence: with every offset 0 the frame is the rate-distortion frame byte for byte (G[63] = 1.0, the scan starts at -30).
 * The two tables are integers, so no libm result is part of a frame; atracdenc_amd/csrc/at3p_psy.inc holds them, written by
 * tools/gen_at3p_psy.py, which says how they were formed: spread from the Bark distance of the units' centre frequencies with a
 * 12 dB signal-to-mask distance and slopes of 10 dB per Bark upwards and 27 dB per Bark downwards, ath from the threshold in quiet
 * against the spectrum energy of a full-scale sine. These integers are the definition.
 *  spread[q'][q], row q' = 0..31 (255: no masking):
 *     6  14  22  30  36  42  48  53  59 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255
 *    29   6  14  21  28  34  39  44  50  57  62 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255
 *    50  27   6  13  20  26  31  36  42  49  54  59  62 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255
 *   255  47  26   6  13  19  24  29  35  42  47  51  55  58  61 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255
 *   255 255  44  24   6  12  17  22  28  35  40  45  48  52  54  57  61 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255
 *   255 255  60  40  22   6  11  16  22  29  34  39  42  46  48  51  54  59  62 255 255 255 255 255 255 255 255 255 255 255 255 255
 *   255 255 255  55  37  20   6  11  17  23  29  33  37  40  43  46  49  53  57  60  63 255 255 255 255 255 255 255 255 255 255 255
 *   255 255 255 255  50  33  19   6  12  19  24  28  32  35  38  41  44  49  52  55  58  61 255 255 255 255 255 255 255 255 255 255
 *   255 255 255 255 255  50  35  22   6  13  18  22  26  29  32  35  38  42  46  49  52  55  58  62 255 255 255 255 255 255 255 255
 *   255 255 255 255 255 255  53  40  24   6  11  16  19  23  26  28  32  36  39  43  46  48  51  55  58  60  61  62  63 255 255 255
 *   255 255 255 255 255 255 255  55  38  20   6  10  14  17  20  23  26  30  34  37  40  43  46  50  52  54  56  57  58  59  60  60
 *   255 255 255 255 255 255 255 255  50  32  18   6  10  13  16  18  22  26  30  33  36  38  42  45  48  50  51  53  54  54  55  56
 *   255 255 255 255 255 255 255 255  60  42  28  16   6   9  12  15  18  22  26  29  32  35  38  41  44  46  48  49  50  51  51  52
 *   255 255 255 255 255 255 255 255 255  51  37  25  15   6   9  11  15  19  23  26  29  31  35  38  41  43  44  46  47  47  48  49
 *   255 255 255 255 255 255 255 255 255  59  44  33  22  14   6   9  12  16  20  23  26  29  32  35  38  40  42  43  44  45  45  46
 *   255 255 255 255 255 255 255 255 255 255  51  40  29  21  13   6   9  14  17  21  23  26  29  33  35  37  39  40  41  42  43  43
 *   255 255 255 255 255 255 255 255 255 255  61  49  39  30  22  15   6  10  14  17  20  23  26  29  32  34  35  37  38  39  39  40
 *   255 255 255 255 255 255 255 255 255 255 255  60  50  41  33  27  17   6  10  13  16  18  22  25  28  30  31  33  34  34  35  36
 *   255 255 255 255 255 255 255 255 255 255 255 255  60  51  43  36  27  16   6   9  12  15  18  21  24  26  28  29  30  31  31  32
 *   255 255 255 255 255 255 255 255 255 255 255 255 255  60  52  45  36  25  15   6   9  11  15  18  21  23  24  26  27  27  28  29
 *   255 255 255 255 255 255 255 255 255 255 255 255 255 255  60  53  44  33  23  14   6   9  12  15  18  20  22  23  24  25  25  26
 *   255 255 255 255 255 255 255 255 255 255 255 255 255 255 255  60  51  39  30  21  13   6   9  13  15  17  19  20  21  22  23  23
 *   255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255  59  48  39  30  22  15   6   9  12  14  16  17  18  19  19  20
 *   255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255  58  48  39  31  24  15   6   9  11  12  13  14  15  16  17
 *   255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255  55  46  38  31  22  13   6   8  10  11  12  13  13  14
 *   255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255  60  52  44  37  28  18  11   6   8   9  10  11  11  12
 *   255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255  56  48  41  32  23  16  10   6   7   8   9  10  10
 *   255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255  59  51  44  35  26  19  14   9   6   7   8   8   9
 *   255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255  62  54  47  38  29  22  16  12   9   6   7   7   8
 *   255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255  56  49  40  31  24  18  14  11   8   6   7   7
 *   255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255  58  51  42  33  26  20  16  13  10   8   6   7
 *   255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255 255  60  53  44  34  27  22  18  14  12   9   8   6
 *  ath[q], q = 0..31:
 *    19  14  13  12  12  12  11  11  10   9   9   8   8   8   7   7   8   9  11  13  14  15  16  16  15  15  17  21  29  35  41  47
 * Known limits. With the tone analysis the written spectrum is the residual, so the extracted sines do not count as maskers: the
 * threshold is then too low, never too high, which costs gain and not quality. No temporal masking, no tonality estimate: every
 * masker is taken for noise-like. Still ABI 1.6: a library that has the symbol at3phip_host_allocate_psy takes the flag; a build
 * without the masking-weighted writer (at3p_psy.hip) has neither. */
#define AT3PHIP_ALLOC_PSY 1024u

/* Steps A3-A5 on a caller-supplied cost table, on the host (no GPU needed).
 *   sfi        [channels][32] scale factor indices, each 0..63
 *   bits       [channels][32][8] uint16: entry w = B[ch][qu][w]; entry 0 is not read
 *   tail_bits  the tail's bits (A4), 0..16381
 *   wl_out     [channels][32]: the word lengths of A(t*, k*), 0 at and above N
 *   n_units, t, k   N, t*, k*
 * Where no t fits (possible only with a table that no spectrum gives) t* = 63 and k* = 0 are reported. AT3HIP_EINVAL on a null
 * pointer, a channel count other than 1 or 2, an sfi above 63 or tail_bits out of range. */
int at3phip_host_allocate(const uint8_t* sfi, const uint16_t* bits, int32_t channels, int32_t tail_bits, uint8_t* wl_out, int32_t* n_units,
                          int32_t* t, int32_t* k);

/* The smallest admissible frame sizes (FRAME SIZE above); tests/test_at3p_rate_cpu.py derives them from the tables. */
#define AT3PHIP_MIN_FRAME_BYTES_MONO 176
#define AT3PHIP_MIN_FRAME_BYTES_STEREO 224

/* The same against the budget 8 * frame_bytes - 3; tail_bits in 0..8 * frame_bytes - 3. at3phip_host_allocate is this call at
 * 2048. Also AT3HIP_EINVAL for a frame size that is not admissible for the channel count. Still ABI 1.6: a library that has this
 * symbol has the frame-size setters below. */
int at3phip_host_allocate_sized(const uint8_t* sfi, const uint16_t* bits, int32_t channels, int32_t tail_bits, int32_t frame_bytes,
                                uint8_t* wl_out, int32_t* n_units, int32_t* t, int32_t* k);

/* A3s, A4s and A5 (SPARSE WORD LENGTHS) on a caller-supplied cost table, on the host (no GPU needed): arguments, results and errors
 * as at3phip_host_allocate_sized; wl_out may hold 0 below N. Entry 0 of `bits` is not read. */
int at3phip_host_allocate_sparse(const uint8_t* sfi, const uint16_t* bits, int32_t channels, int32_t tail_bits, int32_t frame_bytes,
                                 uint8_t* wl_out, int32_t* n_units, int32_t* t, int32_t* k);

/* R2-R4 (RATE-DISTORTION WORD LENGTHS) on caller-supplied tables, on the host (no GPU needed): sfi, bits, channels, tail_bits,
 * frame_bytes, wl_out and n_units as at3phip_host_allocate_sparse; dist [channels][32][8] uint64 is S of R1 (every entry is read,
 * each at most 2^47). j and k receive j* and k* of R3 whichever allocation is written; chose_rd receives 1 when wl_out is R(j*, k*)
 * and 0 when the guard of R4 fell back to A(t*, k*). Errors as at3phip_host_allocate_sparse, also for a null dist or chose_rd and
 * an S above 2^47. */
int at3phip_host_allocate_rd(const uint8_t* sfi, const uint16_t* bits, const uint64_t* dist, int32_t channels, int32_t tail_bits,
                             int32_t frame_bytes, uint8_t* wl_out, int32_t* n_units, int32_t* j, int32_t* k, int32_t* chose_rd);

/* M1-M6 (MASKING-WEIGHTED WORD LENGTHS) on caller-supplied tables, on the host (no GPU needed): sfi, bits, dist, channels, tail_bits,
 * frame_bytes, wl_out, n_units, j and k as at3phip_host_allocate_rd. offsets_in null: the offsets are M1-M3's, from dist and sfi;
 * offsets_in [channels][32], each 0..32: they are used as given (O is their largest). chose_psy receives 1 when wl_out is P(j*, k*)
 * and 0 when the guard of M6 fell back to A(t*, k*); offsets_out [channels][32], which may be null, the offsets used. Errors as
 * at3phip_host_allocate_rd, also for an offset above 32. */
int at3phip_host_allocate_psy(const uint8_t* sfi, const uint16_t* bits, const uint64_t* dist, const uint8_t* offsets_in, int32_t channels,
                              int32_t tail_bits, int32_t frame_bytes, uint8_t* wl_out, int32_t* n_units, int32_t* j, int32_t* k,
                              int32_t* chose_psy, uint8_t* offsets_out);

/* The context's frame size (FRAME SIZE above). Given an admissible size the setter first waits for everything queued on the
 * context, as at3phip_sync does (a queued call still writes frames of the old size), then stores the size: it allocates and
 * uploads nothing (the staging buffers are sized for 2048 bytes, the upper bound) and does
 * not touch stream state - frames do not depend on one another, so a stream may change its size between calls. From then on
 * `frames` of at3phip_write_frames, at3phip_write_frames_tonal, at3phip_encode_frames, at3phip_encode_frames_short,
 * at3phip_encode_frames_tonal and at3phip_encode_frames_tonal_short is [n_streams][n_frames][frame_bytes], dense; a frame is
 * 4-byte aligned in it whenever the buffer is, which the writer's word stores rely on. At a size other than 2048 each of the six
 * is refused with AT3HIP_EINVAL unless `flags` has AT3PHIP_ALLOC_ADAPTIVE ("the fixed table is defined for 2048-byte frames
 * only"), before anything is queued: no output byte is written and no stream state moves. AT3HIP_EINVAL with a last-error text,
 * and the size unchanged, for a size that is not admissible; AT3HIP_EINVAL for a null context. A context on which the setter was
 * never called behaves byte for byte as before. Still ABI 1.6: a host looks for the symbol.
 * (The command-line tool, at3hipenc: --bitrate chooses among ten of these sizes; `-d` names the bitrate in its codec line for
 * every size but 2048, whose line stays the text it always was.) */
int at3phip_set_frame_bytes(at3phip_ctx* ctx, int32_t frame_bytes);
int at3phip_get_frame_bytes(const at3phip_ctx* ctx, int32_t* frame_bytes);

/* With AT3HIP_ASYNC in `flags` at3phip_encode_frames only queues the call (pcm must stay valid, frames must not be read)
 * and the frame writer of one call runs beside the filter bank and transform of the next (its own stream, spectra
 * double-buffered); at3phip_sync waits for everything queued. Without the flag the call waits itself. A queued call records no
 * stage-timing events (they sit between the kernels and cost the chain): the timing getters then read zero; a synchronous call
 * is timed as before. */
int at3phip_sync(at3phip_ctx* ctx);

/* Device milliseconds the frame writer took in the last at3phip_write_frames / at3phip_encode_frames call. */
int at3phip_get_write_timing(const at3phip_ctx* ctx, float* write_ms);

/* Device milliseconds of the last call: {pqf, mdct}. */
int at3phip_get_timings(const at3phip_ctx* ctx, float* pqf_ms, float* mdct_ms);

/* The constant tables as at3phip_create builds them, on the host (no GPU needed); bytes = AT3PHIP_TABLES_BYTES. */
#define AT3PHIP_TABLES_BYTES 3456
int at3phip_host_tables(void* dst, size_t bytes);
/* The frame writer's tables (code tables, scale table, the spectrum-independent leading bits per channel count and
 * number of quant units) as at3phip_create builds them; bytes = AT3PHIP_WRITE_TABLES_BYTES. */
#define AT3PHIP_WRITE_TABLES_BYTES 41384
int at3phip_host_write_tables(void* dst, size_t bytes);

/* ---- decoder ---------------------------------------------------------------------------------------------------------------
 * A batched ATRAC3plus decoder: frames as TAt3PBitStream::WriteFrame writes them without a tonal block (at3p_bitstream.cpp:
 * 101-726) -> PCM, for a batch of independent streams, every frame of a call in parallel. The reference has no ATRAC3plus decoder;
 * steps 1, 2 and 4 are this project's definition, steps 3 and 5 restate the reference's synthesis half bit for bit.
 *
 * Definition. A frame is frame_bytes bytes (AT3PHIP_FRAME_BYTES, 2048, unless at3phip_decoder_set_frame_bytes was called) holding
 * one channel unit of `channels` channels; it gives 2048 samples per channel.
 *   1. Unpack, MSB first, in the writer's order (every "must" failing rejects the frame, rule 7):
 *      - 1 bit, must be 0; block type (2 bits), must be channels - 1; quant units - 1 (5 bits) = nqu - 1; mute (1 bit), must be 0.
 *      - Word lengths (TWordLenEncoder, :170-252). Channel 0: mode (2 bits, must be 3), weight index and coded values (2 bits
 *        each, must be 0), a table index i (2 bits), wl0[0] (3 bits), then per further unit a code of AT3P_WL_VLC[i]:
 *        wl0[q] = (wl0[q-1] + d) & 7. Channel 1: mode (2 bits, must be 1), 2 bits (must be 0), a table index i (2 bits), then per
 *        unit a code d of AT3P_WL_VLC[i]: wl1[q] = (wl0[q] + d) & 7.
 *        Decision: a word length of 0 (never written: allocTable's minimum is 1) is an out-of-range value and rejects the frame.
 *      - Scale-factor indices (TSfIdxEncoder, :254-276): per channel mode (2 bits, must be 0), then 6 bits per unit.
 *      - Code-table indices (:278-306): the full-table flag f (1 bit); per channel table type (1 bit), mode (2 bits) and
 *        coded-values flag (1 bit), all must be 0, then an index of f + 2 bits per unit.
 *      - Per channel, the spectra (EncodeQuSpectra, :310-373): unit q is coded with spectra table wl - 1 + 7 * index
 *        (atrac3p_spectra_tabs: group size, coefficients per code, bits, signedness); each group of a table whose group size is
 *        not 1 is preceded by a flag bit, 0 = the group is all zero; a code carries its coefficients in `bits`-bit fields from the
 *        low end (two's complement for signed tables); an unsigned table puts one sign bit (1 = negative) after the code per
 *        non-zero coefficient, in coefficient order. Then 4 x subband_to_num_powgrps[qu_to_subband[nqu - 1]] bits of power
 *        compensation levels, each must be 15.
 *      - Stereo: swap / negate (2 bits), must be 0. Per channel the window shape: 0 = all sine; 1 0 = all 16 subbands steep;
 *        1 1 = one bit per subband b = 0..15 (1 = steep). Decision: 16 bits whatever nqu, the writer's layout: its tonal part is
 *        formed once, in the pass with 32 units (sbNum = qu_to_subband[31] + 1, at3p_bitstream.cpp:663-684), so reading
 *        qu_to_subband[nqu - 1] + 1 bits would misread its frames with fewer units.
 *      - Per channel gain compensation (1 bit), must be 0; the tonal flag (1 bit), must be 0; the noise flag (1 bit), must be 0;
 *        the terminator (2 bits), must be 3. Bits after it are ignored.
 *   2. Dequantise: line k of unit q = (float)m * atrac3p_mant_tab[wl] * ScaleTable[sf], left to right in float (no FMA); lines of
 *      no coded unit are +0.0f. Unit boundaries are TScaleTable::SpecsPerBlock's.
 *   3. Per channel TAt3pMIDCT::Do (at3p_mdct.cpp:103-152): odd subbands reversed, TMIDCT<256> at its default scale, frame n's
 *      first half windowed with frame n-1's flags and its second half with frame n's, overlap-added with frame n-1's windowed
 *      second half.
 *   4. Rescale: every subband sample times (float)(32768.0 / 1.122018), one float multiply (undoes EncodeFrame's division,
 *      at3p.cpp:143-147).
 *   5. Per channel ff_atrac3p_ipqf (atrac3plus_pqf/ut/atrac3plusdsp.c): per subband sample column the DCT-IV "dct4" in double,
 *      sum += x[n] * cos((M_PI / 16) * ((double)n + 0.5) * ((double)k + 0.5)) for n = 0..15 (each product and sum rounded, no
 *      FMA; the cosines from the host's libm), stored reversed as (float)(sum * (1.0 / 1024)); a 24-row history ring
 *      (mod23_lut is a mod-24 table: lut[0] = 23, lut[25] = 0), so a frame's first samples reach back 23 columns into frame n-1;
 *      the 12-tap FIR in float, out = out + ((h1 * c1) + (h2 * c2)) tap by tap from +0.0f.
 *   6. Clamp to [-1, 1]; float32, or int16 = lrintf(x * 32767.0f) with AT3PHIP_DECODE_S16. Frame n gives samples
 *      [2048 n, 2048 n + 2048) of the stream: the codec delay (2416 samples against at3phip_encode_frames' input: one frame of
 *      the transform and the filter bank's 368) is not trimmed.
 *   7. A frame is rejected (counted per reason, at3phip_decoder_counters) for: a bad first bit or block type; a syntax element
 *      outside what the writer emits (mute, modes, power levels other than 15, swap / negate, gain compensation, noise); a
 *      tonal block (unless AT3PHIP_DECODE_TONES); an invalid code or an out-of-range value (every code table is complete, so this is a word length of 0);
 *      a read past the frame's frame_bytes bytes; a terminator other than 3. A rejected frame decodes as a zero spectrum in every
 *      channel with all-sine windows, and those are the flags frame n+1 pairs with. */
/* TONAL BLOCKS (AT3PHIP_DECODE_TONES). The sine waves the reference encoder's GHA analysis subtracted from the subband signal
 * (at3p.cpp:118-170, TGhaProcessorBase::ApplyFilter) are added back. Without the flag every step above stands as written.
 *   1. Unpack: when the tonal flag is 1 it is followed, in the order of TTonalComponentEncoder::WriteTonalBlock and
 *      CreateFreqBitPack (at3p_bitstream.cpp:41-95, 487-629), by:
 *      - the amplitude mode (1 bit), must be 1; NumToneBands - 1 as a code of HuffTabs.NumToneBands (at3p_tone_vlc.inc);
 *      - stereo: the tone-sharing flags (0 = none, 1 0 = all, 1 1 + one bit per band); the leader flag as a one-band flag set,
 *        0 or 1 0. Decision: 1 0 swaps channels 0 and 1 for every tone band, as ApplyFilter does; 1 1 (never written) must not
 *        occur. Then the invert-phase flags (1 bit), must be 0;
 *      - per channel (channel 1 skips every shared band): channel 1's envelope-copy bit, must be 0; per band the envelope's
 *        start and stop point, each a presence bit and 5 bits when present; the num-waves mode (ch + 1 bits), must be 0, then
 *        4 bits of wave count per band; channel 1's delta-to-leader bit, must be 0; per band with waves its frequencies: an
 *        order bit (only with 2 or more waves; 0 = ascending). Ascending: the first in 10 bits, then each after a predecessor
 *        p < 512 in 10 bits, else in b = GetFirstSetBit(1023 - p) + 1 bits as f - (1024 - 2^b). Descending: the last wave's in
 *        10 bits, then towards the first each in GetFirstSetBit(p) + 1 bits (GetFirstSetBit(0) = 0). Then the amplitude mode
 *        (ch + 1 bits), must be 0, 6 bits of amp_sf per wave, and 5 bits of phase per wave, band by band.
 *      A "must" failing counts as unsupported_syntax, more than 48 waves in the frame as bad_code, a read past the frame as
 *      read_past_end; tonal_present does not count. Decision: NumToneBands may exceed the quant unit count (the writer aborts
 *      instead of writing such a frame): the synthesis is defined for all 16 subbands.
 *      Per-frame state, as ApplyFilter keeps it: every frame starts with no waves in all 16 bands of both channels; an absent
 *      start point is start_pos -1, an absent stop point stop_pos 32; start_index is assigned band by band, channel 0 first;
 *      a shared band of channel 1 copies channel 0's record, and the leader swap follows the copy. tones_present is 0 for a frame
 *      without a tonal block, a rejected frame and any frame decoded without the flag.
 *   4b. Between steps 4 and 5, per channel and subband sb = 0..15 (every subband, coded or not), where
 *      ff_atrac3p_generate_tones' condition holds (frame n or n-1 has tones present, and the band has waves in frame n or n-1):
 *      let g be that function's output on a zero-filled 128-sample buffer, with tones_info = frame n's block and
 *      tones_info_prev = frame n-1's (its curr_env reconstructed as the function reconstructed it for frame n-1), so
 *      g = 0.0f - (wavreg1 + wavreg2). The rescaled sample s becomes s - g[i]; elsewhere it is left alone. Frame n's block goes
 *      with frame n's subband samples (the overlap of spectra n-1 and n): the encoder writes the previous call's block.
 *      Numerics: amp = (double)amp_sf_tab[amp_sf] (amplitude mode 1); every out += sine_table[pos] * amp is a double multiply
 *      and a double add rounded to float, wave by wave in order; pos = (64 phase + i inc) & 2047 at offset 128 and
 *      (64 phase + (i - 128) inc) & 2047 at offset 0; the envelopes' Hann multiplies and the overlap are float; no FMA. The
 *      tables (sine_table[2048], hann_window[256], amp_sf_tab[64]) are ff_atrac3p_init_dsp_static's, built with the host's libm
 *      (at3phip_decoder_host_tone_tables).
 *   Stream state gains the last three frames' tonal records; calls without the flag leave records without waves, and step 4b
 *   runs only in calls with the flag. */
/* SPARSE WORD LENGTHS (AT3PHIP_DECODE_SPARSE in `flags` of at3phip_decode, alone or with the other decoder flags; without it rule 7
 * stands as written and the rejection counters are what they were). Frames written with AT3PHIP_ALLOC_SPARSE:
 *   1. Step 1's "a word length of 0 rejects the frame" no longer holds. After the word lengths: a frame whose highest unit
 *      (nqu - 1) has word length 0 in every channel is unsupported_syntax. The code-table index is read only for units with a
 *      non-zero word length; for a channel-1 unit with 0 whose channel-0 unit is non-zero, one bit is read in its place, which must
 *      be 1 (0, "copy channel 0's spectrum", is an element the writer does not emit: unsupported_syntax); any other unit with 0
 *      has nothing in the section. Spectra are read only for non-zero units.
 *   2. A unit with word length 0 dequantises to +0.0f in every line.
 *   Frames without a word length of 0 decode exactly as without the flag. Still ABI 1.6: a library that has the symbol
 *   at3phip_host_allocate_sparse takes this flag as it takes AT3PHIP_ALLOC_SPARSE. */
typedef struct at3phip_decoder at3phip_decoder;

typedef struct at3phip_decoder_config {
    int32_t channels;     /* 1 or 2: must match the frames' block type */
    int32_t n_streams;    /* independent streams decoded side by side */
    int32_t max_frames;   /* upper bound of frames per stream per at3phip_decode call */
    int32_t device_id;
} at3phip_decoder_config;

/* The context's stream is non-blocking; see DEVICE BUFFERS AND STREAMS (at3hip.h) and at3phip_decoder_set_stream. */
int at3phip_decoder_create(const at3phip_decoder_config* cfg, at3phip_decoder** out);
void at3phip_decoder_destroy(at3phip_decoder* dec);
const char* at3phip_decoder_last_error(const at3phip_decoder* dec);

#define AT3PHIP_DECODE_S16 8u   /* the bit of AT3HIP_DECODE_S16 */
#define AT3PHIP_DECODE_TONES 16u   /* decode tonal blocks: rule 7 no longer rejects them (TONAL BLOCKS below) */
#define AT3PHIP_DECODE_SPARSE 32u  /* decode word length 0 inside the coded range (SPARSE WORD LENGTHS, decoder); alone or with the others */

/*   frames [n_streams][n_frames][frame_bytes] bytes (2048 by default)
 *   pcm    [n_streams][n_frames][2048][channels]: float32, or int16 with AT3PHIP_DECODE_S16
 * flags: AT3HIP_PCM_ON_DEVICE (frames are device memory), AT3HIP_OUT_ON_DEVICE, AT3HIP_ASYNC (only queue the call: buffers stay
 * valid until at3phip_decoder_sync), AT3PHIP_DECODE_S16. Stream state (the last two frames' IMDCT outputs and window flags)
 * carries across calls: any split of a stream into calls gives the same output as one call. */
int at3phip_decode(at3phip_decoder* dec, const uint8_t* frames, int32_t n_frames, void* pcm, uint32_t flags);

/* The decoder's frame size, with the rules of at3phip_set_frame_bytes: admissible sizes for the channel count, waits for queued
 * work, allocates nothing, leaves stream state and counters alone, AT3HIP_EINVAL and no change otherwise. After it `frames` of
 * at3phip_decode is [n_streams][n_frames][frame_bytes] (any alignment: the unpack kernel loads bytes). */
int at3phip_decoder_set_frame_bytes(at3phip_decoder* dec, int32_t frame_bytes);
int at3phip_decoder_get_frame_bytes(const at3phip_decoder* dec, int32_t* frame_bytes);

/* Waits for everything queued on the decoder. */
int at3phip_decoder_sync(at3phip_decoder* dec);

/* Back to start-of-stream state for every stream; zeroes the counters. */
int at3phip_decoder_reset(at3phip_decoder* dec);

/* Rejected frames per reason (rule 7), summed over streams since create / reset / the last call with reset = 1. Waits for
 * queued work. */
typedef struct at3phip_decoder_counters {
    uint64_t bad_header;
    uint64_t unsupported_syntax;
    uint64_t tonal_present;
    uint64_t bad_code;
    uint64_t read_past_end;
    uint64_t no_terminator;
} at3phip_decoder_counters;
int at3phip_decoder_get_counters(at3phip_decoder* dec, at3phip_decoder_counters* out, int32_t reset);

/* Queue this decoder's work on a caller-provided hipStream_t (NULL = the decoder's own stream), as at3hip_decoder_set_stream. */
int at3phip_decoder_set_stream(at3phip_decoder* dec, void* hip_stream);

/* The decoder's constant tables as at3phip_decoder_create builds them, on the host (no GPU needed); the block starts with the
 * DCT-IV cosines double[16][16] ([k][n]), so that their bits can be pinned on each machine. bytes = AT3PHIP_DECODER_TABLES_BYTES.
 * The decoder is part of ABI 1.6 (see at3hip.h): a host that needs it looks for the symbol at3phip_decoder_create. */
#define AT3PHIP_DECODER_TABLES_BYTES 67328
int at3phip_decoder_host_tables(void* dst, size_t bytes);

/* The tone synthesis' tables as at3phip_decoder_create builds them, on the host (no GPU needed): float sine_table[2048],
 * float hann_window[256], float amp_sf_tab[64], then the 16 uint16 codes of NumToneBands - 1 (code | length << 12).
 * bytes = AT3PHIP_DECODER_TONE_TABLES_BYTES. Still ABI 1.6: a host that needs AT3PHIP_DECODE_TONES looks for this symbol. */
#define AT3PHIP_DECODER_TONE_TABLES_BYTES 9504
int at3phip_decoder_host_tone_tables(void* dst, size_t bytes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
