// Host-side C++ mirror of the reference's surface for the ATRAC3 encode hot path, over the C ABI
// (include/at3hip.h). Same names, argument meaning and error behaviour as the reference classes:
//
//   TAtrac3MDCT      atrac3denc.h:56-92   (Mdct with in-place band mutation, both overloads; CalcGainEnergyScale)
//   TAtrac3Encoder   atrac3denc.h:94-134  (IProcessor::GetLambda() -> functor called once per 1024-sample
//                                          block; ICompressedOutput::WriteFrame once per encoded frame)
//
// The reference encoder is one stream, one frame per lambda call. The GPU path wants thousands of frames
// per launch, so TAtrac3Encoder here buffers `BatchBlocks` lambda calls, returns PROCESSED immediately
// (LOOK_AHEAD for the very first call, as the reference does) and flushes WriteFrame calls in order when
// the batch is full or on Flush()/destruction: observable behaviour equals the reference except latency.
// TAtrac3EncoderBatch is the natural multi-stream form (n independent streams side by side on one GPU) and
// TAtrac3EncoderNode the multi-GPU form: streams are independent, so a node shards them contiguously over its
// devices - one TAtrac3EncoderBatch and one host thread per device, no exchange between devices, no RCCL.
//
// Header-only; link with -lat3hip. Exceptions: std::runtime_error on any at3hip error (the reference
// throws from its sinks and aborts on impossible states; it never returns error codes).
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>
#if defined(__linux__)
#include <sched.h>
#include <cstdio>
#endif

#include "../../include/at1hip.h"
#include "../../include/at3hip.h"
#include "../../include/at3hip_loudness.h"
#include "../../include/at3hip_resample.h"
#include "../../include/at3phip.h"

namespace NAtracDEncHip {

// ---- the two reference interfaces on either side of the hot path (pcmengin.h:111-199, compressed_io.h:56-59)
struct ProcessMeta {
    const uint16_t Channels;
};
enum class EProcessResult { LOOK_AHEAD, PROCESSED };
using TProcessLambda = std::function<EProcessResult(float* data, const ProcessMeta& meta)>;

class ICompressedOutput {
public:
    virtual ~ICompressedOutput() = default;
    virtual void WriteFrame(std::vector<char> data) = 0;
    virtual std::string GetName() const = 0;
    virtual size_t GetChannelNum() const = 0;
};
using TCompressedOutputPtr = std::unique_ptr<ICompressedOutput>;

// NAtrac3::TAtrac3EncoderSettings (atrac/at3/atrac3.h:260-277)
struct TAtrac3EncoderSettings {
    uint32_t Bitrate = 0;            // bit/s; 0 = LP2 132300 (atrac3.cpp:47-53)
    bool NoGainControll = false;
    bool NoTonalComponents = false;
    uint8_t SourceChannels = 2;
    uint32_t BfuIdxConst = 0;
};

struct TGainPoint {                  // TAtrac3Data::SubbandInfo::TGainPoint (atrac3.h:224-227)
    uint32_t Level;
    uint32_t Location;
};

// The library this header runs against must implement at least the ABI minor number the header was written for (at3hip.h lists
// what each one added: three calls in flight need the four-deep wait ring of 1.2, Counters() needs 1.3). Called by every class
// below before its first at3hip_create.
inline void CheckLibraryVersion()
{
    const uint32_t have = at3hip_version();
    if ((have >> 16) != (uint32_t)AT3HIP_VERSION_MAJOR || have < (uint32_t)AT3HIP_VERSION)
        throw std::runtime_error("libat3hip.so implements at3hip ABI " + std::to_string(have >> 16) + "." + std::to_string(have & 0xffffu) +
                                 ", this host layer needs " + std::to_string(AT3HIP_VERSION_MAJOR) + "." + std::to_string(AT3HIP_VERSION_MINOR));
}

inline void Check(int rc, at3hip_ctx* ctx, const char* what)
{
    if (rc != AT3HIP_OK)
        throw std::runtime_error(std::string(what) + ": " + (ctx ? at3hip_last_error(ctx) : "at3hip error " + std::to_string(rc)));
}

// ---- TAtrac3MDCT (atrac3denc.h:56-92) ------------------------------------------------------------------
class TAtrac3MDCT {
public:
    using TGainCurves = std::array<std::vector<TGainPoint>, 4>;  // what MakeGainModulatorArray receives

    explicit TAtrac3MDCT(int deviceId = 0)
    {
        at3hip_config cfg{};
        cfg.channels = 2;
        cfg.n_streams = 1;
        cfg.max_blocks = 2;
        cfg.device_id = deviceId;
        cfg.no_gain_control = 1;
        CheckLibraryVersion();
        Check(at3hip_create(&cfg, &Ctx), nullptr, "at3hip_create");
    }
    ~TAtrac3MDCT() { at3hip_destroy(Ctx); }
    TAtrac3MDCT(const TAtrac3MDCT&) = delete;
    TAtrac3MDCT& operator=(const TAtrac3MDCT&) = delete;

    // Same contract as the reference: bands[b] -> 512 floats [overlap | new], mutated in place.
    void Mdct(float specs[1024], float* bands[4], const TGainCurves& curves = TGainCurves())
    {
        float packed[4 * 512];
        int32_t n[4], level[32] = {0}, loc[32] = {0};
        bool any = false;
        for (int b = 0; b < 4; ++b) {
            memcpy(packed + 512 * b, bands[b], 512 * sizeof(float));
            n[b] = (int32_t)curves[b].size();
            any = any || n[b] > 0;
            for (int i = 0; i < n[b] && i < 8; ++i) {
                level[8 * b + i] = (int32_t)curves[b][i].Level;
                loc[8 * b + i] = (int32_t)curves[b][i].Location;
            }
        }
        Check(at3hip_mdct(Ctx, packed, specs, any ? n : nullptr, any ? level : nullptr, any ? loc : nullptr, 1, 0), Ctx,
              "at3hip_mdct");
        for (int b = 0; b < 4; ++b) memcpy(bands[b], packed + 512 * b, 512 * sizeof(float));
    }

    // The maxLevels overload (atrac3denc.h:80-83): additionally max |new half| per band after gain modulation.
    void Mdct(float specs[1024], float* bands[4], float maxLevels[4], const TGainCurves& curves = TGainCurves())
    {
        float packed[4 * 512];
        int32_t n[4], level[32] = {0}, loc[32] = {0};
        bool any = false;
        for (int b = 0; b < 4; ++b) {
            memcpy(packed + 512 * b, bands[b], 512 * sizeof(float));
            n[b] = (int32_t)curves[b].size();
            any = any || n[b] > 0;
            for (int i = 0; i < n[b] && i < 8; ++i) {
                level[8 * b + i] = (int32_t)curves[b][i].Level;
                loc[8 * b + i] = (int32_t)curves[b][i].Location;
            }
        }
        Check(at3hip_mdct_levels(Ctx, packed, specs, maxLevels, any ? n : nullptr, any ? level : nullptr, any ? loc : nullptr, 1, 0),
              Ctx, "at3hip_mdct_levels");
        for (int b = 0; b < 4; ++b) memcpy(bands[b], packed + 512 * b, 512 * sizeof(float));
    }

    // TAtrac3MDCT::CalcGainEnergyScale (atrac3denc.h:69-79; static in the reference, a member here because the work
    // runs on this object's device context).
    struct TGainEnergyScale {
        float PrevHalf = 1.0f, CurHalf = 1.0f, Frame = 1.0f;
    };
    struct TGainEnergyAnalysis {
        TGainEnergyScale Scale;
        float NextOverlapScale = 1.0f;
    };
    TGainEnergyAnalysis CalcGainEnergyScale(const float prevOverlap[256], const float curInput[256],
                                            const std::vector<TGainPoint>& gainPoints, float prevOverlapScale)
    {
        int32_t n = (int32_t)gainPoints.size(), level[8] = {0}, loc[8] = {0};
        for (int i = 0; i < n && i < 8; ++i) {
            level[i] = (int32_t)gainPoints[i].Level;
            loc[i] = (int32_t)gainPoints[i].Location;
        }
        float out[4];
        Check(at3hip_gain_energy_scale(Ctx, prevOverlap, curInput, n ? &n : nullptr, n ? level : nullptr, n ? loc : nullptr,
                                       &prevOverlapScale, out, 1, 0), Ctx, "at3hip_gain_energy_scale");
        TGainEnergyAnalysis res;
        res.Scale.PrevHalf = out[0];
        res.Scale.CurHalf = out[1];
        res.Scale.Frame = out[2];
        res.NextOverlapScale = out[3];
        return res;
    }

private:
    at3hip_ctx* Ctx = nullptr;
};

// ---- n streams side by side: the batch form of TAtrac3Encoder --------------------------------------------
class TAtrac3EncoderBatch {
public:
    TAtrac3EncoderBatch(const TAtrac3EncoderSettings& s, int nStreams, int maxBlocks, int deviceId = 0)
        : NStreams(nStreams)
    {
        at3hip_config cfg{};
        cfg.bitrate = (int32_t)s.Bitrate;
        cfg.channels = s.SourceChannels;
        cfg.no_gain_control = s.NoGainControll;
        cfg.no_tonal = s.NoTonalComponents;
        cfg.bfu_idx_const = (int32_t)s.BfuIdxConst;
        cfg.n_streams = nStreams;
        cfg.max_blocks = maxBlocks;
        cfg.device_id = deviceId;
        CheckLibraryVersion();
        Check(at3hip_create(&cfg, &Ctx), nullptr, "at3hip_create");
        FrameSz = at3hip_frame_size(Ctx);
        // nothing in this layer reads the stage timings: their HIP events between the kernels cost a pipelined step ~3 % (AT3HIP_OPT_TIMING_EVERY)
        Check(at3hip_set_option(Ctx, AT3HIP_OPT_TIMING_EVERY, 0), Ctx, "at3hip_set_option");
    }
    // Stage timings (at3hip_get_timings / _ago on Handle()) on every Nth call with frames; 0 (this layer's default) = never.
    void SetTimingEvery(int n) { Check(at3hip_set_option(Ctx, AT3HIP_OPT_TIMING_EVERY, n), Ctx, "at3hip_set_option"); }
    ~TAtrac3EncoderBatch() { at3hip_destroy(Ctx); }
    TAtrac3EncoderBatch(const TAtrac3EncoderBatch&) = delete;
    TAtrac3EncoderBatch& operator=(const TAtrac3EncoderBatch&) = delete;

    int FrameSize() const { return FrameSz; }
    // pcm [nStreams][nBlocks][1024][SourceChannels] -> frames [nStreams][nFrames][FrameSize()]; returns nFrames per stream.
    int Encode(const float* pcm, int nBlocks, std::vector<uint8_t>& frames)
    {
        frames.resize((size_t)NStreams * nBlocks * FrameSz);
        int32_t nf = 0;
        Check(at3hip_encode(Ctx, pcm, nBlocks, frames.data(), &nf, 0), Ctx, "at3hip_encode");
        frames.resize((size_t)NStreams * nf * FrameSz);
        return nf;
    }
    // the same with 16-bit samples (converted s / 32768.0f on the device: a 16-bit WAV as sf_readf_float reads it)
    int EncodeS16(const int16_t* pcm, int nBlocks, std::vector<uint8_t>& frames)
    {
        frames.resize((size_t)NStreams * nBlocks * FrameSz);
        int32_t nf = 0;
        Check(at3hip_encode_s16(Ctx, pcm, nBlocks, frames.data(), &nf, 0), Ctx, "at3hip_encode_s16");
        frames.resize((size_t)NStreams * nf * FrameSz);
        return nf;
    }
    void Reset() { Check(at3hip_reset(Ctx), Ctx, "at3hip_reset"); }
    at3hip_ctx* Handle() { return Ctx; }
    // What the reference's TScaler::Scale would have written to stderr for these streams since construction / Reset()
    // ("Scale error: absSpec > MAX_SCALE" per block, "clipping, scaled value" per value; atrac_scale.cpp:150-153, 163-167)
    at3hip_counters Counters(bool reset = false)
    {
        at3hip_counters c{};
        Check(at3hip_get_counters(Ctx, &c, reset ? 1 : 0), Ctx, "at3hip_get_counters");
        return c;
    }

    // A long input fed call by call with the copies hidden: two page-locked PCM buffers and two frame buffers alternate, the
    // calls are asynchronous, so while the GPU encodes call k the host thread fills call k + 1's buffer (`fill`), the copy
    // engine moves it, and call k - 1's frames come back and are handed to `drain` - what TPCMEngine::ApplyProcess
    // (pcmengin.h:152-192) and ICompressedOutput::WriteFrame do around the reference's lambda, batched.
    //   fill(TSample* dst, int maxBlocks) -> blocks written, [nStreams][blocks][1024][channels]; 0 ends the input
    //   drain(const uint8_t* frames, int nFrames): [nStreams][nFrames][FrameSize()], in call order
    // TSample = float, or int16_t (EncodePipelinedS16): 16-bit samples cross the bus at half the bytes - the host-fed rate is
    // bound by exactly those - and become floats on the device.
    // Returns the number of frames per stream.
    template <class TFill, class TDrain>
    long long EncodePipelined(int blocksPerCall, int channels, TFill fill, TDrain drain)
    {
        return EncodePipelinedT<float>(blocksPerCall, channels, fill, drain);
    }
    template <class TFill, class TDrain>
    long long EncodePipelinedS16(int blocksPerCall, int channels, TFill fill, TDrain drain)
    {
        return EncodePipelinedT<int16_t>(blocksPerCall, channels, fill, drain);
    }

private:
    static int EncodeAny(at3hip_ctx* c, const float* pcm, int32_t nb, uint8_t* out, int32_t* nf, uint32_t flags) { return at3hip_encode(c, pcm, nb, out, nf, flags); }
    static int EncodeAny(at3hip_ctx* c, const int16_t* pcm, int32_t nb, uint8_t* out, int32_t* nf, uint32_t flags) { return at3hip_encode_s16(c, pcm, nb, out, nf, flags); }
    template <class TSample, class TFill, class TDrain>
    long long EncodePipelinedT(int blocksPerCall, int channels, TFill fill, TDrain drain)
    {
        struct TPinned {
            at3hip_ctx* Ctx;
            void* P = nullptr;
            TPinned(at3hip_ctx* c, size_t bytes) : Ctx(c) { Check(at3hip_host_alloc(c, bytes, &P), c, "at3hip_host_alloc"); }
            ~TPinned() { at3hip_host_free(Ctx, P); }
        };
        const size_t inFloats = (size_t)NStreams * blocksPerCall * 1024 * channels, outBytes = (size_t)NStreams * blocksPerCall * FrameSz;
        // kDepth calls in flight (at3hip_wait_* reach three calls back, so at most four). Measured on configs[1] (64 x 64 frames per
        // call, profiles/EXPERIMENTS.md round 5): 16-bit samples - the copy of a call is as short as its kernels, and the device
        // overlaps three stages of consecutive calls - 9.6 / 11.5 / 12.4 M frames/s at two / three / four calls in flight (92 % of
        // the bus with four); float samples are bound by the bus at any depth (6.6 / 6.5 / 6.5 M = 95 % of it), so they keep two
        // calls and 64 MB less page-locked memory.
        constexpr int kDepth = sizeof(TSample) == 2 ? 4 : 2;
        std::unique_ptr<TPinned> inBuf[kDepth], outBuf[kDepth];
        TSample* in[kDepth];
        uint8_t* out[kDepth];
        for (int q = 0; q < kDepth; ++q) {
            inBuf[q].reset(new TPinned(Ctx, inFloats * sizeof(TSample)));
            outBuf[q].reset(new TPinned(Ctx, outBytes));
            in[q] = (TSample*)inBuf[q]->P;
            out[q] = (uint8_t*)outBuf[q]->P;
        }
        int32_t nf[kDepth] = {};
        long long total = 0;
        int call = 0, drained = 0;   // calls queued / calls whose frames were handed over
        auto drain_next = [&] {
            const int q = drained % kDepth;
            if (nf[q] > 0) drain(out[q], (int)nf[q]);
            total += nf[q];
            ++drained;
        };
        try {
        for (;; ++call) {
            const int q = call % kDepth;
            if (call >= kDepth) Check(at3hip_wait_input(Ctx, kDepth - 1), Ctx, "at3hip_wait_input");   // call - kDepth read in[q]: gone to the device by now?
            const int nb = fill(in[q], blocksPerCall);
            if (nb <= 0) break;
            // (out[q] is free: the frames of call - kDepth were drained below, after call - 1 was queued)
            Check(EncodeAny(Ctx, in[q], nb, out[q], &nf[q], AT3HIP_ASYNC), Ctx, "at3hip_encode");
            if (call >= kDepth - 1) {   // while the newer calls run: the oldest call's frames
                Check(at3hip_wait_frames(Ctx, kDepth - 1), Ctx, "at3hip_wait_frames");
                drain_next();
            }
        }
        if (call >= 1) {
            Check(at3hip_sync(Ctx), Ctx, "at3hip_sync");
            while (drained < call) drain_next();
        }
        } catch (...) {
            at3hip_sync(Ctx);   // the page-locked buffers are released on the way out: no copy may still be in flight
            throw;
        }
        return total;
    }

    at3hip_ctx* Ctx = nullptr;
    int NStreams;
    int FrameSz = 0;
};

// ---- all GPUs of a node: the stream-sharded form --------------------------------------------------------------
// Contiguous, balanced partition of `total` streams over `parts` devices: (first, count) of part `idx`.
inline std::pair<int, int> ShardStreams(int total, int parts, int idx)
{
    if (parts < 1 || idx < 0 || idx >= parts) throw std::runtime_error("ShardStreams: bad partition");
    const int base = total / parts, rem = total % parts;
    return {idx * base + (idx < rem ? idx : rem), base + (idx < rem ? 1 : 0)};
}

// Pin the calling thread to the host NUMA node of a device (at3hip_device_numa_node; the node's CPUs from
// /sys/devices/system/node/node<N>/cpulist). Memory the thread touches first afterwards - the page-locked staging buffers of
// TAtrac3EncoderBatch::EncodePipelined among it - then lies on that node. Returns the node, or -1 when nothing was changed (unknown
// node, no sysfs, not Linux): a missing pin costs bandwidth on a multi-socket host, never correctness.
inline int PinThreadToDeviceNode(int deviceId)
{
#if defined(__linux__)
    const int node = at3hip_device_numa_node(deviceId);
    if (node < 0) return -1;
    char path[96];
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    FILE* f = fopen(path, "r");
    if (!f) return -1;
    cpu_set_t set;
    CPU_ZERO(&set);
    int n = 0, a = 0, b = 0;
    for (;;) {   // "0-15,128-143"
        if (fscanf(f, "%d", &a) != 1) break;
        b = a;
        int c = fgetc(f);
        if (c == '-') {
            if (fscanf(f, "%d", &b) != 1) break;
            c = fgetc(f);
        }
        for (int cpu = a; cpu <= b && cpu < CPU_SETSIZE; ++cpu) {
            CPU_SET(cpu, &set);
            ++n;
        }
        if (c != ',') break;
    }
    fclose(f);
    if (n == 0 || sched_setaffinity(0, sizeof(set), &set) != 0) return -1;
    return node;
#else
    (void)deviceId;
    return -1;
#endif
}

class TAtrac3EncoderNode {
public:
    // deviceIds: the HIP ordinals to use (e.g. {0,1,...,7}); streams [first, first + count) of ShardStreams go to deviceIds[i]
    TAtrac3EncoderNode(const TAtrac3EncoderSettings& s, int nStreams, int maxBlocks, const std::vector<int>& deviceIds)
        : NStreams(nStreams), Channels(s.SourceChannels)
    {
        if (deviceIds.empty() || nStreams < (int)deviceIds.size()) throw std::runtime_error("TAtrac3EncoderNode: need >= 1 stream per device");
        for (size_t i = 0; i < deviceIds.size(); ++i) {
            const auto part = ShardStreams(nStreams, (int)deviceIds.size(), (int)i);
            First.push_back(part.first);
            Count.push_back(part.second);
            Parts.emplace_back(new TAtrac3EncoderBatch(s, part.second, maxBlocks, deviceIds[i]));
            DeviceIds.push_back(deviceIds[i]);
        }
        FrameSz = Parts[0]->FrameSize();
    }
    int FrameSize() const { return FrameSz; }
    int Devices() const { return (int)Parts.size(); }
    // pcm [nStreams][nBlocks][1024][SourceChannels] -> frames [nStreams][nFrames][FrameSize()]; returns nFrames per stream.
    // Every device encodes its slice on its own host thread; the slices are disjoint in both buffers.
    int Encode(const float* pcm, int nBlocks, std::vector<uint8_t>& frames)
    {
        const size_t blockFloats = (size_t)1024 * Channels;
        std::vector<std::vector<uint8_t>> out(Parts.size());
        std::vector<int> nf(Parts.size(), 0);
        std::vector<std::string> err(Parts.size());
        std::vector<std::thread> th;
        for (size_t i = 0; i < Parts.size(); ++i)
            th.emplace_back([&, i] {
                try {
                    PinThreadToDeviceNode(DeviceIds[i]);   // (the device's feeder thread and what it allocates: on the device's NUMA node)
                    nf[i] = Parts[i]->Encode(pcm + (size_t)First[i] * nBlocks * blockFloats, nBlocks, out[i]);
                } catch (const std::exception& e) {
                    err[i] = e.what();
                }
            });
        for (auto& t : th) t.join();
        for (size_t i = 0; i < Parts.size(); ++i)
            if (!err[i].empty()) throw std::runtime_error("TAtrac3EncoderNode device " + std::to_string(i) + ": " + err[i]);
        frames.resize((size_t)NStreams * nf[0] * FrameSz);
        for (size_t i = 0; i < Parts.size(); ++i)
            memcpy(frames.data() + (size_t)First[i] * nf[0] * FrameSz, out[i].data(), out[i].size());
        return nf[0];
    }
    void Reset()
    {
        for (auto& p : Parts) p->Reset();
    }

    // The same for a long input: pcm [nStreams][nBlocksTotal][1024][SourceChannels] is cut into calls of `blocksPerCall`
    // blocks; every device's host thread runs TAtrac3EncoderBatch::EncodePipelined on its slice (page-locked staging, copies
    // and kernels of consecutive calls overlapping). frames [nStreams][nFrames][FrameSize()]; returns nFrames per stream.
    // STARTS A NEW STREAM: the node is Reset() first - unlike TAtrac3EncoderBatch::EncodePipelined, which continues whatever its
    // context has been fed - because `frames` is laid out for exactly nBlocksTotal - 1 frames per stream, which only holds from
    // start of stream. Blocks fed through Encode() before this call are therefore NOT continued; callers that feed one stream in
    // pieces use Encode() throughout, or TAtrac3EncoderBatch::EncodePipelined on a part. `frames` is resized before any frame
    // arrives, so when a device's thread throws (e.g. the frame-count guard below) its content is unspecified.
    int EncodePipelined(const float* pcm, int nBlocksTotal, int blocksPerCall, std::vector<uint8_t>& frames)
    {
        const size_t blockFloats = (size_t)1024 * Channels;
        // start of stream: the first block is the look-ahead (atrac3denc.cpp:715-718), so nBlocksTotal blocks give
        // nBlocksTotal - 1 frames per stream - the node is reset here so that this holds whatever was encoded before
        Reset();
        const int nfTotal = nBlocksTotal - 1;
        frames.assign((size_t)NStreams * (nfTotal > 0 ? nfTotal : 0) * FrameSz, 0);
        std::vector<std::string> err(Parts.size());
        std::vector<long long> got(Parts.size(), 0);
        std::vector<std::thread> th;
        for (size_t i = 0; i < Parts.size(); ++i)
            th.emplace_back([&, i] {
                try {
                    PinThreadToDeviceNode(DeviceIds[i]);   // before EncodePipelined allocates its page-locked staging: first touch on the device's node
                    int fed = 0, written = 0;
                    got[i] = Parts[i]->EncodePipelined(
                        blocksPerCall, Channels,
                        [&](float* dst, int maxBlocks) {
                            const int nb = std::min(maxBlocks, nBlocksTotal - fed);
                            for (int s = 0; s < Count[i] && nb > 0; ++s)
                                memcpy(dst + (size_t)s * nb * blockFloats, pcm + ((size_t)(First[i] + s) * nBlocksTotal + fed) * blockFloats,
                                       (size_t)nb * blockFloats * sizeof(float));
                            fed += nb > 0 ? nb : 0;
                            return nb;
                        },
                        [&](const uint8_t* fr, int nf) {
                            if (written + nf > nfTotal) throw std::runtime_error("EncodePipelined: more frames than the output holds");
                            for (int s = 0; s < Count[i]; ++s)
                                memcpy(frames.data() + ((size_t)(First[i] + s) * nfTotal + written) * FrameSz, fr + (size_t)s * nf * FrameSz,
                                       (size_t)nf * FrameSz);
                            written += nf;
                        });
                } catch (const std::exception& e) {
                    err[i] = e.what();
                }
            });
        for (auto& t : th) t.join();
        for (size_t i = 0; i < Parts.size(); ++i)
            if (!err[i].empty()) throw std::runtime_error("TAtrac3EncoderNode device " + std::to_string(i) + ": " + err[i]);
        return (int)got[0];
    }

private:
    std::vector<std::unique_ptr<TAtrac3EncoderBatch>> Parts;
    std::vector<int> First, Count, DeviceIds;
    int NStreams;
    int Channels;
    int FrameSz = 0;
};

// ---- TAtrac3Encoder (atrac3denc.h:94-134): lambda in, WriteFrame out -------------------------------------
class TAtrac3Encoder {
public:
    TAtrac3Encoder(TCompressedOutputPtr&& oma, TAtrac3EncoderSettings&& settings, int batchBlocks = 64, int deviceId = 0)
        : Oma(std::move(oma)), Params(settings), BatchBlocks(batchBlocks), Batch(settings, 1, batchBlocks, deviceId),
          BlockFloats(1024u * settings.SourceChannels)
    {
        // one input channel is accepted for the discrete-stereo bitrates (the frame holds the unit twice,
        // atrac3_bitstream.cpp:836-843); at3hip_create refuses the other combinations
        Pending.reserve((size_t)BatchBlocks * BlockFloats);
    }
    ~TAtrac3Encoder()
    {
        try {
            Flush();
        } catch (...) {
        }
    }

    TProcessLambda GetLambda()
    {
        return [this](float* data, const ProcessMeta& meta) {
            if (meta.Channels != Params.SourceChannels) throw std::runtime_error("TAtrac3Encoder(hip): channel count changed");
            Pending.insert(Pending.end(), data, data + BlockFloats);
            const bool first = (Calls++ == 0);
            if ((int)(Pending.size() / BlockFloats) == BatchBlocks) Flush();
            return first ? EProcessResult::LOOK_AHEAD : EProcessResult::PROCESSED;   // atrac3denc.cpp:715-718, 865
        };
    }

    // Encode what is buffered and hand the frames to the sink in order.
    void Flush()
    {
        const int nb = (int)(Pending.size() / BlockFloats);
        if (nb == 0) return;
        std::vector<uint8_t> frames;
        const int nf = Batch.Encode(Pending.data(), nb, frames);
        Pending.clear();
        const int fsz = Batch.FrameSize();
        for (int i = 0; i < nf; ++i)
            Oma->WriteFrame(std::vector<char>(frames.begin() + (size_t)i * fsz, frames.begin() + (size_t)(i + 1) * fsz));
    }
    // TScaler::Scale's overflow diagnostics for what has been encoded so far (TAtrac3EncoderBatch::Counters)
    at3hip_counters Counters() { return Batch.Counters(); }

private:
    TCompressedOutputPtr Oma;
    const TAtrac3EncoderSettings Params;
    const int BatchBlocks;
    TAtrac3EncoderBatch Batch;
    const size_t BlockFloats;
    std::vector<float> Pending;
    uint64_t Calls = 0;
};

// ---- ATRAC1 -----------------------------------------------------------------------
// NAtrac1::TAtrac1EncodeSettings (atrac/at1/atrac1.h:33-54)
struct TAtrac1EncodeSettings {
    enum class EWindowMode { EWM_NOTRANSIENT, EWM_AUTO };
    uint32_t BfuIdxConst = 0;
    EWindowMode WindowMode = EWindowMode::EWM_AUTO;
    uint32_t WindowMask = 0;
    TAtrac1EncodeSettings() = default;
    TAtrac1EncodeSettings(uint32_t bfuIdxConst, EWindowMode windowMode, uint32_t windowMask)
        : BfuIdxConst(bfuIdxConst), WindowMode(windowMode), WindowMask(windowMask)
    {
    }
};

inline void Check1(int rc, at1hip_ctx* ctx, const char* what)
{
    if (rc != AT3HIP_OK) throw std::runtime_error(std::string(what) + ": " + (ctx ? at1hip_last_error(ctx) : "error " + std::to_string(rc)));
}

// TAtrac1Encoder (atrac1denc.h:56-110): lambda in - one call per 512-sample block - and one WriteFrame per channel
// and block out, channel 0 first (atrac1denc.cpp:249-251). The channel count comes from the sink, as in the reference.
// Calls are buffered `batchBlocks` at a time like TAtrac3Encoder above; there is no look-ahead call in this codec.
class TAtrac1Encoder {
public:
    TAtrac1Encoder(TCompressedOutputPtr&& aea, TAtrac1EncodeSettings&& settings, int batchBlocks = 512, int deviceId = 0)
        : Aea(std::move(aea)), Settings(settings), BatchBlocks(batchBlocks), Channels(Aea->GetChannelNum()), BlockFloats(512u * Channels)
    {
        at1hip_config cfg{};
        cfg.channels = (int32_t)Channels;
        cfg.window_auto = Settings.WindowMode == TAtrac1EncodeSettings::EWindowMode::EWM_AUTO;
        cfg.window_mask = (int32_t)Settings.WindowMask;
        cfg.bfu_idx_const = (int32_t)Settings.BfuIdxConst;
        cfg.n_streams = 1;
        cfg.max_blocks = batchBlocks;
        cfg.device_id = deviceId;
        Check1(at1hip_create(&cfg, &Ctx), nullptr, "at1hip_create");
        Pending.reserve((size_t)BatchBlocks * BlockFloats);
    }
    ~TAtrac1Encoder()
    {
        try {
            Flush();
        } catch (...) {
        }
        at1hip_destroy(Ctx);
    }
    TAtrac1Encoder(const TAtrac1Encoder&) = delete;
    TAtrac1Encoder& operator=(const TAtrac1Encoder&) = delete;

    TProcessLambda GetLambda()
    {
        return [this](float* data, const ProcessMeta&) {
            Pending.insert(Pending.end(), data, data + BlockFloats);
            if ((int)(Pending.size() / BlockFloats) == BatchBlocks) Flush();
            return EProcessResult::PROCESSED;
        };
    }

    void Flush()
    {
        const int nb = (int)(Pending.size() / BlockFloats);
        if (nb == 0) return;
        std::vector<uint8_t> units((size_t)nb * Channels * AT1HIP_FRAME_SIZE);
        Check1(at1hip_encode(Ctx, Pending.data(), nb, units.data(), 0), Ctx, "at1hip_encode");
        Pending.clear();
        for (size_t i = 0; i < (size_t)nb * Channels; ++i)
            Aea->WriteFrame(std::vector<char>(units.begin() + i * AT1HIP_FRAME_SIZE, units.begin() + (i + 1) * AT1HIP_FRAME_SIZE));
    }

    // nBlocks blocks of 16-bit PCM [nBlocks][512][channels] (at1hip_encode_short: a sample s is s / 32768.0f, widened on the
    // device), behind whatever the lambda has buffered: the units are those of the lambda on these floats. At most batchBlocks
    // blocks go into one call.
    void EncodeS16(const int16_t* pcm, int nBlocks)
    {
        Flush();
        std::vector<uint8_t> units((size_t)BatchBlocks * Channels * AT1HIP_FRAME_SIZE);
        for (int at = 0; at < nBlocks; at += BatchBlocks) {
            const int nb = std::min(BatchBlocks, nBlocks - at);
            Check1(at1hip_encode_short(Ctx, pcm + (size_t)at * BlockFloats, nb, units.data(), 0), Ctx, "at1hip_encode_short");
            for (size_t i = 0; i < (size_t)nb * Channels; ++i)
                Aea->WriteFrame(std::vector<char>(units.begin() + i * AT1HIP_FRAME_SIZE, units.begin() + (i + 1) * AT1HIP_FRAME_SIZE));
        }
    }

private:
    TCompressedOutputPtr Aea;
    const TAtrac1EncodeSettings Settings;
    const int BatchBlocks;
    const size_t Channels;
    const size_t BlockFloats;
    at1hip_ctx* Ctx = nullptr;
    std::vector<float> Pending;
};

// ---- ATRAC3plus ---------------------------------------------------------------------------------------------------
// TAt3PEnc (at3p.h, at3p.cpp:37-191) with GHA_PASS_INPUT | GHA_WRITE_RESIUDAL and a tonal analysis that finds nothing
// (the analysis itself needs libgha, which the reference does not vendor): lambda in - one call per 2048-sample frame of
// interleaved PCM - and one 2048-byte WriteFrame out per call after the first. The reference looks one frame ahead and
// encodes the frame BEFORE the current one (PrevBuf, at3p.cpp:115-160), so the first call returns LOOK_AHEAD, the second
// writes a silent frame and call k >= 2 writes input frame k - 2; this class keeps that schedule. Frames are encoded
// `batchFrames` at a time like the encoders above and flushed in order.
//
// With a tonal analyser (IAt3PGhaProcessor, shaped like IGhaProcessor::DoAnalize, at3p_gha.h:69-78) the class runs
// EncodeFrame's whole schedule under TAt3PSettings::UseGha: per batch one at3phip_pqf_analyse, then per call the analyser on the
// host - current and next subband buffers const, the previous ones (PrevBuf, what the transform takes) writable -, one
// at3phip_mdct with AT3PHIP_RESIDUAL_SCALE on the possibly modified previous buffers (zeros without GHA_WRITE_RESIUDAL), one
// at3phip_write_frames_tonal. PrevBuf becomes the current buffer under GHA_PASS_INPUT and zeros otherwise; the block returned
// for call k is written with call k + 1 (`delay`, at3p.cpp:128-176) and only under GHA_WRITE_TONAL. Without an analyser nothing
// changes: same calls, same bytes.
struct TAt3PSettings {   // TAt3PEnc::TSettings::UseGha (atrac3p.h:29-47)
    enum GhaProcessingFlags : uint8_t { GHA_PASS_INPUT = 1, GHA_WRITE_TONAL = 1 << 1, GHA_WRITE_RESIUDAL = 1 << 2,
                                        GHA_ENABLED = GHA_PASS_INPUT | GHA_WRITE_TONAL | GHA_WRITE_RESIUDAL };
    uint8_t UseGha = GHA_ENABLED;
};

class IAt3PGhaProcessor {
public:
    using TBufPtr = std::array<const float*, 2>;   // {current, next}: a channel's subband samples [16][128]
    virtual ~IAt3PGhaProcessor() {}
    // b1 / b2: channel 0 / 1 (nulls in mono); w1 / w2: the channels' previous buffers, which the analyser may rewrite (w2 null in
    // mono); raw1Cur / raw2Cur: the current frame's PCM per channel [2048], before the filter bank. Returns the frame's tonal
    // block, valid until the next call, or null.
    virtual const at3phip_tonal_block* DoAnalize(TBufPtr b1, TBufPtr b2, float* w1, float* w2, const float* raw1Cur,
                                                 const float* raw2Cur) = 0;
};


// The tone analysis of include/at3phip.h (FINDING TONES, steps 1-8) on the CPU, as plain C++ with no GPU: what
// at3phip_encode_frames_tonal computes, behind the mirror's analyser interface. A call receives previous, current and next; the
// block it returns is written with the previous buffer's spectrum one call later, so it analyses the pair (previous as passed in,
// current), ignores next, and subtracts from the previous buffer: this block fading in, the block of the call before fading out.
// Every sum runs in the header's order; compile without floating-point contraction (no FMA), like the kernels.
// The same analysis is written out in atracdenc_amd/csrc/at3p_gha.hpp (the kernels); both are pinned bit for bit to one C
// restatement, tests/host/at3p_gha_cpu.c, and a change to the definition changes all of them.
// gated: the analysis with AT3PHIP_TONES_GATED (the header's GATES, G1-G5): onsets and offsets become the blocks' envelope
// points. G1 itself is the library's at3phip_host_tone_gates, which is compiled without contraction whatever this header's user
// compiles with.
// shared: the analysis with AT3PHIP_TONES_SHARED (the header's SHARING, S1-S5): a band that both channels hold identically is
// counted and written once. Nothing in a mono analyser.
class TAt3PToneAnalyser : public IAt3PGhaProcessor {
public:
    explicit TAt3PToneAnalyser(int channels, bool gated = false, bool shared = false) : Channels(channels), Gated(gated), Shared(shared && channels == 2)
    {
        if (at3phip_host_tone_find_tables(&T, sizeof(T)) != AT3HIP_OK) throw std::runtime_error("at3phip_host_tone_find_tables failed");
    }
    const at3phip_tonal_block* DoAnalize(TBufPtr b1, TBufPtr b2, float* w1, float* w2, const float*, const float*) override
    {
        const float* cur[2] = {b1[0], b2[0]};
        float* prev[2] = {w1, w2};
        TWave w[2 * 16 * AT3PHIP_TONE_MAX_BAND_WAVES];
        int nw = 0;
        uint8_t gatePrev[2][16] = {}, gateCur[2][16] = {};   // G1 for both frames, before anything is subtracted from the previous one
        for (int ch = 0; Gated && ch < Channels; ++ch)
            if (at3phip_host_tone_gates(prev[ch], 1, 1, gatePrev[ch]) != AT3HIP_OK || at3phip_host_tone_gates(cur[ch], 1, 1, gateCur[ch]) != AT3HIP_OK)
                throw std::runtime_error("at3phip_host_tone_gates failed");
        for (int ch = 0; ch < Channels; ++ch)
            for (int sb = 0; sb < 16; ++sb) {
                float x[256];
                std::copy(prev[ch] + sb * 128, prev[ch] + sb * 128 + 128, x);
                std::copy(cur[ch] + sb * 128, cur[ch] + sb * 128 + 128, x + 128);
                const int g0 = gatePrev[ch][sb], g1 = gateCur[ch][sb];
                int lo = 0, hi = 63;
                const bool event = (g0 | g1) != 0;
                if (event) {   // G3
                    const TEnv e = CurrEnv(GateBand(g1), GateBand(g0));
                    lo = e.Hs ? e.S : 0;
                    hi = e.He ? e.E : 63;
                }
                const int got = FindBand(x, w + nw, event, lo, hi);
                for (int i = 0; i < got; ++i) {
                    w[nw + i].Ch = ch;
                    w[nw + i].Sb = sb;
                }
                nw += got;
            }
        const at3phip_tonal_block older = Older, before = Block;
        bool twin[16] = {};
        if (Shared) {   // S2, then S3: channel 1's waves of the twin bands leave the population
            for (int sb = 0; sb < 16; ++sb) twin[sb] = Twin(w, nw, gateCur[0][sb], gateCur[1][sb], sb);
            nw = (int)(std::remove_if(w, w + nw, [&](const TWave& v) { return v.Ch == 1 && twin[v.Sb]; }) - w);
        }
        Select(w, nw);
        for (int ch = 0; ch < Channels; ++ch)   // G2: the second frame's event is the block's point pair, wave or no wave
            for (int sb = 0; sb < 16; ++sb) {
                const int g = gateCur[ch][sb];
                if (!g || (ch == 1 && twin[sb])) continue;   // (S4: a twin band of channel 1 stays all zero)
                if (g < 0x80) Block.band[ch][sb].start = (uint8_t)(g + 1);
                else Block.band[ch][sb].stop = (uint8_t)((g & 31) + 1);
                Block.num_tone_bands = (uint8_t)std::max<int>(Block.num_tone_bands, sb + 1);
            }
        for (int sb = 0; sb < Block.num_tone_bands; ++sb)   // S4
            if (twin[sb]) Block.tone_sharing |= (uint16_t)(1u << sb);
        for (int ch = 0; ch < Channels; ++ch)
            for (int sb = 0; sb < 16; ++sb) Subtract(older, before, Block, ch, sb, prev[ch] + sb * 128);
        Older = before;
        return &Block;
    }

private:
    struct TTables {   // the block of at3phip_host_tone_find_tables
        float Sine[2048], Hann[256], AmpSf[64], Tw[256][2];
        double Thr[64], Rs[1024], Rc[1024];
    };
    static_assert(sizeof(TTables) == AT3PHIP_TONE_FIND_TABLES_BYTES, "the table block's documented size");
    struct TWave {
        int Ch, Sb, Freq, AmpSf, Phase;
        double A2;
        bool Keep;
    };
    struct TCpx {
        float r, i;
    };
    // an envelope as ff_atrac3p_generate_tones keeps it: has_start_point, start_pos, has_stop_point, stop_pos
    struct TEnv {
        int Hs, S, He, E;
    };
    // curr_env of a block's band (nx: its start and stop, the record's "+1" convention) after the block before's (nw), as
    // ff_atrac3p_generate_tones reconstructs it (decp_curr_env in the kernels)
    static TEnv CurrEnv(at3phip_tonal_band nx, at3phip_tonal_band nw)
    {
        const int nxStart = (int)nx.start - 1, nxStop = nx.stop ? (int)nx.stop - 1 : 32;
        TEnv r;
        if (nx.start && nxStart < nxStop) r.Hs = 1, r.S = nxStart + 32;
        else if (nw.start) r.Hs = 1, r.S = (int)nw.start - 1;
        else r.Hs = 0, r.S = 0;
        if (nw.stop && (int)nw.stop - 1 >= r.S) r.He = 1, r.E = (int)nw.stop - 1;
        else if (nx.stop) r.He = 1, r.E = nxStop + 32;
        else r.He = 0, r.E = 64;
        return r;
    }
    static at3phip_tonal_band GateBand(int g)
    {
        at3phip_tonal_band b{};
        if (g > 0 && g < 0x80) b.start = (uint8_t)(g + 1);
        if (g >= 0x80) b.stop = (uint8_t)((g & 31) + 1);
        return b;
    }
    // the kissfft-order forward FFT for n = 4^k (kf_work and kf_bfly4, kiss_fft.c:42-90, 238-302)
    void Fft(TCpx* out, const TCpx* in, int n, int fstride) const
    {
        const int m = n / 4;
        if (m == 1) {
            for (int q = 0; q < 4; ++q) out[q] = in[q * fstride];
        } else {
            for (int q = 0; q < 4; ++q) Fft(out + q * m, in + q * fstride, m, fstride * 4);
        }
        auto mul = [this](TCpx a, int t) {
            TCpx r;
            r.r = a.r * T.Tw[t][0] - a.i * T.Tw[t][1];
            r.i = a.r * T.Tw[t][1] + a.i * T.Tw[t][0];
            return r;
        };
        for (int k = 0; k < m; ++k) {
            const TCpx s0 = mul(out[m + k], k * fstride), s1 = mul(out[2 * m + k], 2 * k * fstride), s2 = mul(out[3 * m + k], 3 * k * fstride);
            TCpx s5, s3, s4;
            s5.r = out[k].r - s1.r; s5.i = out[k].i - s1.i;
            out[k].r += s1.r; out[k].i += s1.i;
            s3.r = s0.r + s2.r; s3.i = s0.i + s2.i;
            s4.r = s0.r - s2.r; s4.i = s0.i - s2.i;
            out[2 * m + k].r = out[k].r - s3.r; out[2 * m + k].i = out[k].i - s3.i;
            out[k].r += s3.r; out[k].i += s3.i;
            out[m + k].r = s5.r + s4.i; out[m + k].i = s5.i - s4.r;
            out[3 * m + k].r = s5.r - s4.i; out[3 * m + k].i = s5.i + s4.r;
        }
    }
    // steps 1-5 for one subband: at most AT3PHIP_TONE_MAX_BAND_WAVES waves. event: G4 over the cells [lo, hi] of G3
    int FindBand(const float* x, TWave* out, bool event, int lo, int hi) const
    {
        constexpr int kMax = AT3PHIP_TONE_MAX_BAND_WAVES, kSpan = AT3PHIP_TONE_FINE_SPAN;
        if (event && hi - lo + 1 < AT3PHIP_TONE_GATE_MIN) return 0;
        const int t0 = 4 * lo, t1 = 4 * hi + 3;
        float y[256], wnd[256], P[129];
        TCpx in[256], F[256];
        for (int t = 0; t < 256; ++t) {
            wnd[t] = event && (t < t0 || t > t1) ? 0.0f : T.Hann[t];
            y[t] = x[t] * wnd[t];
            in[t].r = y[t];
            in[t].i = 0.0f;
        }
        Fft(F, in, 256, 1);
        for (int k = 0; k <= 128; ++k) P[k] = F[k].r * F[k].r + F[k].i * F[k].i;
        float sum = 0.0f;
        for (int k = 1; k <= 127; ++k) sum = sum + P[k];
        const double floorP = AT3PHIP_TONE_PEAK_RATIO * ((double)sum / 127.0);
        int ck[kMax], nc = 0;
        for (int k = 0; k <= 128; ++k) {   // (the spectrum of a real signal is even about bins 0 and 128)
            if (!(P[k] > P[k == 0 ? 1 : k - 1] && P[k] >= P[k == 128 ? 127 : k + 1] && (double)P[k] >= floorP)) continue;
            int at = nc;   // by descending power; an equal power stays behind the lower k
            while (at > 0 && P[k] > P[ck[at - 1]]) --at;
            if (at >= kMax) continue;
            for (int j = nc < kMax ? nc : kMax - 1; j > at; --j) ck[j] = ck[j - 1];
            ck[at] = k;
            if (nc < kMax) ++nc;
        }
        int n = 0;
        for (int c = 0; c < nc; ++c) {
            const int flo = std::max(1, 8 * ck[c] - kSpan), fhi = std::min(1023, 8 * ck[c] + kSpan);
            int bf = -1;
            double bs = 0, bc = 0, bp = 0;   // (with an event: a and b in the places of S and C)
            for (int f = flo; f <= fhi; ++f) {
                double S = 0, C = 0;
                for (int t = 0; t < 256; ++t) {
                    const int pos = ((t - 128) * f) & 2047;
                    S = S + (double)y[t] * (double)T.Sine[pos];
                    C = C + (double)y[t] * (double)T.Sine[(pos + 512) & 2047];
                }
                double pw = (S * S) * T.Rs[f] + (C * C) * T.Rc[f];
                if (event) {   // G4: the 2 x 2 normal equations under the gated window
                    double gss = 0, gcc = 0, gsc = 0;
                    for (int t = t0; t <= t1; ++t) {
                        const int pos = ((t - 128) * f) & 2047;
                        const double sn = (double)T.Sine[pos], cs = (double)T.Sine[(pos + 512) & 2047];
                        gss = gss + (double)wnd[t] * (sn * sn);
                        gcc = gcc + (double)wnd[t] * (cs * cs);
                        gsc = gsc + (double)wnd[t] * (sn * cs);
                    }
                    const double det = gss * gcc - gsc * gsc;
                    if (!(det > 0.0)) continue;
                    const double a = (S * gcc - C * gsc) / det, b = (C * gss - S * gsc) / det;
                    pw = a * S + b * C;
                    S = a;
                    C = b;
                }
                if (bf < 0 || pw > bp) {
                    bf = f;
                    bs = S;
                    bc = C;
                    bp = pw;
                }
            }
            if (bf < 0) continue;
            // x[t] = ca sin + cb cos, by least squares under the window
            const double ca = event ? bs : bs * T.Rs[bf], cb = event ? bc : bc * T.Rc[bf];
            const double a2 = ca * ca + cb * cb;
            if (!(a2 >= AT3PHIP_TONE_MIN_AMP * AT3PHIP_TONE_MIN_AMP)) continue;
            int sf = 0;
            for (int i = 0; i < 64; ++i)
                if (a2 >= T.Thr[i]) sf = i;
            int ph = 0;
            double bv = 0;
            for (int q = 0; q < 32; ++q) {
                const double v = ca * (double)T.Sine[(64 * q + 512) & 2047] + cb * (double)T.Sine[64 * q];
                if (q == 0 || v > bv) {
                    ph = q;
                    bv = v;
                }
            }
            out[n].Freq = bf;
            out[n].AmpSf = sf;
            out[n].Phase = ph;
            out[n].A2 = a2;
            ++n;
        }
        return n;
    }
    static bool Before(const TWave& a, const TWave& b)   // the record's order: channel, band, frequency index
    {
        return a.Ch != b.Ch ? a.Ch < b.Ch : a.Sb != b.Sb ? a.Sb < b.Sb : a.Freq < b.Freq;
    }
    // S2: the words of band sb's waves are the same set in both channels, and so are the points G2 writes for the gates g0, g1
    static bool Twin(const TWave* w, int nw, int g0, int g1, int sb)
    {
        auto within = [&](int a, int b) {   // every word of channel a's band is one of channel b's
            for (int i = 0; i < nw; ++i) {
                if (w[i].Ch != a || w[i].Sb != sb) continue;
                bool found = false;
                for (int j = 0; j < nw; ++j)
                    found = found || (w[j].Ch == b && w[j].Sb == sb && AT3PHIP_TONAL_WAVE(w[j].Freq, w[j].AmpSf, w[j].Phase) == AT3PHIP_TONAL_WAVE(w[i].Freq, w[i].AmpSf, w[i].Phase));
                if (!found) return false;
            }
            return true;
        };
        const at3phip_tonal_band e0 = GateBand(g0), e1 = GateBand(g1);
        return within(0, 1) && within(1, 0) && e0.start == e1.start && e0.stop == e1.stop;
    }
    // steps 6-7
    void Select(TWave* w, int nw)
    {
        Block = at3phip_tonal_block{};
        for (int i = 0; i < nw; ++i) {
            int rank = 0;
            for (int j = 0; j < nw; ++j)
                if (j != i && (w[j].A2 > w[i].A2 || (w[j].A2 == w[i].A2 && Before(w[j], w[i])))) ++rank;
            w[i].Keep = rank < AT3PHIP_TONAL_MAX_WAVES;
        }
        for (int i = 0; i < nw; ++i) {
            if (!w[i].Keep) continue;
            int at = 0;
            for (int j = 0; j < nw; ++j)
                if (w[j].Keep && Before(w[j], w[i])) ++at;
            Block.wave[at] = AT3PHIP_TONAL_WAVE(w[i].Freq, w[i].AmpSf, w[i].Phase);
            Block.band[w[i].Ch][w[i].Sb].n_waves++;
            Block.num_tone_bands = (uint8_t)std::max<int>(Block.num_tone_bands, w[i].Sb + 1);
        }
    }
    // a band's waves at the samples of one frame under the envelope e (waves_synth of the decoder's step 4b): reg = 128 fading
    // out, 0 fading in
    void Waves(const at3phip_tonal_block& b, int ch, int sb, const TEnv& e, int reg, float* out) const
    {
        ch = Src(b, ch, sb);
        int first = 0;
        for (int c = 0; c <= ch; ++c)   // channel 0's bands go first
            for (int k = 0; k < (c < ch ? 16 : sb); ++k) first += b.band[c][k].n_waves;
        for (int wn = 0; wn < b.band[ch][sb].n_waves; ++wn) {
            const uint32_t wv = b.wave[first + wn];
            const double amp = (double)T.AmpSf[(wv >> 10) & 63u];
            const int inc = (int)(wv & 1023u);
            int pos = ((int)(((wv >> 16) & 31u) << 6) - (reg ^ 128) * inc) & 2047;
            for (int i = 0; i < 128; ++i) {
                out[i] = (float)((double)out[i] + (double)T.Sine[pos] * amp);
                pos = (pos + inc) & 2047;
            }
        }
        if (e.Hs) {
            const int pos = (e.S << 2) - reg;
            if (pos > 0 && pos <= 128) {
                for (int i = 0; i < pos; ++i) out[i] = 0.0f;
                if (!e.He || e.S != e.E)
                    for (int k = 0; k < 4 && pos + k < 128; ++k) out[pos + k] = out[pos + k] * T.Hann[32 * k];
            }
        }
        if (e.He) {
            const int pos = ((e.E + 1) << 2) - reg;
            if (pos > 0 && pos <= 128) {
                for (int k = 0; k < 4; ++k) out[pos - 4 + k] = out[pos - 4 + k] * T.Hann[96 - 32 * k];
                for (int i = pos; i < 128; ++i) out[i] = 0.0f;
            }
        }
    }
    // step 8 / G5 for one band: ApplyFilter's out -= wavreg1 + wavreg2 as ff_atrac3p_generate_tones forms them for the block
    // `now` after `before`, whose own envelope follows from `older`'s points
    // S5: each record is resolved through its own sharing word (Src)
    void Subtract(const at3phip_tonal_block& older, const at3phip_tonal_block& before, const at3phip_tonal_block& now, int ch, int sb,
                  float* x) const
    {
        const at3phip_tonal_band &bo = older.band[Src(older, ch, sb)][sb], &bb = before.band[Src(before, ch, sb)][sb], &bn = now.band[Src(now, ch, sb)][sb];
        const int n1 = bb.n_waves, n2 = bn.n_waves;
        if (!n1 && !n2) return;
        const TEnv e2 = CurrEnv(bn, bb), e1 = CurrEnv(bb, bo);
        const bool reg1 = e1.E >= 32, reg2 = e2.S < 32;
        float w1[128] = {0}, w2[128] = {0};
        if (n1 && reg1) Waves(before, ch, sb, e1, 128, w1);
        if (n2 && reg2) Waves(now, ch, sb, e2, 0, w2);
        const bool both = n1 && n2 && reg1 && reg2;
        const bool h1 = both || (n1 && !e1.He), h2 = both || (n2 && !e2.Hs);
        for (int i = 0; i < 128; ++i) {
            if (h1) w1[i] = w1[i] * T.Hann[128 + i];
            if (h2) w2[i] = w2[i] * T.Hann[i];
            x[i] -= w1[i] + w2[i];
        }
    }
    // the channel whose band sb a record's channel ch uses: channel 0's where the record shares the band
    static int Src(const at3phip_tonal_block& b, int ch, int sb) { return ch == 1 && ((b.tone_sharing >> sb) & 1) ? 0 : ch; }
    const int Channels;
    const bool Gated, Shared;
    TTables T;
    at3phip_tonal_block Block{};   // the last block found
    at3phip_tonal_block Older{};   // and the one before it: its points decide the last block's envelope
};

class TAt3PEncoder {
public:
    // deviceTones: the tone analysis on the GPU (at3phip_encode_frames_tonal, a batch per call) instead of an analyser on the
    // host: byte for byte the frames of this class around TAt3PToneAnalyser with UseGha = GHA_ENABLED. `gha` must then be null.
    // deviceGated: that analysis with AT3PHIP_TONES_GATED, byte for byte TAt3PToneAnalyser(channels, true)'s frames.
    // deviceShared: with AT3PHIP_TONES_SHARED, byte for byte TAt3PToneAnalyser(channels, deviceGated, true)'s frames.
    // adaptive: every frame-writing call carries AT3PHIP_ALLOC_ADAPTIVE (include/at3phip.h, ADAPTIVE WORD LENGTHS): the word
    // lengths are chosen on the device, with a host analyser too; the mirror has no allocator of its own.
    // frameBytes: the size of the frames written (at3phip_set_frame_bytes; the caller gives CreateAtrac3PlusOutput the same
    // size). Other than AT3PHIP_FRAME_BYTES it needs `adaptive`: the library refuses the fixed table at any other size.
    // sparse: with `adaptive`, every such call also carries AT3PHIP_ALLOC_SPARSE (SPARSE WORD LENGTHS): a unit inside the coded range
    // may keep word length 0. Without `adaptive` it is an error here, as it is one in the library.
    // rd: with both, every such call also carries AT3PHIP_ALLOC_RD (RATE-DISTORTION WORD LENGTHS); an error without either.
    // psy: with all three, every such call also carries AT3PHIP_ALLOC_PSY (MASKING-WEIGHTED WORD LENGTHS); an error without `rd`.
    TAt3PEncoder(TCompressedOutputPtr&& out, int channels, int batchFrames = 64, int deviceId = 0, TAt3PSettings settings = TAt3PSettings(),
                 IAt3PGhaProcessor* gha = nullptr, bool deviceTones = false, bool deviceGated = false, bool deviceShared = false,
                 bool adaptive = false, int frameBytes = AT3PHIP_FRAME_BYTES, bool sparse = false, bool rd = false, bool psy = false)
        : Out(std::move(out)), Channels((size_t)channels), BatchFrames(batchFrames), FrameFloats((size_t)AT3PHIP_FRAME * (size_t)channels),
          Settings(settings), Gha(gha), DeviceTones(deviceTones), ToneFlags((deviceGated ? AT3PHIP_TONES_GATED : 0u) | (deviceShared ? AT3PHIP_TONES_SHARED : 0u)),
          AllocFlag((adaptive ? AT3PHIP_ALLOC_ADAPTIVE : 0u) | (sparse ? AT3PHIP_ALLOC_SPARSE : 0u) | (rd ? AT3PHIP_ALLOC_RD : 0u) | (psy ? AT3PHIP_ALLOC_PSY : 0u)), FrameBytes((size_t)frameBytes)
    {
        if (sparse && !adaptive) throw std::invalid_argument("TAt3PEncoder: sparse needs adaptive");
        if (rd && !(adaptive && sparse)) throw std::invalid_argument("TAt3PEncoder: rd needs adaptive and sparse");
        if (psy && !rd) throw std::invalid_argument("TAt3PEncoder: psy needs rd");
        if (deviceTones && gha) throw std::invalid_argument("TAt3PEncoder: deviceTones takes no host analyser");
        if (deviceGated && !deviceTones) throw std::invalid_argument("TAt3PEncoder: deviceGated needs deviceTones");
        if (deviceShared && !deviceTones) throw std::invalid_argument("TAt3PEncoder: deviceShared needs deviceTones");
        at3phip_config cfg{};
        cfg.channels = channels;
        cfg.n_streams = 1;
        cfg.max_frames = batchFrames;
        cfg.device_id = deviceId;
        const int rc = at3phip_create(&cfg, &Ctx);
        if (rc != AT3HIP_OK) throw std::runtime_error("at3phip_create failed: " + std::to_string(rc));
        if (frameBytes != AT3PHIP_FRAME_BYTES) {   // (a context at the default size is never told so: its calls stay what they were)
            const int src = at3phip_set_frame_bytes(Ctx, frameBytes);
            if (src != AT3HIP_OK) {
                const std::string why = at3phip_last_error(Ctx);
                at3phip_destroy(Ctx);
                throw std::runtime_error("at3phip_set_frame_bytes: " + why);
            }
        }
        Pending.reserve((size_t)BatchFrames * FrameFloats);
    }
    ~TAt3PEncoder()
    {
        try {
            Flush();
        } catch (...) {
        }
        at3phip_destroy(Ctx);
    }
    TAt3PEncoder(const TAt3PEncoder&) = delete;
    TAt3PEncoder& operator=(const TAt3PEncoder&) = delete;

    TProcessLambda GetLambda()
    {
        return [this](float* data, const ProcessMeta&) {
            const bool first = Calls == 0;
            ++Calls;
            Pending.insert(Pending.end(), data, data + FrameFloats);
            if ((int)(Pending.size() / FrameFloats) == BatchFrames) Flush();
            return first ? EProcessResult::LOOK_AHEAD : EProcessResult::PROCESSED;
        };
    }

    // nFrames frames of 16-bit PCM [nFrames][2048][channels] (at3phip_encode_frames_short: a sample s is s / 32768.0f, widened
    // on the device), behind whatever the lambda has buffered; they count as nFrames calls of the lambda on these floats, so the
    // look-ahead schedule is kept (true when the first of them was the stream's first call). At most batchFrames frames go
    // into one call.
    bool EncodeS16(const int16_t* pcm, int nFrames)
    {
        Flush();
        const bool first = Calls == 0 && nFrames > 0;
        if (Gha) {   // the analyser takes float PCM: the same floats as the device's widening, through the float schedule
            for (int at = 0; at < nFrames; at += BatchFrames) {
                const size_t n = (size_t)std::min(BatchFrames, nFrames - at) * FrameFloats;
                for (size_t i = 0; i < n; ++i) Pending.push_back((float)pcm[(size_t)at * FrameFloats + i] * 0x1p-15f);
                Calls += n / FrameFloats;
                Flush();
            }
            return first;
        }
        std::vector<uint8_t> frames((size_t)BatchFrames * FrameBytes);
        for (int at = 0; at < nFrames; at += BatchFrames) {
            const int nf = std::min(BatchFrames, nFrames - at);
            if (DeviceTones) Chk(at3phip_encode_frames_tonal_short(Ctx, pcm + (size_t)at * FrameFloats, nf, frames.data(), ToneFlags | AllocFlag), "at3phip_encode_frames_tonal_short");
            else Chk(at3phip_encode_frames_short(Ctx, pcm + (size_t)at * FrameFloats, nf, frames.data(), AllocFlag), "at3phip_encode_frames_short");
            for (int i = 0; i < nf; ++i) Ready.emplace_back(frames.begin() + (size_t)i * FrameBytes, frames.begin() + (size_t)(i + 1) * FrameBytes);
            Calls += (size_t)nf;
            Flush();
        }
        return first;
    }

    // Encodes what is buffered and writes the frames that are due: after n calls, n - 1 frames have been written.
    void Flush()
    {
        const int nf = (int)(Pending.size() / FrameFloats);
        if (Gha) {
            if (nf > 0) FlushAnalysed(nf);
            return;
        }
        if (nf > 0) {
            std::vector<uint8_t> frames((size_t)nf * FrameBytes);
            if (DeviceTones) Chk(at3phip_encode_frames_tonal(Ctx, Pending.data(), nf, frames.data(), ToneFlags | AllocFlag), "at3phip_encode_frames_tonal");
            else Chk(at3phip_encode_frames(Ctx, Pending.data(), nf, frames.data(), AllocFlag), "at3phip_encode_frames");
            Pending.clear();
            for (int i = 0; i < nf; ++i) Ready.emplace_back(frames.begin() + (size_t)i * FrameBytes, frames.begin() + (size_t)(i + 1) * FrameBytes);
        }
        // call k (0-based) is answered with: nothing (k = 0), silence (k = 1), input frame k - 2; with deviceTones the analysis lags
        // one frame itself (its frame f holds the residual of input frame f - 1), so call k >= 1 is answered with its frame k - 1
        // and the stream's last frame stays behind, as it does on the host
        while (Written + 1 < Calls) {
            if (Written == 0 && !DeviceTones) {
                Out->WriteFrame(SilentFrame());
            } else {
                Out->WriteFrame(std::move(Ready.front()));
                Ready.erase(Ready.begin());
            }
            ++Written;
        }
    }

private:
    void Chk(int rc, const char* what)
    {
        if (rc != AT3HIP_OK) throw std::runtime_error(std::string(what) + ": " + at3phip_last_error(Ctx));
    }
    // The calls that buffered the `nf` pending frames, EncodeFrame by EncodeFrame (at3p.cpp:89-180). Call k >= 1 transforms and
    // writes PrevBuf, which holds input frame k - 2 (or zeros) as call k's analysis left it.
    void FlushAnalysed(int nf)
    {
        const size_t C = Channels, N = AT3PHIP_FRAME;
        std::vector<float> bands((size_t)nf * FrameFloats);
        Chk(at3phip_pqf_analyse(Ctx, Pending.data(), nf, bands.data(), 0), "at3phip_pqf_analyse");
        if (PrevBuf.empty()) {
            PrevBuf.assign(FrameFloats, 0.0f);
            CurBuf.assign(FrameFloats, 0.0f);
            RawCur.assign(FrameFloats, 0.0f);
        }
        const size_t first = Calls - (size_t)nf;   // the call that buffered Pending's first frame
        std::vector<float> prevs;                  // what each writing call transforms [calls][C][16][128]
        std::vector<at3phip_tonal_block> blocks;   // and the block it writes
        for (int i = 0; i < nf; ++i) {
            const float* next = bands.data() + (size_t)i * FrameFloats;
            if (first + (size_t)i > 0) {
                const at3phip_tonal_block* found = Gha->DoAnalize({CurBuf.data(), next}, {C == 2 ? CurBuf.data() + N : nullptr, C == 2 ? next + N : nullptr},
                                                                  PrevBuf.data(), C == 2 ? PrevBuf.data() + N : nullptr, RawCur.data(),
                                                                  C == 2 ? RawCur.data() + N : nullptr);
                prevs.insert(prevs.end(), PrevBuf.begin(), PrevBuf.end());
                blocks.push_back(Delay);
                if (Settings.UseGha & TAt3PSettings::GHA_PASS_INPUT) PrevBuf = CurBuf;
                else std::fill(PrevBuf.begin(), PrevBuf.end(), 0.0f);
                if (found && (Settings.UseGha & TAt3PSettings::GHA_WRITE_TONAL)) Delay = *found;
                else Delay = at3phip_tonal_block{};
            }
            CurBuf.assign(next, next + FrameFloats);
            for (size_t ch = 0; ch < C; ++ch)
                for (size_t k = 0; k < N; ++k) RawCur[ch * N + k] = Pending[(size_t)i * FrameFloats + k * C + ch];
        }
        Pending.clear();
        const int calls = (int)blocks.size();
        if (calls == 0) return;
        if (!(Settings.UseGha & TAt3PSettings::GHA_WRITE_RESIUDAL)) std::fill(prevs.begin(), prevs.end(), 0.0f);
        std::vector<float> specs(prevs.size());
        std::vector<uint8_t> frames((size_t)calls * FrameBytes);
        Chk(at3phip_mdct(Ctx, prevs.data(), calls, nullptr, specs.data(), AT3PHIP_RESIDUAL_SCALE), "at3phip_mdct");
        Chk(at3phip_write_frames_tonal(Ctx, specs.data(), calls, nullptr, blocks.data(), frames.data(), AllocFlag), "at3phip_write_frames_tonal");
        for (int i = 0; i < calls; ++i)
            Out->WriteFrame(std::vector<char>(frames.begin() + (size_t)i * FrameBytes, frames.begin() + (size_t)(i + 1) * FrameBytes));
        Written += (size_t)calls;
    }
    std::vector<char> SilentFrame()   // an all-zero spectrum through the frame writer (the encoder's PrevBuf starts zeroed)
    {
        std::vector<float> specs(FrameFloats, 0.0f);
        std::vector<uint8_t> frame(FrameBytes);
        Chk(at3phip_write_frames(Ctx, specs.data(), 1, nullptr, frame.data(), AllocFlag), "at3phip_write_frames");
        return std::vector<char>(frame.begin(), frame.end());
    }
    TCompressedOutputPtr Out;
    const size_t Channels;
    const int BatchFrames;
    const size_t FrameFloats;
    at3phip_ctx* Ctx = nullptr;
    std::vector<float> Pending;
    std::vector<std::vector<char>> Ready;
    size_t Calls = 0, Written = 0;
    const TAt3PSettings Settings;
    IAt3PGhaProcessor* const Gha;                 // not owned; null: the analysis finds nothing
    const bool DeviceTones;                       // the analysis runs on the GPU
    const uint32_t ToneFlags;                     // and with these flags (AT3PHIP_TONES_GATED, AT3PHIP_TONES_SHARED)
    const uint32_t AllocFlag;                     // AT3PHIP_ALLOC_ADAPTIVE (| AT3PHIP_ALLOC_SPARSE (| AT3PHIP_ALLOC_RD (| AT3PHIP_ALLOC_PSY))) or 0, on every frame-writing call
    const size_t FrameBytes;                      // the context's frame size
    std::vector<float> PrevBuf, CurBuf, RawCur;   // [C][16][128] / [C][2048]: TChannelCtx's PrevBuf, CurBuf and RawCurBuf
    at3phip_tonal_block Delay{};                  // `delay`: the block the next call writes
};

// ---- sample-rate conversion (include/at3hip_resample.h) ------------------------------------------------------------------
// One at3hip_resampler of one stream, owned.
class TResampler {
public:
    TResampler(int inRate, int outRate, int channels, int maxIn, int device) : Channels(channels)
    {
        CheckLibraryVersion();
        at3hip_resampler_config cfg{inRate, outRate, channels, 1, maxIn, device};
        const int rc = at3hip_resampler_create(&cfg, &R);
        if (rc != AT3HIP_OK)
            throw std::runtime_error("at3hip_resampler_create(" + std::to_string(inRate) + " -> " + std::to_string(outRate) +
                                     ") failed (" + std::to_string(rc) + ")");
        Out.resize((size_t)at3hip_resampler_max_out(R) * channels);
    }
    ~TResampler()
    {
        if (R) at3hip_resampler_destroy(R);
    }
    TResampler(const TResampler&) = delete;
    TResampler& operator=(const TResampler&) = delete;

    // n sample frames of interleaved input; appends the outputs they complete to `dst`
    void Process(const float* in, int32_t n, std::vector<float>& dst) { Append(at3hip_resampler_process(R, in, n, Out.data(), &N, 0), dst); }
    // the remaining outputs; then the start state
    void Flush(std::vector<float>& dst) { Append(at3hip_resampler_flush(R, Out.data(), &N, 0), dst); }
    // 16-bit input (at3hip_resampler_process_s16: a sample s is s / 32768.0f, widened on the device), float output
    void ProcessS16(const int16_t* in, int32_t n, std::vector<float>& dst) { Append(at3hip_resampler_process_s16(R, in, n, Out.data(), &N, 0), dst); }
    // 16-bit output (AT3HIP_RESAMPLE_OUT_S16: lrintf(clamp(x, -1, 1) * 32767.0f), the decoders' rule) of float and of 16-bit input
    void Process(const float* in, int32_t n, std::vector<int16_t>& dst)
    {
        Append(at3hip_resampler_process(R, in, n, Out.data(), &N, AT3HIP_RESAMPLE_OUT_S16), dst);
    }
    void ProcessS16(const int16_t* in, int32_t n, std::vector<int16_t>& dst)
    {
        Append(at3hip_resampler_process_s16(R, in, n, Out.data(), &N, AT3HIP_RESAMPLE_OUT_S16), dst);
    }
    void Flush(std::vector<int16_t>& dst) { Append(at3hip_resampler_flush(R, Out.data(), &N, AT3HIP_RESAMPLE_OUT_S16), dst); }

private:
    template <class T>
    void Append(int rc, std::vector<T>& dst)   // (16-bit outputs lie in the front of the float buffer)
    {
        if (rc != AT3HIP_OK) throw std::runtime_error(std::string("at3hip_resampler: ") + at3hip_resampler_last_error(R));
        const size_t at = dst.size();
        dst.resize(at + (size_t)N * Channels);
        memcpy(dst.data() + at, Out.data(), (size_t)N * Channels * sizeof(T));
    }
    at3hip_resampler* R = nullptr;
    int Channels;
    int32_t N = 0;
    std::vector<float> Out;
};

// A PCM source at another rate, converted to `outRate` in chunks of kChunk input samples and flushed at the source's end. TSrc
// has GetChannelNum / GetSampleRate / GetTotalSamples and Read(float*, frames) as TWavSource (at3hip_io.hpp); so does this.
template <class TSrc>
class TResampledSource {
public:
    static constexpr int kChunk = 1 << 16;

    TResampledSource(TSrc& src, int outRate, int device)
        : Src(src), Rate(outRate), Rs((int)src.GetSampleRate(), outRate, (int)src.GetChannelNum(), kChunk, device),
          In((size_t)kChunk * src.GetChannelNum())
    {
        int32_t L = 0, M = 0;
        at3hip_resampler_shape((int32_t)src.GetSampleRate(), outRate, &L, &M, nullptr);
        Total = (src.GetTotalSamples() * (uint64_t)L + (uint64_t)M - 1) / (uint64_t)M;   // ceil(N L / M)
    }

    size_t GetChannelNum() const { return Src.GetChannelNum(); }
    size_t GetSampleRate() const { return (size_t)Rate; }
    uint64_t GetTotalSamples() const { return Total; }

    size_t Read(float* dst, size_t frames)
    {
        const size_t C = Src.GetChannelNum();
        while (Buf.size() / C - Pos < frames && !Done) {
            Buf.erase(Buf.begin(), Buf.begin() + Pos * C);
            Pos = 0;
            const size_t n = Src.Read(In.data(), kChunk);
            if (n) {
                Rs.Process(In.data(), (int32_t)n, Buf);
            } else {
                Rs.Flush(Buf);
                Done = true;
            }
        }
        const size_t n = std::min(frames, Buf.size() / C - Pos);
        std::copy(Buf.begin() + Pos * C, Buf.begin() + (Pos + n) * C, dst);
        Pos += n;
        return n;
    }

private:
    TSrc& Src;
    int Rate;
    TResampler Rs;
    std::vector<float> In, Buf;
    size_t Pos = 0;
    uint64_t Total = 0;
    bool Done = false;
};

// ---- loudness and peak (include/at3hip_loudness.h) ------------------------------------------------------------------------
// One at3hip_loudness of one stream, owned: Process the 44.1 kHz samples the encoder will see, Finish, then Gain gives the one
// constant that brings the stream to a target loudness under a peak ceiling, and Apply multiplies by it.
class TLoudnessMeter {
public:
    static constexpr int kChunk = 1 << 16;

    // maxSamples: the most samples Process will see before Finish (bounds the hops the context keeps)
    TLoudnessMeter(int channels, uint64_t maxSamples, bool truePeak, int device) : Channels(channels)
    {
        CheckLibraryVersion();
        at3hip_loudness_config cfg{channels, 1, kChunk, (int32_t)(maxSamples / AT3HIP_LOUDNESS_HOP + 1), truePeak ? 1 : 0, device};
        const int rc = at3hip_loudness_create(&cfg, &L);
        if (rc != AT3HIP_OK) throw std::runtime_error("at3hip_loudness_create failed (" + std::to_string(rc) + ")");
    }
    ~TLoudnessMeter()
    {
        if (L) at3hip_loudness_destroy(L);
    }
    TLoudnessMeter(const TLoudnessMeter&) = delete;
    TLoudnessMeter& operator=(const TLoudnessMeter&) = delete;

    // n sample frames of interleaved input
    void Process(const float* in, size_t n)
    {
        for (size_t at = 0; at < n; at += kChunk)
            Check(at3hip_loudness_process(L, in + at * Channels, (int32_t)std::min<size_t>(kChunk, n - at), 0));
    }
    // the same for 16-bit PCM (at3hip_loudness_process_s16: a sample s is s / 32768.0f, widened on the device)
    void ProcessS16(const int16_t* in, size_t n)
    {
        for (size_t at = 0; at < n; at += kChunk)
            Check(at3hip_loudness_process_s16(L, in + at * Channels, (int32_t)std::min<size_t>(kChunk, n - at), 0));
    }
    // every sample of a source (GetChannelNum / Read as TWavSource)
    template <class TSrc>
    void ProcessAll(TSrc& src)
    {
        std::vector<float> buf((size_t)kChunk * Channels);
        while (const size_t n = src.Read(buf.data(), kChunk)) Process(buf.data(), n);
    }
    at3hip_loudness_result Finish()
    {
        at3hip_loudness_result r{};
        Check(at3hip_loudness_finish(L, &r));
        return r;
    }
    static float Gain(const at3hip_loudness_result& r, double targetLufs, double ceilingDb)
    {
        float g = 1.0f;
        at3hip_loudness_gain(&r, targetLufs, ceilingDb, &g);
        return g;
    }
    // the peak the gain rule uses: the larger channel's true peak if it was measured, else the larger sample peak
    static float Peak(const at3hip_loudness_result& r)
    {
        const bool measured = r.true_peak[0] != 0.0f || r.true_peak[1] != 0.0f;
        const float* p = measured ? r.true_peak : r.sample_peak;
        return std::max(p[0], p[1]);
    }
    // pcm[i] *= g for n sample frames, on the GPU
    void Apply(float* pcm, size_t n, float g)
    {
        for (size_t at = 0; at < n; at += kChunk)
            Check(at3hip_loudness_apply(L, pcm + at * Channels, (int32_t)std::min<size_t>(kChunk, n - at), &g, pcm + at * Channels, 0));
    }

    // out[i] = (pcm[i] / 32768.0f) * g for n sample frames of 16-bit PCM, on the GPU (at3hip_loudness_apply_s16)
    void ApplyS16(const int16_t* pcm, size_t n, float g, float* out)
    {
        for (size_t at = 0; at < n; at += kChunk)
            Check(at3hip_loudness_apply_s16(L, pcm + at * Channels, (int32_t)std::min<size_t>(kChunk, n - at), &g, out + at * Channels, 0));
    }

private:
    void Check(int rc)
    {
        if (rc != AT3HIP_OK) throw std::runtime_error(std::string("at3hip_loudness: ") + at3hip_loudness_last_error(L));
    }
    at3hip_loudness* L = nullptr;
    int Channels;
};

// A PCM source times one constant (TLoudnessMeter::Apply). TSrc as for TResampledSource, and so is this: with both in use this
// one sits behind the converter, so that the samples scaled are the 44.1 kHz samples that were metered.
template <class TSrc>
class TScaledSource {
public:
    TScaledSource(TSrc& src, float gain, int device) : Src(src), Gain(gain), Meter((int)src.GetChannelNum(), 0, false, device) {}

    size_t GetChannelNum() const { return Src.GetChannelNum(); }
    size_t GetSampleRate() const { return Src.GetSampleRate(); }
    uint64_t GetTotalSamples() const { return Src.GetTotalSamples(); }
    size_t Read(float* dst, size_t frames)
    {
        const size_t n = Src.Read(dst, frames);
        Meter.Apply(dst, n, Gain);
        return n;
    }

private:
    TSrc& Src;
    float Gain;
    TLoudnessMeter Meter;
};

// A PCM source times one constant and through the look-ahead limiter (at3hip_loudness_limit_*: the gain may exceed what the
// peak allows, the limiter holds the ceiling). As TScaledSource it sits behind the converter and hands out exactly the
// source's number of samples: the limiter's latency is taken up here, the held-back samples come with the flush at the
// source's end.
template <class TSrc>
class TLimitedSource {
public:
    static constexpr int kChunk = 1 << 16;

    TLimitedSource(TSrc& src, float gain, float ceiling, bool truePeak, int device)
        : Src(src), Channels((int)src.GetChannelNum()), In((size_t)kChunk * src.GetChannelNum())
    {
        CheckLibraryVersion();
        at3hip_loudness_config cfg{Channels, 1, kChunk, 1, 0, device};
        const int rc = at3hip_loudness_create(&cfg, &L);
        if (rc != AT3HIP_OK) throw std::runtime_error("at3hip_loudness_create failed (" + std::to_string(rc) + ")");
        Check(at3hip_loudness_limit_start(L, &gain, ceiling, truePeak ? AT3HIP_LIMIT_TRUE_PEAK : 0u));
        Out.resize((size_t)std::max<int32_t>(kChunk, at3hip_loudness_limit_delay(AT3HIP_LIMIT_TRUE_PEAK)) * Channels);
    }
    ~TLimitedSource()
    {
        if (L) at3hip_loudness_destroy(L);
    }
    TLimitedSource(const TLimitedSource&) = delete;
    TLimitedSource& operator=(const TLimitedSource&) = delete;

    size_t GetChannelNum() const { return Src.GetChannelNum(); }
    size_t GetSampleRate() const { return Src.GetSampleRate(); }
    uint64_t GetTotalSamples() const { return Src.GetTotalSamples(); }

    size_t Read(float* dst, size_t frames)
    {
        const size_t C = (size_t)Channels;
        while (Buf.size() / C - Pos < frames && !Done) {
            Buf.erase(Buf.begin(), Buf.begin() + Pos * C);
            Pos = 0;
            const size_t n = Src.Read(In.data(), kChunk);
            int32_t got = 0;
            if (n) {
                Check(at3hip_loudness_limit(L, In.data(), (int32_t)n, Out.data(), &got, 0));
            } else {
                Check(at3hip_loudness_limit_flush(L, Out.data(), &got, 0));
                Done = true;
            }
            Buf.insert(Buf.end(), Out.begin(), Out.begin() + (size_t)got * C);
        }
        const size_t n = std::min(frames, Buf.size() / C - Pos);
        std::copy(Buf.begin() + Pos * C, Buf.begin() + (Pos + n) * C, dst);
        Pos += n;
        return n;
    }

    // the run's statistics so far (all of it once Read has returned 0 or every sample)
    at3hip_limit_stats Stats()
    {
        at3hip_limit_stats st{};
        Check(at3hip_loudness_limit_stats(L, &st));
        return st;
    }

private:
    void Check(int rc)
    {
        if (rc != AT3HIP_OK) throw std::runtime_error(std::string("at3hip_loudness: ") + at3hip_loudness_last_error(L));
    }
    TSrc& Src;
    int Channels;
    at3hip_loudness* L = nullptr;
    std::vector<float> In, Out, Buf;
    size_t Pos = 0;
    bool Done = false;
};

}  // namespace NAtracDEncHip
