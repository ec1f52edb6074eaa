// at3hipenc - command-line ATRAC3 / ATRAC1 / ATRAC3plus encoder on libat3hip: the
// reference tool's `-e atrac3` path (main.cpp:367-425, 659-705), `-e atrac1` path (main.cpp:292-345, 630-648) and
// `-e atrac3plus` path (main.cpp:427-483, 679-686; without the tonal analysis, which needs libgha) with the GPU encoders
// behind the same IProcessor-shaped objects.
//
//   at3hipenc -e atrac3 -i in.wav -o out.{oma|at3|wav|raw|dat} [--bitrate kbit] [--bfuidxconst n] [--notonal]
//             [--nogaincontrol] [--container oma|riff|raw] [--nostdout] [--batch blocks] [--device n]
//   at3hipenc -e atrac1 -i in.wav -o out.{aea|raw|dat} [--bfuidxconst 1..8] [--notransient[=mask]]
//             [--container aea|raw] [--nostdout] [--batch blocks] [--device n]
//   at3hipenc -e atrac3plus -i in.wav -o out.{oma|at3|wav|raw|dat} [--adaptive [--sparse [--rd [--psy]]] [--bitrate kbit]] [--tones [--gate] [--share]]
//             [--container oma|riff|raw] [--nostdout] [--batch frames] [--device n]
//             --bitrate: one of kAt3pRates' rows (32 .. 352 kbit/s); below 352 the frames are smaller than the 2048 bytes the
//             fixed word-length table fills, so it needs --adaptive. -d decodes an ATRAC3plus file of any of these frame sizes
//             and names the bitrate in its "Codec:" line for every size but 2048 bytes, whose line stays the text it always was.
//   --resample (all three encoders): a WAV at 8 .. 192 kHz (at3hip_resample.h's list) is converted to 44.1 kHz on the GPU
//             first; the container headers count ceil(N 44100 / rate) samples. A 44.1 kHz input is encoded as without it.
//   --loudness LUFS [--peak dBFS] [--truepeak] (all three encoders): pass one meters the 44.1 kHz samples the encoder will see
//             (after --resample) on the GPU (at3hip_loudness.h: BS.1770 integrated loudness, sample peak or with --truepeak the 4x
//             oversampled peak), pass two encodes them times the one gain that reaches the target with the peak at or below
//             --peak (default -1.0); with --limit the gain is the one to the target alone and the look-ahead limiter of
//             at3hip_loudness.h holds the ceiling (detector: the samples, or with --truepeak the 4x oversampled signal too), and
//             one more line, `limiter: max reduction <x> dB, limited <y> %`, follows the encode. Prints `loudness: I <x> LUFS, peak <y> dBFS, gain <z> dB` unless --nostdout, and for atrac3
//             `clipping: <n> blocks, <m> values` after the encode (at3hip_get_counters).
//   at3hipenc --measure -i in.wav [--resample] [--truepeak]: prints the meter's result and writes nothing.
//   --rate hz (every decoder): the decoded audio is converted to hz (at3hip_resample.h's list) on the GPU, clamped to [-1, 1] and
//             written as lrintf(x * 32767.0f); the WAV counts ceil(N hz / 44100) samples. --rate 44100 writes what -d writes alone.
//   at3hipenc -d -i in.aea -o out.wav [--nostdout] [--batch frames] [--device n]
//             the reference's ATRAC1 decode path (main.cpp:343-365, 697-705) on the GPU decoder (at1hip.h)
//   at3hipenc -d -i in.{oma|at3|wav} -o out.wav [--nostdout] [--batch frames] [--device n]
//             ATRAC3 in an OMA container or in RIFF/WAVE (format 0x270), chosen by content, on the GPU decoder (at3hip.h)
//
// File-level behaviour follows the reference: 44.1 kHz input only (without --resample), numFrames estimate = samples / 1024 in the
// container header, the look-ahead first call, the drain call at end of input.
//
// Structure: every `-e` runs through encode<TCodec> and every `-d` through run_decode<D>; what differs between the codecs is
// the description struct (TAtrac1Encode ..., TAt1Decode ...) each driver is instantiated with.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include <cstdint>
#include <fstream>
#include <memory>
#include <vector>

#include "../../include/at1hip.h"
#include "../../include/at3hip.h"
#include "at3hip_io.hpp"

using namespace NAtracDEncHip;

namespace {

// The two exceptions TAtrac1Decoder's lambda catches and reports as "Skipping invalid ATRAC1 frame: <what>"
// (atrac1denc.cpp:154-162): the text of the one a sound unit raises, or nullptr for a valid unit. The GPU decoder makes the same
// decision (and counts it); the tool re-derives it per unit to print the reference's lines in the reference's order.
const char* at1_unit_fault(const uint8_t* u)
{
    if ((u[0] >> 6) == 3 || ((u[0] >> 4) & 3) == 3) return "invalid ATRAC1 block size mode";   // TBlockSizeMod::Parse
    static const int spb[52] = {8,  8,  8,  8,  4,  4,  4,  4,  8,  8,  8,  8,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  7,  7,
                                7,  7,  9,  9,  9,  9,  10, 10, 10, 10, 12, 12, 12, 12, 12, 12, 12, 12, 20, 20, 20, 20, 20, 20, 20, 20};
    static const int amount[8] = {20, 28, 32, 36, 40, 44, 48, 52};   // BfuAmountTab
    auto bits = [u](int p, int n) {
        uint32_t v = 0;
        for (int k = 0; k < n; ++k, ++p) v = (v << 1) | ((u[p >> 3] >> (7 - (p & 7))) & 1u);
        return v;
    };
    const int nbfu = amount[bits(8, 3)];
    int end = 16 + 10 * nbfu;
    for (int b = 0; b < nbfu; ++b) {
        const int wl = (int)bits(16 + 4 * b, 4);
        end += (wl ? wl + 1 : 0) * spb[b];
    }
    return end > AT1HIP_FRAME_SIZE * 8 ? "read past the end of the bitstream" : nullptr;   // TBitStream::Read, bitstream.cpp:73-74
}

// ATRAC3plus at 44.1 kHz: --bitrate kbit and the frame size it stands for. A frame is 2048 samples per channel, so
// bytes * 8 * 44100 / 2048 is the bit rate: 192 -> 33.1 kbit/s, 376 -> 64.8, 2048 -> 352.8. The sizes are the ones remembered
// from Sony's players; nobody here could check them against a device. 32 kbit/s is a mono rate.
struct TAt3pRate {
    int kbit, frameBytes;
};
const TAt3pRate kAt3pRates[] = {{32, 192}, {48, 280}, {64, 376}, {96, 560}, {128, 744}, {160, 936}, {192, 1120}, {256, 1488}, {320, 1864}, {352, 2048}};

const TAt3pRate* at3p_rate_of_kbit(int kbit)
{
    for (const TAt3pRate& r : kAt3pRates)
        if (r.kbit == kbit) return &r;
    return nullptr;
}
const TAt3pRate* at3p_rate_of_bytes(int frameBytes)
{
    for (const TAt3pRate& r : kAt3pRates)
        if (r.frameBytes == frameBytes) return &r;
    return nullptr;
}
std::string at3p_rate_table()
{
    std::string t;
    for (const TAt3pRate& r : kAt3pRates)
        t += (t.empty() ? "" : ", ") + std::to_string(r.kbit) + (r.kbit == 32 ? " (mono only)" : "") + " -> " + std::to_string(r.frameBytes) + " bytes";
    return t;
}

int fatal(const std::string& what)
{
    std::cerr << "Fatal error: " << what << std::endl;
    return 1;
}

void put_le(std::vector<char>& h, uint32_t v, int bytes)
{
    for (int i = 0; i < bytes; ++i) h.push_back((char)((v >> (8 * i)) & 0xff));
}

// The 44-byte canonical header of a 16-bit PCM WAV at 44100 Hz with `dataBytes` bytes of samples.
void write_wav_header(std::ofstream& out, uint32_t nch, uint32_t dataBytes, uint32_t rate = 44100)
{
    std::vector<char> wav;
    wav.insert(wav.end(), {'R', 'I', 'F', 'F'});
    put_le(wav, 36 + dataBytes, 4);
    wav.insert(wav.end(), {'W', 'A', 'V', 'E', 'f', 'm', 't', ' '});
    put_le(wav, 16, 4);
    put_le(wav, 1, 2);   // PCM
    put_le(wav, nch, 2);
    put_le(wav, rate, 4);
    put_le(wav, rate * 2u * nch, 4);
    put_le(wav, 2u * nch, 2);
    put_le(wav, 16, 2);
    wav.insert(wav.end(), {'d', 'a', 't', 'a'});
    put_le(wav, dataBytes, 4);
    out.write(wav.data(), (std::streamsize)wav.size());
}

// The encoders' input: the WAV file at 44.1 kHz, or with --resample a WAV file at any rate at3hip_resample.h supports, converted
// to 44.1 kHz on the GPU (TResampledSource). Without the flag any other rate is refused, as the reference refuses it (main.cpp:281).
struct TRateInput {
    TWavSource File;
    std::unique_ptr<TResampledSource<TWavSource>> Conv;

    TRateInput(const std::string& path, bool resample, int device) : File(path)
    {
        if (File.GetSampleRate() == 44100) return;
        if (!resample) throw std::runtime_error("unsupported sample rate");
        Conv.reset(new TResampledSource<TWavSource>(File, 44100, device));
    }
    size_t GetChannelNum() const { return File.GetChannelNum(); }
    size_t GetSampleRate() const { return Conv ? Conv->GetSampleRate() : File.GetSampleRate(); }
    uint64_t GetTotalSamples() const { return Conv ? Conv->GetTotalSamples() : File.GetTotalSamples(); }   // ceil(N 44100 / in)
    size_t Read(float* dst, size_t frames) { return Conv ? Conv->Read(dst, frames) : File.Read(dst, frames); }
};

// --loudness / --peak / --truepeak / --limit
struct TLevel {
    bool On = false, TruePeak = false, NoStdOut = false, Limit = false;
    double Target = 0.0, Ceiling = -1.0;
};

// Pass one of --loudness, and all of --measure: the 44.1 kHz samples an encoder would see (after --resample) through the meter
// (at3hip_loudness.h).
at3hip_loudness_result measure_input(const std::string& path, bool resample, int device, bool truePeak)
{
    TRateInput in(path, resample, device);
    TLoudnessMeter meter((int)in.GetChannelNum(), in.GetTotalSamples(), truePeak, device);
    meter.ProcessAll(in);
    return meter.Finish();
}

double db_of(double linear) { return 20.0 * std::log10(linear); }

// The encoders' input with --loudness: pass one meters the file, pass two (this object's Read) hands the encoder the same
// samples times the one gain that brings them to the target loudness with the peak at or below the ceiling (TScaledSource
// behind the converter). With --limit the gain is the one to the target alone and the look-ahead limiter holds the ceiling
// (TLimitedSource; the detector is the true-peak one with --truepeak). Without --loudness this is TRateInput.
struct TEncodeInput {
    TRateInput Base;
    std::unique_ptr<TScaledSource<TRateInput>> Scaled;
    std::unique_ptr<TLimitedSource<TRateInput>> Limited;

    TEncodeInput(const std::string& path, bool resample, int device, const TLevel& level) : Base(path, resample, device)
    {
        if (!level.On) return;
        const at3hip_loudness_result r = measure_input(path, resample, device, level.TruePeak);
        // (--limit: a ceiling that never binds leaves the gain to the target alone)
        const float g = TLoudnessMeter::Gain(r, level.Target, level.Limit ? 400.0 : level.Ceiling);
        if (!level.NoStdOut) {
            char line[160];
            snprintf(line, sizeof(line), "loudness: I %.2f LUFS, peak %.2f dBFS, gain %.2f dB", r.integrated,
                     db_of((double)TLoudnessMeter::Peak(r)), db_of((double)g));
            std::cout << line << std::endl;
        }
        if (level.Limit) Limited.reset(new TLimitedSource<TRateInput>(Base, g, (float)std::pow(10.0, level.Ceiling / 20.0), level.TruePeak, device));
        else Scaled.reset(new TScaledSource<TRateInput>(Base, g, device));
    }
    // --limit: `limiter: max reduction <x> dB, limited <y> %` once the input has been read
    void Report(const TLevel& level)
    {
        if (!Limited || level.NoStdOut) return;
        const at3hip_limit_stats st = Limited->Stats();
        char line[160];
        snprintf(line, sizeof(line), "limiter: max reduction %.2f dB, limited %.2f %%", -db_of((double)st.min_sum / (double)AT3HIP_LIMIT_FULL),
                 st.n_out ? 100.0 * (double)st.n_limited / (double)st.n_out : 0.0);
        std::cout << line << std::endl;
    }
    size_t GetChannelNum() const { return Base.GetChannelNum(); }
    size_t GetSampleRate() const { return Base.GetSampleRate(); }
    uint64_t GetTotalSamples() const { return Base.GetTotalSamples(); }
    size_t Read(float* dst, size_t frames) { return Limited ? Limited->Read(dst, frames) : Scaled ? Scaled->Read(dst, frames) : Base.Read(dst, frames); }
};

// `-d ... --rate <hz>`: the decoder's float output (44.1 kHz, already clamped) converted to another rate on the GPU
// (at3hip_resample.h), clamped to [-1, 1] again and written as lrintf(x * 32767.0f), the rule of the 44.1 kHz output. The WAV
// header counts ceil(N rate / 44100) samples for the N decoded ones; Finish() writes the converter's tail.
class TRateWriter {
public:
    TRateWriter(std::ofstream& out, int rate, int nch, int maxIn, int device) : Out(out), Rs(44100, rate, nch, maxIn, device) {}

    // the samples a decoded stream of n at 44.1 kHz gives at `rate`; -1 for an unsupported rate
    static int64_t Samples(int64_t n, int rate)
    {
        int32_t L = 0, M = 0;
        if (at3hip_resampler_shape(44100, rate, &L, &M, nullptr) != AT3HIP_OK) return -1;
        return (n * L + M - 1) / M;
    }
    void Write(const float* pcm, int32_t n)
    {
        Buf.clear();
        Rs.Process(pcm, n, Buf);
        Emit();
    }
    void Finish()
    {
        Buf.clear();
        Rs.Flush(Buf);
        Emit();
    }

private:
    void Emit()
    {
        S16.resize(Buf.size());
        for (size_t i = 0; i < Buf.size(); ++i) S16[i] = (int16_t)lrintf(std::min(1.0f, std::max(-1.0f, Buf[i])) * 32767.0f);
        Out.write((const char*)S16.data(), (std::streamsize)S16.size() * 2);   // little-endian host
    }
    std::ofstream& Out;
    TResampler Rs;
    std::vector<float> Buf;
    std::vector<int16_t> S16;
};

// The command line.
struct TOptions {
    std::string inFile, outFile, codec, container, rateArg;
    uint32_t bitrate = 0, bfuIdxConst = 0, winMask = 0;
    bool tones = false, gate = false, share = false, adaptive = false, sparse = false, rd = false, psy = false, noTonal = false, noGain = false, noStdOut = false, noTransient = false, decode = false, resample = false, measure = false, peakGiven = false;
    int batch = 256, device = 0, rate = 0;
    TLevel level;
};

// ---- `-d` -------------------------------------------------------------------------------------------------------------------
// One driver (run_decode) runs every decoder; a decoder is a description (TAt1Decode, TAt3Decode, TAt3pDecode below) with
//   Api, the C entry points' prefix, and Create / Decode / LastError / Destroy (/ GetCounters), the entry points themselves
//   Samples per frame and channel, FrameBytes per frame (every channel), Channels, Config(batch, device)
//   S16 / Float, the decode flags of the 16-bit output and of the float output that feeds --rate
//   InputLines, the banner's lines about the input, FrameText for "Can't read <FrameText>" (and Skipped, Reasons(counters))
//   Setup(decoder), run once on the new decoder: null, or the name of the call that failed
// nOut frames are decoded, nRead >= nOut are read, B at a time (0: an empty file, nothing to create); inspect(frames, n) sees
// every batch read, report(decoder) runs after the last one and ends the run with status 1 when it returns false.
template <typename D, typename TInspect, typename TReport>
int run_decode(const D& d, std::ifstream& in, const TOptions& o, int64_t nOut, int64_t nRead, int B, TInspect inspect, TReport report)
{
    if (!o.noStdOut)
        std::cout << "Input\n Filename: " << o.inFile << "\n" << d.InputLines << "\nOutput:\n Filename: " << o.outFile << "\n Codec: PCM" << std::endl;
    std::ofstream out(o.outFile, std::ios::binary);
    if (!out) return fatal("unable to open output file '" + o.outFile + "'");
    const uint32_t nch = (uint32_t)d.Channels;
    const int64_t nSamples = o.rate ? TRateWriter::Samples(nOut * D::Samples, o.rate) : nOut * D::Samples;
    if (nSamples * nch * 2 >= (int64_t)UINT32_MAX - 36) return fatal("output too long for a WAV file");
    write_wav_header(out, nch, (uint32_t)(nSamples * nch * 2), o.rate ? (uint32_t)o.rate : 44100u);
    if (B == 0) {
        if (!o.noStdOut) std::cout << "\nDone" << std::endl;
        return 0;
    }
    // (before the decoder: the converter may refuse, and nothing is then left to free)
    std::unique_ptr<TRateWriter> rw(o.rate ? new TRateWriter(out, o.rate, (int)nch, B * D::Samples, o.device) : nullptr);
    typename D::THandle* made = nullptr;
    const auto cfg = d.Config(B, o.device);
    int rc = D::Create(&cfg, &made);
    if (rc != AT3HIP_OK) return fatal(std::string(D::Api) + "_decoder_create failed (" + std::to_string(rc) + ")");
    const std::unique_ptr<typename D::THandle, void (*)(typename D::THandle*)> dec(made, D::Destroy);
    if (const char* failed = d.Setup(dec.get())) {   // what the description sets on the new decoder; the name of the call that failed
        std::cerr << "Fatal error: " << failed << ": " << D::LastError(dec.get()) << std::endl;
        return 1;
    }
    std::vector<uint8_t> frames((size_t)B * d.FrameBytes);
    std::vector<int16_t> pcm((size_t)B * D::Samples * nch);
    std::vector<float> pcmf(rw ? (size_t)B * D::Samples * nch : 0);
    for (int64_t f0 = 0; f0 < nRead; f0 += B) {
        const int n = (int)std::min<int64_t>(B, nRead - f0);
        if (!in.read((char*)frames.data(), (std::streamsize)n * d.FrameBytes)) return fatal(std::string("Can't read ") + D::FrameText);
        inspect(frames.data(), n);
        const int nDec = (int)std::min<int64_t>(n, nOut - f0);
        if (nDec <= 0) break;
        rc = rw ? D::Decode(dec.get(), frames.data(), nDec, pcmf.data(), D::Float) : D::Decode(dec.get(), frames.data(), nDec, pcm.data(), D::S16);
        if (rc != AT3HIP_OK) {
            std::cerr << "Encode/Decode error: " << D::Api << "_decode: " << D::LastError(dec.get()) << std::endl;
            return 1;
        }
        if (rw) rw->Write(pcmf.data(), nDec * D::Samples);
        else out.write((const char*)pcm.data(), (std::streamsize)nDec * D::Samples * nch * 2);   // little-endian host
    }
    if (rw) rw->Finish();
    if (!report(dec.get())) return 1;
    if (!o.noStdOut) std::cout << "\nDone" << std::endl;
    return 0;
}

// Report of the decoders that count what they reject: one line per reason that occurred.
template <typename D>
bool report_rejections(typename D::THandle* dec)
{
    typename D::TCounters c{};
    const int rc = D::GetCounters(dec, &c, 0);
    if (rc != AT3HIP_OK) {
        std::cerr << "Fatal error: " << D::Api << "_decoder_get_counters failed (" << rc << ")" << std::endl;
        return false;
    }
    for (const auto& r : D::Reasons(c))
        if (r.second) std::cerr << D::Skipped << " (" << r.first << "): " << r.second << std::endl;
    return true;
}

using TReasons = std::vector<std::pair<const char*, uint64_t>>;

// `-d`: TAtrac1Decoder behind TPCMEngine(4096, channels) with a TWav writer (main.cpp:343-365, 697-705).
//  * Length: TAeaInput::GetLengthInSamples = 512 * (units / channels - 5) (aea.cpp:98-108). The engine's ApplyProcess(512) runs
//    the lambda over its whole 4096-sample buffer, i.e. 8 frames per call, and the loop calls it until `processed` reaches that
//    length - at least once. A call whose frames are not all in the file throws TAeaIOError from ReadFrame: the tool reports it
//    and exits 1 with the complete calls written (the reference's behaviour when the count rounds past the file's end, and for
//    files of fewer than 5 frames, whose length wraps around).
//  * Output: 16-bit PCM WAV, 44100 Hz. The reference writes floats through libsndfile (pcm_io_sndfile.cpp:56,114) as
//    SF_FORMAT_WAV | SF_FORMAT_PCM_16 with normalisation, which stores lrintf(x * 32767.0f) behind a 44-byte canonical header.
//    That rule and the header are a restatement of libsndfile's documented behaviour, not pinned against it here; the float
//    samples the conversion starts from are pinned against the reference (tests/golden/at1_decode.npz).
struct TAt1Decode {
    using THandle = at1hip_decoder;
    static constexpr const char *Api = "at1hip", *FrameText = "AEA frame";
    static constexpr auto Create = at1hip_decoder_create;
    static constexpr auto Decode = at1hip_decode;
    static constexpr auto LastError = at1hip_decoder_last_error;
    static constexpr auto Destroy = at1hip_decoder_destroy;
    static constexpr int Samples = 512;
    static constexpr uint32_t S16 = AT1HIP_DECODE_S16, Float = 0;
    int Channels, FrameBytes;
    std::string InputLines;
    at1hip_decoder_config Config(int batch, int device) const { return {Channels, 1, batch, device}; }
    const char* Setup(THandle*) const { return nullptr; }
};

int decode_aea(std::ifstream& in, const TOptions& o)
{
    std::vector<char> hdr(2048);
    if (!in.read(hdr.data(), (std::streamsize)hdr.size())) return fatal("Can't read AEA header");
    if (!(hdr[0] == 0x00 && hdr[1] == 0x08 && hdr[2] == 0x00 && hdr[3] == 0x00 && hdr[264] < 3)) return fatal("invalid AEA header");   // TAeaInput::ReadMeta
    const int nch = hdr[264];
    if (nch < 1) return fatal("AEA header gives no channels");
    in.seekg(0, std::ios::end);
    const int64_t fileSize = (int64_t)in.tellg();
    in.seekg(2048, std::ios::beg);
    const int64_t frames = (fileSize - 2048) / AT1HIP_FRAME_SIZE / nch;   // whole frames in the file
    const int64_t calls = frames >= 5 ? std::max<int64_t>(1, (frames - 5 + 7) / 8) : INT64_MAX;
    const int64_t complete = std::min<int64_t>(calls, frames / 8);
    const int64_t nOut = 8 * complete;
    hdr[19] = 0;
    const TAt1Decode d{nch, nch * AT1HIP_FRAME_SIZE, " Name: " + std::string(&hdr[4]) + "\n Channels: " + std::to_string(nch)};
    // frames the failing call could still read report their faults before ReadFrame throws
    return run_decode(
        d, in, o, nOut, complete < calls ? frames : nOut, o.batch < 1 ? 1 : o.batch,
        [nch](const uint8_t* units, int n) {
            for (int i = 0; i < n * nch; ++i)
                if (const char* what = at1_unit_fault(units + (size_t)i * AT1HIP_FRAME_SIZE))
                    std::cerr << "Skipping invalid ATRAC1 frame: " << what << std::endl;
        },
        [&](at1hip_decoder*) {   // (no counters: the faults were reported per unit)
            if (complete < calls) std::cerr << "Aea IO fatal error: Can't read AEA frame" << std::endl;
            return complete >= calls;
        });
}

// `-d` on an ATRAC3 file: the container is recognised by content, as this repository's writers (at3hip_io.hpp) write it.
//  * OMA: "EA3" header of 96 bytes; the big-endian codec word at byte 32 holds the codec id (0 = ATRAC3, 1 = ATRAC3plus) in its
//    top byte, the joint-stereo flag in bit 17 and FrameSz / 8 in its low 10 bits; the frames follow.
//  * RIFF/WAVE with format tag 0x270: block_align is the frame size, the joint-stereo flag is the extradata's fifth 16-bit
//    word; the frames are the "data" chunk.
// Anything else goes to the AEA path unchanged, except ATRAC3plus (OMA codec id 1, RIFF 0xFFFE) and headerless ATRAC3 (the
// first byte carries the 6-bit unit id 0x28), which are refused. The output is a 16-bit stereo WAV written as the AEA path
// writes it, 1024 samples per frame, the codec delay not trimmed; rejected units are counted and reported per reason.
enum class EInput { AEA, ATRAC3, ATRAC3PLUS, REFUSED };

struct TAt3Input {
    int64_t offset = 0, frames = 0;
    int frameSize = 0, js = 0, channels = 2;
    std::string container;
};

uint32_t le(const uint8_t* p, int bytes)
{
    uint32_t v = 0;
    for (int i = bytes - 1; i >= 0; --i) v = (v << 8) | p[i];
    return v;
}

bool at3_row(int frameSize, int js)
{
    static const int rows[8][2] = {{192, 1}, {272, 1}, {304, 0}, {384, 0}, {424, 0}, {512, 0}, {768, 0}, {1024, 0}};
    for (const auto& r : rows)
        if (r[0] == frameSize && r[1] == js) return true;
    return false;
}

EInput probe_input(const std::string& inFile, TAt3Input& at3)
{
    std::ifstream in(inFile, std::ios::binary);
    if (!in) return EInput::AEA;   // main reports it
    uint8_t h[4096] = {0};
    in.read((char*)h, sizeof(h));
    const int64_t got = in.gcount();
    in.clear();
    in.seekg(0, std::ios::end);
    const int64_t fileSize = (int64_t)in.tellg();
    if (got >= 96 && !memcmp(h, "EA3", 3)) {
        const uint32_t word = (uint32_t)h[32] << 24 | (uint32_t)h[33] << 16 | (uint32_t)h[34] << 8 | h[35];
        const uint32_t id = word >> 24;
        if (id == 1) {   // ATRAC3plus: channel id in bits 10-12, (FrameSz - 8) / 8 in the low 10 bits
            const int chId = (int)((word >> 10) & 7), frameBytes = (int)(word & 0x3FF) * 8 + 8;
            if ((chId != 1 && chId != 2) || !at3p_rate_of_bytes(frameBytes) || (frameBytes == 192 && chId != 1)) {
                std::cerr << "Fatal error: ATRAC3plus decoding is not supported for channel id " << chId << ", frame size "
                          << frameBytes << std::endl;
                return EInput::REFUSED;
            }
            at3.container = "OMA";
            at3.offset = 96;
            at3.frameSize = frameBytes;
            at3.channels = chId;
            at3.frames = (fileSize - 96) / frameBytes;
            return EInput::ATRAC3PLUS;
        }
        if (id != 0) {
            std::cerr << "Fatal error: OMA codec id " << id << " is not ATRAC3" << std::endl;
            return EInput::REFUSED;
        }
        at3.container = "OMA";
        at3.offset = 96;
        at3.frameSize = (int)(word & 0x3FF) * 8;
        at3.js = (int)((word >> 17) & 1);
        at3.frames = at3.frameSize ? (fileSize - 96) / at3.frameSize : 0;
    } else if (got >= 12 && !memcmp(h, "RIFF", 4) && !memcmp(h + 8, "WAVE", 4)) {
        int64_t pos = 12, dataPos = -1, dataLen = 0;
        int tag = -1;
        bool at3pGuid = false;
        while (pos + 8 <= got) {
            const uint32_t sz = le(h + pos + 4, 4);
            if (!memcmp(h + pos, "fmt ", 4) && pos + 8 + 18 <= got) {
                tag = (int)le(h + pos + 8, 2);
                at3.channels = (int)le(h + pos + 10, 2);
                at3.frameSize = (int)le(h + pos + 20, 2);
                // WAVE_FORMAT_EXTENSIBLE: the ATRAC3plus sub-format GUID at byte 24 of the format (at3hip_io.hpp)
                static const uint8_t kAt3pGuid[16] = {0xBF, 0xAA, 0x23, 0xE9, 0x58, 0xCB, 0x71, 0x44,
                                                      0xA1, 0x19, 0xFF, 0xFA, 0x01, 0xE4, 0xCE, 0x62};
                if (tag == 0xFFFE && sz >= 40 && pos + 8 + 40 <= got) at3pGuid = !memcmp(h + pos + 8 + 24, kAt3pGuid, 16);
                if (tag == 0x270 && sz >= 32 && pos + 8 + 32 <= got) at3.js = (int)le(h + pos + 8 + 26, 2);
            } else if (!memcmp(h + pos, "data", 4)) {
                dataPos = pos + 8;
                dataLen = sz;
                break;
            }
            pos += 8 + sz + (sz & 1);
        }
        if (tag == 0xFFFE) {
            if (!at3pGuid || !at3p_rate_of_bytes(at3.frameSize) || (at3.channels != 1 && at3.channels != 2) || (at3.frameSize == 192 && at3.channels != 1)) {
                std::cerr << "Fatal error: ATRAC3plus decoding is not supported for " << (at3pGuid ? "" : "a sub-format other than ATRAC3plus, ")
                          << at3.channels << " channels, block align " << at3.frameSize << std::endl;
                return EInput::REFUSED;
            }
            if (dataPos < 0) {
                std::cerr << "Fatal error: RIFF ATRAC3plus file without a data chunk" << std::endl;
                return EInput::REFUSED;
            }
            at3.container = "RIFF";
            at3.offset = dataPos;
            at3.frames = std::min<int64_t>(dataLen, fileSize - dataPos) / at3.frameSize;
            return EInput::ATRAC3PLUS;
        }
        if (tag != 0x270) return EInput::AEA;
        if (dataPos < 0) {
            std::cerr << "Fatal error: RIFF ATRAC3 file without a data chunk" << std::endl;
            return EInput::REFUSED;
        }
        at3.container = "RIFF";
        at3.offset = dataPos;
        const int64_t avail = std::min<int64_t>(dataLen, fileSize - dataPos);
        at3.frames = at3.frameSize ? avail / at3.frameSize : 0;
    } else {
        if (got > 0 && (h[0] >> 2) == 0x28) {
            std::cerr << "Fatal error: raw ATRAC3 input is not supported (no container gives its frame size): "
                         "decode an OMA or RIFF (.at3 / .wav) file" << std::endl;
            return EInput::REFUSED;
        }
        return EInput::AEA;
    }
    if (!at3_row(at3.frameSize, at3.js)) {
        std::cerr << "Fatal error: unsupported ATRAC3 frame size " << at3.frameSize << (at3.js ? " with" : " without")
                  << " joint stereo" << std::endl;
        return EInput::REFUSED;
    }
    return EInput::ATRAC3;
}

struct TAt3Decode {
    using THandle = at3hip_decoder;
    using TCounters = at3hip_decoder_counters;
    static constexpr const char *Api = "at3hip", *FrameText = "ATRAC3 frame", *Skipped = "Skipped invalid ATRAC3 units";
    static constexpr auto Create = at3hip_decoder_create;
    static constexpr auto Decode = at3hip_decode;
    static constexpr auto LastError = at3hip_decoder_last_error;
    static constexpr auto GetCounters = at3hip_decoder_get_counters;
    static constexpr auto Destroy = at3hip_decoder_destroy;
    static constexpr int Samples = 1024;
    static constexpr uint32_t S16 = AT3HIP_DECODE_S16, Float = 0;
    int Channels = 2, FrameBytes, Js;
    std::string InputLines;

    explicit TAt3Decode(const TAt3Input& f)
        : FrameBytes(f.frameSize), Js(f.js),
          InputLines(" Container: " + f.container + "\n Codec: ATRAC3, frame size " + std::to_string(f.frameSize) + (f.js ? ", joint stereo" : ""))
    {
    }
    at3hip_decoder_config Config(int batch, int device) const { return {1, FrameBytes, Js, batch, device}; }
    const char* Setup(THandle*) const { return nullptr; }
    static TReasons Reasons(const TCounters& c)
    {
        return {{"wrong unit id", c.bad_id}, {"unsupported joint-stereo parameters", c.unsupported_js}, {"read past the end of the unit", c.read_past_end},
                {"tonal component past line 1023", c.tonal_past_end}, {"tonal coding mode", c.bad_tonal_mode}, {"tonal quantiser", c.bad_tonal_quant}};
    }
};

// `-d` on an ATRAC3plus OMA / RIFF file whose frame size is one of kAt3pRates': a 16-bit WAV with the stream's channel count, 2048 samples per frame, the codec delay
// (2416 samples) not trimmed; rejected frames are counted and reported per reason.
struct TAt3pDecode {
    using THandle = at3phip_decoder;
    using TCounters = at3phip_decoder_counters;
    static constexpr const char *Api = "at3phip", *FrameText = "ATRAC3plus frame", *Skipped = "Skipped invalid ATRAC3plus frames";
    static constexpr auto Create = at3phip_decoder_create;
    static constexpr auto Decode = at3phip_decode;
    static constexpr auto LastError = at3phip_decoder_last_error;
    static constexpr auto GetCounters = at3phip_decoder_get_counters;
    static constexpr auto Destroy = at3phip_decoder_destroy;
    static constexpr int Samples = 2048;
    // (tonal blocks and word length 0 inside the coded range are decoded, whatever wrote the file. The sparse parse tests every
    // unit's word length twice more: measured 3 % on the unpack-bound decode of 2048-byte frames, nothing at 376)
    static constexpr uint32_t S16 = AT3PHIP_DECODE_S16 | AT3PHIP_DECODE_TONES | AT3PHIP_DECODE_SPARSE, Float = AT3PHIP_DECODE_TONES | AT3PHIP_DECODE_SPARSE;
    int Channels, FrameBytes;
    std::string InputLines;

    explicit TAt3pDecode(const TAt3Input& f)
        : Channels(f.channels), FrameBytes(f.frameSize),
          InputLines(" Container: " + f.container + "\n Codec: ATRAC3plus, " + std::to_string(f.channels) + (f.channels == 1 ? " channel" : " channels"))
    {   // the bitrate, for every size but the one the line never named (a 2048-byte file prints what it always printed)
        if (f.frameSize != AT3PHIP_FRAME_BYTES)
            InputLines += ", " + std::to_string(at3p_rate_of_bytes(f.frameSize)->kbit) + " kbit/s (" + std::to_string(f.frameSize) + "-byte frames)";
    }
    at3phip_decoder_config Config(int batch, int device) const { return {Channels, 1, batch, device}; }
    const char* Setup(THandle* dec) const   // (a decoder at the default size is never told so)
    {
        return FrameBytes == AT3PHIP_FRAME_BYTES || at3phip_decoder_set_frame_bytes(dec, FrameBytes) == AT3HIP_OK ? nullptr : "at3phip_decoder_set_frame_bytes";
    }
    static TReasons Reasons(const TCounters& c)
    {
        return {{"bad header or block type", c.bad_header}, {"unsupported syntax element", c.unsupported_syntax},
                {"tonal block present", c.tonal_present}, {"invalid code or out-of-range value", c.bad_code},
                {"read past the end of the frame", c.read_past_end}, {"missing terminator", c.no_terminator}};
    }
};

// A file whose container gave the payload's offset and frame count (ATRAC3, ATRAC3plus): every frame is read and decoded,
// rejected ones are counted.
template <typename D>
int decode_container(const D& d, std::ifstream& in, const TAt3Input& f, const TOptions& o)
{
    in.seekg(f.offset, std::ios::beg);
    return run_decode(d, in, o, f.frames, f.frames, (int)std::min<int64_t>(o.batch < 1 ? 1 : o.batch, f.frames),
                      [](const uint8_t*, int) {}, report_rejections<D>);
}

// ---- `-e` -------------------------------------------------------------------------------------------------------------------
// The container of the output: what --container names, among `allowed`, or without it what `select` makes of the file's name.
EContainer container_of(const TOptions& o, EContainer (*select)(const std::string&), std::initializer_list<EContainer> allowed)
{
    static const std::pair<const char*, EContainer> names[] = {
        {"oma", EContainer::OMA}, {"riff", EContainer::RIFF}, {"raw", EContainer::RAW}, {"aea", EContainer::AEA}};
    if (o.container.empty()) return select(o.outFile);
    for (const auto& c : names)
        if (o.container == c.first && std::find(allowed.begin(), allowed.end(), c.second) != allowed.end()) return c.second;
    throw std::runtime_error("unrecognized container: " + o.container);
}

// One driver (encode) runs every encoder; an encoder is a description (TAtrac1Encode, TAtrac3Encode, TAtrac3PlusEncode below)
// made from the options and the input's channel count, with
//   Block, the samples of one ApplyProcess call, and NumFrames(samples, channels), the container header's estimate
//   CheckOptions(o): the codec's range messages, before the input is opened
//   Output(o, channels, numFrames), the container writer, and Encoder(out, o), the encoder object (at3hip_host.hpp)
//   InputLine and CodecLines(): the banner follows the reference's main.cpp, which differs between the codecs
//   Report(encoder, o): what the codec prints after the encode
struct TAtrac1Encode {
    static constexpr size_t Block = 512;
    static constexpr const char* InputLine = "Input";
    static uint64_t NumFrames(uint64_t samples, size_t channels) { return channels * samples / 512; }   // main.cpp:312
    static bool CheckOptions(const TOptions& o)
    {
        if (o.bfuIdxConst > 8) std::cerr << "ATRAC1 mode, --bfuidxconst is a index of max used BFU. Values [1;8] is allowed\n";
        return o.bfuIdxConst <= 8;
    }
    TAtrac1Encode(const TOptions&, size_t) {}
    TCompressedOutputPtr Output(const TOptions& o, size_t channels, uint32_t numFrames) const
    {
        return CreateAtrac1Output(container_of(o, SelectAtrac1Container, {EContainer::AEA, EContainer::RAW}), o.outFile, channels, numFrames);
    }
    std::string CodecLines() const { return "ATRAC1"; }
    TAtrac1Encoder Encoder(TCompressedOutputPtr&& out, const TOptions& o)
    {
        const auto mode = o.noTransient ? TAtrac1EncodeSettings::EWindowMode::EWM_NOTRANSIENT : TAtrac1EncodeSettings::EWindowMode::EWM_AUTO;
        return TAtrac1Encoder(std::move(out), TAtrac1EncodeSettings(o.bfuIdxConst, mode, o.winMask), o.batch, o.device);
    }
    void Report(TAtrac1Encoder&, const TOptions&) const {}
};

struct TAtrac3Encode {
    static constexpr size_t Block = 1024;
    static constexpr const char* InputLine = "Input:";
    static uint64_t NumFrames(uint64_t samples, size_t) { return samples / 1024; }
    static bool CheckOptions(const TOptions& o)
    {
        if (o.bitrate && (o.bitrate < 32 || o.bitrate > 384)) {
            std::cerr << "bitrate must be in [32;384]\n";
            return false;
        }
        if (o.bfuIdxConst > 32) std::cerr << "bfuidxconst must be in [1;32]\n";
        return o.bfuIdxConst <= 32;
    }
    TAtrac3EncoderSettings Settings;
    uint32_t FrameSize = 0;
    bool Js = false;

    TAtrac3Encode(const TOptions& o, size_t channels)
    {
        Settings.Bitrate = o.bitrate * 1024;   // the tool's kbit value reaches the settings as value * 1024 (main.cpp:676)
        Settings.NoGainControll = o.noGain;
        Settings.NoTonalComponents = o.noTonal;
        Settings.SourceChannels = (uint8_t)channels;
        Settings.BfuIdxConst = o.bfuIdxConst;
        // container parameters come from the encoder context (GetContainerParamsForBitrate)
        at3hip_config probe{};
        probe.bitrate = (int32_t)Settings.Bitrate;
        probe.channels = (int32_t)channels;
        probe.n_streams = 1;
        probe.max_blocks = 1;
        probe.device_id = o.device;
        at3hip_ctx* pc = nullptr;
        Check(at3hip_create(&probe, &pc), nullptr, "at3hip_create");
        FrameSize = (uint32_t)at3hip_frame_size(pc);
        Js = at3hip_joint_stereo(pc) != 0;
        at3hip_destroy(pc);
    }
    TCompressedOutputPtr Output(const TOptions& o, size_t channels, uint32_t numFrames) const
    {
        const EContainer c = container_of(o, SelectAtrac3Container, {EContainer::OMA, EContainer::RIFF, EContainer::RAW});
        return CreateAtrac3Output(c, o.outFile, channels, numFrames, FrameSize, Js);
    }
    std::string CodecLines() const { return "ATRAC3\n Bitrate: " + std::to_string(FrameSize == 384 ? 132300 : FrameSize * 44100u * 8u / 1024u); }
    TAtrac3Encoder Encoder(TCompressedOutputPtr&& out, const TOptions& o) { return TAtrac3Encoder(std::move(out), std::move(Settings), o.batch, o.device); }
    void Report(TAtrac3Encoder& encoder, const TOptions& o) const
    {
        if (!o.level.On || o.noStdOut) return;   // what TScaler::Scale would still have clamped after the gain (at3hip_get_counters)
        const at3hip_counters c = encoder.Counters();
        std::cout << "clipping: " << c.scale_overflow << " blocks, " << c.clipped_values << " values" << std::endl;
    }
};

struct TAtrac3PlusEncode {
    static constexpr size_t Block = 2048;
    static constexpr const char* InputLine = "Input:";
    static uint64_t NumFrames(uint64_t samples, size_t) { return samples / 2048; }   // main.cpp:440
    static bool CheckOptions(const TOptions& o)
    {
        if (!o.bitrate) return true;
        const TAt3pRate* r = at3p_rate_of_kbit((int)o.bitrate);
        if (!r) {
            std::cerr << "ATRAC3plus mode, --bitrate takes one of: " << at3p_rate_table() << "\n";
            return false;
        }
        if (r->frameBytes != AT3PHIP_FRAME_BYTES && !o.adaptive) {
            std::cerr << "--bitrate " << r->kbit << " needs --adaptive: the fixed word-length table is defined for 2048-byte frames (352 kbit/s) only, "
                      << "and only the adaptive writer chooses word lengths that fit a frame of " << r->frameBytes << " bytes\n";
            return false;
        }
        return true;
    }
    size_t Channels;
    const TAt3pRate* Rate;   // null: no --bitrate, 2048-byte frames

    TAtrac3PlusEncode(const TOptions& o, size_t channels) : Channels(channels), Rate(o.bitrate ? at3p_rate_of_kbit((int)o.bitrate) : nullptr)
    {
        if (Rate && Rate->kbit == 32 && channels != 1) throw std::runtime_error("--bitrate 32 is a mono rate: the input has " + std::to_string(channels) + " channels");
    }
    uint32_t FrameBytes() const { return Rate ? (uint32_t)Rate->frameBytes : (uint32_t)AT3PHIP_FRAME_BYTES; }
    TCompressedOutputPtr Output(const TOptions& o, size_t channels, uint32_t numFrames) const
    {
        const EContainer c = container_of(o, SelectAtrac3PlusContainer, {EContainer::OMA, EContainer::RIFF, EContainer::RAW});
        return CreateAtrac3PlusOutput(c, o.outFile, channels, numFrames, FrameBytes());
    }
    std::string CodecLines() const
    {
        return Rate ? "ATRAC3Plus\n Bitrate: " + std::to_string(Rate->kbit) + " kbit/s (" + std::to_string(Rate->frameBytes) + "-byte frames)" : "ATRAC3Plus";
    }
    TAt3PEncoder Encoder(TCompressedOutputPtr&& out, const TOptions& o)
    {   // --tones: the tone analysis of at3phip_encode_frames_tonal (--gate: with AT3PHIP_TONES_GATED, --share: with AT3PHIP_TONES_SHARED); the frame count is the plain encode's
        return TAt3PEncoder(std::move(out), (int)Channels, o.batch > 64 ? 64 : o.batch, o.device, TAt3PSettings(), nullptr, o.tones, o.gate, o.share, o.adaptive,
                            (int)FrameBytes(), o.sparse, o.rd, o.psy);
    }
    void Report(TAt3PEncoder&, const TOptions&) const {}
};

template <typename TCodec>
int encode(const TOptions& o)
{
    if (!TCodec::CheckOptions(o)) return 1;
    try {
        TEncodeInput wav(o.inFile, o.resample, o.device, o.level);
        const size_t numChannels = wav.GetChannelNum();
        const uint64_t totalSamples = wav.GetTotalSamples();
        TCodec codec(o, numChannels);
        TCompressedOutputPtr out = codec.Output(o, numChannels, (uint32_t)TCodec::NumFrames(totalSamples, numChannels));
        if (!o.noStdOut)
            std::cout << TCodec::InputLine << "\n Filename: " << o.inFile << "\n Channels: " << numChannels << "\n SampleRate: " << wav.GetSampleRate()
                      << "\n Duration (sec): " << totalSamples / wav.GetSampleRate() << "\nOutput:\n Filename: " << o.outFile
                      << "\n Codec: " << codec.CodecLines() << std::endl;
        TPCMEngine engine(4096, numChannels, [&wav](float* dst, size_t frames) { return wav.Read(dst, frames); });
        auto encoder = codec.Encoder(std::move(out), o);
        auto lambda = encoder.GetLambda();
        try {
            while (totalSamples > engine.ApplyProcess(TCodec::Block, lambda)) {
            }
        } catch (const TNoDataToRead&) {
            std::cerr << "No more data to read from input" << std::endl;
        }
        encoder.Flush();
        codec.Report(encoder, o);
        wav.Report(o.level);
        if (!o.noStdOut) std::cout << "\nDone" << std::endl;
    } catch (const std::exception& ex) {
        return fatal(ex.what());
    }
    return 0;
}

}  // namespace

static int usage()
{
    std::cerr << "usage: at3hipenc -e atrac3 -i in.wav -o out.oma [--bitrate kbit] [--bfuidxconst n] [--notonal] [--nogaincontrol]\n"
                 "                 [--container oma|riff|raw] [--nostdout] [--batch blocks] [--device n]\n"
                 "       at3hipenc -e atrac1 -i in.wav -o out.aea [--bfuidxconst 1..8] [--notransient[=mask]]\n"
                 "                 [--container aea|raw] [--nostdout] [--batch blocks] [--device n]\n"
                 "       at3hipenc -e atrac3plus -i in.wav -o out.oma [--adaptive [--sparse [--rd [--psy]]] [--bitrate kbit]] [--tones [--gate] [--share]] [--container oma|riff|raw] [--nostdout] [--batch frames] [--device n]\n"
                 "                 (--adaptive: word lengths chosen per frame on the GPU to fill the frame, instead of the fixed table)\n"
                 "                 (--sparse: with --adaptive, a quant unit inside the coded range may get no bits at all; for the low bitrates)\n"
                 "                 (--rd: with --adaptive --sparse, each unit's word length is chosen by rate and distortion instead of by its peak)\n"
                 "                 (--psy: with --adaptive --sparse --rd, a unit under the threshold in quiet or next to a loud one pays more for a bit)\n"
                 "                 (--bitrate: 32 (mono), 48, 64, 96, 128, 160, 192, 256, 320 or 352 kbit/s; below 352 with --adaptive only)\n"
                 "                 (--tones: find sine waves on the GPU and write them as tonal blocks; --gate: with envelope points at\n"
                 "                  their onsets and offsets; --share: a band that both channels of a stereo input hold identically is\n"
                 "                  written once)\n"
                 "       (every encoder: --resample converts an input at 8 .. 192 kHz to 44.1 kHz first)\n"
                 "       (every encoder: --loudness LUFS [--peak dBFS] [--truepeak] brings the input to a programme loudness first;\n"
                 "        with --limit the gain reaches the target and a look-ahead limiter holds the peak)\n"
                 "       at3hipenc --measure -i in.wav [--resample] [--truepeak]   (prints loudness and peaks, writes nothing)\n"
                 "       at3hipenc -d -i in.aea -o out.wav [--nostdout] [--batch frames] [--device n]\n"
                 "       at3hipenc -d -i in.{oma|at3|wav} -o out.wav [--nostdout] [--batch frames] [--device n]   (ATRAC3 / ATRAC3plus, by content)\n"
                 "                 (ATRAC3plus: any frame size of the --bitrate table; the codec line names the bitrate except at 352 kbit/s)\n"
                 "       (every decoder: --rate hz writes the WAV at 8 .. 192 kHz instead of 44.1 kHz)\n";
    return 1;
}

int main(int argc, char** argv)
{
    TOptions o;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* what) -> const char* {
            if (i + 1 >= argc) {
                std::cerr << "missing value for " << what << "\n";
                exit(usage());
            }
            return argv[++i];
        };
        if (a == "-e" || a == "--encode") o.codec = need("-e");
        else if (a == "-d" || a == "--decode") o.decode = true;
        else if (a == "-i") o.inFile = need("-i");
        else if (a == "-o") o.outFile = need("-o");
        else if (a == "--bitrate") o.bitrate = (uint32_t)atoi(need("--bitrate"));
        else if (a == "--bfuidxconst") o.bfuIdxConst = (uint32_t)atoi(need("--bfuidxconst"));
        else if (a == "--notonal") o.noTonal = true;
        else if (a == "--tones") o.tones = true;
        else if (a == "--gate") o.gate = true;
        else if (a == "--share") o.share = true;
        else if (a == "--adaptive") o.adaptive = true;
        else if (a == "--sparse") o.sparse = true;
        else if (a == "--rd") o.rd = true;
        else if (a == "--psy") o.psy = true;
        else if (a == "--nogaincontrol") o.noGain = true;
        else if (a == "--nostdout") o.noStdOut = true;
        else if (a == "--resample") o.resample = true;
        else if (a == "--loudness") {
            o.level.On = true;
            o.level.Target = atof(need("--loudness"));
        }
        else if (a == "--peak") {
            o.peakGiven = true;
            o.level.Ceiling = atof(need("--peak"));
        }
        else if (a == "--truepeak") o.level.TruePeak = true;
        else if (a == "--limit") o.level.Limit = true;
        else if (a == "--measure") o.measure = true;
        else if (a == "--rate") {   // a positive decimal number, else refused below as an unsupported rate
            const char* v = need("--rate");
            o.rateArg = v;
            char* end = nullptr;
            const long x = strtol(v, &end, 10);
            o.rate = (*v && !*end && x > 0 && x <= 1000000) ? (int)x : -1;
        }
        else if (a.rfind("--notransient", 0) == 0 && (a.size() == 13 || a[13] == '=')) {   // optional_argument, main.cpp:568-577
            o.noTransient = true;
            if (a.size() > 14) o.winMask = (uint32_t)atoi(a.c_str() + 14);
        }
        else if (a == "--container") o.container = need("--container");
        else if (a == "--batch") o.batch = atoi(need("--batch"));
        else if (a == "--device") o.device = atoi(need("--device"));
        else return usage();
    }
    o.level.NoStdOut = o.noStdOut;
    if (o.measure) {   // prints the meter's result, writes nothing
        if (o.decode || !o.codec.empty() || o.inFile.empty() || !o.outFile.empty() || o.level.On || o.level.Limit || o.peakGiven || o.rate || o.adaptive || o.sparse || o.rd || o.psy) return usage();
        try {
            const at3hip_loudness_result r = measure_input(o.inFile, o.resample, o.device, o.level.TruePeak);
            char line[256];
            int n = snprintf(line, sizeof(line), "loudness: I %.2f LUFS, M max %.2f LUFS, S max %.2f LUFS, sample peak %.2f dBFS", r.integrated,
                             r.momentary_max, r.short_term_max, db_of((double)std::max(r.sample_peak[0], r.sample_peak[1])));
            if (o.level.TruePeak)
                snprintf(line + n, sizeof(line) - (size_t)n, ", true peak %.2f dBFS", db_of((double)std::max(r.true_peak[0], r.true_peak[1])));
            std::cout << line << std::endl;
        } catch (const std::exception& ex) {
            return fatal(ex.what());
        }
        return 0;
    }
    if (o.decode) {
        if (!o.codec.empty() || o.inFile.empty() || o.outFile.empty() || o.level.On || o.level.Limit || o.peakGiven || o.level.TruePeak || o.adaptive || o.sparse || o.rd || o.psy) return usage();
        TAt3Input at3;
        const EInput kind = probe_input(o.inFile, at3);
        if (kind == EInput::REFUSED) return 1;
        if (o.rate == 44100) o.rate = 0;   // the decoders' own rate: written as without --rate
        if (o.rate && TRateWriter::Samples(0, o.rate) < 0) return fatal("unsupported output rate " + o.rateArg + " (at3hip_resample.h lists the rates)");
        std::ifstream in(o.inFile, std::ios::binary);
        if (!in) return fatal("unable to open input file '" + o.inFile + "'");
        try {
            if (kind == EInput::ATRAC3) return decode_container(TAt3Decode(at3), in, at3, o);
            if (kind == EInput::ATRAC3PLUS) return decode_container(TAt3pDecode(at3), in, at3, o);
            return decode_aea(in, o);
        } catch (const std::exception& ex) {
            return fatal(ex.what());
        }
    }
    if ((o.codec != "atrac3" && o.codec != "atrac1" && o.codec != "atrac3plus") || o.inFile.empty() || o.outFile.empty() || o.rate) return usage();
    if (!o.level.On && (o.peakGiven || o.level.TruePeak || o.level.Limit)) return usage();   // --peak, --truepeak and --limit belong to --loudness (--truepeak also to --measure)
    if ((o.gate || o.share) && !o.tones) return usage();      // the gates and the sharing are the tone analysis'
    if (o.tones && o.codec != "atrac3plus") return usage();   // the tone analysis is ATRAC3plus'
    if (o.adaptive && o.codec != "atrac3plus") return usage();   // and so are the adaptive word lengths
    if (o.psy && !(o.adaptive && o.sparse && o.rd)) {
        std::cerr << "--psy needs --adaptive --sparse --rd: the masking threshold weights the rate-distortion choice and is nothing without it\n";
        return usage();
    }
    if (o.rd && !(o.adaptive && o.sparse)) {
        std::cerr << "--rd needs --adaptive --sparse: the rate-distortion choice may give a quant unit inside the coded range word length 0\n";
        return usage();
    }
    if (o.sparse && !o.adaptive) {
        std::cerr << "--sparse needs --adaptive: word length 0 inside the coded range is a choice of the adaptive writer, the fixed table has none\n";
        return usage();
    }
    if (o.codec == "atrac3plus") return encode<TAtrac3PlusEncode>(o);
    if (o.codec == "atrac1") return encode<TAtrac1Encode>(o);
    return encode<TAtrac3Encode>(o);
}
