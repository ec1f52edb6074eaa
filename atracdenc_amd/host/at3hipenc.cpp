// at3hipenc - command-line ATRAC3 / ATRAC1 / ATRAC3plus encoder on libat3hip: the
// reference tool's `-e atrac3` path (main.cpp:367-425, 659-705), `-e atrac1` path (main.cpp:292-345, 630-648) and
// `-e atrac3plus` path (main.cpp:427-483, 679-686; without the tonal analysis, which needs libgha) with the GPU encoders
// behind the same IProcessor-shaped objects.
//
//   at3hipenc -e atrac3 -i in.wav -o out.{oma|at3|wav|raw|dat} [--bitrate kbit] [--bfuidxconst n] [--notonal]
//             [--nogaincontrol] [--container oma|riff|raw] [--nostdout] [--batch blocks] [--device n]
//   at3hipenc -e atrac1 -i in.wav -o out.{aea|raw|dat} [--bfuidxconst 1..8] [--notransient[=mask]]
//             [--container aea|raw] [--nostdout] [--batch blocks] [--device n]
//   at3hipenc -e atrac3plus -i in.wav -o out.{oma|at3|wav|raw|dat} [--container oma|riff|raw] [--nostdout]
//             [--batch frames] [--device n]
//   at3hipenc -d -i in.aea -o out.wav [--nostdout] [--batch frames] [--device n]
//             the reference's ATRAC1 decode path (main.cpp:343-365, 697-705) on the GPU decoder (at1hip.h)
//
// File-level behaviour follows the reference: 44.1 kHz input only, numFrames estimate = samples / 1024 in the
// container header, the look-ahead first call, the drain call at end of input.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include <cstdint>
#include <fstream>
#include <vector>

#include "../../include/at1hip.h"
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

void put_le(std::vector<char>& h, uint32_t v, int bytes)
{
    for (int i = 0; i < bytes; ++i) h.push_back((char)((v >> (8 * i)) & 0xff));
}

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
int decode_aea(const std::string& inFile, const std::string& outFile, bool noStdOut, int batch, int device)
{
    std::ifstream in(inFile, std::ios::binary);
    if (!in) {
        std::cerr << "Fatal error: unable to open input file '" << inFile << "'" << std::endl;
        return 1;
    }
    std::vector<char> hdr(2048);
    if (!in.read(hdr.data(), (std::streamsize)hdr.size())) {
        std::cerr << "Fatal error: Can't read AEA header" << std::endl;
        return 1;
    }
    if (!(hdr[0] == 0x00 && hdr[1] == 0x08 && hdr[2] == 0x00 && hdr[3] == 0x00 && hdr[264] < 3)) {   // TAeaInput::ReadMeta
        std::cerr << "Fatal error: invalid AEA header" << std::endl;
        return 1;
    }
    const int nch = hdr[264];
    if (nch < 1) {
        std::cerr << "Fatal error: AEA header gives no channels" << std::endl;
        return 1;
    }
    in.seekg(0, std::ios::end);
    const int64_t fileSize = (int64_t)in.tellg();
    in.seekg(2048, std::ios::beg);
    const int64_t frames = (fileSize - 2048) / AT1HIP_FRAME_SIZE / nch;   // whole frames in the file
    const int64_t calls = frames >= 5 ? std::max<int64_t>(1, (frames - 5 + 7) / 8) : INT64_MAX;
    const int64_t complete = std::min<int64_t>(calls, frames / 8);
    const int64_t nOut = 8 * complete;
    if (!noStdOut) {
        hdr[19] = 0;
        std::cout << "Input\n Filename: " << inFile << "\n Name: " << std::string(&hdr[4]) << "\n Channels: " << nch
                  << "\nOutput:\n Filename: " << outFile << "\n Codec: PCM" << std::endl;
    }
    std::ofstream out(outFile, std::ios::binary);
    if (!out) {
        std::cerr << "Fatal error: unable to open output file '" << outFile << "'" << std::endl;
        return 1;
    }
    const uint32_t dataBytes = (uint32_t)(nOut * 512 * nch * 2);
    std::vector<char> wav;
    wav.insert(wav.end(), {'R', 'I', 'F', 'F'});
    put_le(wav, 36 + dataBytes, 4);
    wav.insert(wav.end(), {'W', 'A', 'V', 'E', 'f', 'm', 't', ' '});
    put_le(wav, 16, 4);
    put_le(wav, 1, 2);   // PCM
    put_le(wav, (uint32_t)nch, 2);
    put_le(wav, 44100, 4);
    put_le(wav, 44100u * 2u * (uint32_t)nch, 4);
    put_le(wav, 2u * (uint32_t)nch, 2);
    put_le(wav, 16, 2);
    wav.insert(wav.end(), {'d', 'a', 't', 'a'});
    put_le(wav, dataBytes, 4);
    out.write(wav.data(), (std::streamsize)wav.size());

    const int B = batch < 1 ? 1 : batch;
    at1hip_decoder* dec = nullptr;
    at1hip_decoder_config cfg{nch, 1, B, device};
    int rc = at1hip_decoder_create(&cfg, &dec);
    if (rc != AT3HIP_OK) {
        std::cerr << "Fatal error: at1hip_decoder_create failed (" << rc << ")" << std::endl;
        return 1;
    }
    // frames the failing call could still read report their faults before ReadFrame throws
    const int64_t nReport = complete < calls ? frames : nOut;
    std::vector<uint8_t> units((size_t)B * nch * AT1HIP_FRAME_SIZE);
    std::vector<int16_t> pcm((size_t)B * 512 * nch);
    for (int64_t f0 = 0; f0 < nReport; f0 += B) {
        const int n = (int)std::min<int64_t>(B, nReport - f0);
        in.read((char*)units.data(), (std::streamsize)n * nch * AT1HIP_FRAME_SIZE);
        for (int i = 0; i < n * nch; ++i)
            if (const char* what = at1_unit_fault(&units[(size_t)i * AT1HIP_FRAME_SIZE]))
                std::cerr << "Skipping invalid ATRAC1 frame: " << what << std::endl;
        const int nDec = (int)std::min<int64_t>(n, nOut - f0);
        if (nDec <= 0) break;
        rc = at1hip_decode(dec, units.data(), nDec, pcm.data(), AT1HIP_DECODE_S16);
        if (rc != AT3HIP_OK) {
            std::cerr << "Encode/Decode error: at1hip_decode: " << at1hip_decoder_last_error(dec) << std::endl;
            at1hip_decoder_destroy(dec);
            return 1;
        }
        out.write((const char*)pcm.data(), (std::streamsize)nDec * 512 * nch * 2);   // little-endian host
    }
    at1hip_decoder_destroy(dec);
    if (complete < calls) {
        std::cerr << "Aea IO fatal error: Can't read AEA frame" << std::endl;
        return 1;
    }
    if (!noStdOut) std::cout << "\nDone" << std::endl;
    return 0;
}

}  // namespace

static int usage()
{
    std::cerr << "usage: at3hipenc -e atrac3 -i in.wav -o out.oma [--bitrate kbit] [--bfuidxconst n] [--notonal] [--nogaincontrol]\n"
                 "                 [--container oma|riff|raw] [--nostdout] [--batch blocks] [--device n]\n"
                 "       at3hipenc -e atrac1 -i in.wav -o out.aea [--bfuidxconst 1..8] [--notransient[=mask]]\n"
                 "                 [--container aea|raw] [--nostdout] [--batch blocks] [--device n]\n"
                 "       at3hipenc -e atrac3plus -i in.wav -o out.oma [--container oma|riff|raw] [--nostdout] [--batch frames] [--device n]\n"
                 "       at3hipenc -d -i in.aea -o out.wav [--nostdout] [--batch frames] [--device n]\n";
    return 1;
}

int main(int argc, char** argv)
{
    std::string inFile, outFile, codec, container;
    uint32_t bitrate = 0, bfuIdxConst = 0;
    bool noTonal = false, noGain = false, noStdOut = false, noTransient = false, decode = false;
    uint32_t winMask = 0;
    int batch = 256, device = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* what) -> const char* {
            if (i + 1 >= argc) {
                std::cerr << "missing value for " << what << "\n";
                exit(usage());
            }
            return argv[++i];
        };
        if (a == "-e" || a == "--encode") codec = need("-e");
        else if (a == "-d" || a == "--decode") decode = true;
        else if (a == "-i") inFile = need("-i");
        else if (a == "-o") outFile = need("-o");
        else if (a == "--bitrate") bitrate = (uint32_t)atoi(need("--bitrate"));
        else if (a == "--bfuidxconst") bfuIdxConst = (uint32_t)atoi(need("--bfuidxconst"));
        else if (a == "--notonal") noTonal = true;
        else if (a == "--nogaincontrol") noGain = true;
        else if (a == "--nostdout") noStdOut = true;
        else if (a.rfind("--notransient", 0) == 0 && (a.size() == 13 || a[13] == '=')) {   // optional_argument, main.cpp:568-577
            noTransient = true;
            if (a.size() > 14) winMask = (uint32_t)atoi(a.c_str() + 14);
        }
        else if (a == "--container") container = need("--container");
        else if (a == "--batch") batch = atoi(need("--batch"));
        else if (a == "--device") device = atoi(need("--device"));
        else return usage();
    }
    if (decode) {
        if (!codec.empty() || inFile.empty() || outFile.empty()) return usage();
        return decode_aea(inFile, outFile, noStdOut, batch, device);
    }
    if ((codec != "atrac3" && codec != "atrac1" && codec != "atrac3plus") || inFile.empty() || outFile.empty()) return usage();
    if (codec == "atrac3plus") {
        try {
            TWavSource wav(inFile);
            if (wav.GetSampleRate() != 44100) throw std::runtime_error("unsupported sample rate");
            const size_t numChannels = wav.GetChannelNum();
            const uint64_t totalSamples = wav.GetTotalSamples();
            const uint64_t numFrames = totalSamples / 2048;   // main.cpp:440
            EContainer cont;
            if (container.empty()) cont = SelectAtrac3PlusContainer(outFile);
            else if (container == "oma") cont = EContainer::OMA;
            else if (container == "riff") cont = EContainer::RIFF;
            else if (container == "raw") cont = EContainer::RAW;
            else throw std::runtime_error("unrecognized container: " + container);
            TCompressedOutputPtr out = CreateAtrac3PlusOutput(cont, outFile, numChannels, (uint32_t)numFrames, 2048);
            if (!noStdOut)
                std::cout << "Input:\n Filename: " << inFile << "\n Channels: " << numChannels << "\n SampleRate: " << wav.GetSampleRate()
                          << "\n Duration (sec): " << totalSamples / wav.GetSampleRate() << "\nOutput:\n Filename: " << outFile
                          << "\n Codec: ATRAC3Plus" << std::endl;
            TPCMEngine engine(4096, numChannels, [&wav](float* dst, size_t frames) { return wav.Read(dst, frames); });
            TAt3PEncoder encoder(std::move(out), (int)numChannels, batch > 64 ? 64 : batch, device);
            auto lambda = encoder.GetLambda();
            uint64_t processed = 0;
            try {
                while (totalSamples > (processed = engine.ApplyProcess(2048, lambda))) {
                }
            } catch (const TNoDataToRead&) {
                std::cerr << "No more data to read from input" << std::endl;
            }
            encoder.Flush();
            if (!noStdOut) std::cout << "\nDone" << std::endl;
        } catch (const std::exception& ex) {
            std::cerr << "Fatal error: " << ex.what() << std::endl;
            return 1;
        }
        return 0;
    }
    if (codec == "atrac1") {
        if (bfuIdxConst > 8) {
            std::cerr << "ATRAC1 mode, --bfuidxconst is a index of max used BFU. Values [1;8] is allowed\n";
            return 1;
        }
        try {
            TWavSource wav(inFile);
            if (wav.GetSampleRate() != 44100) throw std::runtime_error("unsupported sample rate");
            const size_t numChannels = wav.GetChannelNum();
            const uint64_t totalSamples = wav.GetTotalSamples();
            const uint64_t numFrames = numChannels * totalSamples / 512;   // main.cpp:312
            EContainer cont;
            if (container.empty()) cont = SelectAtrac1Container(outFile);
            else if (container == "aea") cont = EContainer::AEA;
            else if (container == "raw") cont = EContainer::RAW;
            else throw std::runtime_error("unrecognized container: " + container);
            TCompressedOutputPtr out = CreateAtrac1Output(cont, outFile, numChannels, (uint32_t)numFrames);
            if (!noStdOut)
                std::cout << "Input\n Filename: " << inFile << "\n Channels: " << numChannels << "\n SampleRate: " << wav.GetSampleRate()
                          << "\n Duration (sec): " << totalSamples / wav.GetSampleRate() << "\nOutput:\n Filename: " << outFile
                          << "\n Codec: ATRAC1" << std::endl;
            TPCMEngine engine(4096, numChannels, [&wav](float* dst, size_t frames) { return wav.Read(dst, frames); });
            TAtrac1Encoder encoder(std::move(out),
                                   TAtrac1EncodeSettings(bfuIdxConst,
                                                         noTransient ? TAtrac1EncodeSettings::EWindowMode::EWM_NOTRANSIENT
                                                                     : TAtrac1EncodeSettings::EWindowMode::EWM_AUTO,
                                                         winMask),
                                   batch, device);
            auto lambda = encoder.GetLambda();
            uint64_t processed = 0;
            try {
                while (totalSamples > (processed = engine.ApplyProcess(512, lambda))) {
                }
            } catch (const TNoDataToRead&) {
                std::cerr << "No more data to read from input" << std::endl;
            }
            encoder.Flush();
            if (!noStdOut) std::cout << "\nDone" << std::endl;
        } catch (const std::exception& ex) {
            std::cerr << "Fatal error: " << ex.what() << std::endl;
            return 1;
        }
        return 0;
    }
    if (bitrate && (bitrate < 32 || bitrate > 384)) {
        std::cerr << "bitrate must be in [32;384]\n";
        return 1;
    }
    if (bfuIdxConst > 32) {
        std::cerr << "bfuidxconst must be in [1;32]\n";
        return 1;
    }
    try {
        TWavSource wav(inFile);
        if (wav.GetSampleRate() != 44100) throw std::runtime_error("unsupported sample rate");
        const size_t numChannels = wav.GetChannelNum();
        const uint64_t totalSamples = wav.GetTotalSamples();
        const uint64_t numFrames = totalSamples / 1024;

        TAtrac3EncoderSettings settings;
        settings.Bitrate = bitrate * 1024;   // the tool's kbit value reaches the settings as value * 1024 (main.cpp:676)
        settings.NoGainControll = noGain;
        settings.NoTonalComponents = noTonal;
        settings.SourceChannels = (uint8_t)numChannels;
        settings.BfuIdxConst = bfuIdxConst;

        // container parameters come from the encoder context (GetContainerParamsForBitrate)
        at3hip_config probe{};
        probe.bitrate = (int32_t)settings.Bitrate;
        probe.channels = (int32_t)numChannels;
        probe.n_streams = 1;
        probe.max_blocks = 1;
        probe.device_id = device;
        at3hip_ctx* pc = nullptr;
        Check(at3hip_create(&probe, &pc), nullptr, "at3hip_create");
        const uint32_t frameSize = (uint32_t)at3hip_frame_size(pc);
        const bool js = at3hip_joint_stereo(pc) != 0;
        at3hip_destroy(pc);

        EContainer cont;
        if (container.empty()) cont = SelectAtrac3Container(outFile);
        else if (container == "oma") cont = EContainer::OMA;
        else if (container == "riff") cont = EContainer::RIFF;
        else if (container == "raw") cont = EContainer::RAW;
        else throw std::runtime_error("unrecognized container: " + container);

        TCompressedOutputPtr out = CreateAtrac3Output(cont, outFile, numChannels, (uint32_t)numFrames, frameSize, js);
        if (!noStdOut)
            std::cout << "Input:\n Filename: " << inFile << "\n Channels: " << numChannels << "\n SampleRate: " << wav.GetSampleRate()
                      << "\n Duration (sec): " << totalSamples / wav.GetSampleRate() << "\nOutput:\n Filename: " << outFile
                      << "\n Codec: ATRAC3\n Bitrate: " << (frameSize == 384 ? 132300 : frameSize * 44100u * 8u / 1024u) << std::endl;

        TPCMEngine engine(4096, numChannels, [&wav](float* dst, size_t frames) { return wav.Read(dst, frames); });
        TAtrac3Encoder encoder(std::move(out), std::move(settings), batch, device);
        auto lambda = encoder.GetLambda();
        uint64_t processed = 0;
        try {
            while (totalSamples > (processed = engine.ApplyProcess(1024, lambda))) {
            }
        } catch (const TNoDataToRead&) {
            std::cerr << "No more data to read from input" << std::endl;
        }
        encoder.Flush();
        if (!noStdOut) std::cout << "\nDone" << std::endl;
    } catch (const std::exception& ex) {
        std::cerr << "Fatal error: " << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
