"""Helpers of the tonal-block WRITER tests and their golden generator (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports
this module).

  * WRITER_CASES / writer_case: the cases of at3phip_write_frames_tonal, 2 streams x 3 frames each with a frame without a block
    between two with one; spectra are regenerated from a seed, blocks are stored in the golden as flat ints.
  * ref_write_tonal_win: the REFERENCE's TAt3PBitStream::WriteFrame with hand-built TAt3PGhaData and window flags, through a
    driver compiled at generation time (at3p_tonal_lib.ref_write_tonal's, which takes no window flags, with the flags added).
  * ref_schedule: the REFERENCE's own TAt3PEnc (atrac/at3p/at3p.cpp, compiled at generation time) around the deterministic
    stand-in analyser tests/host/at3p_fake_gha.h, for a UseGha flag combination.
Nothing of the reference is stored in the repository.
"""
import os
import subprocess
import tempfile

import numpy as np

from at3_testlib import REF_SO
from at3p_decode_lib import FRAME, REF_SRC
from at3p_tonal_lib import _block_ints, random_block

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "at3p_tonal_write.npz")
STREAMS, FRAMES = 2, 3
SCHEDULE_FLAGS = (0, 1, 5, 7)     # UseGha: GHA_PASS_INPUT 1, GHA_WRITE_TONAL 2, GHA_WRITE_RESIUDAL 4
SCHEDULE_CALLS = 8                # lambda calls per schedule case: 7 frames
SCHEDULE_CASES = [(2, f) for f in SCHEDULE_FLAGS] + [(1, 7)]   # (channels, UseGha)


# ---- blocks ------------------------------------------------------------------------------------------------------------------
def band(waves=(), start=None, stop=None):
    return {"start": start, "stop": stop, "waves": [tuple(w) for w in waves]}


def waves_of(freqs, k=0):
    return [(f, (7 * i + k) % 64, (5 * i + 3 * k) % 32) for i, f in enumerate(freqs)]


def block(nch, bands0, bands1=None, shared=None, leader=False):
    """a block from channel 0's bands; channel 1 gets bands1, or channel 0's frequencies mirrored (1023 - f) where it is not shared"""
    nb = len(bands0)
    shared = [False] * nb if shared is None else [bool(x) for x in shared]
    rows = [list(bands0)]
    if nch == 2:
        if bands1 is None:
            bands1 = [band(sorted((1023 - f, a, p) for f, a, p in b["waves"]), b["stop"], b["start"]) for b in bands0]
        rows.append([band() if shared[i] else b for i, b in enumerate(bands1)])
    return {"nb": nb, "shared": shared if nch == 2 else [False] * nb, "leader": bool(leader and nch == 2), "bands": rows}


def largest_block(nch, seed=0):
    """16 bands, 48 waves, both envelope points everywhere, frequencies below 512 (10 bits each in either order), no sharing and,
    in stereo, the long sharing form: the most bits a block can take"""
    rng = np.random.RandomState(100 + seed)
    per = [3] * 16 if nch == 1 else [2, 1] * 8       # 48 = 16 x 3 = 2 x (8 x 2 + 8 x 1)
    rows = []
    for ch in range(nch):
        row = []
        for b in range(16):
            n = per[(b + ch) % 16] if nch == 2 else per[b]
            fr = sorted(int(x) for x in rng.choice(512, n, replace=False))
            row.append(band([(f, int(rng.randint(64)), int(rng.randint(32))) for f in fr], int(rng.randint(32)), int(rng.randint(32))))
        rows.append(row)
    return {"nb": 16, "shared": [False] * 16, "leader": False, "bands": rows}


def _case_blocks(name, nch):
    """[STREAMS][FRAMES] blocks (None: no tonal block) of a case"""
    rng = np.random.default_rng(sum(map(ord, name)) * 4 + nch)
    if name == "small":        # one band with one wave; an envelope without waves; 15 waves in one band; 16 bands, 48 waves, both points
        one = block(nch, [band([(440, 20, 5)])])
        env = block(nch, [band([], 3, 29), band([(10, 1, 1)])])
        b15 = block(nch, [band([], None, 7), band(waves_of(range(5, 1000, 70)), 0, None)], bands1=[band(), band([(700, 63, 31)], 31, 31)])
        return [[one, None, env], [b15, None, largest_block(nch)]]
    if name == "freq":         # CreateFreqBitPack: ascending cheaper, descending cheaper, equal (takes descending), predecessors >= 512, equal frequencies
        asc = block(nch, [band(waves_of([1000, 1010, 1020])), band(waves_of([600, 700], 1)), band(waves_of([900, 1000, 1023, 1023], 2))],
                    bands1=[band(waves_of([1015, 1016, 1017, 1018, 1019])), band(), band(waves_of([768, 769]))])
        desc = block(nch, [band(waves_of([1, 2, 3])), band(waves_of([0, 0, 1], 1)), band(waves_of([5, 300, 511, 512], 2))],
                     bands1=[band(waves_of([0, 1])), band(waves_of([2, 40, 41])), band()])
        equal = block(nch, [band(waves_of([100, 600])), band(waves_of([511, 1023], 3)), band(waves_of([0, 512, 768], 1))],
                      bands1=[band(waves_of([256, 512])), band(waves_of([300, 300])), band(waves_of([511, 512]))])
        pred = block(nch, [band(waves_of([512, 512])), band(waves_of([1023, 1023], 1)), band(waves_of([800, 800, 800], 2)),
                           band(waves_of([300, 300])), band(waves_of([511, 600, 1022, 1023], 5))],
                     bands1=[band(waves_of([767, 1023])), band(waves_of([1022, 1022, 1023])), band(), band(waves_of([0, 0])), band(waves_of([640, 641]))])
        return [[asc, None, desc], [equal, None, pred]]
    if name in ("steep", "random", "loud"):
        out = [[random_block(rng, nch), None, random_block(rng, nch)], [random_block(rng, nch, nb=16), None, random_block(rng, nch)]]
        if name == "loud":
            out[0][0] = largest_block(nch, 1)
            out[1][2] = largest_block(nch, 2)
        return out
    if name in ("share_a", "share_b"):   # sharing none, some and all, each with and without the leader flag
        def sh(kind, leader, k):
            nb = 5 + k
            bands0 = [band(waves_of(sorted(int(x) for x in rng.choice(1024, int(rng.integers(0, 4)), replace=False)), i),
                           None if i % 2 else i, None if i % 3 else 31 - i) for i in range(nb)]
            shared = {"none": [False] * nb, "all": [True] * nb, "some": [i % 2 == k % 2 for i in range(nb)]}[kind]
            return block(2, bands0, shared=shared, leader=leader)
        if name == "share_a":
            return [[sh("none", True, 0), None, sh("some", False, 1)], [sh("all", True, 2), None, sh("some", True, 3)]]
        return [[sh("all", False, 0), None, sh("none", False, 1)], [sh("some", True, 2), None, sh("all", True, 11)]]
    raise KeyError(name)


# name -> (channel counts, amplitude of the white spectra, has window flags)
WRITER_CASES = {"small": ((1, 2), 0.05, False), "freq": ((1, 2), 0.05, False), "steep": ((1, 2), 0.05, True), "random": ((1, 2), 0.02, False),
                "share_a": ((2,), 0.05, False), "share_b": ((2,), 0.05, False), "loud": ((2,), 1.0, False)}
LOUD_SEED = 1   # the seed of "loud": chosen so that the reference keeps fewer units with the block than without (the generator asserts it)


def writer_case_ids():
    return [f"{name}_{nch}" for name, (chs, _, _) in WRITER_CASES.items() for nch in chs]


def case_seed(cid):
    name, nch = cid.rsplit("_", 1)
    return LOUD_SEED if name == "loud" else 1000 + 10 * list(WRITER_CASES).index(name) + int(nch)


def case_specs(cid, seed=None):
    """the case's spectra [STREAMS][FRAMES][C][2048], white, from its seed"""
    name, nch = cid.rsplit("_", 1)
    rng = np.random.RandomState(case_seed(cid) if seed is None else seed)
    return (WRITER_CASES[name][1] * rng.standard_normal((STREAMS, FRAMES, int(nch), 2048))).astype(np.float32)


def case_flags(cid):
    """the case's window flags [STREAMS][FRAMES][C] or None: the `1 1` form next to blocks, and `1 0` / sine on single frames"""
    name, nch = cid.rsplit("_", 1)
    if not WRITER_CASES[name][2]:
        return None
    fl = np.random.RandomState(case_seed(cid) + 1).randint(1, 0xff, size=(STREAMS, FRAMES, int(nch))).astype(np.uint16) << 3   # never all steep below 8
    fl[0, 0, 0] = 0x01ff ^ 0x0010
    fl[1, 1] = 0xffff
    fl[1, 2, -1] = 0
    return fl


def case_blocks(cid):
    name, nch = cid.rsplit("_", 1)
    return _case_blocks(name, int(nch))


def block_ints(nch, blocks):
    """[STREAMS][FRAMES] blocks as one flat int32 array (at3p_tonal_lib's form per block: nb, leader, shared[16], then per channel and
    band start, stop, wave count and the waves)"""
    return np.array([x for row in blocks for b in row for x in _block_ints(nch, b)], np.int32)


def blocks_from_ints(nch, ints, shape=(STREAMS, FRAMES)):
    ints = [int(x) for x in ints]
    k = 0
    out = []
    for _ in range(shape[0]):
        row = []
        for _ in range(shape[1]):
            nb, leader, shared = ints[k], ints[k + 1], ints[k + 2:k + 18]
            k += 18
            if nb == 0:
                row.append(None)
                continue
            rows = []
            for _ch in range(nch):
                r = []
                for _b in range(nb):
                    st, sp, nw = ints[k:k + 3]
                    k += 3
                    r.append(band([tuple(ints[k + 3 * i:k + 3 * i + 3]) for i in range(nw)], None if st < 0 else st, None if sp < 0 else sp))
                    k += 3 * nw
                rows.append(r)
            row.append({"nb": nb, "shared": [bool(x) for x in shared[:nb]], "leader": bool(leader), "bands": rows})
        out.append(row)
    assert k == len(ints)
    return out


def record_fields(rec):
    """at3p_tonal_lib.unpack_tonal's record [REC_INTS] -> the block in dict form as ApplyFilter's bookkeeping shows it (a shared
    band of channel 1 copied from channel 0, the leader swap applied), or None"""
    if not rec[0]:
        return None
    out = []
    for ch in range(2):
        row = []
        for b in range(16):
            nw, idx, hs, sp, he, ep = (int(x) for x in rec[1 + (ch * 16 + b) * 6:1 + (ch * 16 + b) * 6 + 6])
            wv = [(int(rec[193 + idx + i]), int(rec[193 + 48 + idx + i]), int(rec[193 + 96 + idx + i])) for i in range(nw)]
            row.append(band(wv, sp if hs else None, ep if he else None))
        out.append(row)
    return out


def expected_fields(nch, b):
    """the same from the block handed to the writer"""
    if b is None:
        return None
    empty = band()
    rows = [[b["bands"][0][i] if i < b["nb"] else empty for i in range(16)]]
    if nch == 2:
        rows.append([(b["bands"][0][i] if b["shared"][i] else b["bands"][1][i]) if i < b["nb"] else empty for i in range(16)])
        if b["leader"]:
            rows = rows[::-1]
    else:
        rows.append([empty] * 16)
    return [[band(x["waves"], x["start"], x["stop"]) for x in r] for r in rows]


# ---- the reference's writer, with window flags ----------------------------------------------------------------------------------
REF_INC = [f"-I{REF_SRC}", f"-I{REF_SRC}/lib", f"-I{REF_SRC}/lib/liboma/include", f"-I{REF_SRC}/lib/fft/kissfft_impl"]

REF_WRITER_WIN = r"""
#include "atrac/at3p/at3p_bitstream.h"
#include "atrac/at3p/at3p_gha.h"
#include "atrac/at3p/at3p_tables.h"
#include "atrac/atrac_scale.h"
#include "compressed_io.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace NAtracDEnc;
namespace {
struct TMem : public ICompressedOutput {
    std::vector<std::vector<char>>* F;
    explicit TMem(std::vector<std::vector<char>>* f) : F(f) {}
    void WriteFrame(std::vector<char> d) override { F->push_back(std::move(d)); }
    std::string GetName() const override { return "mem"; }
    size_t GetChannelNum() const override { return 2; }
};
template <class T> std::vector<T> slurp(const char* path)
{
    std::vector<T> v;
    FILE* f = fopen(path, "rb");
    T x;
    while (f && fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
    if (f) fclose(f);
    return v;
}
}
// argv = n C specs.f32 blocks.i32 flags.u16 out.u8: specs [n][C][2048], flags [n][C] (bit b: steep window in subband b), blocks as
// flat ints per frame (nb, leader, shared[16], then per channel and band start, stop (-1: absent), wave count, (freq, amp_sf, phase)
// per wave; nb = 0: no tonal block)
int main(int argc, char** argv)
{
    if (argc != 7) return 2;
    const int n = atoi(argv[1]), C = atoi(argv[2]);
    const std::vector<float> specs = slurp<float>(argv[3]);
    const std::vector<int> blk = slurp<int>(argv[4]);
    const std::vector<unsigned short> flags = slurp<unsigned short>(argv[5]);
    if (specs.size() != (size_t)n * C * 2048 || flags.size() != (size_t)n * C) return 3;
    std::vector<std::vector<char>> frames;
    TMem mem(&frames);
    TAt3PBitStream bs(&mem, 2048);
    TScaler<NAt3p::TScaleTable> scaler;
    size_t k = 0;
    FILE* out = fopen(argv[6], "wb");
    for (int fr = 0; fr < n; ++fr) {
        std::vector<TAt3PBitStream::TSingleChannelElement> sces(C);
        for (int ch = 0; ch < C; ++ch) {
            std::vector<float> x(specs.begin() + ((size_t)fr * C + ch) * 2048, specs.begin() + ((size_t)fr * C + ch + 1) * 2048);
            sces[ch].ScaledBlocks = scaler.ScaleFrame(x, NAt3p::TScaleTable::TBlockSizeMod());
            for (int sb = 0; sb < 16; ++sb)
                if ((flags[(size_t)fr * C + ch] >> sb) & 1) sces[ch].SubbandInfo.Win.SetSteepWin(sb);
        }
        TAt3PGhaData d;
        d.NumToneBands = (uint8_t)blk.at(k++);
        d.SecondIsLeader = blk.at(k++) != 0;
        for (int i = 0; i < 16; ++i) d.ToneSharing[i] = blk.at(k++) != 0;
        for (int ch = 0; ch < C; ++ch)
            for (int i = 0; i < d.NumToneBands; ++i) {
                TAt3PGhaData::TWaveSbInfo sb;
                const int st = blk.at(k), sp = blk.at(k + 1), nw = blk.at(k + 2);
                k += 3;
                sb.Envelope = {st < 0 ? TAt3PGhaData::EMPTY_POINT : (uint32_t)st, sp < 0 ? TAt3PGhaData::EMPTY_POINT : (uint32_t)sp};
                sb.WaveIndex = d.Waves[ch].WaveParams.size();
                sb.WaveNums = nw;
                for (int w = 0; w < nw; ++w, k += 3) {
                    TAt3PGhaData::TWaveParam p;
                    p.FreqIndex = blk.at(k);
                    p.AmpSf = blk.at(k + 1);
                    p.AmpIndex = 0;
                    p.PhaseIndex = blk.at(k + 2);
                    d.Waves[ch].WaveParams.push_back(p);
                }
                d.Waves[ch].WaveSbInfos.push_back(sb);
            }
        bs.WriteFrame(C, d.NumToneBands ? &d : nullptr, sces);
        if (frames.size() != 1 || frames[0].size() != 2048) return 4;
        fwrite(frames[0].data(), 1, 2048, out);
        frames.clear();
    }
    fclose(out);
    return k == blk.size() ? 0 : 5;
}
"""

# The reference's TAt3PEnc with MakeGhaProcessor0 defined here: the stand-in analyser of tests/host/at3p_fake_gha.h, its record
# converted to TAt3PGhaData.
REF_SCHEDULE = r"""
#include <atrac3p.h>
#include "atrac/at3p/at3p_gha.h"
#include "compressed_io.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "at3p_fake_gha.h"
using namespace NAtracDEnc;
namespace {
struct TMem : public ICompressedOutput {
    FILE* Out;
    explicit TMem(FILE* f) : Out(f) {}
    void WriteFrame(std::vector<char> d) override { fwrite(d.data(), 1, d.size(), Out); }
    std::string GetName() const override { return "mem"; }
    size_t GetChannelNum() const override { return 2; }
};
class TFake : public IGhaProcessor {
public:
    explicit TFake(bool stereo) : Channels(stereo ? 2 : 1) {}
    const TAt3PGhaData* DoAnalize(TBufPtr, TBufPtr, float* w1, float* w2, const float*, const float*) override
    {
        const int k = Calls++;
        at3p_fake_gha_modify(k, w1, w2);
        at3phip_tonal_block b;
        if (!at3p_fake_gha_block(k, Channels, &b)) return nullptr;
        Data = TAt3PGhaData();
        Data.NumToneBands = b.num_tone_bands;
        Data.SecondIsLeader = b.second_is_leader != 0;
        for (int i = 0; i < 16; ++i) Data.ToneSharing[i] = (b.tone_sharing >> i) & 1;
        int at = 0;
        for (int ch = 0; ch < Channels; ++ch)
            for (int i = 0; i < b.num_tone_bands; ++i) {
                const at3phip_tonal_band& bd = b.band[ch][i];
                TAt3PGhaData::TWaveSbInfo sb;
                sb.Envelope = {bd.start ? (uint32_t)bd.start - 1 : TAt3PGhaData::EMPTY_POINT, bd.stop ? (uint32_t)bd.stop - 1 : TAt3PGhaData::EMPTY_POINT};
                sb.WaveIndex = Data.Waves[ch].WaveParams.size();
                sb.WaveNums = bd.n_waves;
                for (int w = 0; w < bd.n_waves; ++w, ++at)
                    Data.Waves[ch].WaveParams.push_back({b.wave[at] & 1023u, (b.wave[at] >> 10) & 63u, 0u, (b.wave[at] >> 16) & 31u});
                Data.Waves[ch].WaveSbInfos.push_back(sb);
            }
        return &Data;
    }
private:
    const int Channels;
    int Calls = 0;
    TAt3PGhaData Data;
};
}
namespace NAtracDEnc {
std::unique_ptr<IGhaProcessor> MakeGhaProcessor0(bool stereo, bool, int) { return std::unique_ptr<IGhaProcessor>(new TFake(stereo)); }
}
// argv = C use_gha n_calls pcm.f32 out.u8: pcm [n_calls][2048][C] interleaved; every frame the encoder writes, in order
int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const int C = atoi(argv[1]), useGha = atoi(argv[2]), n = atoi(argv[3]);
    std::vector<float> pcm((size_t)n * 2048 * C);
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(pcm.data(), 4, pcm.size(), f) != pcm.size()) return 3;
    fclose(f);
    FILE* out = fopen(argv[5], "wb");
    {
        TAt3PEnc::TSettings settings;
        settings.UseGha = (uint8_t)useGha;
        std::unique_ptr<IProcessor> enc(new TAt3PEnc(TCompressedOutputPtr(new TMem(out)), C, settings));   // (TImpl is complete in at3p.cpp only)
        auto lambda = enc->GetLambda();
        const TPCMEngine::ProcessMeta meta = {(uint16_t)C};
        for (int i = 0; i < n; ++i) lambda(pcm.data() + (size_t)i * 2048 * C, meta);
    }
    fclose(out);
    return 0;
}
"""

_built = {}


def have_ref():
    return os.path.exists(REF_SO) and os.path.isdir(REF_SRC)


def _build(name, source, extra=()):
    if name not in _built:
        d = tempfile.mkdtemp(prefix="at3ptw_")
        src, exe = os.path.join(d, name + ".cpp"), os.path.join(d, name)
        open(src, "w").write(source)
        libdir = os.path.dirname(REF_SO)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-DNDEBUG", "-ffp-contract=off", *REF_INC, f"-I{os.path.join(HERE, 'host')}", src, *extra,
                               "-o", exe, f"-L{libdir}", "-lat3ref", f"-Wl,-rpath,{libdir}"])
        _built[name] = exe
    return _built[name]


def ref_write_tonal_win(specs, blocks, flags=None):
    """the REFERENCE's ScaleFrame and WriteFrame(C, &block or nullptr, sces) per frame: specs [n][C][2048], blocks [n], flags [n][C]"""
    specs = np.ascontiguousarray(specs, np.float32)
    n, C = specs.shape[0], specs.shape[1]
    fl = np.zeros((n, C), np.uint16) if flags is None else np.ascontiguousarray(flags, np.uint16)
    with tempfile.TemporaryDirectory(prefix="at3ptw_run_") as d:
        sp, bp, fp, op = (os.path.join(d, x) for x in ("specs.f32", "blocks.i32", "flags.u16", "out.u8"))
        specs.tofile(sp)
        np.array([x for b in blocks for x in _block_ints(C, b)], np.int32).tofile(bp)
        fl.tofile(fp)
        subprocess.run([_build("ref_writer_win", REF_WRITER_WIN), str(n), str(C), sp, bp, fp, op], check=True)
        return np.fromfile(op, np.uint8).reshape(n, FRAME)


def schedule_pcm(nch, use_gha):
    """[SCHEDULE_CALLS][2048][C]: a few sines and noise, the same whatever the flags"""
    rng = np.random.RandomState(77 + nch)
    t = np.arange(SCHEDULE_CALLS * 2048)
    x = np.stack([0.3 * np.sin(2 * np.pi * (441.0 + 97 * c) * t / 44100) + 0.1 * np.sin(2 * np.pi * 5512.5 * t / 44100) +
                  0.05 * rng.standard_normal(t.size) for c in range(nch)], axis=-1)
    return np.ascontiguousarray(x.reshape(SCHEDULE_CALLS, 2048, nch), np.float32)


def ref_schedule(nch, use_gha):
    """the frames the REFERENCE's TAt3PEnc writes for schedule_pcm under UseGha = use_gha with the stand-in analyser:
    [SCHEDULE_CALLS - 1][2048]"""
    at3p = os.path.join(REF_SRC, "atrac", "at3p", "at3p.cpp")
    exe = _build("ref_schedule", REF_SCHEDULE, [at3p])
    with tempfile.TemporaryDirectory(prefix="at3ptw_run_") as d:
        pp, op = os.path.join(d, "pcm.f32"), os.path.join(d, "out.u8")
        schedule_pcm(nch, use_gha).tofile(pp)
        subprocess.run([exe, str(nch), str(use_gha), str(SCHEDULE_CALLS), pp, op], check=True)
        return np.fromfile(op, np.uint8).reshape(-1, FRAME)


def export_schedule(path, g):
    """the schedule cases for tests/host/test_host_shim_at3p_tonal.cpp: int32 n_cases, then per case int32 channels, use_gha,
    n_calls, n_frames, the PCM as float32 and the golden frames"""
    with open(path, "wb") as f:
        np.array([len(SCHEDULE_CASES)], np.int32).tofile(f)
        for nch, flags in SCHEDULE_CASES:
            fr = g[f"schedule_{nch}_{flags}"]
            np.array([nch, flags, SCHEDULE_CALLS, fr.shape[0]], np.int32).tofile(f)
            schedule_pcm(nch, flags).tofile(f)
            np.ascontiguousarray(fr, np.uint8).tofile(f)
