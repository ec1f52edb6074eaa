"""A driver for the REFERENCE's ATRAC3plus part coders under a caller-supplied allocation, the cases of the tests that hold the
adaptive and sparse writers to it, and the golden file tests/golden/at3p_ref_parts.npz (TEST INFRASTRUCTURE: nothing under
atracdenc_amd/ imports this module).

In the reference only TConfigure holds the fixed word-length table. TWordLenEncoder, TSfIdxEncoder, TQuantUnitsEncoder and
TTonalComponentEncoder (atrac/at3p/at3p_bitstream_impl.h) code whatever TSpecFrame::WordLen holds, so with a configure part of this
project in front of them the reference's own code writes any allocation:

  * REF_PARTS: the driver's C++ text, compiled on first use against the reference's headers and oracle/_ref/libat3ref.so with
    at3p_tonal_write_lib._build's flags. Its own parts are TOwnConfigure (unit count, word lengths and scale factor indices into the
    frame record, the 5 + 1 bits), TTailAt32 (hands TTonalComponentEncoder the 32 units it sees in the reference's first pass, where
    it forms its bits once) and, for sparse frames only, TSparseUnits (the code-table section of include/at3phip.h, A4s / A6s; each
    unit's spectrum and code-table index from the reference's TQuantUnitsEncoder::TUnit::GetOrCompute). Nothing of the reference is
    stored in the repository.
  * ref_write: frames, the bit count of the reference's TBitStream and, on request, the reference's integer mantissas.
  * write_restatement: the three restatements behind one call; edge_spectra, steps_specs, table7_specs, tonal_case: spectra, window
    flags and tonal blocks of the tests, from the existing seeded builders.
  * cells, cell_inputs, golden_build, golden_load: the golden file (tools/gen_golden_at3p_ref_parts.py).
"""
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

import at3p_writer_lib as W
import at3p_tonal_write_lib as TW
from at3p_tonal_lib import _block_ints

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "at3p_ref_parts.npz")
REPEAT_STATUS = 7      # the reference asked for a repeat: the allocation does not fit by its count

REF_PARTS = r"""
#include "atrac/at3p/at3p_bitstream_impl.h"
#include "atrac/at3p/at3p_tables.h"
#include "atrac/at3p/ff/atrac3plus_data.h"
#include "env.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace NAtracDEnc;
namespace {
template <class T> std::vector<T> slurp(const char* path)
{
    std::vector<T> v;
    FILE* f = fopen(path, "rb");
    T x;
    while (f && fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
    if (f) fclose(f);
    return v;
}
// the allocation of one frame: N, then wl[2][32]
struct TAlloc { int N; int Wl[2][32]; };
int wl_of(const TSpecFrame* fr, int ch, int qu) { return ch ? fr->WordLen[qu].second : fr->WordLen[qu].first; }

// in TConfigure's place: the caller's allocation. A second entry is the reference's repeat and ends the run.
class TOwnConfigure : public TDumper {
public:
    explicit TOwnConfigure(const TAlloc* a) : A(a) {}
    EStatus Encode(void* frameData, TBitAllocHandler&) override
    {
        if (Entered++) exit(7);
        TSpecFrame* fr = TSpecFrame::Cast(frameData);
        fr->NumQuantUnits = A->N;
        fr->WordLen.resize(A->N);
        fr->SfIdx.resize(A->N);
        fr->SpecTabIdx.resize(A->N);
        for (int i = 0; i < A->N; ++i) {
            fr->WordLen[i] = {(uint8_t)A->Wl[0][i], (uint8_t)A->Wl[fr->Chs.size() > 1][i]};
            fr->SfIdx[i].first = fr->Chs[0].Sce.ScaledBlocks.at(i).ScaleFactorIndex;
            if (fr->Chs.size() > 1) fr->SfIdx[i].second = fr->Chs[1].Sce.ScaledBlocks.at(i).ScaleFactorIndex;
        }
        Insert(A->N - 1, 5), Insert(0, 1);      // the unit count and the mute bit
        fr->AllocatedBits = GetConsumption();
        return EStatus::Ok;
    }
private:
    const TAlloc* A;
    int Entered = 0;
};

// The reference's tail part forms its bits once, in its first pass, which has 32 units, and keeps them while the unit count
// shrinks: the window shapes are written for 16 subbands whatever N becomes. Here N is final from the start, so the part is shown
// 32 units while it runs; its verdict on the frame's size does not depend on the count.
class TTailAt32 : public IBitStreamPartEncoder {
public:
    EStatus Encode(void* frameData, TBitAllocHandler& ba) override
    {
        TSpecFrame* fr = TSpecFrame::Cast(frameData);
        const uint32_t n = fr->NumQuantUnits;
        fr->NumQuantUnits = 32;
        const EStatus st = Tail.Encode(frameData, ba);
        fr->NumQuantUnits = n;
        return st;
    }
    void Dump(NBitStream::TBitStream& bs) override { Tail.Dump(bs); }
    void Reset() noexcept override { Tail.Reset(); }
    uint32_t GetConsumption() const noexcept override { return Tail.GetConsumption(); }
private:
    TTonalComponentEncoder Tail;
};

// in TQuantUnitsEncoder's place for frames that hold a word length of 0 (TUnit indexes table wl - 1): the code-table section of
// include/at3phip.h, A4s / A6s; spectra and table indices are TUnit::GetOrCompute's, the power groups as the reference writes them
class TSparseUnits : public TDumper {
public:
    std::vector<int> Mant[2][32];
    EStatus Encode(void* frameData, TBitAllocHandler&) override
    {
        TSpecFrame* fr = TSpecFrame::Cast(frameData);
        const int N = fr->NumQuantUnits, C = fr->Chs.size();
        std::vector<std::vector<std::pair<uint16_t, uint8_t>>> data;
        int tab[2][32];
        for (int ch = 0; ch < C; ++ch) {
            for (int qu = 0; qu < N; ++qu) {
                Mant[ch][qu].clear();
                if (!wl_of(fr, ch, qu)) continue;
                TQuantUnitsEncoder::TUnit unit(qu, wl_of(fr, ch, qu));
                data.emplace_back();
                tab[ch][qu] = unit.GetOrCompute(fr->Chs[ch].Sce.ScaledBlocks.at(qu).Values.data(), data.back());
                Mant[ch][qu] = unit.GetMantisas();
            }
            data.emplace_back();
            for (int i = 0; i < atrac3p_subband_to_num_powgrps[atrac3p_qu_to_subband[N - 1]]; ++i) data.back().emplace_back(15, 4);
        }
        Insert(1, 1);                               // the full-table flag
        for (int ch = 0; ch < C; ++ch) {
            Insert(0, 1), Insert(0, 2), Insert(0, 1);   // the channel's 4 header bits
            for (int qu = 0; qu < N; ++qu) {
                if (wl_of(fr, ch, qu)) Insert(tab[ch][qu], 3);
                else if (ch && wl_of(fr, 0, qu)) Insert(1, 1);
            }
        }
        for (const auto& x : data)
            for (const auto& p : x) Insert(p.first, p.second);
        return EStatus::Ok;
    }
};
}
// argv = sparse n C frame_bytes specs.f32 blocks.i32 flags.u16 alloc.i32 frames.u8 bits.i32 mant.i32: specs [n][C][2048], flags [n][C]
// (bit b: steep window in subband b), blocks as at3p_tonal_write_lib's driver takes them, alloc [n][65] (N, wl[2][32]);
// out: frames [n][frame_bytes], the bit stream's size [n], and per frame the mantissas [C][2048] (0 where nothing is coded) followed
// by ScaleFrame's scale factor indices [C][32]
int main(int argc, char** argv)
{
    if (argc != 12) return 2;
    const int sparse = atoi(argv[1]), n = atoi(argv[2]), C = atoi(argv[3]), fb = atoi(argv[4]);
    const std::vector<float> specs = slurp<float>(argv[5]);
    const std::vector<int> blk = slurp<int>(argv[6]);
    const std::vector<unsigned short> flags = slurp<unsigned short>(argv[7]);
    const std::vector<int> alloc = slurp<int>(argv[8]);
    if (specs.size() != (size_t)n * C * 2048 || flags.size() != (size_t)n * C || alloc.size() != (size_t)n * 65) return 3;
    NEnv::SetRoundFloat();
    TScaler<NAt3p::TScaleTable> scaler;
    size_t k = 0;
    FILE* out = fopen(argv[9], "wb");
    FILE* outBits = fopen(argv[10], "wb");
    FILE* outMant = fopen(argv[11], "wb");
    for (int f = 0; f < n; ++f) {
        std::vector<TAt3PBitStream::TSingleChannelElement> sces(C);
        for (int ch = 0; ch < C; ++ch) {
            std::vector<float> x(specs.begin() + ((size_t)f * C + ch) * 2048, specs.begin() + ((size_t)f * C + ch + 1) * 2048);
            sces[ch].ScaledBlocks = scaler.ScaleFrame(x, NAt3p::TScaleTable::TBlockSizeMod());
            for (int sb = 0; sb < 16; ++sb)
                if ((flags[(size_t)f * C + ch] >> sb) & 1) sces[ch].SubbandInfo.Win.SetSteepWin(sb);
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
        TAlloc a;
        a.N = alloc[(size_t)f * 65];
        for (int i = 0; i < 64; ++i) a.Wl[i / 32][i % 32] = alloc[(size_t)f * 65 + 1 + i];
        if (a.N < 1 || a.N > 32) return 6;
        TQuantUnitsEncoder* units = sparse ? nullptr : new TQuantUnitsEncoder();
        TSparseUnits* sparseUnits = sparse ? new TSparseUnits() : nullptr;
        IBitStreamPartEncoder* const order[5] = {new TOwnConfigure(&a), new TWordLenEncoder(), new TSfIdxEncoder(),
                                                 sparse ? (IBitStreamPartEncoder*)sparseUnits : (IBitStreamPartEncoder*)units, new TTailAt32()};
        std::vector<IBitStreamPartEncoder::TPtr> chain;
        for (IBitStreamPartEncoder* part : order) chain.emplace_back(part);
        TBitStreamEncoder enc(std::move(chain));
        TSpecFrame frame((uint32_t)fb * 8 - 3, a.N, C, d.NumToneBands ? &d : nullptr, sces);
        NBitStream::TBitStream stream;
        stream.Write(0, 1), stream.Write(C - 1, 2);     // the three leading bits
        enc.Do(&frame, stream);
        const int bits = (int)stream.GetSizeInBits();
        if (bits > fb * 8) return 4;
        std::vector<char> buf = stream.GetBytes();
        buf.resize(fb);
        fwrite(buf.data(), 1, fb, out);
        fwrite(&bits, sizeof(bits), 1, outBits);
        std::vector<int> mant((size_t)C * 2048, 0);
        for (int ch = 0; ch < C; ++ch)
            for (int qu = 0; qu < a.N; ++qu) {
                const int wl = a.Wl[ch][qu];
                if (!wl) continue;
                const std::vector<int>& m = sparse ? sparseUnits->Mant[ch][qu]
                                                   : units->UnitBuffers.at(TQuantUnitsEncoder::TUnit::MakeKey(ch, qu, wl)).GetMantisas();
                for (size_t i = 0; i < m.size(); ++i) mant[(size_t)ch * 2048 + NAt3p::TScaleTable::BlockSizeTab[qu] + i] = m[i];
            }
        fwrite(mant.data(), sizeof(int), mant.size(), outMant);
        for (int ch = 0; ch < C; ++ch)
            for (int qu = 0; qu < 32; ++qu) {
                const int sf = sces[ch].ScaledBlocks.at(qu).ScaleFactorIndex;
                fwrite(&sf, sizeof(sf), 1, outMant);
            }
    }
    fclose(out);
    fclose(outBits);
    fclose(outMant);
    return k == blk.size() ? 0 : 5;
}
"""


class RefRepeat(Exception):
    """the reference's parts asked for a repeat: by their count the allocation does not fit the frame"""


have_ref = TW.have_ref


def ref_write(specs, frame_bytes, N, wl, sparse, win=None, blocks=None, mant=False):
    """the REFERENCE's part coders on specs float32 [n, C, 2048] under the allocation N [n], wl [n, 2, 32]; win uint16 [n, C] or
    None, blocks [n] dicts / None -> (frames uint8 [n, frame_bytes], bits int32 [n]: TBitStream's size, the three leading bits
    included[, the reference's mantissas int32 [n, C, 2048], ScaleFrame's scale factor indices int32 [n, C, 32]]). sparse: TSparseUnits
    in TQuantUnitsEncoder's place. Raises RefRepeat where the reference's count says the allocation does not fit."""
    specs = np.ascontiguousarray(specs, np.float32)
    n, C = specs.shape[0], specs.shape[1]
    fl = np.zeros((n, C), np.uint16) if win is None else np.ascontiguousarray(win, np.uint16)
    blocks = [None] * n if blocks is None else list(blocks)
    alloc = np.zeros((n, 65), np.int32)
    alloc[:, 0] = N
    alloc[:, 1:] = np.asarray(wl).reshape(n, 64)
    exe = TW._build("ref_parts", REF_PARTS, ["-fno-access-control"])
    with tempfile.TemporaryDirectory(prefix="at3prp_run_") as d:
        sp, bp, fp, ap, op, cp, mp = (os.path.join(d, x) for x in ("specs.f32", "blocks.i32", "flags.u16", "alloc.i32", "out.u8", "bits.i32", "mant.i32"))
        specs.tofile(sp)
        np.array([x for b in blocks for x in _block_ints(C, b)], np.int32).tofile(bp)
        fl.tofile(fp)
        alloc.tofile(ap)
        r = subprocess.run([exe, str(int(bool(sparse))), str(n), str(C), str(int(frame_bytes)), sp, bp, fp, ap, op, cp, mp])
        if r.returncode == REPEAT_STATUS:
            raise RefRepeat(f"frame_bytes {frame_bytes}")
        assert r.returncode == 0, r.returncode
        out = (np.fromfile(op, np.uint8).reshape(n, frame_bytes), np.fromfile(cp, np.int32))
        if not mant:
            return out
        m = np.fromfile(mp, np.int32).reshape(n, C * 2080)
        return out + (m[:, :C * 2048].reshape(n, C, 2048), m[:, C * 2048:].reshape(n, C, 32))


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
WRITERS = ("alloc", "rate", "sparse_off", "sparse_on")


def write_restatement(writer, specs, frame_bytes, win=None, blocks=None):
    """(frames, info records) of tests/host/at3p_writer_cpu.c; the writers' names are those of the restatements it was folded from
    (`alloc`: 2048 bytes only; `alloc`, `rate` and `sparse_off` are one writer now, and the tests keep their cases' names)"""
    assert writer in WRITERS and (writer != "alloc" or frame_bytes == 2048)
    return W.write_adaptive(specs, frame_bytes, writer == "sparse_on", win, blocks, info=True)[:2]


# ---- spectra ------------------------------------------------------------------------------------------------------------------------
def edge_spectra(nch):
    """{name: (spectra [n, C, 2048], blocks [n] or None)}: the float domain's and the allocation's edges"""
    rng = np.random.RandomState(40 + nch)
    e_sp, e_bl = W.edge_specs(nch)
    out = {"fullscale": (W.full_scale_noise(2, nch), None), "odd": (W.odd_specs(nch), None), "silence": (np.zeros((1, nch, 2048), np.float32), None),
           "edge0": (e_sp[:1], e_bl[:1]), "edge123": (e_sp[1:], None),
           "loud3": ((3.0 * rng.standard_normal((2, nch, 2048))).astype(np.float32), None),
           "tiny": ((1e-7 * rng.standard_normal((2, nch, 2048))).astype(np.float32), None)}
    if nch == 1:
        out["quiet"] = (W.quiet_mono(2), None)
    else:   # channel 1 two mantissa bits under channel 0: every difference between the channels' word lengths is 0 or 2
        q = W.specs_of("mix", 2, 2)
        q[:, 1] = q[:, 0] * np.float32(0.25)
        out["quarter"] = (q, None)
    return out


def steps_specs(nch, n=4, seed=77):
    """white spectra whose level steps by whole mantissa bits from unit to unit, a different staircase per frame and channel: units
    that signals keep quiet reach the long word lengths and units they keep loud the short ones"""
    rng = np.random.RandomState(seed + nch)
    x = rng.standard_normal((n, nch, 2048))
    for f in range(n):
        for ch in range(nch):
            for q in range(32):
                x[f, ch, W.QU_START[q]:W.QU_START[q + 1]] *= 2.0 ** -((3 * q + 5 * f + 2 * ch + (q * q) % 7) % 9 + (f % 2) * (q % 3))
    return (0.4 * x).astype(np.float32)


def float_table(name):
    """a float table of the generated table files (AT3P_INV_MANT, AT3P_SCALE, AT3P_MANT) as float32"""
    import re
    csrc = os.path.join(HERE, "..", "atracdenc_amd", "csrc")
    t = open(os.path.join(csrc, "at3p_vlc.inc")).read() + open(os.path.join(csrc, "at3p_mant.inc")).read()
    m = re.search(name + r"\[\d+\]\s*=\s*\{(.*?)\};", t, re.S)
    return np.array([float.fromhex(x.rstrip("f")) for x in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+f?", m.group(1))], np.float32)


# mantissa pairs of a 128-line unit at word length 6 for which the eighth code table (index 7, the one with group flags) is the
# cheapest: a linear programme over the eight tables' code lengths gave this mix, 10 bits under the next table
TABLE7_PAIRS = [(-13, 0)] * 27 + [(-10, -10)] * 5 + [(-1, -6)] * 16 + [(0, -2)] * 5 + [(0, 0)] * 11
TABLE7_BYTES = {1: 376, 2: 744}


def table7_specs(nch, n=6, base=50):
    """[n, C, 2048] for TABLE7_BYTES: quiet noise, and in unit 24 of every channel TABLE7_PAIRS dequantised at word length 6 under
    scale factor index base + frame: some frame's allocation gives the unit word length 6, and then code table 7"""
    sp = (0.001 * np.random.RandomState(3).standard_normal((n, nch, 2048))).astype(np.float32)
    m = np.array(TABLE7_PAIRS, np.float64).reshape(-1)
    inv, scale = float_table("AT3P_INV_MANT"), float_table("AT3P_SCALE")
    for f in range(n):
        sp[f, :, W.QU_START[24]:W.QU_START[25]] = (m / float(inv[6]) * float(scale[base + f])).astype(np.float32)
    return sp


def tonal_case(nch):
    """(spectra [6, C, 2048], window flags [6, C], blocks [6]): at3p_tonal_write_lib's `steep` case, the one with window flags"""
    cid = f"steep_{nch}"
    return TW.case_specs(cid).reshape(6, nch, 2048), TW.case_flags(cid).reshape(6, nch), [b for row in TW.case_blocks(cid) for b in row]


# ---- the golden file's cells -----------------------------------------------------------------------------------------------------------
G_S, G_F = 3, 4
G_SIZES = {1: (176, 376, 2048), 2: (224, 376, 2048)}
G_TONAL_BYTES = 744


def golden_streams(nch):
    """spectra [3, 4, C, 2048]: noise and tones; the float domain's edges beside mix; the allocation's special cases"""
    e = edge_spectra(nch)
    s1 = np.concatenate([W.odd_specs(nch, 2), e["fullscale"][0][:1], W.specs_of("mix", nch, 1)])
    s2 = np.concatenate([e["edge123"][0], e["silence"][0]])
    return np.stack([np.concatenate([W.specs_of("noise", nch, 2), W.specs_of("tones", nch, 2)]), s1, s2])


def golden_tonal(nch):
    """(spectra [3, 4, C, 2048], window flags [3, 4, C], blocks [3][4]): the `steep` case's six frames, then the largest block beside
    silence with one loud unit, the largest block on noise, and four frames of steps_specs under the flags of the first four"""
    sp, fl, bl = tonal_case(nch)
    e_sp, e_bl = W.edge_specs(nch)
    sp = np.concatenate([sp, e_sp[:1], W.specs_of("noise", nch, 1), steps_specs(nch)])
    fl = np.concatenate([fl, np.zeros((2, nch), np.uint16), fl[:4]])
    bl = bl + [e_bl[0], TW.largest_block(nch), None, None, None, None]
    return sp.reshape(G_S, G_F, nch, 2048), fl.reshape(G_S, G_F, nch), [bl[4 * s:4 * s + 4] for s in range(G_S)]


def cells():
    """[(key, nch, frame_bytes, sparse, tonal)] of the golden file"""
    out = []
    for nch in (1, 2):
        for sparse in (False, True):
            out += [(f"{'sparse' if sparse else 'adaptive'}_{nch}_{fb}", nch, fb, sparse, False) for fb in G_SIZES[nch]]
            out.append((f"{'sparse' if sparse else 'adaptive'}_{nch}_tonal", nch, G_TONAL_BYTES, sparse, True))
    return out


def cell_inputs(nch, tonal):
    """(spectra [3, 4, C, 2048], window flags [3, 4, C] or None, blocks [3][4] or None, SHA-256 of all three)"""
    sp, fl, bl = golden_tonal(nch) if tonal else (golden_streams(nch), None, None)
    h = hashlib.sha256(np.ascontiguousarray(sp).tobytes())
    if tonal:
        h.update(np.ascontiguousarray(fl).tobytes())
        h.update(np.array([x for row in bl for b in row for x in _block_ints(nch, b)], np.int32).tobytes())
    return sp, fl, bl, h.hexdigest()


def golden_build():
    """the golden file's arrays, written by the reference's code: per cell the restatement chooses N and wl, the driver writes the
    frames and counts the bits. Needs the reference."""
    out, meta = {}, {}
    for key, nch, fb, sparse, tonal in cells():
        sp, fl, bl, sha = cell_inputs(nch, tonal)
        flat = sp.reshape(G_S * G_F, nch, 2048)
        blocks = None if bl is None else [b for row in bl for b in row]
        _, rec = write_restatement("sparse_on" if sparse else "sparse_off", flat, fb, None if fl is None else fl.reshape(G_S * G_F, nch), blocks)
        frames, bits = ref_write(flat, fb, rec["num_quant_units"], rec["wl"], sparse, None if fl is None else fl.reshape(G_S * G_F, nch), blocks)
        out[f"{key}_frames"] = frames.reshape(G_S, G_F, fb)
        out[f"{key}_n"] = rec["num_quant_units"].astype(np.uint8).reshape(G_S, G_F)
        out[f"{key}_wl"] = rec["wl"].reshape(G_S, G_F, 2, 32)
        out[f"{key}_bits"] = bits.astype(np.int32).reshape(G_S, G_F)
        meta[key] = {"channels": nch, "frame_bytes": fb, "sparse": sparse, "tonal": tonal, "inputs_sha256": sha}
    out["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return out


def golden_load():
    g = np.load(GOLDEN)
    return g, json.loads(str(g["meta"]))
