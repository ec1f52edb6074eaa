"""Helpers of the tonal-block tests and golden generator (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * CpuTonalDecoder: the C restatement tests/host/at3p_tonal_cpu.c (tonal blocks and step 4b of include/at3phip.h), compiled on
    first use with the reference's arithmetic flags.
  * tonal_bits / splice_tonal / make_tonal_frame: a restated tonal-block writer in the order of WriteTonalBlock and
    CreateFreqBitPack, spliced into a frame without a tonal block at its tonal flag (the frame's unit count is unaffected).
  * random_block: seeded tonal blocks within the writer's syntax.
  * ref_write_tonal: the REFERENCE's TAt3PBitStream::WriteFrame with hand-built TAt3PGhaData, through a driver compiled at
    generation time against the reference's headers and oracle/_ref/libat3ref.so.
  * ref_tonal_back_half: the restatement's steps 1-2, then the REFERENCE's TAt3pMIDCT::Do, the rescale, the REFERENCE's
    ff_atrac3p_generate_tones (ff/atrac3plusdsp.c, compiled into a driver at generation time and fed ApplyFilter's bookkeeping)
    and the reference's at3pref_ipqf, then the clamp. Nothing of the reference is stored in the repository.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from at3_testlib import REF_SO, _vp
from at3p_decode_lib import CFLAGS, FRAME, REASONS, RESCALE, BitWriter, make_frame, mutate_frames, ref_driver, REF_SRC

HERE = os.path.dirname(os.path.abspath(__file__))
TONAL_SRC = os.path.join(HERE, "host", "at3p_tonal_cpu.c")
GOLDEN = os.path.join(HERE, "golden", "at3p_tonal.npz")
REC_INTS = 1 + 2 * 16 * 6 + 3 * 48
TONE_VLC = None


def tone_vlc():
    """[(code, len)] of NumToneBands - 1 from the generated table file"""
    global TONE_VLC
    if TONE_VLC is None:
        import re
        t = open(os.path.join(HERE, "..", "atracdenc_amd", "csrc", "at3p_tone_vlc.inc")).read()
        v = [int(x, 16) for x in re.findall(r"0x[0-9a-f]+", t[t.index("{"):])]
        TONE_VLC = [(e & 0xfff, e >> 12) for e in v]
    return TONE_VLC


_so = None


def tonal_lib():
    global _so
    if _so is None:
        d = tempfile.mkdtemp(prefix="at3ptonal_")
        so = os.path.join(d, "libat3ptonal_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, TONAL_SRC, "-lm"])
        _so = so
    lib = ctypes.CDLL(_so)
    lib.at3pt_state_bytes.restype = ctypes.c_size_t
    lib.at3pt_reset.argtypes = [ctypes.c_void_p]
    lib.at3pt_decode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_int]
    lib.at3pt_unpack_frame.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.at3pt_tone_tables.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.at3pt_filter_bytes.restype = ctypes.c_size_t
    lib.at3pt_apply_filter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


class CpuTonalDecoder:
    """One stream of the restatement; state carries across decode() calls."""

    def __init__(self, channels, tones=True):
        self.lib = tonal_lib()
        self.channels, self.tones = int(channels), int(bool(tones))
        self.state = np.zeros(self.lib.at3pt_state_bytes(), np.uint8)
        self.rejected = np.zeros(len(REASONS), np.uint64)
        self.lib.at3pt_reset(_vp(self.state))

    def decode(self, frames):
        frames = np.ascontiguousarray(frames, np.uint8)
        n = frames.shape[0]
        pcm = np.zeros((n, FRAME, self.channels), np.float32)
        self.lib.at3pt_decode(_vp(self.state), self.channels, _vp(frames), n, _vp(pcm), _vp(self.rejected), self.tones)
        return pcm


def cpu_tonal_decode(frames, channels, tones=True):
    d = CpuTonalDecoder(channels, tones)
    pcm = d.decode(frames)
    return pcm, d.rejected.astype(np.int64).copy()


def tone_tables():
    lib = tonal_lib()
    s, h, a = np.zeros(2048, np.float32), np.zeros(256, np.float32), np.zeros(64, np.float32)
    lib.at3pt_tone_tables(_vp(s), _vp(h), _vp(a))
    return s, h, a


# ---- the restated writer -------------------------------------------------------------------------------------------------
def _fsb1(x):
    """GetFirstSetBit(x) + 1"""
    return max(int(x).bit_length(), 1)


def freq_pack(freqs):
    """CreateFreqBitPack: (order, [(code, bits)])"""
    n = len(freqs)
    asc, bits_a = [(freqs[0], 10)], 10
    for i in range(1, n):
        p, c = freqs[i - 1], freqs[i]
        if p < 512:
            asc.append((c, 10))
            bits_a += 10
        else:
            b = _fsb1(1023 - p)
            asc.append((c - (1024 - (1 << b)), b))
            bits_a += b
    if n == 1:
        return 0, asc
    desc, bits_d = [(freqs[-1], 10)], 10
    for i in range(n - 2, -1, -1):
        b = _fsb1(freqs[i + 1])
        desc.append((freqs[i], b))
        bits_d += b
    return (0, asc) if bits_a < bits_d else (1, desc)


def _flags(w, flags):
    s = sum(flags)
    if s == 0:
        w.append((0, 1))
    elif s == len(flags):
        w += [(1, 1), (0, 1)]
    else:
        w += [(1, 1), (1, 1)] + [(int(f), 1) for f in flags]


def tonal_bits(channels, block, amp_mode=1, leader_bits=None, invert=0, env_copy=0, nw_mode=0, delta=0, amp_sf_mode=0):
    """WriteTonalBlock's bits [(value, nbits)] for block = {"nb", "shared" [nb] bools, "leader" bool,
    "bands": [ch][nb] {"start": None | 0..31, "stop": None | 0..31, "waves": [(freq, amp_sf, phase)]}}; the keyword arguments
    override what the writer emits, for the rejection cases."""
    nb, shared = block["nb"], block.get("shared", [False] * block["nb"])
    w = [(amp_mode, 1), tone_vlc()[nb - 1]]
    if channels == 2:
        _flags(w, shared)
        if leader_bits is not None:
            w += leader_bits
        else:
            _flags(w, [block.get("leader", False)])
        w.append((invert, 1))
    for ch in range(channels):
        bands = block["bands"][ch]
        own = [i for i in range(nb) if not (ch and shared[i])]
        if ch:
            w.append((env_copy, 1))
        for i in own:
            for pt in (bands[i]["start"], bands[i]["stop"]):
                w += [(0, 1)] if pt is None else [(1, 1), (pt, 5)]
        w.append((nw_mode, ch + 1))
        for i in own:
            w.append((len(bands[i]["waves"]), 4))
        if ch:
            w.append((delta, 1))
        for i in own:
            wv = bands[i]["waves"]
            if not wv:
                continue
            order, data = freq_pack([x[0] for x in wv])
            if len(wv) > 1:
                w.append((order, 1))
            w += data
        w.append((amp_sf_mode, ch + 1))
        for i in own:
            w += [(x[1], 6) for x in bands[i]["waves"]]
        for i in own:
            w += [(x[2], 5) for x in bands[i]["waves"]]
    return w


def tonal_flag_pos(frame):
    """the bit position of the tonal flag of a frame without a tonal block: the frame ends in tonal 0, noise 0, terminator 11"""
    b = np.unpackbits(np.asarray(frame, np.uint8))
    last = int(np.nonzero(b)[0][-1])
    assert b[last - 1] == 1 and b[last - 2] == 0 and b[last - 3] == 0
    return last - 3


def splice_tonal(frame, bits_list, noise=0, term=3, cut=False):
    """frame (tonal flag 0) with a tonal block after its tonal flag; None when the result would not fit the frame (with cut: the
    bits that do not fit are dropped, a frame that ends inside its tonal block)"""
    p = tonal_flag_pos(frame)
    out = np.unpackbits(np.asarray(frame, np.uint8)).copy()
    out[p:] = 0
    tail = [(1, 1)] + list(bits_list) + [(noise, 1), (term, 2)]
    pos = p
    for v, n in tail:
        for k in range(n - 1, -1, -1):
            if pos >= FRAME * 8:
                return np.packbits(out) if cut else None
            out[pos] = (v >> k) & 1
            pos += 1
    return np.packbits(out)


def make_tonal_frame(channels, block, seed=0, **kw):
    """a small frame of make_frame's with `block` spliced in"""
    nq = 6
    base = make_frame(channels, nqu=nq, wl=[[3] * nq for _ in range(channels)], sf=[[30 + q + seed % 7 for q in range(nq)]
                                                                                   for _ in range(channels)],
                      mant=lambda ch, qu, k: ((k * 5 + qu * 3 + ch + seed) % 5) - 2)
    return splice_tonal(base, tonal_bits(channels, block, **kw))


def random_block(rng, channels, nb=None, max_total=48):
    """a tonal block within the writer's syntax: ascending frequencies per band, at most max_total waves"""
    nb = int(nb or rng.integers(1, 17))
    shared = [bool(x) for x in rng.integers(0, 2, nb)] if channels == 2 and rng.random() < 0.5 else [False] * nb
    if channels == 2 and rng.random() < 0.2:
        shared = [True] * nb
    total = 0
    bands = []
    for ch in range(channels):
        row = []
        for i in range(nb):
            if ch and shared[i]:
                row.append({"start": None, "stop": None, "waves": []})
                continue
            n = int(min(rng.integers(0, 16) if rng.random() < 0.3 else rng.integers(0, 4), max_total - total))
            total += n
            fr = sorted(int(x) for x in rng.choice(1024, n, replace=False))
            waves = [(f, int(rng.integers(0, 64)), int(rng.integers(0, 32))) for f in fr]
            st = None if rng.random() < 0.6 else int(rng.integers(0, 32))
            sp = None if rng.random() < 0.6 else int(rng.integers(0, 32))
            row.append({"start": st, "stop": sp, "waves": waves})
        bands.append(row)
    return {"nb": nb, "shared": shared, "leader": bool(channels == 2 and rng.random() < 0.4), "bands": bands}


# ---- the inputs of the GPU tests and of the SIMT-harness tests (the same bytes from the same seeds) ---------------------------
def side_by_side(g, names, nch):
    cases = [n for n in names if int(g[f"{n}_channels"]) == nch]
    nf = max(g[f"{n}_frames"].shape[0] for n in cases)
    frames = np.zeros((len(cases), nf, 2048), np.uint8)   # zero frames past a case's end: rejected, decoded after its PCM
    for i, n in enumerate(cases):
        fr = g[f"{n}_frames"]
        frames[i, :fr.shape[0]] = fr
    return cases, frames


def plain(nch):
    """a frame without a tonal block"""
    return make_frame(nch, nqu=6, wl=[[3] * 6 for _ in range(nch)], sf=[[30] * 6 for _ in range(nch)],
                      mant=lambda ch, qu, k: (k % 3) - 1)


def pool(rng, nch, n):
    frames = []
    while len(frames) < n:
        b = random_block(rng, nch)
        for row in b["bands"]:
            for bd in row:
                bd["waves"] = [(f, int(rng.integers(0, 40)), p) for f, _, p in bd["waves"]]
        fr = make_tonal_frame(nch, b, seed=len(frames))
        if fr is not None:
            frames.append(fr)
    return np.stack(frames)


def fuzz_tonal_streams(nch, streams, nf, seed=None):
    """[streams][nf][2048] drawn from a pool of random tonal blocks, some with flipped bits, some without a tonal block (seed
    1000 + nch by default: the streams of the GPU suite's test_fuzzed_tonal_frames_equal_restatement)"""
    rng = np.random.default_rng(1000 + nch if seed is None else seed)
    pl = pool(rng, nch, 96)
    pl = np.concatenate([pl, mutate_frames(pl[:32], rng, n_flips=2)])
    frames = pl[rng.integers(0, pl.shape[0], (streams, nf))]
    is_plain = rng.random((streams, nf)) < 0.15
    frames[is_plain] = plain(nch)
    return frames


# ---- the reference's tone synthesis ----------------------------------------------------------------------------------------
REF_TONE_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "atrac3plusdsp.c"   /* included, so that its static tables can be written out */
/* argv = n C rec.i32 sub.f32: records [n][REC] as at3pt_unpack_frame writes them, subband samples [C][n][16][128], rewritten in
 * place; ApplyFilter's bookkeeping, then ff_atrac3p_generate_tones where its condition holds, subtracting from the samples */
int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "tables")) {   /* argv = tables out.f32: sine_table, hann_window, amp_sf_tab */
        ff_atrac3p_init_dsp_static();
        FILE* t = fopen(argv[2], "wb");
        fwrite(sine_table, sizeof(float), 2048, t);
        fwrite(hann_window, sizeof(float), 256, t);
        fwrite(amp_sf_tab, sizeof(float), 64, t);
        fclose(t);
        return 0;
    }
    if (argc != 5) return 2;
    const int n = atoi(argv[1]), C = atoi(argv[2]), R = %d;
    int* rec = malloc(sizeof(int) * (size_t)n * R);
    float* sub = malloc(sizeof(float) * (size_t)n * C * 2048);
    FILE* f = fopen(argv[3], "rb");
    if (fread(rec, sizeof(int), (size_t)n * R, f) != (size_t)n * R) return 3;
    fclose(f);
    f = fopen(argv[4], "rb");
    if (fread(sub, sizeof(float), (size_t)n * C * 2048, f) != (size_t)n * C * 2048) return 3;
    fclose(f);
    ff_atrac3p_init_dsp_static();
    static Atrac3pChanUnitCtx u;
    for (int ch = 0; ch < 2; ++ch) {
        u.channels[ch].tones_info = u.channels[ch].tones_info_hist[0];
        u.channels[ch].tones_info_prev = u.channels[ch].tones_info_hist[1];
    }
    u.waves_info = &u.wave_synth_hist[0];
    u.waves_info_prev = &u.wave_synth_hist[1];
    for (int fr = 0; fr < n; ++fr) {
        const int* r = rec + (size_t)fr * R;
        for (int ch = 0; ch < 2; ++ch) memset(u.channels[ch].tones_info, 0, sizeof(Atrac3pWavesData) * 16);
        u.waves_info->tones_present = r[0];
        if (r[0]) {
            memset(u.waves_info->waves, 0, sizeof(u.waves_info->waves));
            u.waves_info->amplitude_mode = 1;
            for (int ch = 0; ch < 2; ++ch)
                for (int b = 0; b < 16; ++b) {
                    const int* t = r + 1 + (ch * 16 + b) * 6;
                    Atrac3pWavesData* w = &u.channels[ch].tones_info[b];
                    w->num_wavs = t[0];
                    w->start_index = t[1];
                    w->pend_env.has_start_point = t[2];
                    w->pend_env.start_pos = t[3];
                    w->pend_env.has_stop_point = t[4];
                    w->pend_env.stop_pos = t[5];
                }
            for (int i = 0; i < 48; ++i) {
                u.waves_info->waves[i].freq_index = r[1 + 192 + i];
                u.waves_info->waves[i].amp_sf = r[1 + 192 + 48 + i];
                u.waves_info->waves[i].phase_index = r[1 + 192 + 96 + i];
            }
        }
        for (int ch = 0; ch < C; ++ch) {
            float* x = sub + ((size_t)ch * n + fr) * 2048;
            if (u.waves_info->tones_present || u.waves_info_prev->tones_present)
                for (int sb = 0; sb < 16; ++sb)
                    if (u.channels[ch].tones_info[sb].num_wavs || u.channels[ch].tones_info_prev[sb].num_wavs) {
                        /* the decoder adds what the encoder's call subtracts: g from a zero buffer, then s - g */
                        float g[128];
                        memset(g, 0, sizeof(g));
                        ff_atrac3p_generate_tones(&u, ch, sb, g);
                        for (int i = 0; i < 128; ++i) x[sb * 128 + i] = x[sb * 128 + i] - g[i];
                    }
        }
        for (int ch = 0; ch < 2; ++ch) {
            Atrac3pWavesData* t = u.channels[ch].tones_info;
            u.channels[ch].tones_info = u.channels[ch].tones_info_prev;
            u.channels[ch].tones_info_prev = t;
        }
        Atrac3pWaveSynthParams* t = u.waves_info;
        u.waves_info = u.waves_info_prev;
        u.waves_info_prev = t;
    }
    f = fopen(argv[4], "wb");
    fwrite(sub, sizeof(float), (size_t)n * C * 2048, f);
    fclose(f);
    return 0;
}
""" % REC_INTS

FF_DIR = os.path.join(REF_SRC, "atrac", "at3p", "ff")
_tone_driver = None


def have_ref_tones():
    return os.path.exists(REF_SO) and os.path.isdir(FF_DIR)


def ref_tone_driver():
    global _tone_driver
    if _tone_driver is None:
        d = tempfile.mkdtemp(prefix="at3ptref_")
        src = os.path.join(d, "tone_driver.c")
        open(src, "w").write(REF_TONE_DRIVER)
        exe = os.path.join(d, "tone_driver")
        subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-w", f"-I{FF_DIR}", src,
                               "-o", exe, "-lm"])
        _tone_driver = exe
    return _tone_driver


def ref_tone_tables():
    """(sine_table, hann_window, amp_sf_tab) as the reference's ff_atrac3p_init_dsp_static builds them"""
    with tempfile.TemporaryDirectory(prefix="at3pttab_") as d:
        p = os.path.join(d, "t.f32")
        subprocess.run([ref_tone_driver(), "tables", p], check=True)
        t = np.fromfile(p, np.float32)
    return t[:2048], t[2048:2304], t[2304:2368]


def unpack_tonal(frames, channels):
    """(specs [N][C][2048], win [N][C], records [N][REC_INTS] int32, reasons [N])"""
    lib = tonal_lib()
    frames = np.ascontiguousarray(frames, np.uint8)
    n = frames.shape[0]
    specs = np.zeros((n, channels, FRAME), np.float32)
    win = np.zeros((n, channels), np.uint16)
    rec = np.zeros((n, REC_INTS), np.int32)
    why = np.zeros(n, np.int32)
    for f in range(n):
        why[f] = lib.at3pt_unpack_frame(_vp(frames[f]), channels, _vp(specs[f]), _vp(win[f]), _vp(rec[f]))
    return specs, win, rec, why


def ref_tonal_back_half(frames, channels):
    """(pcm [N][2048][C] float32, rejected per reason): the restatement's unpack, the reference's synthesis with tones"""
    specs, win, rec, why = unpack_tonal(frames, channels)
    rejected = np.array([(why == k + 1).sum() for k in range(len(REASONS))], np.int64)
    n = specs.shape[0]
    with tempfile.TemporaryDirectory(prefix="at3ptref_run_") as d:
        subs = []
        for ch in range(channels):
            sp, wp, op = (os.path.join(d, x) for x in ("specs.f32", "win.u16", "out.f32"))
            np.ascontiguousarray(specs[:, ch]).tofile(sp)
            np.ascontiguousarray(win[:, ch]).tofile(wp)
            subprocess.run([ref_driver(), str(n), sp, wp, op], check=True)
            subs.append(np.fromfile(op, np.float32).reshape(n, 2048) * RESCALE)   # step 4
        sub = np.ascontiguousarray(np.stack(subs), np.float32)                    # [C][n][2048]
        rp, sbp = os.path.join(d, "rec.i32"), os.path.join(d, "sub.f32")
        rec.tofile(rp)
        sub.tofile(sbp)
        subprocess.run([ref_tone_driver(), str(n), str(channels), rp, sbp], check=True)   # step 4b
        sub = np.fromfile(sbp, np.float32).reshape(channels, n, 2048)
    lib = ctypes.CDLL(REF_SO)
    pcm = np.zeros((n, FRAME, channels), np.float32)
    for ch in range(channels):
        out = np.zeros((n, FRAME), np.float32)
        lib.at3pref_ipqf(_vp(np.ascontiguousarray(sub[ch])), n, _vp(out))
        pcm[:, :, ch] = np.clip(out, np.float32(-1.0), np.float32(1.0))
    return pcm, rejected


# ---- the reference's writer --------------------------------------------------------------------------------------------------
REF_WRITER = r"""
#include "atrac/at3p/at3p_bitstream.h"
#include "atrac/at3p/at3p_gha.h"
#include "atrac/at3p/at3p_tables.h"
#include "atrac/atrac_scale.h"
#include "compressed_io.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
}
// argv = n C specs.f32 blocks.i32 out.u8: specs [n][C][2048]; per frame a block as flat ints (nb, leader, shared[16], then per
// channel and band: start, stop (-1 = absent), wave count, then (freq, amp_sf, phase) per wave; nb = 0: no tonal block)
int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const int n = atoi(argv[1]), C = atoi(argv[2]);
    std::vector<float> specs((size_t)n * C * 2048);
    FILE* f = fopen(argv[3], "rb");
    if (fread(specs.data(), 4, specs.size(), f) != specs.size()) return 3;
    fclose(f);
    f = fopen(argv[4], "rb");
    std::vector<int> blk;
    int v;
    while (fread(&v, 4, 1, f) == 1) blk.push_back(v);
    fclose(f);
    std::vector<std::vector<char>> frames;
    TMem mem(&frames);
    TAt3PBitStream bs(&mem, 2048);
    TScaler<NAt3p::TScaleTable> scaler;
    size_t k = 0;
    FILE* out = fopen(argv[5], "wb");
    for (int fr = 0; fr < n; ++fr) {
        std::vector<TAt3PBitStream::TSingleChannelElement> sces(C);
        for (int ch = 0; ch < C; ++ch) {
            std::vector<float> x(specs.begin() + ((size_t)fr * C + ch) * 2048, specs.begin() + ((size_t)fr * C + ch + 1) * 2048);
            sces[ch].ScaledBlocks = scaler.ScaleFrame(x, NAt3p::TScaleTable::TBlockSizeMod());
        }
        TAt3PGhaData d;
        d.NumToneBands = (uint8_t)blk[k++];
        d.SecondIsLeader = blk[k++] != 0;
        for (int i = 0; i < 16; ++i) d.ToneSharing[i] = blk[k++] != 0;
        for (int ch = 0; ch < C; ++ch)
            for (int i = 0; i < d.NumToneBands; ++i) {
                TAt3PGhaData::TWaveSbInfo sb;
                const int st = blk[k++], sp = blk[k++], nw = blk[k++];
                sb.Envelope = {st < 0 ? TAt3PGhaData::EMPTY_POINT : (uint32_t)st, sp < 0 ? TAt3PGhaData::EMPTY_POINT : (uint32_t)sp};
                sb.WaveIndex = d.Waves[ch].WaveParams.size();
                sb.WaveNums = nw;
                for (int w = 0; w < nw; ++w) {
                    TAt3PGhaData::TWaveParam p;
                    p.FreqIndex = blk[k++];
                    p.AmpSf = blk[k++];
                    p.AmpIndex = 0;
                    p.PhaseIndex = blk[k++];
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
    return 0;
}
"""

_ref_writer = None


def ref_writer():
    global _ref_writer
    if _ref_writer is None:
        d = tempfile.mkdtemp(prefix="at3ptwr_")
        src = os.path.join(d, "ref_writer.cpp")
        open(src, "w").write(REF_WRITER)
        exe = os.path.join(d, "ref_writer")
        libdir = os.path.dirname(REF_SO)
        inc = [f"-I{REF_SRC}", f"-I{REF_SRC}/lib", f"-I{REF_SRC}/lib/liboma/include", f"-I{REF_SRC}/lib/fft/kissfft_impl"]
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-DNDEBUG", *inc, src, "-o", exe, f"-L{libdir}", "-lat3ref",
                               f"-Wl,-rpath,{libdir}"])
        _ref_writer = exe
    return _ref_writer


def _block_ints(C, b):
    if b is None:
        return [0, 0] + [0] * 16
    nb = b["nb"]
    sh = list(b.get("shared", [False] * nb)) + [False] * (16 - nb)
    out = [nb, int(bool(b.get("leader", False)))] + [int(x) for x in sh]
    for ch in range(C):
        for i in range(nb):
            bd = b["bands"][ch][i]
            out += [-1 if bd["start"] is None else bd["start"], -1 if bd["stop"] is None else bd["stop"], len(bd["waves"])]
            for fq, sf, ph in bd["waves"]:
                out += [fq, sf, ph]
    return out


def ref_write_tonal(specs, blocks):
    """the REFERENCE's TAt3PBitStream::WriteFrame(C, &block or nullptr, sces) per frame: specs [n][C][2048], blocks [n]"""
    specs = np.ascontiguousarray(specs, np.float32)
    n, C = specs.shape[0], specs.shape[1]
    with tempfile.TemporaryDirectory(prefix="at3ptwr_run_") as d:
        sp, bp, op = (os.path.join(d, x) for x in ("specs.f32", "blocks.i32", "out.u8"))
        specs.tofile(sp)
        np.array([x for b in blocks for x in _block_ints(C, b)], np.int32).tofile(bp)
        subprocess.run([ref_writer(), str(n), str(C), sp, bp, op], check=True)
        return np.fromfile(op, np.uint8).reshape(n, FRAME)


def n_qu(frame):
    """the frame's quant-unit count: bits 3..7 hold nqu - 1"""
    return (int(frame[0]) & 0x1F) + 1
