"""Helpers of the ATRAC3 decoder's tests, golden generator and benchmark (TEST INFRASTRUCTURE: nothing under atracdenc_amd/
imports this module).

  * CpuDecoder: the C restatement tests/host/at3_decode_cpu.c (the decoder of include/at3hip.h), compiled on first use into a
    temporary directory with the reference's arithmetic flags (gcc -O2 -ffp-contract=off -fno-fast-math).
  * ref_back_half: the restatement's steps 1-2 (unpack, dequantise) followed by the REFERENCE's TAtrac3MDCT::Midct,
    TGainProcessor::Demodulate and TQmf::Synthesis (steps 3-6), run by a small driver compiled at generation time against
    oracle/_ref/libat3ref.so and the reference's headers (atrac3denc.h, which includes gain_processor.h and qmf/qmf.h). Nothing of the reference is stored in the repository.
  * crafted_frames / mutate_frames: malformed and extreme inputs.
  * code_corpus / corpus_expected_spectrum: every mantissa code of the seven selectors at every bit position mod 32 of its unit.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from at3_testlib import REF_SO, _vp

HERE = os.path.dirname(os.path.abspath(__file__))
CPU_SRC = os.path.join(HERE, "host", "at3_decode_cpu.c")
CFLAGS = ["-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]
REF_SRC = "/root/reference/src"
GOLDEN = os.path.join(HERE, "golden", "at3_decode.npz")

# the eight container rows (atrac3.h: ContainerParams): bitrate, frame size, joint stereo
ROWS = ((66150, 192, True), (93713, 272, True), (104738, 304, False), (132300, 384, False), (146081, 424, False),
        (176400, 512, False), (264600, 768, False), (352800, 1024, False))
REASONS = ("bad_id", "unsupported_js", "read_past_end", "tonal_past_end", "bad_tonal_mode", "bad_tonal_quant")
# the codec's end-to-end delay in samples: output sample t of the decoder (frames from the stream's first encoded frame) is input
# sample t - DELAY of the encoder; measured on the restatement (test_round_trip_delay)
DELAY = 1162


class Gains(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32 * 4), ("level", (ctypes.c_int32 * 8) * 4), ("loc", (ctypes.c_int32 * 8) * 4)]


class Fields(ctypes.Structure):
    _fields_ = [("reason", ctypes.c_int32), ("n_qmf", ctypes.c_int32), ("n_bfu", ctypes.c_int32), ("coding_mode", ctypes.c_int32),
                ("g", Gains), ("wl", ctypes.c_int32 * 32), ("sf", ctypes.c_int32 * 32), ("n_tonal", ctypes.c_int32),
                ("tonal_mode", ctypes.c_int32), ("tonal_pos", ctypes.c_int32 * 128), ("tonal_len", ctypes.c_int32 * 128),
                ("tonal_sf", ctypes.c_int32 * 128), ("tonal_quant", ctypes.c_int32 * 128)]


FIELDS_DTYPE = np.dtype([("reason", "<i4"), ("n_qmf", "<i4"), ("n_bfu", "<i4"), ("coding_mode", "<i4"), ("n_points", "<i4", (4,)),
                         ("level", "<i4", (4, 8)), ("loc", "<i4", (4, 8)), ("wl", "<i4", (32,)), ("sf", "<i4", (32,)),
                         ("n_tonal", "<i4"), ("tonal_mode", "<i4"), ("tonal_pos", "<i4", (128,)), ("tonal_len", "<i4", (128,)),
                         ("tonal_sf", "<i4", (128,)), ("tonal_quant", "<i4", (128,))])
assert FIELDS_DTYPE.itemsize == ctypes.sizeof(Fields)


def row_of(frame_sz):
    return next(r for r in ROWS if r[1] == frame_sz)


_cpu_so = None


def cpu_lib(outdir=None):
    """ctypes handle of the restatement (built once per process, into `outdir` or a fresh temporary directory)."""
    global _cpu_so
    if _cpu_so is None:
        d = str(outdir or tempfile.mkdtemp(prefix="at3dec_"))
        so = os.path.join(d, "libat3decode_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, CPU_SRC, "-lm"])
        _cpu_so = so
    lib = ctypes.CDLL(_cpu_so)
    lib.at3d_state_bytes.restype = ctypes.c_size_t
    lib.at3d_fields_bytes.restype = ctypes.c_size_t
    lib.at3d_reset.argtypes = [ctypes.c_void_p]
    lib.at3d_unpack_frame.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.at3d_decode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_void_p]
    assert lib.at3d_fields_bytes() == FIELDS_DTYPE.itemsize
    return lib


class CpuDecoder:
    """One stream of the C restatement; state carries across decode() calls."""

    def __init__(self, frame_sz, js, lib=None):
        self.lib = lib or cpu_lib()
        self.frame_sz, self.js = int(frame_sz), bool(js)
        self.state = np.zeros(self.lib.at3d_state_bytes(), np.uint8)
        self.rejected = np.zeros(len(REASONS), np.uint64)
        self.reset()

    def reset(self):
        self.lib.at3d_reset(_vp(self.state))
        self.rejected[:] = 0

    def decode(self, frames, fields=False):
        """frames [N][frame_sz] uint8 -> pcm [N][1024][2] float32 (and the units' fields [N][2] with fields=True)"""
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.ndim == 2 and frames.shape[1] == self.frame_sz, frames.shape
        n = frames.shape[0]
        pcm = np.zeros((n, 1024, 2), np.float32)
        fl = np.zeros((n, 2), FIELDS_DTYPE) if fields else None
        self.lib.at3d_decode(_vp(self.state), self.frame_sz, int(self.js), _vp(frames), n, _vp(pcm), _vp(self.rejected),
                             _vp(fl) if fields else None)
        return (pcm, fl) if fields else pcm


def cpu_decode(frames, frame_sz, js, fields=False):
    """from start-of-stream state: (pcm [N][1024][2], rejected per reason [6] int64[, fields])"""
    d = CpuDecoder(frame_sz, js)
    r = d.decode(frames, fields)
    pcm, fl = r if fields else (r, None)
    out = (pcm, d.rejected.astype(np.int64).copy())
    return out + (fl,) if fields else out


def unpack(frames, frame_sz, js, lib=None):
    """steps 1-2 of the restatement: (spectra [N][2][1024] float32, fields [N][2])"""
    lib = lib or cpu_lib()
    frames = np.ascontiguousarray(frames, np.uint8)
    n = frames.shape[0]
    specs = np.zeros((n, 2, 1024), np.float32)
    fl = np.zeros((n, 2), FIELDS_DTYPE)
    for f in range(n):
        lib.at3d_unpack_frame(_vp(frames[f]), frame_sz, int(js), _vp(specs[f]), _vp(fl[f]))
    return specs, fl


# ---- the reference's back half --------------------------------------------------------------------------------------------
REF_DRIVER = r"""
#include "atrac3denc.h"   // brings gain_processor.h and qmf/qmf.h (gain_processor.h has no include guard)
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace NAtracDEnc;
using namespace NAtracDEnc::NAtrac3;
typedef TAtrac3Data::SubbandInfo::TGainPoint TGP;
// stdin-free: argv = js n specs.f32 gains.i32 out.f32; specs [n][2][1024], gains [n][2][4][17] = count, level[8], loc[8]
int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const int js = atoi(argv[1]), n = atoi(argv[2]);
    std::vector<float> specs((size_t)n * 2048);
    std::vector<int32_t> gains((size_t)n * 2 * 4 * 17);
    FILE* f = fopen(argv[3], "rb");
    if (fread(specs.data(), sizeof(float), specs.size(), f) != specs.size()) return 3;
    fclose(f);
    f = fopen(argv[4], "rb");
    if (fread(gains.data(), sizeof(int32_t), gains.size(), f) != gains.size()) return 3;
    fclose(f);
    TAtrac3Data tables;   // fills the static windows and gain tables
    (void)tables;
    static TAtrac3MDCT mdct[2];
    static float bands[2][4][512];
    std::vector<TGP> prev[2][4];
    static TQmf<512> q1[2], q2[2];
    static TQmf<1024> q3[2];
    std::vector<float> out((size_t)n * 2048);
    for (int fr = 0; fr < n; ++fr) {
        float sub[2][4][256];
        for (int u = 0; u < 2; ++u) {
            std::vector<TGP> cur[4];
            TAtrac3MDCT::TGainDemodulatorArray dem;
            for (int b = 0; b < 4; ++b) {
                const int32_t* g = &gains[(((size_t)fr * 2 + u) * 4 + b) * 17];
                for (int i = 0; i < g[0]; ++i) cur[b].push_back({(uint32_t)g[1 + i], (uint32_t)g[9 + i]});
                dem[b] = mdct[u].GainProcessor.Demodulate(prev[u][b], cur[b]);
            }
            float* p[4] = {bands[u][0], bands[u][1], bands[u][2], bands[u][3]};
            mdct[u].Midct(&specs[((size_t)fr * 2 + u) * 1024], p, dem);
            for (int b = 0; b < 4; ++b) {
                for (int i = 0; i < 256; ++i) sub[u][b][i] = bands[u][b][i];
                prev[u][b] = cur[b];
            }
        }
        if (js)
            for (int b = 0; b < 4; ++b)
                for (int i = 0; i < 256; ++i) {
                    const float m = sub[0][b][i], s = sub[1][b][i];
                    sub[0][b][i] = m + s;
                    sub[1][b][i] = m - s;
                }
        for (int c = 0; c < 2; ++c) {
            float buf1[512], buf2[512], pcm[1024];
            q1[c].Synthesis(buf1, sub[c][0], sub[c][1]);
            q2[c].Synthesis(buf2, sub[c][3], sub[c][2]);
            q3[c].Synthesis(pcm, buf1, buf2);
            for (int i = 0; i < 1024; ++i) {
                float v = pcm[i];
                v = v > 1.0f ? 1.0f : v;
                v = v < -1.0f ? -1.0f : v;
                out[((size_t)fr * 1024 + i) * 2 + c] = v;
            }
        }
    }
    f = fopen(argv[5], "wb");
    fwrite(out.data(), sizeof(float), out.size(), f);
    fclose(f);
    return 0;
}
"""

_ref_driver = None


def have_ref_back_half():
    return os.path.exists(REF_SO) and os.path.isdir(REF_SRC)


def ref_driver(outdir=None):
    global _ref_driver
    if _ref_driver is None:
        d = outdir or tempfile.mkdtemp(prefix="at3dref_")
        src = os.path.join(d, "at3_ref_back_half.cpp")
        with open(src, "w") as f:
            f.write(REF_DRIVER)
        exe = os.path.join(d, "at3_ref_back_half")
        libdir = os.path.dirname(REF_SO)
        inc = [f"-I{REF_SRC}", f"-I{REF_SRC}/lib", f"-I{REF_SRC}/lib/liboma/include", f"-I{REF_SRC}/lib/fft/kissfft_impl"]
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-DNDEBUG", *inc, src, "-o", exe, f"-L{libdir}", "-lat3ref",
                               f"-Wl,-rpath,{libdir}"])
        _ref_driver = exe
    return _ref_driver


def gains_array(fields):
    """fields [N][2] -> int32 [N][2][4][17] (count, level[8], loc[8] per band)"""
    g = np.zeros(fields.shape + (4, 17), np.int32)
    g[..., 0] = fields["n_points"]
    g[..., 1:9] = fields["level"]
    g[..., 9:17] = fields["loc"]
    return g


def ref_back_half(frames, frame_sz, js):
    """(pcm [N][1024][2] float32, rejected per reason, fields): the restatement's unpack, the reference's synthesis"""
    specs, fl = unpack(frames, frame_sz, js)
    rejected = np.array([(fl["reason"] == k + 1).sum() for k in range(len(REASONS))], np.int64)
    n = specs.shape[0]
    with tempfile.TemporaryDirectory(prefix="at3dref_run_") as d:
        sp, gp, op = (os.path.join(d, x) for x in ("specs.f32", "gains.i32", "out.f32"))
        specs.tofile(sp)
        gains_array(fl).tofile(gp)
        subprocess.run([ref_driver(), str(int(js)), str(n), sp, gp, op], check=True)
        pcm = np.fromfile(op, np.float32).reshape(n, 1024, 2)
    return pcm, rejected, fl


# ---- crafted frames -------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self, nbytes):
        self.buf = bytearray(nbytes)
        self.pos = 0

    def put(self, v, n):
        for k in range(n - 1, -1, -1):
            if self.pos < len(self.buf) * 8 and (v >> k) & 1:
                self.buf[self.pos >> 3] |= 0x80 >> (self.pos & 7)
            self.pos += 1


_VLC = None


def vlc_tables():
    """{selector 1..7: [(code, length)] by symbol} parsed from c_huff, c_huff_off (csrc/at3_common.hpp) and c_huff_size
    (csrc/at3_decode.hpp): the 130 entries the decoder's look-up is expanded from (selectors 1 and 4 share their nine)"""
    global _VLC
    if _VLC is None:
        import re
        csrc = os.path.join(HERE, "..", "atracdenc_amd", "csrc")
        common, dec = open(os.path.join(csrc, "at3_common.hpp")).read(), open(os.path.join(csrc, "at3_decode.hpp")).read()
        body = common[common.index("c_huff[130] = {"):]
        flat = [(int(c, 16), int(n)) for c, n in re.findall(r"HE\((0x[0-9A-Fa-f]+), (\d+)\)", body[:body.index("};")])]
        off = [int(x) for x in re.search(r"c_huff_off\[7\] = \{([^}]*)\}", common).group(1).split(",")]
        size = [int(x) for x in re.search(r"c_huff_size\[7\] = \{([^}]*)\}", dec).group(1).split(",")]
        assert len(flat) == 130
        _VLC = {s: flat[off[s - 1]:off[s - 1] + size[s - 1]] for s in range(1, 8)}
    return _VLC


# what a symbol stands for: a pair of mantissas at selector 1, else symbols 0, 1, 2, 3, 4 .. = mantissas 0, 1, -1, 2, -2 ..
VLC_PAIRS = [(0, 0), (0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)]


def vlc_mantissas(selector, sym):
    return VLC_PAIRS[sym] if selector == 1 else ((sym + 1) >> 1 if sym & 1 else -(sym >> 1),)


HUFF = {1: [(0x0, 1), (0x4, 3), (0x5, 3), (0xC, 4), (0xD, 4), (0x1C, 5), (0x1D, 5), (0x1E, 5), (0x1F, 5)],
        2: [(0x0, 1), (0x4, 3), (0x5, 3), (0x6, 3), (0x7, 3)],
        3: [(0x0, 1), (0x4, 3), (0x5, 3), (0xC, 4), (0xD, 4), (0xE, 4), (0xF, 4)]}


def make_unit(nbytes, js_second=False, js_params=(0, 7, 3, 3, 3, 3), unit_id=None, gains=((),), tonal=None, nbfu=32,
              coding_mode=1, wl=None, sf=None, mant=None, trace=None):
    """A unit from its fields. gains: per QMF band a list of (level, location); tonal: (mode, [(flags, coded_values, quant,
    [(block, [(sf, rel_pos, [raw mantissa bits])])])]) written with CLC (mode 1) or as raw words; wl / sf per BFU;
    mant(bfu, i, bits) -> raw CLC word with coding_mode 1 (CLC), the symbol of selector wl[bfu] with coding_mode 0 (VLC: bits is
    then the position of the code in the unit; a symbol of selector 1 is a pair of lines). trace: a list that receives (selector,
    symbol, bit position, length) of every VLC code. Bits past nbytes are dropped."""
    w = BitWriter(nbytes)
    if js_second:
        weight, delay, *mats = js_params
        w.put(weight, 1)
        w.put(delay, 3)
        for m in mats:
            w.put(m, 2)
        w.put(3 if unit_id is None else unit_id, 2)
    else:
        w.put(0x28 if unit_id is None else unit_id, 6)
    w.put(len(gains) - 1, 2)
    for pts in gains:
        w.put(len(pts), 3)
        for lev, loc in pts:
            w.put(lev, 4)
            w.put(loc, 5)
    if not tonal:
        w.put(0, 5)
    else:
        mode, groups = tonal
        w.put(len(groups), 5)
        w.put(mode, 2)
        for flags, cv, q, blocks in groups:
            for fl in flags:
                w.put(fl, 1)
            w.put(cv - 1, 3)
            w.put(q, 3)
            for comps in blocks:
                w.put(len(comps), 3)
                for csf, rel, vals in comps:
                    w.put(csf, 6)
                    w.put(rel, 6)
                    for v in vals:
                        w.put(v & ((1 << [0, 4, 3, 3, 4, 4, 5, 6][q]) - 1), [0, 4, 3, 3, 4, 4, 5, 6][q])
    wl = list(wl) if wl is not None else [0] * 32
    sf = list(sf) if sf is not None else [0] * 32
    w.put(nbfu - 1, 5)
    w.put(coding_mode, 1)
    for i in range(nbfu):
        w.put(wl[i], 3)
    for i in range(nbfu):
        if wl[i]:
            w.put(sf[i], 6)
    start = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 224, 256, 288, 320, 352, 384, 416, 448,
             480, 512, 576, 640, 704, 768, 896, 1024]
    clc = [0, 4, 3, 3, 4, 4, 5, 6]
    for i in range(nbfu):
        if wl[i]:
            cnt = (start[i + 1] - start[i]) // (2 if wl[i] == 1 else 1)
            for k in range(cnt):
                if coding_mode == 0:
                    sym = mant(i, k, w.pos) if mant else 0
                    code, n = vlc_tables()[wl[i]][sym]
                    if trace is not None:
                        trace.append((wl[i], sym, w.pos, n))
                    w.put(code, n)
                else:
                    w.put(mant(i, k, clc[wl[i]]) if mant else 0, clc[wl[i]])
    return bytes(w.buf)


def frame_of(units, frame_sz, js):
    """two units -> one frame (unit 1 of a joint-stereo frame is stored reversed from the end; the units overlap where their
    bytes are both non-zero: OR-ed)"""
    if not js:
        h = frame_sz // 2
        return np.frombuffer(units[0][:h].ljust(h, b"\0") + units[1][:h].ljust(h, b"\0"), np.uint8)
    a = np.frombuffer(units[0][:frame_sz].ljust(frame_sz, b"\0"), np.uint8)
    b = np.frombuffer(units[1][:frame_sz].ljust(frame_sz, b"\0"), np.uint8)[::-1]
    return a | b


def crafted_frames(frame_sz, js, seed):
    """Malformed and extreme frames [N][frame_sz]: every rejection reason, tonal components at the spectrum's edge, seven gain
    points in every band, full-scale spectra that clamp, and seeded random bytes."""
    rng = np.random.default_rng(seed)
    nb = frame_sz if js else frame_sz // 2
    ok = make_unit(nb, js_second=False, nbfu=4, wl=[3] * 4, sf=[40] * 4, mant=lambda b, i, n: (i * 3 + b) & 7)
    ok2 = make_unit(nb, js_second=js, nbfu=2, wl=[2, 2], sf=[30, 30], mant=lambda b, i, n: i & 7) if js else ok
    units = []

    def add(u0, u1=None):
        units.append(frame_of((u0, u1 if u1 is not None else ok2), frame_sz, js))

    small = nb if not js else frame_sz // 2   # keep unit 0 of a joint-stereo frame to the front half
    add(make_unit(small, unit_id=0x29))                                               # bad id
    add(ok, make_unit(small, js_second=js, unit_id=(2 if js else 0x00)))              # bad id of unit 1
    if js:
        for params in ((1, 7, 3, 3, 3, 3), (0, 5, 3, 3, 3, 3), (0, 7, 3, 0, 3, 3), (0, 7, 1, 2, 3, 0)):
            add(ok, make_unit(small, js_second=True, js_params=params))                # unsupported joint stereo
    # read past the end: every BFU at word length 7 needs far more than the unit holds
    add(make_unit(nb, nbfu=32, wl=[7] * 32, sf=[10] * 32, mant=lambda b, i, n: 0x15))
    # gain points: seven per band in every band, rising, falling, equal and unordered locations, every level
    g7 = [[((b * 5 + i * 3) % 16, min(31, 2 + 4 * i + b)) for i in range(7)] for b in range(4)]
    g_odd = [[(15, 31), (0, 0), (7, 3)], [(0, 31)], [(15, 0), (15, 0)], [(4, 16), (3, 8), (5, 24), (1, 30)]]
    spec = dict(nbfu=20, wl=[5] * 20, sf=[45 + (b % 10) for b in range(20)], mant=lambda b, i, n: (i * 7 + b * 3) & 15)
    add(make_unit(small, gains=g7, **spec), make_unit(small, js_second=js, gains=g_odd, **spec))
    add(make_unit(small, gains=g_odd, **spec), make_unit(small, js_second=js, gains=g7, **spec))
    add(make_unit(small, gains=[[], [(0, 0)], [], []], **spec))
    # tonal components: CLC mode, at the last lines of the spectrum (block 15, positions 56 .. 63), one past the end, every
    # coded-value count; bad mode (2, 3) and bad quantisers (0, 1)
    all4 = [[1, 1, 1, 1]]

    def tonal_unit(mode, q, cv, blocks, **kw):
        return make_unit(small, gains=[[], [], [], []], tonal=(mode, [(all4[0], cv, q, blocks)]), nbfu=1, wl=[0], **kw)

    edge = [[] for _ in range(15)] + [[(50, 64 - 8, [3, -2, 1, 0, -1, 2, 3, -3])]]
    add(tonal_unit(1, 4, 8, edge))
    add(tonal_unit(1, 7, 1, [[] for _ in range(15)] + [[(63, 63, [31])]]))
    add(tonal_unit(1, 3, 2, [[] for _ in range(15)] + [[(40, 63, [1, 1])]]))                    # runs past line 1023
    add(tonal_unit(1, 5, 3, [[(20, 0, [1, 2, 3]), (20, 0, [-1, -2, -3]), (33, 1, [7, 7, 7])]] + [[]] * 15))   # overlapping
    add(tonal_unit(2, 4, 2, [[(40, 3, [1, 1])]] + [[]] * 15))
    add(tonal_unit(3, 4, 2, [[(40, 3, [1, 1])]] + [[]] * 15))
    add(tonal_unit(1, 0, 2, [[(40, 3, [1, 1])]] + [[]] * 15))
    add(tonal_unit(1, 1, 2, [[(40, 3, [1, 1])]] + [[]] * 15))
    # full scale: scale factor 63 (1.0) and the largest mantissas: decodes far beyond +-1 and clamps
    add(make_unit(small, nbfu=12, wl=[7] * 12, sf=[63] * 12, mant=lambda b, i, n: 31 if (i + b) % 2 else 0x21))
    add(make_unit(small, nbfu=8, coding_mode=1, wl=[1] * 8, sf=[63] * 8, mant=lambda b, i, n: (i * 5 + b) & 15))
    units += [rng.integers(0, 256, frame_sz, dtype=np.uint8) for _ in range(8)]
    return np.ascontiguousarray(np.stack(units))


def mutate_frames(frames, rng, n_flips=3):
    """copies of `frames` with n_flips random bits flipped each"""
    out = frames.copy()
    for f in range(out.shape[0]):
        for _ in range(n_flips):
            p = int(rng.integers(0, out.shape[1] * 8))
            out[f, p >> 3] ^= 0x80 >> (p & 7)
    return out


# ---- the fuzz inputs of the GPU tests and of the SIMT-harness tests (the same bytes from the same seeds) ----------------------
def fuzz_frames(golden, fsz, n_streams, n_frames, seed):
    """encoder frames of the row, the same with a few bits flipped, crafted frames and random bytes, shuffled per stream"""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([golden[f"{c}_frames"] for c in golden["cases"] if int(golden[f"{c}_row"][0]) == fsz])
    out = np.empty((n_streams, n_frames, fsz), np.uint8)
    for s in range(n_streams):
        enc = pool[rng.integers(0, pool.shape[0], n_frames)]
        kind = rng.integers(0, 4, n_frames)
        mut = mutate_frames(enc, rng, n_flips=int(rng.integers(1, 6)))
        rnd = rng.integers(0, 256, (n_frames, fsz), dtype=np.uint8)
        out[s] = np.where((kind == 0)[:, None], enc, np.where((kind == 1)[:, None], mut, rnd))
        k = min(n_frames, 8)
        out[s, :k] = crafted_frames(fsz, fsz in (192, 272), seed=seed + s)[:k]
    return out


def cpu_ref(frames, fsz, js):
    """[S][N][fsz] -> ([S][N][1024][2], rejected per reason summed over streams)"""
    outs, rej = [], np.zeros(len(REASONS), np.int64)
    for s in range(frames.shape[0]):
        d = CpuDecoder(fsz, js)
        outs.append(d.decode(frames[s]))
        rej += d.rejected.astype(np.int64)
    return np.stack(outs), rej.tolist()


# ---- the exhaustive code corpus ---------------------------------------------------------------------------------------------
# Every code of the seven selectors at every bit position mod 32 of its unit, in a plain unit and in the byte-reversed second unit of a
# joint-stereo frame. A unit of (selector s, shift r) has r % 4 gain points in its first band, a prefix BFU 0 of selector 7 whose
# eight symbols are searched so that BFU 1's first code starts at r mod 32, and behind it BFUs of selector s that carry the
# selector's symbols in symbol order, again and again to the end of the last BFU. Frame (s, r) holds the units (s, r) and (8 - s, r).
BFU_START = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 224, 256, 288, 320, 352, 384, 416, 448, 480, 512,
             576, 640, 704, 768, 896, 1024]
CORPUS_SHIFTS = 32
_PREFIX_FILLS = None


def _prefix_fills():
    """{bits: eight symbols of selector 7}, one way per total"""
    global _PREFIX_FILLS
    if _PREFIX_FILLS is None:
        by_len = {}
        for sym, (_, n) in enumerate(vlc_tables()[7]):
            by_len.setdefault(n, sym)
        reach = {0: ()}
        for _ in range(8):
            reach = {t + n: syms + (sym,) for t, syms in reversed(list(reach.items())) for n, sym in by_len.items()}
        _PREFIX_FILLS = reach
        assert len({b % 32 for b in reach}) == 32
    return _PREFIX_FILLS


def corpus_unit(nbytes, selector, r, js_second):
    """(unit bytes, trace [(selector, symbol, position, length)], mantissas int [1024], wl [32], sf [32])"""
    table = vlc_tables()[selector]
    per = 2 if selector == 1 else 1
    nbfu = next(n for n in range(2, 33) if BFU_START[n] - 8 >= len(table) * per)
    wl = [7] + [selector] * (nbfu - 1)
    sf = [(2 * r + 5 * selector + b) % 64 for b in range(nbfu)]
    prefix = {}

    def mant(bfu, k, pos):
        if bfu:
            return ((BFU_START[bfu] - 8) // per + k) % len(table)
        if not prefix:   # k == 0: pos is where BFU 0 starts
            need = (r - pos) % 32
            prefix["syms"] = next(v for b, v in sorted(_prefix_fills().items()) if b % 32 == need)
        return prefix["syms"][k]

    trace = []
    gains = [[(4 + i, 3 + 5 * i) for i in range(r % 4)]]
    unit = make_unit(nbytes, js_second=js_second, gains=gains, nbfu=nbfu, coding_mode=0, wl=wl, sf=sf, mant=mant, trace=trace)
    assert trace[8][2] % 32 == r and trace[-1][2] + trace[-1][3] <= 8 * nbytes, (selector, r, trace[8], trace[-1])
    lines = np.zeros(1024, np.int32)
    k = 0
    for sel, sym, _, _ in trace:
        m = vlc_mantissas(sel, sym)
        lines[k:k + len(m)] = m
        k += len(m)
    assert k == BFU_START[nbfu]
    wl32, sf32 = np.zeros(32, np.int32), np.zeros(32, np.int32)
    wl32[:nbfu], sf32[:nbfu] = wl, sf
    return unit, trace, lines, wl32, sf32


_CORPUS = {}


def code_corpus(js):
    """The corpus of plain units (js False) or joint-stereo frames (js True), built once per process: a dict of frame_sz (the
    smallest container row of that kind that holds every frame), frames [32][7][frame_sz] uint8 (stream = shift, frame = selector - 1),
    mant int32 [32][7][2][1024], wl / sf int32 [32][7][2][32]. Its own assertion: each of the 130 + 9 (selector, symbol) codes at every
    bit position mod 32, in unit 0 and in unit 1."""
    if js in _CORPUS:
        return _CORPUS[js]
    for _, fsz, row_js in ROWS:
        if row_js != js:
            continue
        nb = fsz if js else fsz // 2
        frames = np.zeros((CORPUS_SHIFTS, 7, fsz), np.uint8)
        mant, wl, sf = (np.zeros((CORPUS_SHIFTS, 7, 2) + tail, np.int32) for tail in ((1024,), (32,), (32,)))
        seen = set()
        try:
            for r in range(CORPUS_SHIFTS):
                for s in range(1, 8):
                    units, bits = [], 0
                    for u, sel in enumerate((s, 8 - s)):
                        unit, trace, mant[r, s - 1, u], wl[r, s - 1, u], sf[r, s - 1, u] = corpus_unit(nb, sel, r, js and u == 1)
                        units.append(unit)
                        bits += trace[-1][2] + trace[-1][3]
                        seen.update((u, sel, sym, pos % 32) for sel, sym, pos, _ in trace)
                    assert bits <= 8 * fsz
                    frames[r, s - 1] = frame_of(units, fsz, js)
        except AssertionError:
            continue   # the row is too small
        every = {(u, s, sym, ph) for u in range(2) for s in range(1, 8) for sym in range(len(vlc_tables()[s])) for ph in range(32)}
        assert seen == every and len(every) == 2 * 139 * 32
        _CORPUS[js] = dict(frame_sz=fsz, frames=frames, mant=mant, wl=wl, sf=sf)
        return _CORPUS[js]
    raise AssertionError(js)


def corpus_expected_spectrum(corpus):
    """(float32(m) * ScaleTable[sf]) * InvMaxQuant[wl], two roundings left to right, with ScaleTable[i] = 2^(i / 3 - 21) and
    InvMaxQuant[wl] = 1 / (1.5, 2.5, 3.5, 4.5, 7.5, 15.5, 31.5)[wl - 1] rounded once to float: [32][7][2][1024] float32"""
    scale = np.array([2.0 ** (i / 3.0 - 21.0) for i in range(64)]).astype(np.float32)
    inv = np.array([0.0] + [1.0 / q for q in (1.5, 2.5, 3.5, 4.5, 7.5, 15.5, 31.5)]).astype(np.float32)
    bfu_of_line = np.repeat(np.arange(32), np.diff(BFU_START))
    wl_line, sf_line = corpus["wl"][..., bfu_of_line], corpus["sf"][..., bfu_of_line]
    q = (corpus["mant"].astype(np.float32) * scale[sf_line]).astype(np.float32)
    return (q * inv[wl_line]).astype(np.float32)


# ---- files -----------------------------------------------------------------------------------------------------------------
def oma_bytes(frames, frame_sz, js, codec_id=0):
    """an OMA file as at3hip_io.hpp's TOmaOutput writes it: 96-byte EA3 header, then the frames"""
    h = bytearray(96)
    h[0:3] = b"EA3"
    h[3], h[5], h[6], h[7] = 1, 96, 0xFF, 0xFF
    word = (codec_id << 24) | (int(js) << 17) | (1 << 13) | (frame_sz // 8)
    h[32:36] = word.to_bytes(4, "big")
    return bytes(h) + np.ascontiguousarray(frames, np.uint8).tobytes()


def riff_at3_bytes(frames, frame_sz, js, nch=2, tag=0x270, data=True):
    """an ATRAC3 RIFF/WAVE file as TAt3RiffOutput writes it (format tag 0x270, 14 bytes of extradata, "fact", "data")"""
    import struct
    body = np.ascontiguousarray(frames, np.uint8).tobytes()
    n = len(body) // frame_sz
    fmt = struct.pack("<HHIIHHH", tag, nch, 44100, frame_sz * 44100 // 1024, frame_sz, 0, 14) + \
        struct.pack("<HIHHHH", 1, 0x1000, int(js), int(js), 1, 0)
    out = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"fact" + struct.pack("<III", 8, n * 1024, 1024)
    if data:
        out += b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", len(out)) + out


def container_frames(data, frame_sz):
    """the frames of an OMA or ATRAC3 RIFF file written by at3hipenc"""
    if data[:3] == b"EA3":
        body = data[96:]
    else:
        i = data.index(b"data")
        n = int.from_bytes(data[i + 4:i + 8], "little")
        body = data[i + 8:i + 8 + n]
    return np.frombuffer(body[:len(body) // frame_sz * frame_sz], np.uint8).reshape(-1, frame_sz)
