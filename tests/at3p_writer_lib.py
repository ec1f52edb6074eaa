"""Helpers of the ATRAC3plus adaptive-writer tests (word lengths per frame, frame sizes, sparse and rate-distortion word lengths),
their golden generators, SIMT-harness drivers and bench tools (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * writer_lib: the C restatement tests/host/at3p_rd_cpu.c, which includes at3p_writer_cpu.c (include/at3phip.h: ADAPTIVE WORD
    LENGTHS with FRAME SIZE and SPARSE WORD LENGTHS), at3p_tonal_cpu.c and at3p_decode_cpu.c; compiled once, on first use, with the
    reference's arithmetic flags.
  * tail_bits_list: the frame's tail (window shapes, gain-compensation bits, tonal flag and block, noise flag, terminator) with the
    restated tonal-block writer of at3p_tonal_lib.
  * write_adaptive / write_rd / write_streams / cost_table / tables / allocate / allocate_rd: the writer's entry points;
    Decoder / decode / decode_streams / unpack: the decoder's, each with the frame size and `sparse`.
  * parse_head: an independent parser of a frame's head, written from the header's text; recount_bits (word-length section by the
    oracle's at3po_wordlen_bits, the reference's coder) and count_bits (pure Python): Bits(A) recounted from its output.
  * the signals, frame sizes, edge cases, random tables and bounds of the tests, and the cases of tests/golden/at3p_alloc.npz,
    at3p_sparse.npz, at3p_rd.npz and at3p_writer_fold.npz.
"""
import ctypes
import functools
import hashlib
import os
import re
import subprocess
import tempfile

import numpy as np

from at3_testlib import ORACLE_SO, _vp, at3p_specs, oracle
from at3p_decode_lib import CFLAGS, FIELDS_DTYPE, REASONS
from at3p_tonal_lib import tonal_bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WRITER_SRC = os.path.join(HERE, "host", "at3p_rd_cpu.c")
SIZE_BITS = 2048 * 8 - 3
T_MIN, T_MAX, K_MAX = -21, 63, 64
J_MIN, J_MAX = -30, 69
INFO_DTYPE = np.dtype([("t", "<i4"), ("k", "<i4"), ("num_quant_units", "<i4"), ("bits", "<i4"), ("wl", "u1", (2, 32)), ("sfi", "u1", (2, 32)),
                       ("tab", "u1", (2, 32))])
# rate-distortion and masking-weighted frames: chose, T and T_sparse are the guard's outcome and its two sums (T of R4, Tw of M6); O, o and
# mu are M3's and M2's, zero for rate-distortion frames
RD_INFO_DTYPE = np.dtype([("j", "<i4"), ("k", "<i4"), ("num_quant_units", "<i4"), ("bits", "<i4"), ("chose", "<i4"), ("t", "<i4"),
                          ("k_sparse", "<i4"), ("O", "<i4"), ("T", "<f8"), ("T_sparse", "<f8"), ("o", "u1", (2, 32)), ("mu", "<i4", (2, 32)),
                          ("wl", "u1", (2, 32)), ("sfi", "u1", (2, 32)), ("tab", "u1", (2, 32))])
SIGNALS = ("noise", "mix", "stress", "tones", "burst")
SNR_FRAMES = 14
QU_START = [0, 16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 224, 256, 288, 320, 352, 384, 448, 512, 576, 640, 704, 768, 896, 1024, 1152, 1280, 1408,
            1536, 1664, 1792, 1920, 2048]
QU_TO_SB = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
SB_POWGRPS = [1, 2, 2, 3, 3, 3, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5]
LINES = np.diff(np.array(QU_START))
MIN_BYTES = {1: 176, 2: 224}                       # AT3PHIP_MIN_FRAME_BYTES_MONO / _STEREO (test_min_frame_bytes derives them)
# kbit/s -> frame bytes, the command line's table (atracdenc_amd/host/at3hipenc.cpp, kAt3pRates)
BITRATES = {32: 192, 48: 280, 64: 376, 96: 560, 128: 744, 160: 936, 192: 1120, 256: 1488, 320: 1864, 352: 2048}
# where a guard or a stride can go wrong: the minimum, table sizes, 2040 (admissible, not in the table) and 2048
SIZES = {1: (192, 376, 2040, 2048), 2: (MIN_BYTES[2], 280, 376, 1120, 1864, 2040, 2048)}

_so = None


def writer_lib():
    global _so
    if _so is None:
        d = tempfile.mkdtemp(prefix="at3pwriter_")
        so = os.path.join(d, "libat3pwriter_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, WRITER_SRC, "-lm"])
        _so = so
    lib = ctypes.CDLL(_so)
    I, P = ctypes.c_int, ctypes.c_void_p
    lib.at3pw_state_bytes.restype = ctypes.c_size_t
    lib.at3pw_reset.argtypes = [P]
    lib.at3pw_decode.argtypes = [P, I, P, I, I, P, P, I, I]
    lib.at3pw_unpack_frame.argtypes = [P, I, I, P, P, I, I, P]
    lib.at3pw_write_frames.argtypes = [P, I, I, I, I, P, P, P, P]
    lib.at3pw_allocate.argtypes = [P, P, I, I, I, I, P, P, P, P]
    lib.at3pw_cost_table.argtypes = [P, I, P, P, P, P]
    lib.at3prd_tables.argtypes = [P, I, P, P, P, P, P]
    lib.at3prd_allocate.argtypes = [P, P, P, P, I, I, I, I, P, P, P]
    lib.at3prd_write_frames.argtypes = [P, I, I, I, I, P, P, P, P]
    assert lib.at3pw_frame_info_size() == INFO_DTYPE.itemsize and lib.at3prd_frame_info_size() == RD_INFO_DTYPE.itemsize
    assert (lib.at3prd_j_min(), lib.at3prd_j_max()) == (J_MIN, J_MAX)
    return lib


# ---- the tail ------------------------------------------------------------------------------------------------------------------
def tail_bits_list(nch, win=None, block=None):
    """[(value, nbits)] of the tail as TTonalComponentEncoder forms it: win uint16 [nch] or None, block a dict of at3p_tonal_lib or
    None"""
    w = [(0, 2)] if nch == 2 else []
    for ch in range(nch):
        fl = 0 if win is None else int(win[ch])
        if fl == 0:
            w.append((0, 1))
        elif (fl & 0xff) == 0xff:     # TAt3pMDCTWin::IsAllSteep keeps its mask in a uint8_t
            w += [(1, 1), (0, 1)]
        else:
            w += [(1, 1), (1, 1)] + [((fl >> i) & 1, 1) for i in range(16)]
    w += [(0, 1)] * nch               # gain compensation
    w += [(0, 1)] if block is None else [(1, 1)] + list(tonal_bits(nch, block))
    return w + [(0, 1), (3, 2)]       # no noise info, terminator


def pack_tail(bits_list, nbytes):
    bits = [(v >> k) & 1 for v, n in bits_list for k in range(n - 1, -1, -1)]
    out = np.zeros(nbytes * 8, np.uint8)
    out[:len(bits)] = bits
    return np.packbits(out), len(bits)


def _blocks_as_dicts(nch, blocks, n):
    """blocks: None, a list of dicts / None, or records of the binding's tonal block dtype"""
    if blocks is None:
        return [None] * n
    if isinstance(blocks, np.ndarray):
        from at3p_gha_lib import block_dict
        return [block_dict(r, nch) for r in blocks.reshape(-1)]
    return list(blocks)


# ---- the encoder ---------------------------------------------------------------------------------------------------------------
def _write(call, dtype, specs, frame_bytes, win, blocks, info):
    lib = writer_lib()
    specs = np.ascontiguousarray(specs, np.float32)
    n, nch = specs.shape[0], specs.shape[1]
    tb = lib.at3pw_tail_bytes()
    tails, nbits = np.zeros((n, tb), np.uint8), np.zeros(n, np.int32)
    for f, b in enumerate(_blocks_as_dicts(nch, blocks, n)):
        tails[f], nbits[f] = pack_tail(tail_bits_list(nch, None if win is None else win[f], b), tb)
    out, rec = np.zeros((n, frame_bytes), np.uint8), np.zeros(n, dtype)
    assert call(lib, _vp(specs), nch, n, _vp(tails), _vp(nbits), _vp(out), _vp(rec)) == n
    return (out, rec, nbits) if info else out


def write_adaptive(specs, frame_bytes=2048, sparse=False, win=None, blocks=None, info=False):
    """specs float32 [n, C, 2048], win uint16 [n, C] or None, blocks [n] (dicts, records or None) -> frames uint8 [n, frame_bytes]
    (and the per-frame records of INFO_DTYPE and the tails' bits with info=True)"""
    return _write(lambda lib, sp, nch, n, tails, nbits, out, rec: lib.at3pw_write_frames(sp, nch, n, int(frame_bytes), int(bool(sparse)), tails, nbits,
                                                                                         out, rec), INFO_DTYPE, specs, frame_bytes, win, blocks, info)


def write_rd(specs, frame_bytes, win=None, blocks=None, info=False, psy=False):
    """the same with RATE-DISTORTION WORD LENGTHS, or with psy MASKING-WEIGHTED WORD LENGTHS (sparse frames; records of RD_INFO_DTYPE: j*,
    k*, which of the two allocations was written, both T, and with psy the offsets)"""
    return _write(lambda lib, sp, nch, n, tails, nbits, out, rec: lib.at3prd_write_frames(sp, nch, n, int(frame_bytes), int(bool(psy)), tails, nbits,
                                                                                          out, rec), RD_INFO_DTYPE, specs, frame_bytes, win, blocks, info)


def write_streams(specs, frame_bytes=2048, sparse=False, win=None, blocks=None):
    """write_adaptive for [S, F, C, 2048] -> [S, F, frame_bytes]"""
    S, F = specs.shape[:2]
    flat = write_adaptive(specs.reshape((S * F,) + specs.shape[2:]), frame_bytes, sparse, None if win is None else win.reshape(S * F, -1),
                          None if blocks is None else (blocks.reshape(-1) if isinstance(blocks, np.ndarray) else blocks))
    return flat.reshape(S, F, frame_bytes)


def tables(spec):
    """A1 + A2 + R1 of one frame [C, 2048]: (sfi uint8 [C, 32], bits uint16 [C, 32, 8], dist uint64 [C, 32, 8])"""
    spec = np.ascontiguousarray(spec, np.float32)
    nch = spec.shape[0]
    sfi, bits, tab = np.zeros((nch, 32), np.uint8), np.zeros((nch, 32, 8), np.uint16), np.zeros((nch, 32, 8), np.uint8)
    dist = np.zeros((nch, 32, 8), np.uint64)
    assert writer_lib().at3prd_tables(_vp(spec), nch, _vp(sfi), _vp(bits), _vp(tab), _vp(dist), None) == 0
    return sfi, bits, dist


def cost_table(spec):
    """A1 + A2 of one frame [C, 2048]: (sfi uint8 [C, 32], bits uint16 [C, 32, 8], tab uint8 [C, 32, 8]; entry 0 of both unused)"""
    spec = np.ascontiguousarray(spec, np.float32)
    nch = spec.shape[0]
    sfi, bits, tab = np.zeros((nch, 32), np.uint8), np.zeros((nch, 32, 8), np.uint16), np.zeros((nch, 32, 8), np.uint8)
    assert writer_lib().at3pw_cost_table(_vp(spec), nch, _vp(sfi), _vp(bits), _vp(tab), None) == 0
    return sfi, bits, tab


def allocate(sfi, bits, tail_bits, frame_bytes=2048, sparse=False):
    """A3-A5 of the restatement against 8 * frame_bytes - 3: (wl uint8 [C, 32], N, t*, k*, Bits)"""
    sfi, bits = np.ascontiguousarray(sfi, np.uint8), np.ascontiguousarray(bits, np.uint16)
    nch = sfi.shape[0]
    wl, out = np.zeros((nch, 32), np.uint8), np.zeros(3, np.int32)
    total = writer_lib().at3pw_allocate(_vp(sfi), _vp(bits), nch, int(tail_bits), int(frame_bytes), int(bool(sparse)), _vp(wl), _vp(out[0:1]),
                                        _vp(out[1:2]), _vp(out[2:3]))
    return wl, int(out[0]), int(out[1]), int(out[2]), int(total)


def allocate_rd(sfi, bits, dist, tail_bits, frame_bytes, offsets=None, psy=False):
    """R2-R4 of the restatement, or M1-M6 with psy or with offsets uint8 [C, 32], which replace M1-M3's: (wl uint8 [C, 32], N, record of
    RD_INFO_DTYPE with j, k, chose, t, k_sparse, O, T, T_sparse, o, mu, bits)"""
    sfi, bits, dist = np.ascontiguousarray(sfi, np.uint8), np.ascontiguousarray(bits, np.uint16), np.ascontiguousarray(dist, np.uint64)
    nch = sfi.shape[0]
    off = None if offsets is None else np.ascontiguousarray(offsets, np.uint8)
    wl, n, rec = np.zeros((nch, 32), np.uint8), np.zeros(1, np.int32), np.zeros(1, RD_INFO_DTYPE)
    rec["bits"] = writer_lib().at3prd_allocate(_vp(sfi), _vp(bits), _vp(dist), None if off is None else _vp(off), int(bool(psy)), nch, int(tail_bits),
                                               int(frame_bytes), _vp(wl), _vp(n), _vp(rec))
    return wl, int(n[0]), rec[0]


# ---- the decoder ---------------------------------------------------------------------------------------------------------------
class Decoder:
    """One stream of the restatement; state carries across decode() calls, the frame size may change between them."""

    def __init__(self, channels, tones=False, sparse=False):
        self.lib = writer_lib()
        self.channels, self.tones, self.sparse = int(channels), int(bool(tones)), int(bool(sparse))
        self.state = np.zeros(self.lib.at3pw_state_bytes(), np.uint8)
        self.rejected = np.zeros(len(REASONS), np.uint64)
        self.lib.at3pw_reset(_vp(self.state))

    def decode(self, frames):
        """frames [N][frame_bytes] uint8 -> pcm [N][2048][channels] float32"""
        frames = np.ascontiguousarray(frames, np.uint8)
        n, fb = frames.shape
        pcm = np.zeros((n, 2048, self.channels), np.float32)
        self.lib.at3pw_decode(_vp(self.state), self.channels, _vp(frames), fb, n, _vp(pcm), _vp(self.rejected), self.tones, self.sparse)
        return pcm


def decode(frames, channels, tones=False, sparse=False):
    """from start-of-stream state: (pcm [N][2048][channels], rejected per reason [6] int64)"""
    d = Decoder(channels, tones, sparse)
    pcm = d.decode(frames)
    return pcm, d.rejected.astype(np.int64).copy()


def decode_streams(frames, channels, tones=False, sparse=False):
    """[S, F, frame_bytes] -> (pcm [S, F, 2048, C], rejected summed over the streams)"""
    out = [decode(f, channels, tones, sparse) for f in frames]
    return np.stack([p for p, _ in out]), sum(r for _, r in out)


def unpack(frames, channels, tones=False, sparse=False):
    """steps 1-2: (spectra [N][channels][2048] float32, window flags [N][channels] uint16, fields [N])"""
    lib = writer_lib()
    frames = np.ascontiguousarray(frames, np.uint8)
    n, fb = frames.shape
    specs, win, fl = np.zeros((n, channels, 2048), np.float32), np.zeros((n, channels), np.uint16), np.zeros(n, FIELDS_DTYPE)
    for f in range(n):
        lib.at3pw_unpack_frame(_vp(frames[f]), fb, channels, _vp(specs[f]), _vp(win[f]), int(tones), int(bool(sparse)), _vp(fl[f:f + 1]))
    return specs, win, fl


# ---- an independent parser of the head, from the header's text -----------------------------------------------------------------
def inc_tables():
    """the integer tables of at3p_vlc.inc by name, flat"""
    t = open(os.path.join(ROOT, "atracdenc_amd", "csrc", "at3p_vlc.inc")).read()
    out = {}
    for m in re.finditer(r"(AT3P_[A-Z0-9_]+)((?:\[[^\]]*\])+)\s*=\s*\{(.*?)\};", t, re.S):
        if "p+" not in m.group(3) and "p-" not in m.group(3):   # (the float tables are not needed)
            out[m.group(1)] = [int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", m.group(3))]
    return out


class _Bits:
    def __init__(self, frame):
        self.bits = np.unpackbits(np.asarray(frame, np.uint8))
        self.pos = 0

    def rd(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | int(self.bits[self.pos])
            self.pos += 1
        return v

    def vlc(self, table):
        """table: 8 entries code | length << 12, a complete prefix code"""
        for sym, e in enumerate(table):
            ln, code = e >> 12, e & 0xfff
            if ln and self.pos + ln <= len(self.bits) and int("".join(map(str, self.bits[self.pos:self.pos + ln])), 2) == code:
                self.pos += ln
                return sym
        raise AssertionError("no word-length code matches")


def parse_head(frame, nch):
    """Everything in front of the spectra of a frame of the adaptive writer, with or without AT3PHIP_ALLOC_SPARSE, read back without
    the writer's help: dict with N, wl [nch][N], sf, tab (None for a unit without an index), clone (channel-1 units that carry the
    flag, with its value; clone_pos: the flag's bit), wl_bits, the word-length section's length, and pos or data_pos, the first bit of
    channel 0's spectra."""
    tb = inc_tables()
    wlv = [tb["AT3P_WL_VLC"][8 * i:8 * i + 8] for i in range(4)]
    b = _Bits(frame)
    assert b.rd(1) == 0 and b.rd(2) == nch - 1
    N = b.rd(5) + 1
    assert b.rd(1) == 0   # mute
    start = b.pos
    assert (b.rd(2), b.rd(2), b.rd(2)) == (3, 0, 0)
    idx = b.rd(2)
    wl = [[b.rd(3)], []]
    for _ in range(1, N):
        wl[0].append((wl[0][-1] + b.vlc(wlv[idx])) & 7)
    if nch == 2:
        assert (b.rd(2), b.rd(2)) == (1, 0)
        idx = b.rd(2)
        for q in range(N):
            wl[1].append((wl[0][q] + b.vlc(wlv[idx])) & 7)
    wl_bits = b.pos - start
    sf = []
    for ch in range(nch):
        assert b.rd(2) == 0
        sf.append([b.rd(6) for _ in range(N)])
    assert b.rd(1) == 1   # the full-table flag
    tab, clone, clone_pos = [], {}, {}
    for ch in range(nch):
        assert (b.rd(1), b.rd(2), b.rd(1)) == (0, 0, 0)
        row = []
        for q in range(N):
            if wl[ch][q]:
                row.append(b.rd(3))
            else:
                row.append(None)
                if ch and wl[0][q]:
                    clone_pos[q] = b.pos
                    clone[q] = b.rd(1)
        tab.append(row)
    return {"N": N, "wl": wl[:nch], "sf": sf, "tab": tab, "clone": clone, "clone_pos": clone_pos, "wl_bits": wl_bits, "pos": b.pos, "data_pos": b.pos}


def terminator_pos(frame):
    """the bit position of the last set bit: the terminator's second bit"""
    b = np.unpackbits(np.asarray(frame, np.uint8))
    return int(np.nonzero(b)[0][-1])


def recount_bits(parsed, nch, bits, tail_bits):
    """Bits(A) of A4 from a parsed head (no word length 0 below N), the cost table `bits` [nch][32][8] of its spectra and its tail:
    the word-length section by the oracle's at3po_wordlen_bits"""
    oracle()
    lib = ctypes.CDLL(ORACLE_SO)
    N = parsed["N"]
    wl0 = np.array(parsed["wl"][0] + [0] * (32 - N), np.uint8)
    wl1 = np.array((parsed["wl"][1] if nch == 2 else parsed["wl"][0]) + [0] * (32 - N), np.uint8)
    sec = lib.at3po_wordlen_bits(_vp(wl0), _vp(wl1), N, nch, None)
    total = 5 + 1 + sec + nch * (2 + 6 * N) + 1 + nch * (4 + 3 * N) + nch * 4 * SB_POWGRPS[QU_TO_SB[N - 1]] + tail_bits
    for ch in range(nch):
        for qu in range(N):
            total += int(bits[ch][qu][parsed["wl"][ch][qu]])
    return total, sec


def count_bits(head, nch, unit_bits, tail_bits):
    """Bits(A) of A4s from a parsed head, in Python from the header's text: unit_bits[ch][qu][w] the cost table, everything but the
    three leading bits"""
    tb = inc_tables()
    wlv = [tb["AT3P_WL_VLC"][8 * i:8 * i + 8] for i in range(4)]
    N, wl = head["N"], head["wl"]
    total = 5 + 1

    def section(deltas, first_counts):
        m = 0
        for d in deltas:
            m |= abs(d)
        cand = (2, 3) if m >= 3 else (1,) if m == 2 else (0,)
        best = None
        for i in cand:
            n = sum(wlv[i][d & 7] >> 12 for d in deltas[1:])
            if best is None or n < best[0]:
                best = (n, i)
        return best[0] + (wlv[best[1]][deltas[0] & 7] >> 12 if first_counts and deltas else 0)

    total += 11 + section([0] + [wl[0][q] - wl[0][q - 1] for q in range(1, N)], False)
    if nch == 2:
        total += 6 + section([wl[1][q] - wl[0][q] for q in range(N)], True)
    total += nch * (2 + 6 * N) + 1
    for ch in range(nch):
        total += 4 + sum(3 for q in range(N) if wl[ch][q]) + (sum(1 for q in range(N) if not wl[1][q] and wl[0][q]) if ch else 0)
        total += sum(int(unit_bits[ch][q][wl[ch][q]]) for q in range(N) if wl[ch][q])
        total += 4 * tb["AT3P_SB_POWGRPS"][QU_TO_SB[N - 1]]
    return total + tail_bits


# ---- signals and cases -----------------------------------------------------------------------------------------------------------
def specs_of(name, nch, n=SNR_FRAMES):
    """[n, C, 2048]: the spectra at3phip_encode_frames forms for a test signal (oracle PQF and MDCT)"""
    if name == "silence":
        return np.zeros((n, nch, 2048), np.float32)
    if name == "fullscale":
        return full_scale_noise(n, nch)
    return at3p_specs(name, n, nch)


def specs_of_pcm(pcm):
    """pcm [n, 2048, C] of one stream from its start -> [n, C, 2048]: the spectra at3phip_encode_frames hands its writer"""
    from at3_testlib import at3p_mdct, at3p_pqf
    from at3p_gha_lib import SCALE
    out = np.zeros((pcm.shape[0], pcm.shape[2], 2048), np.float32)
    for c in range(pcm.shape[2]):
        bands = at3p_pqf(np.ascontiguousarray(pcm[:, :, c]))
        out[:, c] = at3p_mdct((bands.astype(np.float64) / SCALE).astype(np.float32))
    return out


def full_scale_noise(n, nch, seed=5):
    """white spectra at full scale: every unit's scale factor index is at the table's top"""
    return np.clip(np.random.RandomState(seed).standard_normal((n, nch, 2048)) * 0.5, -1.0, 1.0).astype(np.float32)


def quiet_mono(n=1, seed=6):
    """white spectra at 2^-12: a frame that fits at t = -21"""
    return (np.random.RandomState(seed).standard_normal((n, 1, 2048)) * 2.0 ** -12).astype(np.float32)


def odd_specs(nch, n=3, seed=9):
    """spectra holding NaN, +-inf and +-FLT_MAX among ordinary values"""
    x = (0.1 * np.random.RandomState(seed).standard_normal((n, nch, 2048))).astype(np.float32)
    fmax = np.finfo(np.float32).max
    flat = x.reshape(-1)
    for i, v in enumerate((np.nan, np.inf, -np.inf, fmax, -fmax)):
        flat[7 + 131 * i::977] = v
    x[n // 2, 0, 384:448] = np.nan     # a unit of nothing but NaN
    x[n - 1, -1, 768:896] = np.inf
    return x


def random_cost_tables(n=1000, seed=2026):
    """[(sfi [C, 32], bits [C, 32, 8], tail_bits)]: plausible tables (bits growing with w and with the unit's size), tables made
    non-monotone in w on purpose (B at w + 1 below B at w), and tables whose totals fit, fail to fit and fit again as t rises (a
    cheap word length between dear ones at units whose sfi share a residue class): where a full scan and a bisection differ"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        nch = 1 + int(rng.integers(0, 2))
        kind = i % 4
        size = np.diff(QU_START)
        base = rng.integers(0, 64)
        sfi = np.clip(base - np.arange(32) * rng.integers(0, 3) + rng.integers(-6, 7, (nch, 32)), 0, 63).astype(np.uint8)
        if kind == 3:
            sfi = np.clip((rng.integers(0, 21, (nch, 1)) * 3 + rng.integers(0, 2, (nch, 32))), 0, 63).astype(np.uint8)
        per = rng.uniform(0.3, 1.6, (nch, 32, 1)) * np.arange(8)[None, None, :] * size[None, :, None]
        bits = per + rng.integers(0, 12, (nch, 32, 8))
        if kind >= 1:     # non-monotone: some word lengths cheaper than the one below
            drop = rng.random((nch, 32, 8)) < 0.3
            bits = np.where(drop, bits * rng.uniform(0.1, 0.9, bits.shape), bits)
        if kind >= 2:     # one word length very dear, the next very cheap: totals that fit, fail and fit again
            w = int(rng.integers(2, 7))
            bits[:, :, w] = bits[:, :, w] * 6 + 900
            bits[:, :, w + 1] = bits[:, :, w + 1] * 0.2
        scale = rng.choice([0.2, 1.0, 2.5])
        bits = np.clip(bits * scale, 0, 65535).astype(np.uint16)
        out.append((sfi, bits, int(rng.integers(8, 1700))))
    return out


def random_dist_tables(tables_in, seed=77):
    """[(sfi, bits, dist, tail_bits)] from random_cost_tables' cases: S falling with w by a random factor per step, with steps that do
    not fall and units of all-zero distortion among them"""
    rng = np.random.default_rng(seed)
    out = []
    for i, (sfi, bits, tail) in enumerate(tables_in):
        nch = sfi.shape[0]
        s0 = (rng.uniform(0.0, 1.0, (nch, 32)) ** 2 * LINES[None, :] * 2.0 ** 40).astype(np.float64)
        fall = rng.uniform(0.1, 0.6, (nch, 32, 8))
        if i % 3 == 0:
            fall = np.where(rng.random((nch, 32, 8)) < 0.2, rng.uniform(0.9, 1.3, (nch, 32, 8)), fall)
        fall[:, :, 0] = 1.0
        dist = (s0[:, :, None] * np.cumprod(fall, axis=2)).astype(np.uint64)
        if i % 5 == 0:
            dist[rng.random((nch, 32)) < 0.2] = 0
        out.append((sfi, bits, np.minimum(dist, np.uint64(1) << np.uint64(47)), tail))
    return out


# ---- the smallest admissible sizes, from the tables ------------------------------------------------------------------------------
def worst_front_one_unit(nch, tb=None):
    """upper bound of everything in front of the tail in A(63, 0), without the three leading bits: N = 1, every word-length code at
    its longest, unit 0 (16 lines) at word length 1 under the cheapest-in-the-worst-case of its eight tables"""
    tb = tb or inc_tables()
    best = None
    for i in range(8):
        t = 1 - 1 + 7 * i
        gs, nc = tb["AT3P_SPEC_TAB"][2 * t] & 15, tb["AT3P_SPEC_TAB"][2 * t] >> 4
        signed = tb["AT3P_SPEC_TAB"][2 * t + 1] >> 4
        longest = max(e >> 12 for e in tb["AT3P_VLC"][tb["AT3P_VLC_OFF"][t]:tb["AT3P_VLC_OFF"][t + 1]])
        nsym = 16 // nc
        bits = nsym * (longest + (0 if signed else nc)) + (nsym // gs if gs != 1 else 0)
        best = bits if best is None else min(best, bits)
    wl = max(e >> 12 for e in tb["AT3P_WL_VLC"])
    bits = 5 + 1 + (2 + 2 + 2 + 2 + 3) + (nch == 2) * (2 + 2 + 2 + wl)
    bits += nch * (2 + 6) + 1 + nch * (4 + 3) + nch * 4 * tb["AT3P_SB_POWGRPS"][tb["AT3P_QU_TO_SB"][0]]
    return bits + nch * best


def worst_tail(nch):
    """upper bound of the tail, formed as tests/test_at3p_tonal_write_cpu.py forms it for stereo"""
    from at3p_tonal_lib import tone_vlc
    blk = 1 + max(n for _, n in tone_vlc()) + (nch == 2) * (2 + 16 + 2 + 1)
    for ch in range(nch):
        blk += ch + 16 * 12 + (ch + 1) + 16 * 4 + ch + (ch + 1)
    blk += 48 * 10 + 24 + 48 * (6 + 5)
    return (nch == 2) * 2 + nch * 18 + nch + 1 + blk + 1 + 2


def min_frame_bytes(nch):
    """the smallest multiple of 8 with worst front + worst tail <= 8 * bytes - 3"""
    need = worst_front_one_unit(nch) + worst_tail(nch) + 3
    return -(-need // 64) * 8


def snr_db(ref, got):
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    err = float(np.sum((ref - got) ** 2))
    return float("inf") if err == 0 else 10.0 * np.log10(float(np.sum(ref ** 2)) / err)


# ---- the sparse definition's special cases as cost tables --------------------------------------------------------------------------
def edge_tables():
    """{name: (sfi uint8 [C, 32], bits uint16 [C, 32, 8], tail_bits, frame_bytes)}; bits are 16 x lines x w / 16-ish figures
    that make the budget bind where the case needs it"""
    def bits_of(nch, per_line=1.0):
        b = np.zeros((nch, 32, 8), np.uint16)
        for w in range(1, 8):
            b[:, :, w] = np.minimum(65535, (LINES * w * per_line).astype(np.int64) + 2)
        return b

    out = {}
    # no unit wanted: every unit but (0, 0) steps from 0 to 1 between t = 3 and t = 2 and one bit for any of them is beyond the budget,
    # unit (0, 0) wants nothing at either; so t* = 3, k* = 0, N = 1 and unit 0 of channel 0 takes 1
    sfi, b = np.full((2, 32), 5, np.uint8), np.full((2, 32, 8), 60000, np.uint16)
    sfi[0, 0], b[0, 0, :] = 0, 40
    out["nothing_wanted"] = (sfi, b, 40, 224)
    for top in (28, 29, 30):   # the highest wanted unit: N becomes 32 and unit 31 of channel 0 takes 1
        sfi = np.zeros((2, 32), np.uint8)
        sfi[:, :4] = 30
        sfi[1, top] = 30
        out[f"top_{top}"] = (sfi, bits_of(2, 1.5), 12, 376)
    sfi = np.zeros((2, 32), np.uint8)   # channel 1 silent under a loud channel 0: clone bits
    sfi[0, :20] = 40
    sfi[1, 3] = 40
    out["clone_bits"] = (sfi, bits_of(2, 1.2), 12, 376)
    out["flat"] = (np.full((2, 32), 33, np.uint8), bits_of(2, 1.0), 12, 376)   # every want steps at the same t: k alone extends N
    out["flat_mono"] = (np.full((1, 32), 33, np.uint8), bits_of(1, 1.0), 10, 192)
    return out


# ---- crafted frames for the sparse decoder ---------------------------------------------------------------------------------------
def _put(bits, val, n):
    bits.extend((val >> k) & 1 for k in range(n - 1, -1, -1))


def crafted_frames(nch, frame_bytes):
    """uint8 [1 or 2, frame_bytes]: a frame whose highest unit has word length 0 in every channel (N = 2, word lengths 1, 0), and in
    stereo a good sparse frame with one clone flag cleared; both are unsupported_syntax with AT3PHIP_DECODE_SPARSE"""
    wlv = inc_tables()["AT3P_WL_VLC"][:8]
    bits = []
    _put(bits, 0, 1), _put(bits, nch - 1, 2), _put(bits, 1, 5), _put(bits, 0, 1)
    _put(bits, 3, 2), _put(bits, 0, 2), _put(bits, 0, 2), _put(bits, 0, 2), _put(bits, 1, 3)
    _put(bits, wlv[7] & 0xfff, wlv[7] >> 12)            # delta -1: unit 1 of channel 0 at 0
    if nch == 2:
        _put(bits, 1, 2), _put(bits, 0, 2), _put(bits, 0, 2)
        _put(bits, wlv[0] & 0xfff, wlv[0] >> 12), _put(bits, wlv[0] & 0xfff, wlv[0] >> 12)   # channel 1 as channel 0
    out = [np.packbits(np.array(bits + [0] * (8 * frame_bytes - len(bits)), np.uint8))]
    if nch == 2:
        sp = specs_of("mix", 2, 1)
        sp[:, 1] = sp[:, 0] * np.float32(2.0 ** -6)     # channel 1 six bits under channel 0: zeros under coded units
        fr = write_adaptive(sp, frame_bytes, True)[0].copy()
        head = parse_head(fr, 2)
        assert head["clone_pos"] and all(v == 1 for v in head["clone"].values())
        pos = sorted(head["clone_pos"].values())[len(head["clone_pos"]) // 2]
        fr[pos >> 3] &= 0xff ^ (0x80 >> (pos & 7))
        out.append(fr)
    return np.stack(out)


# ---- the sparse special cases through real spectra -----------------------------------------------------------------------------------
def edge_specs(nch):
    """(spectra [4][C][2048], blocks [4]) for the smallest frame size of the channel count, where the budget binds:
      0  silence but for unit 31 of the last channel at full scale, beside the largest tonal record: the tail leaves room for one
         unit, unit (0, 0) wants nothing at t* or t* - 1 and unit 31's first bit does not fit: k* = 0, the empty frame, unit 0 of
         channel 0 takes 1 (A3s' first fix-up decides the frame);
      1  units 0-3 and unit 29 of the last channel alone: N becomes 32 and unit 31 of channel 0 takes 1 above zeros;
      2  `mix` with channel 1 six bits under channel 0: zeros under coded units, clone flags (stereo);
      3  one level everywhere: a flat sfi, A(t*, 0) is empty and k alone extends N."""
    from at3p_tonal_write_lib import largest_block
    sp = np.zeros((4, nch, 2048), np.float32)
    rng = np.random.default_rng(5)
    sp[0, nch - 1, QU_START[31]:] = rng.uniform(-0.9, 0.9, 128)
    sp[1, :, :64] = rng.uniform(-0.5, 0.5, (nch, 64))
    sp[1, nch - 1, QU_START[29]:QU_START[30]] = rng.uniform(-0.5, 0.5, 128)
    sp[2] = specs_of("mix", nch, 1)[0]
    if nch == 2:
        sp[2, 1] = sp[2, 0] * np.float32(2.0 ** -6)
    sp[3] = np.where(rng.integers(0, 2, (nch, 2048)) > 0, 0.3, -0.3).astype(np.float32)
    return sp, [largest_block(nch), None, None, None]


def edge_cases_reached(rec, nch):
    """the names of edge_specs' cases that the restatement's info records `rec` [4] do NOT show (empty: all reached)"""
    wl, N, k = rec["wl"].astype(int), rec["num_quant_units"], rec["k"]
    missed = []
    if not (N[0] == 1 and k[0] == 0 and wl[0, 0, 0] == 1 and wl[0].sum() == 1):
        missed.append("empty frame")
    if not (N[1] == 32 and wl[1, 0, 31] == 1 and wl[1, 1, 31] == 0 and not wl[1, :, 30].any() and not wl[1, :, 4:29].any() and wl[1, nch - 1, 29] > 0):
        missed.append("29..31")
    if nch == 2 and not ((wl[2, 1, :N[2]] == 0) & (wl[2, 0, :N[2]] > 0)).sum() >= 5:
        missed.append("clone flags")
    if not (k[3] > 1 and (wl[3] > 0).sum() == k[3] and wl[3].max() == 1 and N[3] == (k[3] + nch - 1) // nch):
        missed.append("flat")
    return missed


# ---- rate-distortion: T recomputed, the guard, the J_MAX bound -------------------------------------------------------------------------
def scale_table():
    """ScaleTable as float32 [64]: 2^(i / 3 - 21) rounded to float; entry i + 3 is exactly twice entry i"""
    t = open(os.path.join(ROOT, "atracdenc_amd", "csrc", "at3p_vlc.inc")).read()
    t = t[t.index("AT3P_SCALE[64]"):]
    return np.array([float.fromhex(x.rstrip("f")) for x in re.findall(r"0x[0-9a-f.]+p[+-]\d+f", t[:t.index("};")])], np.float32)


def total_distortion(sfi, dist, wl):
    """T of R4: the serial double sum of D[ch][qu][wl] in the order of the walk, from +0.0"""
    sc = scale_table().astype(np.float64)
    T = np.float64(0.0)
    for qu in range(32):
        for ch in range(sfi.shape[0]):
            T = T + np.float64(int(dist[ch, qu, int(wl[ch, qu])])) * (sc[sfi[ch, qu]] * sc[sfi[ch, qu]])
    return float(T)


def guard_table():
    """(sfi [1, 32], bits [1, 32, 8], dist [1, 32, 8], tail_bits, frame_bytes) on which R(j*, k*) has more distortion than A(t*, k*), a
    mono frame at 176 bytes (1405 bits) in which unit 0 alone has any distortion. Its S barely falls from w = 0 to 6 and drops to 0 at
    w = 7, which costs 5000 bits: per bit nothing gains as much as w = 7, so unit 0's pick is 0 or 7 at every j, 7 never fits, and
    R(j*, k*) is the empty frame, whose closing rule gives unit 0 word length 1: T(R) = D[1]. Word lengths 1..3 cost 100 bits each and
    fit, 4..6 cost 2000 and more: A3s walks unit 0's want down with t to 3, T(A) = D[3] < D[1], and the guard writes A(t*, k*)."""
    sfi = np.zeros((1, 32), np.uint8)
    bits = np.full((1, 32, 8), 60000, np.uint16)
    dist = np.zeros((1, 32, 8), np.uint64)
    sfi[0, 0] = 30
    bits[0, 0] = [0, 100, 200, 300, 2000, 2100, 2200, 5000]
    dist[0, 0] = [(1 << 40) - 1000 * w for w in range(7)] + [0]
    return sfi, bits, dist, 10, 176


def min_chunk_bits():
    """the fewest bits any of the 56 code tables spends on a 16-line chunk, over all mantissas: per table the cheapest way to code 16
    lines (every group's flag bit, and where a group is not skipped its cheapest codes), from at3p_vlc.inc"""
    tb = inc_tables()
    best = None
    for t in range(56):
        group_size, num_coeffs = tb["AT3P_SPEC_TAB"][2 * t] & 15, tb["AT3P_SPEC_TAB"][2 * t] >> 4
        lens = [e >> 12 for e in tb["AT3P_VLC"][tb["AT3P_VLC_OFF"][t]:tb["AT3P_VLC_OFF"][t + 1]] if e >> 12]
        n_groups = 16 // (group_size * num_coeffs) if group_size * num_coeffs <= 16 else 1
        per_group = (1 if group_size != 1 else 0) + group_size * min(lens)   # (the writer never skips a group: its flag is always 1)
        bits = n_groups * per_group
        best = bits if best is None else min(best, bits)
    return best


def j_max_bound():
    """the smallest j at which lambda_j / 2^40 >= lines / (lines / 16 * min_chunk_bits + 3) for every unit size: every unit picks 0"""
    sc = scale_table().astype(np.float64)
    cmin = min_chunk_bits()
    need = max(float(n) / (n // 16 * cmin + 3) for n in (16, 32, 64, 128))
    for j in range(0, 200):
        q, r = divmod(j, 3)
        lam = sc[r] * sc[r] * 4.0 ** q          # lambda_j / 2^40; G[63] = 1 bounds every G
        if lam >= need:
            return j
    raise AssertionError


# ---- golden files ------------------------------------------------------------------------------------------------------------------
ALLOC_GOLDEN = os.path.join(HERE, "golden", "at3p_alloc.npz")
ALLOC_GOLDEN_CASES = [(name, nch) for name in SIGNALS + ("silence", "fullscale") for nch in (1, 2)]
ALLOC_GOLDEN_FRAMES = 4
SPARSE_GOLDEN = os.path.join(HERE, "golden", "at3p_sparse.npz")
SPARSE_GOLDEN_CASES = [(name, nch, fb) for name in ("noise", "tones") for nch in (1, 2) for fb in (376, 2048)]
SPARSE_GOLDEN_FRAMES = 3
RD_GOLDEN = os.path.join(HERE, "golden", "at3p_rd.npz")
RD_GOLDEN_CASES = [(name, nch, fb) for name in ("noise", "tones", "mix") for nch in (1, 2) for fb in (376, 2048)]
RD_GOLDEN_FRAMES = 3
FOLD_GOLDEN = os.path.join(HERE, "golden", "at3p_writer_fold.npz")


def alloc_golden_entry(name, nch):
    """(t*, k*, N per frame as int32 [F, 3], SHA-256 of the frames) of the restatement at 2048 bytes for a golden case"""
    frames, rec, _ = write_adaptive(specs_of(name, nch, ALLOC_GOLDEN_FRAMES), info=True)
    return np.stack([rec["t"], rec["k"], rec["num_quant_units"]], axis=1).astype(np.int32), hashlib.sha256(frames.tobytes()).hexdigest()


def sparse_golden_entry(name, nch, fb):
    """the sparse restatement on 3 frames of a signal: {frames uint8 [3, fb], choice int32 [3, 3] (t*, k*, N), wl uint8 [3, 2, 32],
    pcm_sha256: the SHA-256 of the sparse decoder's PCM [3, 2048, C] float32 as bytes}"""
    frames, rec, _ = write_adaptive(specs_of(name, nch, SPARSE_GOLDEN_FRAMES), fb, True, info=True)
    pcm, rej = decode(frames, nch, False, True)
    assert rej.sum() == 0
    return {"frames": frames, "choice": np.stack([rec["t"], rec["k"], rec["num_quant_units"]], axis=1).astype(np.int32), "wl": rec["wl"],
            "pcm_sha256": np.array(hashlib.sha256(np.ascontiguousarray(pcm).tobytes()).hexdigest())}


def rd_golden_entry(name, nch, fb):
    """the rate-distortion restatement on 3 frames of a signal: {frames uint8 [3, fb], choice int32 [3, 4] (j*, k*, N, chose_rd),
    wl uint8 [3, 2, 32], T float64 [3, 2] (T(R), T(A))}"""
    frames, rec, _ = write_rd(specs_of(name, nch, RD_GOLDEN_FRAMES), fb, info=True)
    return {"frames": frames, "choice": np.stack([rec["j"], rec["k"], rec["num_quant_units"], rec["chose"]], axis=1).astype(np.int32),
            "wl": rec["wl"], "T": np.stack([rec["T"], rec["T_sparse"]], axis=1)}


# ---- at3p_writer_fold.npz: what the six restatements gave before they were folded into one ----------------
def sha(*parts):
    """SHA-256 (32 bytes as uint8) of arrays and plain values: dtype, shape and bytes of each"""
    h = hashlib.sha256()
    for p in parts:
        a = np.ascontiguousarray(p)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8)


_RD_INFO_22 = np.dtype([("j", "<i4"), ("k", "<i4"), ("num_quant_units", "<i4"), ("bits", "<i4"), ("chose_rd", "<i4"), ("t", "<i4"),
                        ("k_sparse", "<i4"), ("pad", "<i4"), ("T_rd", "<f8"), ("T_sparse", "<f8"), ("wl", "u1", (2, 32)), ("sfi", "u1", (2, 32)),
                        ("tab", "u1", (2, 32))])


def _rd_info_bytes_22(rec):
    """the bytes of rate-distortion records in the layout they had when at3p_writer_fold.npz was written, whose digests are of those bytes"""
    rec = np.asarray(rec)
    old = np.zeros(rec.shape, _RD_INFO_22)
    for name in _RD_INFO_22.names:
        if name != "pad":
            old[name] = rec[{"chose_rd": "chose", "T_rd": "T"}.get(name, name)]
    return old.reshape(-1).view(np.uint8)


def fold_inputs(nch):
    """[(spectra, window flags or None, tonal blocks or None)]: the inputs of the two cross-pin tests"""
    import at3p_tonal_write_lib as TW
    cases = [(specs_of(n, nch, 4), None, None) for n in SIGNALS + ("silence", "fullscale")]
    cases.append((odd_specs(nch, 3), None, None))
    cases.append((specs_of("noise", nch, 2), np.array([[0x01ef] * nch, [0xffff] * nch], np.uint16), None))
    cases.append((np.concatenate([full_scale_noise(2, nch), specs_of("mix", nch, 14)[:1]]), None,
                  [TW.largest_block(nch), None, TW.case_blocks(f"small_{nch}")[0][0]]))
    return cases


@functools.lru_cache(maxsize=None)
def fold_entries(nch, part="abcd"):
    """{label: SHA-256}: what tests/golden/at3p_writer_fold.npz holds for a channel count, or the parts of it named. Labels ending in
    `_in` are digests of inputs, the others of what the restatement makes of them."""
    import at3p_decode_lib as D
    out = {}
    if "a" in part:   # the cross-pin inputs at 2048 bytes, 376 and the smallest size: frames, records, PCM and counters
        rng = np.random.default_rng(11)
        cases = fold_inputs(nch)
        for i, (sp, win, blocks) in enumerate(cases):
            tails = [pack_tail(tail_bits_list(nch, None if win is None else win[f], None if blocks is None else blocks[f]), 256)
                     for f in range(len(sp))]
            out[f"a{i}_in"] = sha(sp.view(np.uint32), *[t for t, _ in tails], [n for _, n in tails])
        for fb in (2048, 376, MIN_BYTES[nch]):
            for i, (sp, win, blocks) in enumerate(cases):
                frames, rec, _ = write_adaptive(sp, fb, False, win, blocks, info=True)
                out[f"a{i}_{fb}_frames"], out[f"a{i}_{fb}_info"] = sha(frames), sha(rec.view(np.uint8))
                flipped = D.mutate_frames(frames, rng, n_flips=2)
                out[f"a{i}_{fb}_flipped_in"] = sha(flipped)
                for kind, fr in (("plain", frames), ("flipped", flipped)):
                    for tones in (False, True):
                        pcm, rej = decode(fr, nch, tones, False)
                        out[f"a{i}_{fb}_{kind}_tones{int(tones)}"] = sha(pcm.view(np.uint32), rej)
    if "b" in part:   # the crafted malformed frames of at3p_decode_lib
        crafted, _ = D.crafted_frames(nch, 3)
        out["b_in"] = sha(crafted)
        for tones in (False, True):
            pcm, rej = decode(crafted, nch, tones, False)
            out[f"b_tones{int(tones)}"] = sha(pcm.view(np.uint32), rej)
            out[f"b_fields{int(tones)}"] = sha(unpack(crafted, nch, tones, False)[2].view(np.uint8))
    if "c" in part:   # the first 100 random cost tables
        for i, (sfi, bits, tail) in enumerate(random_cost_tables()[:100]):
            if sfi.shape[0] == nch:
                out[f"c{i}_in"] = sha(sfi, bits, tail)
                for fb in (MIN_BYTES[nch], 2048):
                    wl, *rest = allocate(sfi, bits, min(tail, 8 * fb - 3), fb, False)
                    out[f"c{i}_{fb}"] = sha(wl, rest)
    if "d" in part:   # sparse and rate-distortion, where the definition has special cases
        sp, blocks = edge_specs(nch)
        tails = [pack_tail(tail_bits_list(nch, None, b), 256) for b in blocks]
        out["d_specs_in"] = sha(sp.view(np.uint32), *[t for t, _ in tails], [n for _, n in tails])
        for fb in (MIN_BYTES[nch], 2048):
            for name, (frames, rec, _) in (("sparse", write_adaptive(sp, fb, True, None, blocks, info=True)),
                                           ("rd", write_rd(sp, fb, None, blocks, info=True))):
                out[f"d_specs_{name}_{fb}_frames"] = sha(frames)
                out[f"d_specs_{name}_{fb}_info"] = sha(rec.view(np.uint8) if name == "sparse" else _rd_info_bytes_22(rec))
        for fb in (MIN_BYTES[nch], 376):                # (at 2048 bytes a stereo frame of `mix` has no clone flag to clear)
            bad = crafted_frames(nch, fb)
            out[f"d_crafted_{fb}_in"] = sha(bad)
            pcm, rej = decode(bad, nch, True, True)
            out[f"d_crafted_{fb}"] = sha(pcm.view(np.uint32), rej, unpack(bad, nch, True, True)[2].view(np.uint8))
        for name, (sfi, bits, tail, fb) in edge_tables().items():
            if sfi.shape[0] == nch:
                wl, *rest = allocate(sfi, bits, tail, fb, True)
                out[f"d_table_{name}_in"], out[f"d_table_{name}"] = sha(sfi, bits, tail, fb), sha(wl, rest)
        sfi, bits, dist, tail, fb = guard_table()
        if nch == 1:
            wl, N, rec = allocate_rd(sfi, bits, dist, tail, fb)
            out["d_guard_in"], out["d_guard"] = sha(sfi, bits, dist, tail, fb), sha(wl, N, _rd_info_bytes_22(rec))
    return out


def fold_file_arrays():
    """the arrays of the file: per channel count the labels and the digests [n, 32] in the labels' order"""
    arrays = {}
    for nch in (1, 2):
        e = fold_entries(nch)
        arrays[f"labels_{nch}"], arrays[f"sha256_{nch}"] = np.array(list(e)), np.stack(list(e.values()))
    return arrays


def fold_golden(nch):
    """{label: SHA-256} of the committed file for a channel count"""
    gold = np.load(FOLD_GOLDEN)
    return dict(zip(gold[f"labels_{nch}"].tolist(), gold[f"sha256_{nch}"]))
