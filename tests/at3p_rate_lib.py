"""Helpers of the ATRAC3plus frame-size tests, their SIMT-harness driver and tools/at3p_rate_bench.py (TEST INFRASTRUCTURE: nothing
under atracdenc_amd/ imports this module).

  * rate_lib: the C restatement tests/host/at3p_rate_cpu.c - the adaptive writer (include/at3phip.h, ADAPTIVE WORD LENGTHS with
    FRAME SIZE) and the decoder with the frame size as an argument -, compiled on first use with the reference's arithmetic flags.
  * write_adaptive / allocate / RateDecoder / decode / unpack: its entry points.
  * min_frame_bytes: the smallest admissible frame size of a channel count, derived from the code tables.
  * the frame sizes the tests use, the command line's bitrate table, the signals of the round-trip table and its SNR.
"""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

from at3_testlib import _vp
from at3p_alloc_lib import INFO_DTYPE, _blocks_as_dicts, pack_tail, tail_bits_list
from at3p_decode_lib import CFLAGS, FIELDS_DTYPE, REASONS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RATE_SRC = os.path.join(HERE, "host", "at3p_rate_cpu.c")
MIN_BYTES = {1: 176, 2: 224}                       # AT3PHIP_MIN_FRAME_BYTES_MONO / _STEREO (test_min_frame_bytes derives them)
# kbit/s -> frame bytes, the command line's table (atracdenc_amd/host/at3hipenc.cpp, kAt3pRates)
BITRATES = {32: 192, 48: 280, 64: 376, 96: 560, 128: 744, 160: 936, 192: 1120, 256: 1488, 320: 1864, 352: 2048}
# where a guard or a stride can go wrong: the minimum, table sizes, 2040 (admissible, not in the table) and 2048
SIZES = {1: (192, 376, 2040, 2048), 2: (MIN_BYTES[2], 280, 376, 1120, 1864, 2040, 2048)}

_so = None


def rate_lib():
    global _so
    if _so is None:
        d = tempfile.mkdtemp(prefix="at3prate_")
        so = os.path.join(d, "libat3prate_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, RATE_SRC, "-lm"])
        _so = so
    lib = ctypes.CDLL(_so)
    lib.at3pr_state_bytes.restype = ctypes.c_size_t
    lib.at3pr_reset.argtypes = [ctypes.c_void_p]
    lib.at3pr_decode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_int]
    lib.at3pr_unpack_frame.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.at3pr_write_frames.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p]
    lib.at3pr_allocate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
    assert lib.at3pr_frame_info_size() == INFO_DTYPE.itemsize
    return lib


# ---- the encoder ---------------------------------------------------------------------------------------------------------------
def write_adaptive(specs, frame_bytes, win=None, blocks=None, info=False):
    """specs float32 [n, C, 2048], win uint16 [n, C] or None, blocks [n] (dicts, records or None) -> frames uint8 [n, frame_bytes]
    (and the per-frame record of at3p_alloc_lib.INFO_DTYPE with info=True)"""
    lib = rate_lib()
    specs = np.ascontiguousarray(specs, np.float32)
    n, nch = specs.shape[0], specs.shape[1]
    tb = lib.at3pr_tail_bytes()
    tails, nbits = np.zeros((n, tb), np.uint8), np.zeros(n, np.int32)
    for f, b in enumerate(_blocks_as_dicts(nch, blocks, n)):
        tails[f], nbits[f] = pack_tail(tail_bits_list(nch, None if win is None else win[f], b), tb)
    out, rec = np.zeros((n, frame_bytes), np.uint8), np.zeros(n, INFO_DTYPE)
    assert lib.at3pr_write_frames(_vp(specs), nch, n, int(frame_bytes), _vp(tails), _vp(nbits), _vp(out), _vp(rec)) == n
    return (out, rec) if info else out


def write_streams(specs, frame_bytes, win=None, blocks=None):
    """the same for [S, F, C, 2048] -> [S, F, frame_bytes]"""
    S, F = specs.shape[:2]
    flat = write_adaptive(specs.reshape((S * F,) + specs.shape[2:]), frame_bytes, None if win is None else win.reshape(S * F, -1),
                          None if blocks is None else (blocks.reshape(-1) if isinstance(blocks, np.ndarray) else blocks))
    return flat.reshape(S, F, frame_bytes)


def allocate(sfi, bits, tail_bits, frame_bytes):
    """A3-A5 of the restatement against 8 * frame_bytes - 3: (wl uint8 [C, 32], N, t*, k*, Bits)"""
    sfi, bits = np.ascontiguousarray(sfi, np.uint8), np.ascontiguousarray(bits, np.uint16)
    nch = sfi.shape[0]
    wl, out = np.zeros((nch, 32), np.uint8), np.zeros(3, np.int32)
    total = rate_lib().at3pr_allocate(_vp(sfi), _vp(bits), nch, int(tail_bits), int(frame_bytes), _vp(wl), _vp(out[0:1]), _vp(out[1:2]),
                                      _vp(out[2:3]))
    return wl, int(out[0]), int(out[1]), int(out[2]), int(total)


# ---- the decoder ---------------------------------------------------------------------------------------------------------------
class RateDecoder:
    """One stream of the restatement; state carries across decode() calls, the frame size may change between them."""

    def __init__(self, channels, tones=False):
        self.lib = rate_lib()
        self.channels, self.tones = int(channels), int(bool(tones))
        self.state = np.zeros(self.lib.at3pr_state_bytes(), np.uint8)
        self.rejected = np.zeros(len(REASONS), np.uint64)
        self.lib.at3pr_reset(_vp(self.state))

    def decode(self, frames):
        """frames [N][frame_bytes] uint8 -> pcm [N][2048][channels] float32"""
        frames = np.ascontiguousarray(frames, np.uint8)
        n, fb = frames.shape
        pcm = np.zeros((n, 2048, self.channels), np.float32)
        self.lib.at3pr_decode(_vp(self.state), self.channels, _vp(frames), fb, n, _vp(pcm), _vp(self.rejected), self.tones)
        return pcm


def decode(frames, channels, tones=False):
    """from start-of-stream state: (pcm [N][2048][channels], rejected per reason [6] int64)"""
    d = RateDecoder(channels, tones)
    pcm = d.decode(frames)
    return pcm, d.rejected.astype(np.int64).copy()


def decode_streams(frames, channels, tones=False):
    """[S, F, frame_bytes] -> (pcm [S, F, 2048, C], rejected summed over the streams)"""
    out = [decode(f, channels, tones) for f in frames]
    return np.stack([p for p, _ in out]), sum(r for _, r in out)


def unpack(frames, channels, tones=False):
    """steps 1-2: (spectra [N][channels][2048] float32, window flags [N][channels] uint16, fields [N])"""
    lib = rate_lib()
    frames = np.ascontiguousarray(frames, np.uint8)
    n, fb = frames.shape
    specs, win, fl = np.zeros((n, channels, 2048), np.float32), np.zeros((n, channels), np.uint16), np.zeros(n, FIELDS_DTYPE)
    for f in range(n):
        lib.at3pr_unpack_frame(_vp(frames[f]), fb, channels, _vp(specs[f]), _vp(win[f]), int(tones), _vp(fl[f:f + 1]))
    return specs, win, fl


# ---- the smallest admissible sizes, from the tables ------------------------------------------------------------------------------
def inc_tables():
    t = open(os.path.join(ROOT, "atracdenc_amd", "csrc", "at3p_vlc.inc")).read()
    out = {}
    for m in re.finditer(r"(AT3P_[A-Z0-9_]+)((?:\[[^\]]*\])+)\s*=\s*\{(.*?)\};", t, re.S):
        if "p+" not in m.group(3) and "p-" not in m.group(3):   # (the float tables are not needed)
            out[m.group(1)] = [int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", m.group(3))]
    return out


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


# ---- round trip -------------------------------------------------------------------------------------------------------------------
def snr_db(ref, got):
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    err = float(np.sum((ref - got) ** 2))
    return float("inf") if err == 0 else 10.0 * np.log10(float(np.sum(ref ** 2)) / err)
