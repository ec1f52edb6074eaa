"""Helpers of the adaptive word-length tests, their golden generator and their SIMT-harness driver (TEST INFRASTRUCTURE: nothing
under atracdenc_amd/ imports this module).

  * alloc_lib: the C restatement tests/host/at3p_alloc_cpu.c (include/at3phip.h, ADAPTIVE WORD LENGTHS, steps A1-A6), compiled on
    first use with the reference's arithmetic flags.
  * tail_bits_list: the frame's tail (window shapes, gain-compensation bits, tonal flag and block, noise flag, terminator) with the
    restated tonal-block writer of at3p_tonal_lib.
  * write_adaptive: the restatement's frames for spectra, window flags and tonal blocks (dicts or records); cost_table / allocate:
    its steps A1-A2 and A3-A5 alone.
  * parse_frame: an independent parser of a frame's head (unit count, word lengths, scale factor and table indices) and the
    recount of Bits(A) from the parsed fields.
  * the signals and cases of the tests: specs_of, edge frames, random cost tables, the golden's cases.
"""
import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np

from at3_testlib import ORACLE_SO, _vp, at3p_specs, oracle
from at3p_decode_lib import CFLAGS
from at3p_tonal_lib import tonal_bits

HERE = os.path.dirname(os.path.abspath(__file__))
ALLOC_SRC = os.path.join(HERE, "host", "at3p_alloc_cpu.c")
GOLDEN = os.path.join(HERE, "golden", "at3p_alloc.npz")
SIZE_BITS = 2048 * 8 - 3
T_MIN, T_MAX, K_MAX = -21, 63, 64
INFO_DTYPE = np.dtype([("t", "<i4"), ("k", "<i4"), ("num_quant_units", "<i4"), ("bits", "<i4"), ("wl", "u1", (2, 32)), ("sfi", "u1", (2, 32)),
                       ("tab", "u1", (2, 32))])
SIGNALS = ("noise", "mix", "stress", "tones", "burst")
SNR_FRAMES = 14
QU_START = [0, 16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 224, 256, 288, 320, 352, 384, 448, 512, 576, 640, 704, 768, 896, 1024, 1152, 1280, 1408,
            1536, 1664, 1792, 1920, 2048]
QU_TO_SB = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
SB_POWGRPS = [1, 2, 2, 3, 3, 3, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5]

_so = None


def alloc_lib():
    global _so
    if _so is None:
        d = tempfile.mkdtemp(prefix="at3palloc_")
        so = os.path.join(d, "libat3palloc_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, ALLOC_SRC, "-lm"])
        _so = so
    lib = ctypes.CDLL(_so)
    assert lib.at3pa_frame_info_size() == INFO_DTYPE.itemsize
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


def write_adaptive(specs, win=None, blocks=None, info=False):
    """the restatement: specs float32 [n, C, 2048], win uint16 [n, C] or None, blocks [n] -> frames uint8 [n, 2048] (and the
    per-frame record of INFO_DTYPE when info=True)"""
    lib = alloc_lib()
    specs = np.ascontiguousarray(specs, np.float32)
    n, nch = specs.shape[0], specs.shape[1]
    tb = lib.at3pa_tail_bytes()
    tails, nbits = np.zeros((n, tb), np.uint8), np.zeros(n, np.int32)
    for f, b in enumerate(_blocks_as_dicts(nch, blocks, n)):
        tails[f], nbits[f] = pack_tail(tail_bits_list(nch, None if win is None else win[f], b), tb)
    out, rec = np.zeros((n, 2048), np.uint8), np.zeros(n, INFO_DTYPE)
    assert lib.at3pa_write_frames(_vp(specs), nch, n, _vp(tails), _vp(nbits), _vp(out), _vp(rec)) == n
    return (out, rec) if info else out


def cost_table(specs):
    """A1-A2 of one frame: specs [C, 2048] -> (sfi uint8 [C, 32], bits uint16 [C, 32, 8], tab uint8 [C, 32, 8])"""
    specs = np.ascontiguousarray(specs, np.float32)
    nch = specs.shape[0]
    sfi, bits, tab = np.zeros((nch, 32), np.uint8), np.zeros((nch, 32, 8), np.uint16), np.zeros((nch, 32, 8), np.uint8)
    assert alloc_lib().at3pa_cost_table(_vp(specs), nch, _vp(sfi), _vp(bits), _vp(tab), None) == 0
    return sfi, bits, tab


def allocate(sfi, bits, tail_bits):
    """A3-A5 of the restatement: (wl uint8 [C, 32], N, t*, k*, Bits)"""
    sfi, bits = np.ascontiguousarray(sfi, np.uint8), np.ascontiguousarray(bits, np.uint16)
    nch = sfi.shape[0]
    wl, out = np.zeros((nch, 32), np.uint8), np.zeros(3, np.int32)
    lib = alloc_lib()
    total = lib.at3pa_allocate(_vp(sfi), _vp(bits), nch, int(tail_bits), _vp(wl), _vp(out[0:1]), _vp(out[1:2]), _vp(out[2:3]))
    return wl, int(out[0]), int(out[1]), int(out[2]), int(total)


# ---- an independent parser ------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, frame):
        self.b, self.pos = np.unpackbits(np.asarray(frame, np.uint8)), 0

    def get(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | int(self.b[self.pos])
            self.pos += 1
        return v


def _wl_vlc():
    """[4][8] (code, len) from the generated table file"""
    import re
    t = open(os.path.join(HERE, "..", "atracdenc_amd", "csrc", "at3p_vlc.inc")).read()
    t = t[t.index("AT3P_WL_VLC[4][8]"):]
    v = [int(x, 16) for x in re.findall(r"0x[0-9a-f]{4}", t[:t.index("};")])]
    return [[(e & 0xfff, e >> 12) for e in v[8 * i:8 * i + 8]] for i in range(4)]


def _read_vlc(r, table):
    code, n = 0, 0
    while n < 6:
        code, n = (code << 1) | r.get(1), n + 1
        for sym, (c, ln) in enumerate(table):
            if ln == n and c == code:
                return sym
    raise ValueError("no word-length code")


def parse_frame(frame, nch):
    """the frame's head, read back without the writer's help: {"N", "wl" [nch][N], "sfi", "tab", "wl_bits": the word-length
    section's length, "data_pos": the first bit of channel 0's spectra}"""
    vlc = _wl_vlc()
    r = _Bits(frame)
    assert r.get(1) == 0 and r.get(2) == nch - 1
    N = r.get(5) + 1
    assert r.get(1) == 0   # mute
    start = r.pos
    assert r.get(2) == 3 and r.get(2) == 0 and r.get(2) == 0
    idx = r.get(2)
    wl = [[r.get(3)]]
    for _ in range(1, N):
        wl[0].append((wl[0][-1] + _read_vlc(r, vlc[idx])) & 7)
    if nch == 2:
        assert r.get(2) == 1 and r.get(2) == 0
        idx = r.get(2)
        wl.append([(wl[0][i] + _read_vlc(r, vlc[idx])) & 7 for i in range(N)])
    wl_bits = r.pos - start
    sfi = []
    for _ in range(nch):
        assert r.get(2) == 0
        sfi.append([r.get(6) for _ in range(N)])
    assert r.get(1) == 1
    tab = []
    for _ in range(nch):
        assert r.get(1) == 0 and r.get(2) == 0 and r.get(1) == 0
        tab.append([r.get(3) for _ in range(N)])
    return {"N": N, "wl": wl, "sfi": sfi, "tab": tab, "wl_bits": wl_bits, "data_pos": r.pos}


def terminator_pos(frame):
    """the bit position of the last set bit: the terminator's second bit"""
    b = np.unpackbits(np.asarray(frame, np.uint8))
    return int(np.nonzero(b)[0][-1])


def recount_bits(parsed, nch, bits, tail_bits):
    """Bits(A) of A4 from a parsed frame, the cost table `bits` [nch][32][8] of its spectra and its tail: the word-length section
    by the oracle's at3po_wordlen_bits"""
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


# ---- signals and cases -----------------------------------------------------------------------------------------------------------
def specs_of(name, nch, n=SNR_FRAMES):
    """[n, C, 2048]: the spectra at3phip_encode_frames forms for a test signal (oracle PQF and MDCT)"""
    if name == "silence":
        return np.zeros((n, nch, 2048), np.float32)
    if name == "fullscale":
        return full_scale_noise(n, nch)
    return at3p_specs(name, n, nch)


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


GOLDEN_CASES = [(name, nch) for name in SIGNALS + ("silence", "fullscale") for nch in (1, 2)]
GOLDEN_FRAMES = 4


def golden_entry(name, nch):
    """(t*, k*, N per frame as int32 [F, 3], SHA-256 of the frames) of the restatement for a golden case"""
    frames, rec = write_adaptive(specs_of(name, nch, GOLDEN_FRAMES), info=True)
    return np.stack([rec["t"], rec["k"], rec["num_quant_units"]], axis=1).astype(np.int32), hashlib.sha256(frames.tobytes()).hexdigest()
