"""Helpers of the ATRAC3plus sparse-allocation tests, their SIMT-harness driver and tools/at3p_sparse_bench.py (TEST INFRASTRUCTURE:
nothing under atracdenc_amd/ imports this module).

  * sparse_lib: the C restatement tests/host/at3p_sparse_cpu.c - the adaptive writer and the decoder of include/at3phip.h with
    SPARSE WORD LENGTHS and the frame size as arguments -, compiled on first use with the reference's arithmetic flags.
  * write_adaptive / allocate / cost_table / SparseDecoder / decode / unpack: its entry points, each with `sparse`.
  * parse_head / count_bits: an independent parser of a frame's head (everything in front of the spectra) and Bits(A) recounted
    from a frame's word lengths, written from the header's text and not from the restatement.
  * edge_tables: the hand-built cost tables of the definition's special cases; edge_specs / edge_cases_reached: spectra that reach
    the same cases through the writer at the smallest frame size, and the check that they did.
  * GOLDEN, golden_entry: tests/golden/at3p_sparse.npz (tools/gen_golden_at3p_sparse.py) and what it holds per case.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from at3_testlib import _vp
from at3p_alloc_lib import INFO_DTYPE, QU_TO_SB, _blocks_as_dicts, pack_tail, tail_bits_list
from at3p_decode_lib import CFLAGS, FIELDS_DTYPE, REASONS
from at3p_rate_lib import inc_tables

HERE = os.path.dirname(os.path.abspath(__file__))
SPARSE_SRC = os.path.join(HERE, "host", "at3p_sparse_cpu.c")

_so = None


def sparse_lib():
    global _so
    if _so is None:
        d = tempfile.mkdtemp(prefix="at3psparse_")
        so = os.path.join(d, "libat3psparse_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, SPARSE_SRC, "-lm"])
        _so = so
    lib = ctypes.CDLL(_so)
    I, P = ctypes.c_int, ctypes.c_void_p
    lib.at3ps_state_bytes.restype = ctypes.c_size_t
    lib.at3ps_reset.argtypes = [P]
    lib.at3ps_decode.argtypes = [P, I, P, I, I, P, P, I, I]
    lib.at3ps_unpack_frame.argtypes = [P, I, I, P, P, I, I, P]
    lib.at3ps_write_frames.argtypes = [P, I, I, I, I, P, P, P, P]
    lib.at3ps_allocate.argtypes = [P, P, I, I, I, I, P, P, P, P]
    lib.at3ps_cost_table.argtypes = [P, I, P, P, P, P]
    assert lib.at3ps_frame_info_size() == INFO_DTYPE.itemsize
    return lib


# ---- the encoder ---------------------------------------------------------------------------------------------------------------
def write_adaptive(specs, frame_bytes, sparse, win=None, blocks=None, info=False):
    """specs float32 [n, C, 2048], win uint16 [n, C] or None, blocks [n] (dicts, records or None) -> frames uint8 [n, frame_bytes]
    (and the per-frame record of at3p_alloc_lib.INFO_DTYPE with info=True)"""
    lib = sparse_lib()
    specs = np.ascontiguousarray(specs, np.float32)
    n, nch = specs.shape[0], specs.shape[1]
    tb = lib.at3ps_tail_bytes()
    tails, nbits = np.zeros((n, tb), np.uint8), np.zeros(n, np.int32)
    for f, b in enumerate(_blocks_as_dicts(nch, blocks, n)):
        tails[f], nbits[f] = pack_tail(tail_bits_list(nch, None if win is None else win[f], b), tb)
    out, rec = np.zeros((n, frame_bytes), np.uint8), np.zeros(n, INFO_DTYPE)
    assert lib.at3ps_write_frames(_vp(specs), nch, n, int(frame_bytes), int(bool(sparse)), _vp(tails), _vp(nbits), _vp(out), _vp(rec)) == n
    return (out, rec, nbits) if info else out


def write_streams(specs, frame_bytes, sparse, win=None, blocks=None):
    """the same for [S, F, C, 2048] -> [S, F, frame_bytes]"""
    S, F = specs.shape[:2]
    flat = write_adaptive(specs.reshape((S * F,) + specs.shape[2:]), frame_bytes, sparse, None if win is None else win.reshape(S * F, -1),
                          None if blocks is None else (blocks.reshape(-1) if isinstance(blocks, np.ndarray) else blocks))
    return flat.reshape(S, F, frame_bytes)


def cost_table(spec):
    """A1 + A2 of one frame [C, 2048]: (sfi uint8 [C, 32], bits uint16 [C, 32, 8])"""
    spec = np.ascontiguousarray(spec, np.float32)
    nch = spec.shape[0]
    sfi, bits, tab = np.zeros((nch, 32), np.uint8), np.zeros((nch, 32, 8), np.uint16), np.zeros((nch, 32, 8), np.uint8)
    assert sparse_lib().at3ps_cost_table(_vp(spec), nch, _vp(sfi), _vp(bits), _vp(tab), None) == 0
    return sfi, bits


def allocate(sfi, bits, tail_bits, frame_bytes, sparse):
    """A3-A5 of the restatement against 8 * frame_bytes - 3: (wl uint8 [C, 32], N, t*, k*, Bits)"""
    sfi, bits = np.ascontiguousarray(sfi, np.uint8), np.ascontiguousarray(bits, np.uint16)
    nch = sfi.shape[0]
    wl, out = np.zeros((nch, 32), np.uint8), np.zeros(3, np.int32)
    total = sparse_lib().at3ps_allocate(_vp(sfi), _vp(bits), nch, int(tail_bits), int(frame_bytes), int(bool(sparse)), _vp(wl), _vp(out[0:1]),
                                        _vp(out[1:2]), _vp(out[2:3]))
    return wl, int(out[0]), int(out[1]), int(out[2]), int(total)


# ---- the decoder ---------------------------------------------------------------------------------------------------------------
class SparseDecoder:
    """One stream of the restatement; state carries across decode() calls."""

    def __init__(self, channels, tones=False, sparse=True):
        self.lib = sparse_lib()
        self.channels, self.tones, self.sparse = int(channels), int(bool(tones)), int(bool(sparse))
        self.state = np.zeros(self.lib.at3ps_state_bytes(), np.uint8)
        self.rejected = np.zeros(len(REASONS), np.uint64)
        self.lib.at3ps_reset(_vp(self.state))

    def decode(self, frames):
        """frames [N][frame_bytes] uint8 -> pcm [N][2048][channels] float32"""
        frames = np.ascontiguousarray(frames, np.uint8)
        n, fb = frames.shape
        pcm = np.zeros((n, 2048, self.channels), np.float32)
        self.lib.at3ps_decode(_vp(self.state), self.channels, _vp(frames), fb, n, _vp(pcm), _vp(self.rejected), self.tones, self.sparse)
        return pcm


def decode(frames, channels, tones=False, sparse=True):
    """from start-of-stream state: (pcm [N][2048][channels], rejected per reason [6] int64)"""
    d = SparseDecoder(channels, tones, sparse)
    pcm = d.decode(frames)
    return pcm, d.rejected.astype(np.int64).copy()


def decode_streams(frames, channels, tones=False, sparse=True):
    """[S, F, frame_bytes] -> (pcm [S, F, 2048, C], rejected summed over the streams)"""
    out = [decode(f, channels, tones, sparse) for f in frames]
    return np.stack([p for p, _ in out]), sum(r for _, r in out)


def unpack(frames, channels, tones=False, sparse=True):
    """steps 1-2: (spectra [N][channels][2048] float32, window flags [N][channels] uint16, fields [N])"""
    lib = sparse_lib()
    frames = np.ascontiguousarray(frames, np.uint8)
    n, fb = frames.shape
    specs, win, fl = np.zeros((n, channels, 2048), np.float32), np.zeros((n, channels), np.uint16), np.zeros(n, FIELDS_DTYPE)
    for f in range(n):
        lib.at3ps_unpack_frame(_vp(frames[f]), fb, channels, _vp(specs[f]), _vp(win[f]), int(tones), int(bool(sparse)), _vp(fl[f:f + 1]))
    return specs, win, fl


# ---- an independent parser of the head, from the header's text -----------------------------------------------------------------
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
    """Everything in front of the spectra of a frame written with AT3PHIP_ALLOC_SPARSE: dict with N, wl [nch][N], sf, tab (None for a
    unit without an index), clone (channel-1 units that carry the flag, with its value; clone_pos: the flag's bit) and pos, the
    spectra's first bit."""
    tb = inc_tables()
    wlv = [tb["AT3P_WL_VLC"][8 * i:8 * i + 8] for i in range(4)]
    b = _Bits(frame)
    assert b.rd(1) == 0 and b.rd(2) == nch - 1
    N = b.rd(5) + 1
    assert b.rd(1) == 0
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
    return {"N": N, "wl": wl[:nch], "sf": sf, "tab": tab, "clone": clone, "clone_pos": clone_pos, "pos": b.pos}


def count_bits(head, nch, unit_bits, tail_bits):
    """Bits(A) of A4s from a parsed head: unit_bits[ch][qu][w] the cost table, everything but the three leading bits"""
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


# ---- the definition's special cases as cost tables ---------------------------------------------------------------------------------
def edge_tables():
    """{name: (sfi uint8 [C, 32], bits uint16 [C, 32, 8], tail_bits, frame_bytes)}; bits are 16 x lines x w / 16-ish figures
    that make the budget bind where the case needs it"""
    lines = np.diff(np.array([0, 16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 224, 256, 288, 320, 352, 384, 448, 512, 576, 640, 704, 768, 896, 1024,
                              1152, 1280, 1408, 1536, 1664, 1792, 1920, 2048]))

    def bits_of(nch, per_line=1.0):
        b = np.zeros((nch, 32, 8), np.uint16)
        for w in range(1, 8):
            b[:, :, w] = np.minimum(65535, (lines * w * per_line).astype(np.int64) + 2)
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


# ---- crafted frames for the decoder ------------------------------------------------------------------------------------------------
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
        from at3p_alloc_lib import specs_of
        sp = specs_of("mix", 2, 1)
        sp[:, 1] = sp[:, 0] * np.float32(2.0 ** -6)     # channel 1 six bits under channel 0: zeros under coded units
        fr = write_adaptive(sp, frame_bytes, True)[0].copy()
        head = parse_head(fr, 2)
        assert head["clone_pos"] and all(v == 1 for v in head["clone"].values())
        pos = sorted(head["clone_pos"].values())[len(head["clone_pos"]) // 2]
        fr[pos >> 3] &= 0xff ^ (0x80 >> (pos & 7))
        out.append(fr)
    return np.stack(out)


# ---- the special cases through real spectra ------------------------------------------------------------------------------------------
def edge_specs(nch):
    """(spectra [4][C][2048], blocks [4]) for the smallest frame size of the channel count, where the budget binds:
      0  silence but for unit 31 of the last channel at full scale, beside the largest tonal record: the tail leaves room for one
         unit, unit (0, 0) wants nothing at t* or t* - 1 and unit 31's first bit does not fit: k* = 0, the empty frame, unit 0 of
         channel 0 takes 1 (A3s' first fix-up decides the frame);
      1  units 0-3 and unit 29 of the last channel alone: N becomes 32 and unit 31 of channel 0 takes 1 above zeros;
      2  `mix` with channel 1 six bits under channel 0: zeros under coded units, clone flags (stereo);
      3  one level everywhere: a flat sfi, A(t*, 0) is empty and k alone extends N."""
    from at3p_alloc_lib import QU_START, specs_of
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


# ---- golden ------------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(HERE, "golden", "at3p_sparse.npz")
GOLDEN_CASES = [(name, nch, fb) for name in ("noise", "tones") for nch in (1, 2) for fb in (376, 2048)]
GOLDEN_FRAMES = 3


def golden_entry(name, nch, fb):
    """the restatement on 3 frames of a signal: {frames uint8 [3, fb], choice int32 [3, 3] (t*, k*, N), wl uint8 [3, 2, 32],
    pcm_sha256: the SHA-256 of the sparse decoder's PCM [3, 2048, C] float32 as bytes}"""
    import hashlib
    from at3p_alloc_lib import specs_of
    frames, rec, _ = write_adaptive(specs_of(name, nch, GOLDEN_FRAMES), fb, True, info=True)
    pcm, rej = decode(frames, nch, False, True)
    assert rej.sum() == 0
    return {"frames": frames, "choice": np.stack([rec["t"], rec["k"], rec["num_quant_units"]], axis=1).astype(np.int32), "wl": rec["wl"],
            "pcm_sha256": np.array(hashlib.sha256(np.ascontiguousarray(pcm).tobytes()).hexdigest())}
