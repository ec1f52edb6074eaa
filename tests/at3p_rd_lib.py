"""Helpers of the ATRAC3plus rate-distortion allocation tests, their SIMT-harness driver, tools/gen_golden_at3p_rd.py and
tools/at3p_rd_bench.py (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * rd_lib: the C restatement tests/host/at3p_rd_cpu.c - the sparse restatement with RATE-DISTORTION WORD LENGTHS (include/at3phip.h,
    R1-R5) -, compiled on first use with the reference's arithmetic flags.
  * write_rd / write_streams / tables / allocate: its entry points; specs_of_pcm: the spectra of a PCM stream; INFO_DTYPE: its per-frame record (j*, k*, which of the two
    allocations was written, both T).
  * total_distortion: T of R4 recomputed in Python from a distortion table and word lengths.
  * guard_table: a hand-built table on which the guard of R4 fires.
  * min_chunk_bits / j_max_bound: the J_MAX bound of R3 re-derived from at3p_vlc.inc.
  * GOLDEN, golden_entry: tests/golden/at3p_rd.npz (tools/gen_golden_at3p_rd.py) and what it holds per case.
Decoding, the head's parser and Bits(A) recounted are at3p_sparse_lib's: the frames are sparse frames.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from at3_testlib import _vp
from at3p_alloc_lib import QU_START, _blocks_as_dicts, pack_tail, tail_bits_list
from at3p_decode_lib import CFLAGS
from at3p_rate_lib import inc_tables

HERE = os.path.dirname(os.path.abspath(__file__))
RD_SRC = os.path.join(HERE, "host", "at3p_rd_cpu.c")
J_MIN, J_MAX = -30, 69
INFO_DTYPE = np.dtype([("j", "<i4"), ("k", "<i4"), ("num_quant_units", "<i4"), ("bits", "<i4"), ("chose_rd", "<i4"), ("t", "<i4"), ("k_sparse", "<i4"),
                       ("pad", "<i4"), ("T_rd", "<f8"), ("T_sparse", "<f8"), ("wl", "u1", (2, 32)), ("sfi", "u1", (2, 32)), ("tab", "u1", (2, 32))])
LINES = np.diff(np.array(QU_START))

_so = None


def rd_lib():
    global _so
    if _so is None:
        d = tempfile.mkdtemp(prefix="at3prd_")
        so = os.path.join(d, "libat3prd_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, RD_SRC, "-lm"])
        _so = so
    lib = ctypes.CDLL(_so)
    I, P = ctypes.c_int, ctypes.c_void_p
    lib.at3prd_tables.argtypes = [P, I, P, P, P, P, P]
    lib.at3prd_allocate.argtypes = [P, P, P, I, I, I, P, P, P]
    lib.at3prd_write_frames.argtypes = [P, I, I, I, P, P, P, P]
    assert lib.at3prd_frame_info_size() == INFO_DTYPE.itemsize
    assert (lib.at3prd_j_min(), lib.at3prd_j_max()) == (J_MIN, J_MAX)
    return lib


def write_rd(specs, frame_bytes, win=None, blocks=None, info=False):
    """specs float32 [n, C, 2048], win uint16 [n, C] or None, blocks [n] (dicts, records or None) -> frames uint8 [n, frame_bytes]
    (and the per-frame records of INFO_DTYPE and the tails' bits with info=True)"""
    lib = rd_lib()
    specs = np.ascontiguousarray(specs, np.float32)
    n, nch = specs.shape[0], specs.shape[1]
    tb = lib.at3ps_tail_bytes()
    tails, nbits = np.zeros((n, tb), np.uint8), np.zeros(n, np.int32)
    for f, b in enumerate(_blocks_as_dicts(nch, blocks, n)):
        tails[f], nbits[f] = pack_tail(tail_bits_list(nch, None if win is None else win[f], b), tb)
    out, rec = np.zeros((n, frame_bytes), np.uint8), np.zeros(n, INFO_DTYPE)
    assert lib.at3prd_write_frames(_vp(specs), nch, n, int(frame_bytes), _vp(tails), _vp(nbits), _vp(out), _vp(rec)) == n
    return (out, rec, nbits) if info else out


def write_streams(specs, frame_bytes, win=None, blocks=None):
    """the same for [S, F, C, 2048] -> [S, F, frame_bytes]"""
    S, F = specs.shape[:2]
    flat = write_rd(specs.reshape((S * F,) + specs.shape[2:]), frame_bytes, None if win is None else win.reshape(S * F, -1),
                    None if blocks is None else (blocks.reshape(-1) if isinstance(blocks, np.ndarray) else blocks))
    return flat.reshape(S, F, frame_bytes)


def specs_of_pcm(pcm):
    """pcm [n, 2048, C] of one stream from its start -> [n, C, 2048]: the spectra at3phip_encode_frames hands its writer"""
    from at3_testlib import at3p_mdct, at3p_pqf
    from at3p_gha_lib import SCALE
    out = np.zeros((pcm.shape[0], pcm.shape[2], 2048), np.float32)
    for c in range(pcm.shape[2]):
        bands = at3p_pqf(np.ascontiguousarray(pcm[:, :, c]))
        out[:, c] = at3p_mdct((bands.astype(np.float64) / SCALE).astype(np.float32))
    return out


def tables(spec):
    """A1 + A2 + R1 of one frame [C, 2048]: (sfi uint8 [C, 32], bits uint16 [C, 32, 8], dist uint64 [C, 32, 8])"""
    spec = np.ascontiguousarray(spec, np.float32)
    nch = spec.shape[0]
    sfi, bits, tab = np.zeros((nch, 32), np.uint8), np.zeros((nch, 32, 8), np.uint16), np.zeros((nch, 32, 8), np.uint8)
    dist = np.zeros((nch, 32, 8), np.uint64)
    assert rd_lib().at3prd_tables(_vp(spec), nch, _vp(sfi), _vp(bits), _vp(tab), _vp(dist), None) == 0
    return sfi, bits, dist


def allocate(sfi, bits, dist, tail_bits, frame_bytes):
    """R2-R4 of the restatement: (wl uint8 [C, 32], N, record of INFO_DTYPE with j, k, chose_rd, t, k_sparse, T_rd, T_sparse, bits)"""
    sfi, bits, dist = np.ascontiguousarray(sfi, np.uint8), np.ascontiguousarray(bits, np.uint16), np.ascontiguousarray(dist, np.uint64)
    nch = sfi.shape[0]
    wl, n, rec = np.zeros((nch, 32), np.uint8), np.zeros(1, np.int32), np.zeros(1, INFO_DTYPE)
    rec["bits"] = rd_lib().at3prd_allocate(_vp(sfi), _vp(bits), _vp(dist), nch, int(tail_bits), int(frame_bytes), _vp(wl), _vp(n), _vp(rec))
    return wl, int(n[0]), rec[0]


def scale_table():
    """ScaleTable as float32 [64]: 2^(i / 3 - 21) rounded to float; entry i + 3 is exactly twice entry i"""
    import re
    t = open(os.path.join(HERE, "..", "atracdenc_amd", "csrc", "at3p_vlc.inc")).read()
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


def random_dist_tables(tables_in, seed=77):
    """[(sfi, bits, dist, tail_bits)] from at3p_alloc_lib.random_cost_tables' cases: S falling with w by a random factor per step, with
    steps that do not fall and units of all-zero distortion among them"""
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


# ---- golden ------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(HERE, "golden", "at3p_rd.npz")
GOLDEN_CASES = [(name, nch, fb) for name in ("noise", "tones", "mix") for nch in (1, 2) for fb in (376, 2048)]
GOLDEN_FRAMES = 3


def golden_entry(name, nch, fb):
    """the restatement on 3 frames of a signal: {frames uint8 [3, fb], choice int32 [3, 4] (j*, k*, N, chose_rd), wl uint8 [3, 2, 32],
    T float64 [3, 2] (T(R), T(A))}"""
    from at3p_alloc_lib import specs_of
    frames, rec, _ = write_rd(specs_of(name, nch, GOLDEN_FRAMES), fb, info=True)
    return {"frames": frames, "choice": np.stack([rec["j"], rec["k"], rec["num_quant_units"], rec["chose_rd"]], axis=1).astype(np.int32),
            "wl": rec["wl"], "T": np.stack([rec["T_rd"], rec["T_sparse"]], axis=1)}
