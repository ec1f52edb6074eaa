"""Helpers of the MASKING-WEIGHTED WORD LENGTHS tests (include/at3phip.h, M1-M7), their golden generator, SIMT-harness driver and bench
tool (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * psy_lib: the C restatement tests/host/at3p_psy_cpu.c, which includes at3p_rd_cpu.c and through it every restatement of the adaptive
    writer; compiled once, on first use, with the reference's arithmetic flags.
  * write_psy / allocate_psy: the restatement's entry points, as at3p_writer_lib's write_rd / allocate_rd.
  * psy_tables: the two integer tables of at3p_psy.inc; weighted_total: Tw of M6 recomputed in Python; offsets_py: M1-M3 in Python.
  * masked_twin: the spectrum of the one test of behaviour; the cases of tests/golden/at3p_psy.npz.
"""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

import at3p_writer_lib as W
from at3_testlib import _vp
from at3p_decode_lib import CFLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PSY_SRC = os.path.join(HERE, "host", "at3p_psy_cpu.c")
PSY_INC = os.path.join(ROOT, "atracdenc_amd", "csrc", "at3p_psy.inc")
MU_HI, O_MAX = 73, 32
PSY_INFO_DTYPE = np.dtype([("j", "<i4"), ("k", "<i4"), ("num_quant_units", "<i4"), ("bits", "<i4"), ("chose_psy", "<i4"), ("t", "<i4"),
                           ("k_sparse", "<i4"), ("O", "<i4"), ("Tw_psy", "<f8"), ("Tw_sparse", "<f8"), ("o", "u1", (2, 32)), ("mu", "<i4", (2, 32)),
                           ("wl", "u1", (2, 32)), ("sfi", "u1", (2, 32)), ("tab", "u1", (2, 32))])
_so = None


def psy_lib():
    global _so
    if _so is None:
        d = tempfile.mkdtemp(prefix="at3ppsy_")
        so = os.path.join(d, "libat3ppsy_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, PSY_SRC, "-lm"])
        _so = so
    lib = ctypes.CDLL(_so)
    I, P = ctypes.c_int, ctypes.c_void_p
    lib.at3ppsy_allocate.argtypes = [P, P, P, P, I, I, I, P, P, P]
    lib.at3ppsy_write_frames.argtypes = [P, I, I, I, P, P, P, P]
    assert lib.at3ppsy_frame_info_size() == PSY_INFO_DTYPE.itemsize
    return lib


def write_psy(specs, frame_bytes, win=None, blocks=None, info=False):
    """at3p_writer_lib.write_rd with MASKING-WEIGHTED WORD LENGTHS (records of PSY_INFO_DTYPE)"""
    psy_lib()
    return W._write(lambda lib, sp, nch, n, tails, nbits, out, rec: psy_lib().at3ppsy_write_frames(sp, nch, n, int(frame_bytes), tails, nbits, out, rec),
                    PSY_INFO_DTYPE, specs, frame_bytes, win, blocks, info)


def write_psy_streams(specs, frame_bytes, blocks=None):
    """write_psy for [S, F, C, 2048] -> [S, F, frame_bytes]; blocks [S][F] or None"""
    return np.stack([write_psy(specs[s], frame_bytes, None, None if blocks is None else blocks[s]) for s in range(specs.shape[0])])


def allocate_psy(sfi, bits, dist, tail_bits, frame_bytes, offsets=None):
    """M1-M6 of the restatement: (wl uint8 [C, 32], N, record of PSY_INFO_DTYPE); offsets uint8 [C, 32] replace M1-M3's"""
    sfi, bits, dist = np.ascontiguousarray(sfi, np.uint8), np.ascontiguousarray(bits, np.uint16), np.ascontiguousarray(dist, np.uint64)
    nch = sfi.shape[0]
    off = None if offsets is None else np.ascontiguousarray(offsets, np.uint8)
    wl, n, rec = np.zeros((nch, 32), np.uint8), np.zeros(1, np.int32), np.zeros(1, PSY_INFO_DTYPE)
    rec["bits"] = psy_lib().at3ppsy_allocate(_vp(sfi), _vp(bits), _vp(dist), None if off is None else _vp(off), nch, int(tail_bits), int(frame_bytes),
                                             _vp(wl), _vp(n), _vp(rec))
    return wl, int(n[0]), rec[0]


def psy_tables():
    """(spread uint8 [32, 32] as [q'][q], ath uint8 [32]) of at3p_psy.inc"""
    t = re.sub(r"//[^\n]*", "", open(PSY_INC).read())
    body = lambda name: [int(x) for x in re.findall(r"\d+", t[t.index(name):].split("=", 1)[1].split(";", 1)[0])]
    return np.array(body("AT3P_PSY_SPREAD"), np.uint8).reshape(32, 32), np.array(body("AT3P_PSY_ATH"), np.uint8)


def g_table():
    """G[i] = (double)ScaleTable[i]^2, float64 [64]"""
    sc = W.scale_table().astype(np.float64)
    return sc * sc


def lam(i):
    """lambda_i of R2 for any integer i, exact"""
    q, r = divmod(int(i), 3)
    return float(np.ldexp(g_table()[r], 40 + 2 * q))


def offsets_py(sfi, dist):
    """M1-M3 in Python from the header's text: (mu int [C, 32], o uint8 [C, 32], O)"""
    spread, ath = psy_tables()
    G = g_table()
    nch = sfi.shape[0]
    lams = [lam(i) for i in range(MU_HI + 1)]
    mu = np.zeros((nch, 32), int)
    for ch in range(nch):
        E = [np.float64(int(dist[ch, m, 0])) * G[sfi[ch, m]] for m in range(32)]
        for q in range(32):
            th = lam(ath[q])
            for m in range(32):
                if spread[m, q] <= 63:
                    th = max(th, float(E[m] * G[63 - spread[m, q]]))
            mu[ch, q] = max(i for i in range(MU_HI + 1) if lams[i] <= th)
    live = dist[:, :, 0] > 0
    o = np.zeros((nch, 32), np.uint8)
    if live.any():
        o[live] = np.minimum(mu[live] - mu[live].min(), O_MAX)
    return mu, o, int(o.max())


def weighted_total(sfi, dist, wl, o):
    """Tw of M6: the serial double sum of D[ch][qu][wl] * G[63 - o] in the order of the walk, from +0.0"""
    G = g_table()
    T = np.float64(0.0)
    for qu in range(32):
        for ch in range(sfi.shape[0]):
            D = np.float64(int(dist[ch, qu, int(wl[ch, qu])])) * G[sfi[ch, qu]]
            T = T + D * G[63 - int(o[ch, qu])]
    return float(T)


def random_offsets(tables_in, seed=91):
    """offsets uint8 [C, 32] per case of random_dist_tables: none, a ramp, random 0..32, and the extremes side by side"""
    rng = np.random.default_rng(seed)
    out = []
    for i, (sfi, _, _, _) in enumerate(tables_in):
        nch = sfi.shape[0]
        kind = i % 4
        if kind == 0:
            o = rng.integers(0, 33, (nch, 32))
        elif kind == 1:
            o = np.tile(np.arange(32), (nch, 1)) + rng.integers(0, 2, (nch, 32))
        elif kind == 2:
            o = rng.choice([0, 32], (nch, 32))
        else:
            o = rng.integers(0, 6, (nch, 32))
        out.append(np.clip(o, 0, 32).astype(np.uint8))
    return out


def masked_twin(seed=3):
    """mono spectrum [1, 1, 2048]: unit 1 loud (noise at 0.25), units 2 and 7 line for line the same 16 values 30 dB below; unit 2 is next
    to the masker, unit 7 six Bark up"""
    rng = np.random.default_rng(seed)
    sp = np.zeros((1, 1, 2048), np.float32)
    sp[0, 0, 16:32] = (0.25 * rng.standard_normal(16)).clip(-0.9, 0.9)
    twin = (0.25 * 10.0 ** (-30.0 / 20.0) * rng.standard_normal(16)).astype(np.float32)
    sp[0, 0, 32:48] = twin
    sp[0, 0, 112:128] = twin
    return sp


# ---- golden file ---------------------------------------------------------------------------------------------------------------------
PSY_GOLDEN = os.path.join(HERE, "golden", "at3p_psy.npz")
PSY_GOLDEN_CASES = [(name, nch, fb) for name in ("noise", "tones", "mix") for nch in (1, 2) for fb in (376, 2048)]
PSY_GOLDEN_FRAMES = 3


def psy_golden_entry(name, nch, fb):
    """the restatement on 3 frames of a signal: {frames uint8 [3, fb], choice int32 [3, 5] (j*, k*, N, chose_psy, O), o uint8 [3, 2, 32],
    wl uint8 [3, 2, 32], Tw float64 [3, 2] (Tw(P), Tw(A))}"""
    frames, rec, _ = write_psy(W.specs_of(name, nch, PSY_GOLDEN_FRAMES), fb, info=True)
    return {"frames": frames, "choice": np.stack([rec["j"], rec["k"], rec["num_quant_units"], rec["chose_psy"], rec["O"]], axis=1).astype(np.int32),
            "o": rec["o"], "wl": rec["wl"], "Tw": np.stack([rec["Tw_psy"], rec["Tw_sparse"]], axis=1)}
