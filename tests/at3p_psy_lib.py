"""Helpers of the MASKING-WEIGHTED WORD LENGTHS tests (include/at3phip.h, M1-M7), their golden generator, SIMT-harness driver and bench
tool (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * write_psy / allocate_psy: at3p_writer_lib's write_rd / allocate_rd with psy: the restatement tests/host/at3p_rd_cpu.c states both.
  * psy_tables: the two integer tables of at3p_psy.inc; weighted_total: Tw of M6 recomputed in Python; offsets_py: M1-M3 in Python.
  * masked_twin: the spectrum of the one test of behaviour; the cases of tests/golden/at3p_psy.npz; the inputs and digests of
    tests/golden/at3p_rd_fold.npz.
"""
import os
import re

import numpy as np

import at3p_writer_lib as W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PSY_INC = os.path.join(ROOT, "atracdenc_amd", "csrc", "at3p_psy.inc")
MU_HI, O_MAX = 73, 32


def write_psy(specs, frame_bytes, win=None, blocks=None, info=False):
    """at3p_writer_lib.write_rd with MASKING-WEIGHTED WORD LENGTHS"""
    return W.write_rd(specs, frame_bytes, win, blocks, info, psy=True)


def write_psy_streams(specs, frame_bytes, blocks=None):
    """write_psy for [S, F, C, 2048] -> [S, F, frame_bytes]; blocks [S][F] or None"""
    return np.stack([write_psy(specs[s], frame_bytes, None, None if blocks is None else blocks[s]) for s in range(specs.shape[0])])


def allocate_psy(sfi, bits, dist, tail_bits, frame_bytes, offsets=None):
    """M1-M6 of the restatement: (wl uint8 [C, 32], N, record of W.RD_INFO_DTYPE); offsets uint8 [C, 32] replace M1-M3's"""
    return W.allocate_rd(sfi, bits, dist, tail_bits, frame_bytes, offsets, psy=True)


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
    return {"frames": frames, "choice": np.stack([rec["j"], rec["k"], rec["num_quant_units"], rec["chose"], rec["O"]], axis=1).astype(np.int32),
            "o": rec["o"], "wl": rec["wl"], "Tw": np.stack([rec["T"], rec["T_sparse"]], axis=1)}


# ---- at3p_rd_fold.npz: what the two restatements and the two host allocators gave before they were folded ----
RD_FOLD_GOLDEN = os.path.join(HERE, "golden", "at3p_rd_fold.npz")
SIZES = {1: (176, 376, 744, 2048), 2: (224, 376, 744, 2048)}
CELLS = [(name, nch, fb) for name in ("noise", "tones", "mix", "burst") for nch in (1, 2) for fb in SIZES[nch]]
_rand = []


def random_tables():
    """2000 x (sfi, bits, dist, tail_bits, offsets, frame_bytes)"""
    if not _rand:
        tabs = W.random_dist_tables(W.random_cost_tables(2000))
        for i, ((sfi, bits, dist, tail), off) in enumerate(zip(tabs, random_offsets(tabs))):
            fb = SIZES[sfi.shape[0]][i % 4]
            _rand.append((sfi, bits, dist, min(tail, 8 * fb - 3), off, fb))
    return _rand


def rd_fold_entries():
    """{label: SHA-256} of tests/golden/at3p_rd_fold.npz, field by field and never a record's bytes. Per hundred of random_tables: the
    inputs (`in`); wl, N, j*, k*, the guard's outcome, Bits and both T of the restatement (`rest`) and wl, N, j*, k* and the outcome of
    the host function (`host`) with rate-distortion word lengths (`rd`), masking-weighted with the offsets given (`psy`, with o, O and mu,
    and the host function's offsets out) and, on every fourth table, with the offsets left to M1-M3 (`m`). Per cell of CELLS: the
    spectra of 3 frames, and the frames, tail bits and every field of the record of write_rd and of write_psy."""
    from atracdenc_amd.binding import at3p_host_allocate_psy, at3p_host_allocate_rd
    rest = lambda wl, N, r, more=(): [wl, N] + [r[f] for f in ("j", "k", "chose", "bits", "T", "T_sparse") + more]
    out, tabs = {}, random_tables()
    for g in range(0, len(tabs), 100):
        parts = {k: [] for k in ("in", "rd_rest", "rd_host", "psy_rest", "psy_host", "m_rest", "m_host")}
        for i in range(g, g + 100):
            sfi, bits, dist, tail, off, fb = tabs[i]
            parts["in"] += [sfi, bits, dist, tail, off, fb]
            parts["rd_rest"] += rest(*W.allocate_rd(sfi, bits, dist, tail, fb))
            parts["rd_host"] += list(at3p_host_allocate_rd(sfi, bits, dist, tail, fb))
            parts["psy_rest"] += rest(*W.allocate_rd(sfi, bits, dist, tail, fb, offsets=off), more=("o", "O", "mu"))
            parts["psy_host"] += list(at3p_host_allocate_psy(sfi, bits, dist, tail, fb, offsets=off))
            if i % 4 == 0:
                parts["m_rest"] += rest(*W.allocate_rd(sfi, bits, dist, tail, fb, psy=True), more=("o", "O", "mu"))
                parts["m_host"] += list(at3p_host_allocate_psy(sfi, bits, dist, tail, fb))
        for k, v in parts.items():
            out[f"t{g // 100:02d}_{k}"] = W.sha(*v)
    for name, nch, fb in CELLS:
        sp = W.specs_of(name, nch, 3)
        out[f"{name}_{nch}_{fb}_in"] = W.sha(sp.view(np.uint32))
        for mode in ("rd", "psy"):
            frames, rec, nbits = W.write_rd(sp, fb, info=True, psy=mode == "psy")
            out[f"{name}_{nch}_{fb}_{mode}"] = W.sha(frames, nbits, *[rec[f] for f in ("j", "k", "num_quant_units", "bits", "chose", "t", "k_sparse", "O", "T",
                                                                                     "T_sparse", "o", "mu", "wl", "sfi", "tab")])
    return out


def rd_fold_file_arrays():
    e = rd_fold_entries()
    return {"labels": np.array(list(e)), "sha256": np.stack(list(e.values()))}
