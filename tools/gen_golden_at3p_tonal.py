#!/usr/bin/env python3
"""Write tests/golden/at3p_tonal.npz: frames with tonal blocks and the PCM the ATRAC3plus decoder of include/at3phip.h must give
for them with AT3PHIP_DECODE_TONES.

Frames: the REFERENCE's writer, TAt3PBitStream::WriteFrame with hand-built TAt3PGhaData over the residual spectra of a test
signal (cases refw_*, their blocks stored as JSON so that the tests can compare the restated writer's bytes with them), and the
restated tonal-block writer (tests/at3p_tonal_lib.py) spliced into small frames without a tonal block, mono and stereo: 1, a few and 16 tone bands; sharing none, all and mixed; the leader swap on and off; envelope points at 0 and 31,
start < stop, start == stop and across frames; ascending and descending frequency packing with frequencies of 0 and >= 512;
15 waves in a band and 48 in a frame; tonal frames next to tone-free ones; crafted frames for each new rejection (a frame that
ends inside its tonal block among them); random blocks.
PCM: the restatement's steps 1-2, then the REFERENCE's TAt3pMIDCT::Do, the rescale, the REFERENCE's ff_atrac3p_generate_tones
(step 4b), at3pref_ipqf and the clamp (at3p_tonal_lib.ref_tonal_back_half). Stored as SHA-256 digests of the bit patterns, with
the reference's own tone tables (written out by the driver that runs ff_atrac3p_generate_tones). Run where oracle/_ref and the reference sources exist."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from at3_testlib import at3p_specs, pin_digest   # noqa: E402
from at3p_decode_lib import make_frame   # noqa: E402
import at3p_tonal_lib as L   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "at3p_tonal.npz")
SEQS = []   # (channels, blocks) of every seq() case, written again by the reference's writer


def band(waves=(), start=None, stop=None):
    return {"start": start, "stop": stop, "waves": list(waves)}


def block(nb, bands, shared=None, leader=False):
    return {"nb": nb, "shared": shared or [False] * nb, "leader": leader, "bands": bands}


def plain(C, nb, waves_of, start=None, stop=None):
    return block(nb, [[band(waves_of(ch, i), start, stop) for i in range(nb)] for ch in range(C)])


def silent_frame(C, seed):
    nq = 6
    return make_frame(C, nqu=nq, wl=[[3] * nq for _ in range(C)], sf=[[20 + q for q in range(nq)] for _ in range(C)],
                      mant=lambda ch, qu, k: ((k * 3 + qu + ch + seed) % 3) - 1)


def seq(C, blocks, seed=0):
    """frames: a block per entry (None = a frame without a tonal block)"""
    SEQS.append((C, blocks))
    out = []
    for i, b in enumerate(blocks):
        base = silent_frame(C, seed + i)
        out.append(base if b is None else L.splice_tonal(base, L.tonal_bits(C, b)))
    return np.stack(out)


def cases():
    out = []
    for C in (1, 2):
        one = plain(C, 1, lambda ch, i: [(37 + 5 * ch, 24, 3)])
        few = plain(C, 4, lambda ch, i: [(20 * i + 3 + ch, 18 + i, 7 * i % 32), (300 + 11 * i, 20, 1)])
        full = plain(C, 16, lambda ch, i: [(600 + 7 * i + ch, 16 + (i % 8), i % 32)] if (i + ch) % 3 else [])
        out.append((f"bands1_{C}ch", C, seq(C, [None, one, one, one, None, None])))
        out.append((f"bands4_{C}ch", C, seq(C, [few, few, None, few, few, few])))
        out.append((f"bands16_{C}ch", C, seq(C, [full, full, full, None, full])))
        # envelope points: 0, 31, start < stop, start == stop, start > stop, across frames
        envs = [plain(C, 3, lambda ch, i: [(100 + 40 * i, 22, 5 + i)], start=s, stop=e)
                for s, e in ((0, None), (None, 31), (4, 20), (9, 9), (25, 6), (None, 0), (31, None))]
        out.append((f"envelopes_{C}ch", C, seq(C, envs + [None] + envs[::-1])))
        # frequency packing: ascending over 512 (short codes), descending, 0 and 1023; 15 waves in a band
        hi = plain(C, 2, lambda ch, i: [(f, 14 + j % 10, (3 * j) % 32) for j, f in
                                        enumerate([0, 511, 512, 700, 900, 1000, 1020, 1023] if i == 0 else [1, 2, 4, 8, 16, 900])])
        fifteen = plain(C, 1, lambda ch, i: [(60 * j + 7 + ch, 10 + j, j) for j in range(15)])
        out.append((f"freqs_{C}ch", C, seq(C, [hi, fifteen, hi, None, fifteen])))
        # 48 waves in a frame
        n48 = plain(C, 8 if C == 2 else 4, lambda ch, i: [(64 * j + 5 * i + ch, 12, (i + j) % 32)
                                                           for j in range(3 if C == 2 else 12)])
        out.append((f"waves48_{C}ch", C, seq(C, [n48, n48, None, n48])))
        if C == 2:
            for name, sh in (("none", [False] * 6), ("all", [True] * 6), ("mixed", [True, False, False, True, False, True])):
                for lead in (False, True):
                    b = block(6, [[band([(30 * i + 9 + 400 * ch, 20 + ch, i)], *((i, None) if ch else (None, 20 + i)))
                                   for i in range(6)] for ch in range(2)], sh, lead)
                    out.append((f"share_{name}_lead{int(lead)}", C, seq(C, [b, b, None, b])))
        # a tonal frame whose unit count drops to 28: a loud frame of the writer spliced when it fits
        loud = make_frame(C, nqu=28, wl=[[2] * 28 for _ in range(C)], sf=[[25] * 28 for _ in range(C)],
                          mant=lambda ch, qu, k: (k + qu) % 3 - 1)
        t28 = L.splice_tonal(loud, L.tonal_bits(C, few))
        assert t28 is not None
        out.append((f"nqu28_{C}ch", C, np.stack([t28, t28, silent_frame(C, 3)])))
        # crafted rejections
        kws = [dict(amp_mode=0), dict(nw_mode=1), dict(amp_sf_mode=1)]
        if C == 2:
            kws += [dict(leader_bits=[(1, 1), (1, 1), (1, 1)]), dict(invert=1), dict(env_copy=1), dict(delta=1)]
        crafted = [L.make_tonal_frame(C, few, seed=k, **kw) for k, kw in enumerate(kws)]
        over = plain(C, 4, lambda ch, i: [(64 * j + i, 12, j) for j in range(15 if C == 1 else 7)])   # 60 / 56 waves
        crafted.append(L.make_tonal_frame(C, over))
        base = silent_frame(C, 9)
        crafted.append(L.splice_tonal(base, L.tonal_bits(C, few), noise=1))
        crafted.append(L.splice_tonal(base, L.tonal_bits(C, few), term=1))
        cut = L.splice_tonal(base, L.tonal_bits(C, few))
        bits = np.unpackbits(cut)
        bits[L.tonal_flag_pos(base) + 12:] = 0
        crafted.append(np.packbits(bits))                                                 # ends inside the block: no terminator
        # a long frame whose tonal block runs past the 2048 bytes
        longf = LONG_FRAME[C]
        crafted.append(L.splice_tonal(longf, L.tonal_bits(C, n48), cut=True))
        out.append((f"crafted_{C}ch", C, np.stack(crafted + [seq(C, [one])[0]])))
        rng = np.random.default_rng(300 + C)
        rnd = []
        for i in range(12):
            b = L.random_block(rng, C) if rng.random() < 0.8 else None
            if b is not None:
                for row in b["bands"]:
                    for bd in row:
                        bd["waves"] = [(f, int(rng.integers(0, 36)), p) for f, _, p in bd["waves"]]
            rnd.append(b)
        out.append((f"random_{C}ch", C, seq(C, rnd, seed=50)))
    return out


LONG_FRAME = {1: 0, 2: 0}


def long_frame(C, block_bits):
    """a full-scale frame whose tonal flag leaves fewer bits than a tonal block of block_bits needs"""
    for q in range(32, 0, -1):
        for cap in range(31, 0, -1):   # the largest mantissa magnitude
            f = make_frame(C, nqu=q, wl=[[7] * q for _ in range(C)], sf=[[50] * q for _ in range(C)],
                           mant=lambda ch, qu, k: min(24 + (k * 7 + qu) % 8, cap) * (1 if k % 2 else -1))
            if np.unpackbits(f)[-8:].sum() == 0 and 2048 * 8 - block_bits < L.tonal_flag_pos(f) < 2048 * 8 - 64:
                return f
    raise AssertionError(C)


def ref_cases():
    """every seq() case again, its frames written by the reference's writer over the spectra of a test signal"""
    out = []
    for i, (C, blocks) in enumerate(list(SEQS)):
        specs = at3p_specs("mix", len(blocks), C, scale=0.5)
        out.append((f"refw{i:02d}_{C}ch", C, L.ref_write_tonal(specs, blocks), blocks))
    return out


def main():
    for C in (1, 2):
        big = plain(C, 8 if C == 2 else 4, lambda ch, i: [(64 * j + 5 * i + ch, 12, (i + j) % 32) for j in range(3 if C == 2 else 12)])
        LONG_FRAME[C] = long_frame(C, sum(n for _, n in L.tonal_bits(C, big)))
    store, names = {}, []
    plain_cases = cases()
    for name, C, frames, blocks in [c + (None,) for c in plain_cases] + ref_cases():
        if blocks is not None:
            store[f"{name}_blocks"] = np.array(json.dumps(blocks))
        pcm, rej = L.ref_tonal_back_half(frames, C)
        cpu, crej = L.cpu_tonal_decode(frames, C)
        assert np.array_equal(cpu.view(np.uint32), pcm.view(np.uint32)) and np.array_equal(crej, rej), name
        _, rej_off = L.cpu_tonal_decode(frames, C, tones=False)
        names.append(name)
        store[f"{name}_channels"] = np.int32(C)
        store[f"{name}_frames"] = np.ascontiguousarray(frames, np.uint8)
        store[f"{name}_pcm_sha256"] = pin_digest(pcm)
        store[f"{name}_rejected"] = rej
        store[f"{name}_rejected_off"] = rej_off
        print(f"{name}: {frames.shape[0]} frames, rejected {rej.tolist()}, without the flag {rej_off.tolist()}, "
              f"peak {float(np.abs(pcm).max()):.3f}")
    store["cases"] = np.array(names)
    s, h, a = L.ref_tone_tables()
    s2, h2, a2 = L.tone_tables()
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in ((s, s2), (h, h2), (a, a2)))
    store["host_sine"], store["host_hann"], store["host_amp_sf"] = s, h, a
    store["meta"] = np.array(["frames: reference TAt3PBitStream::WriteFrame (refw_*) / restated tonal writer spliced into make_frame "
                              "frames; pcm: restatement steps 1-2, reference "
                              "TAt3pMIDCT::Do + rescale + ff_atrac3p_generate_tones + at3pref_ipqf + clamp "
                              "(tools/gen_golden_at3p_tonal.py)"])
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
