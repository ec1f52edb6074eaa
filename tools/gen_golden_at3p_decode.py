#!/usr/bin/env python3
"""Write tests/golden/at3p_decode.npz: frames and the PCM the ATRAC3plus decoder of include/at3phip.h must give for them.

Frames: the REFERENCE's frame writer (at3pref_write_frames, TAt3PBitStream::WriteFrame) over the residual spectra of every test
signal, mono and stereo, and over loud white spectra that force the quant-unit count below 32; four window patterns (all sine,
all steep, mixed per band, steep and sine alternating frame by frame, the last pinning the (n-1, n) window pairing) and loud
frames with mixed windows (pinning the window section's 16 bits when the unit count is below 32); crafted frames (every rejection
reason, group flag 0, full-table flag 0, the word-length-0 decision, clamped output) and random bytes.
PCM: the restatement's steps 1-2 (tests/host/at3p_decode_cpu.c), then the REFERENCE's TAt3pMIDCT::Do and ff_atrac3p_ipqf with
the definition's rescale and clamp (at3p_decode_lib.ref_back_half). Stored as SHA-256 digests of the bit patterns; full PCM for
the random cases only. Run where oracle/_ref and the reference sources exist."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from at3_testlib import at3p_specs, at3p_write_frames, pin_digest   # noqa: E402
from at3p_decode_lib import SIGNAL_NAMES, crafted_frames, host_tables, ref_back_half, specs_with_windows   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "at3p_decode.npz")
NF = 6


def window_patterns(nf, nch):
    pats = {"sine": np.zeros((nf, nch), np.uint16), "steep": np.full((nf, nch), 0xFFFF, np.uint16)}
    mixed = np.zeros((nf, nch), np.uint16)
    mixed[:, 0] = 0x5A3C
    if nch == 2:
        mixed[:, 1] = 0x0FF0
    pats["mixed"] = mixed
    alt = np.zeros((nf, nch), np.uint16)
    alt[1::2] = 0xFFFF
    pats["alternating"] = alt
    return pats


def loud_specs(nf, nch, seed, level):
    rng = np.random.RandomState(seed)
    return (level * rng.standard_normal((nf, nch, 2048))).astype(np.float32)


def cases():
    """(name, channels, frames, store full pcm)"""
    out = []
    for nch in (1, 2):
        for name in SIGNAL_NAMES:
            out.append((f"sig_{name}_{nch}ch", nch, at3p_write_frames(at3p_specs(name, NF, nch), which="ref"), False))
        out.append((f"loud_{nch}ch", nch, at3p_write_frames(loud_specs(4, nch, 11 + nch, 0.5), which="ref"), False))
        for pat, fl in window_patterns(NF, nch).items():
            sp = specs_with_windows("mix", NF, nch, fl)
            out.append((f"win_{pat}_{nch}ch", nch, at3p_write_frames(sp, fl, which="ref"), False))
        fl = window_patterns(4, nch)["mixed"]
        fl[1::2] = 0x3C5A
        out.append((f"win_mixed_loud_{nch}ch", nch, at3p_write_frames(loud_specs(4, nch, 21 + nch, 0.5), fl, which="ref"), False))
        frames, _ = crafted_frames(nch, seed=100 + nch)
        out.append((f"crafted_{nch}ch", nch, frames, False))
        rng = np.random.default_rng(200 + nch)
        rnd = rng.integers(0, 256, (4, 2048), dtype=np.uint8)
        rnd[:, 0] = (rnd[:, 0] & 0x1F) | ((nch - 1) << 5)   # a valid header in front of random bits
        out.append((f"random_{nch}ch", nch, rnd, True))
    return out


def main():
    store = {}
    names = []
    for name, nch, frames, full in cases():
        pcm, rej, fl = ref_back_half(frames, nch)
        names.append(name)
        store[f"{name}_channels"] = np.int32(nch)
        store[f"{name}_frames"] = np.ascontiguousarray(frames, np.uint8)
        store[f"{name}_pcm_sha256"] = pin_digest(pcm)
        store[f"{name}_rejected"] = rej
        store[f"{name}_n_qu"] = fl["n_qu"].astype(np.int32)
        if full:
            store[f"{name}_pcm"] = pcm
        print(f"{name}: {frames.shape[0]} frames, quant units {sorted(set(fl['n_qu'].tolist()))}, rejected {rej.tolist()}")
    store["cases"] = np.array(names)
    cos16, sine128, sine64 = host_tables()   # this host's libm: the tables every decoder must reproduce bit for bit
    store["host_cos16"], store["host_sine128"], store["host_sine64"] = cos16, sine128, sine64
    store["meta"] = np.array(["frames: reference writer (at3pref_write_frames) / crafted / random; pcm: restatement steps 1-2, "
                              "reference TAt3pMIDCT::Do + rescale + at3pref_ipqf + clamp (tools/gen_golden_at3p_decode.py)"])
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
