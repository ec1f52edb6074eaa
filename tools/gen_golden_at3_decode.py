#!/usr/bin/env python3
"""Generate tests/golden/at3_decode.npz: the ATRAC3 decoder's goldens.

Frames come from the REAL reference encoder (ref_encode of oracle/_ref/libat3ref.so) - every signal of SIGNALS on all eight
container rows, stereo and mono, with and without gain control and tonal extraction - plus crafted units (every rejection
reason, tonal components at the spectrum's edge, seven gain points per band, full-scale spectra) and random bytes. The PCM is
the C restatement's steps 1-2 (tests/host/at3_decode_cpu.c: unpack, dequantise) followed by the REFERENCE's TAtrac3MDCT::Midct,
TGainProcessor::Demodulate and TQmf::Synthesis (steps 3-6), run by a driver compiled at generation time against the reference's
headers and oracle/_ref/libat3ref.so (tests/at3_decode_lib.py: ref_back_half).

Run where oracle/_ref and the reference sources exist:  python tools/gen_golden_at3_decode.py
Per case the fixture holds the frames, the reference encoder's tap fields of those frames (gain points, scale-factor indices,
tonal component lengths and scale factors: small ints), the rejected units per reason and the SHA-256 of the PCM's bit patterns
(at3_testlib.pin_digest); the PCM itself only for the random cases (mostly
rejected units), which keeps the fixture at about 300 KB (311 KB). No reference source is stored."""
import os
import platform
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from at3_decode_lib import ROWS, crafted_frames, have_ref_back_half, ref_back_half  # noqa: E402
from at3_testlib import ROOT, SIGNALS, pin_digest, ref  # noqa: E402

NBLOCKS = 4          # -> 3 frames per case
FULL_PCM = ("random_",)   # the rest by digest: float32 audio does not compress


def encoded_cases():
    """(name, bitrate, nch, no_gain, no_tonal) in a fixed order"""
    for br, fsz, js in ROWS:
        for sig in SIGNALS:
            yield f"{sig}_{fsz}_ch2", br, sig, 2, 0, 0
        for sig in ("mix", "burst"):
            yield f"{sig}_{fsz}_ch1", br, sig, 1, 0, 0
        yield f"burst_{fsz}_ch2_nogain", br, "burst", 2, 1, 0
        yield f"tones_{fsz}_ch2_notonal", br, "tones", 2, 0, 1


def tap_fields(taps):
    """the reference encoder's taps [N][nch] -> small-int arrays of both units (zeros for a missing second channel)"""
    n, nch = taps.shape
    out = dict(n_points=np.zeros((n, 2, 4), np.int8), level=np.zeros((n, 2, 4, 8), np.int8), loc=np.zeros((n, 2, 4, 8), np.int8),
               sfi=np.zeros((n, 2, 32), np.int8), n_tonal=np.zeros((n, 2), np.int16), tonal_len=np.zeros((n, 2, 64), np.int8),
               tonal_sfi=np.zeros((n, 2, 64), np.int8))
    for k in out:
        src = "tonal_sfi" if k == "tonal_sfi" else k
        out[k][:, :nch] = taps[src]
    return out


def cases():
    r = ref()
    for name, br, sig, nch, ng, nt in encoded_cases():
        fsz, js = next((f, j) for b, f, j in ROWS if b == br)
        pcm = SIGNALS[sig](NBLOCKS)[:, :, :nch]
        frames, taps = r.encode(pcm, br, ng, nt, taps=True)
        yield name, fsz, js, frames, tap_fields(taps)
    for br, fsz, js in ROWS:
        yield f"crafted_{fsz}", fsz, js, crafted_frames(fsz, js, seed=fsz), None
    for br, fsz, js in (ROWS[0], ROWS[3], ROWS[7]):
        yield f"random_{fsz}", fsz, js, np.random.default_rng(fsz + 1).integers(0, 256, (6, fsz), dtype=np.uint8), None


def main():
    if not have_ref_back_half():
        raise SystemExit("needs oracle/_ref/libat3ref.so (make -C oracle ref) and the reference sources")
    d = dict(meta=np.array(repr(dict(glibc=platform.libc_ver()[1], machine=platform.machine()))))
    names = []
    for name, fsz, js, frames, taps in cases():
        pcm, rejected, _ = ref_back_half(frames, fsz, js)
        d[f"{name}_frames"] = np.ascontiguousarray(frames, np.uint8)
        d[f"{name}_row"] = np.array([fsz, int(js)], np.int32)
        d[f"{name}_rejected"] = rejected
        d[f"{name}_pcm_sha256"] = pin_digest(pcm)
        if name.startswith(FULL_PCM):
            d[f"{name}_pcm"] = pcm
        if taps is not None:
            for k, v in taps.items():
                d[f"{name}_tap_{k}"] = v
        names.append(name)
    d["cases"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "at3_decode.npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
