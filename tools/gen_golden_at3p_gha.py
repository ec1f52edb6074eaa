#!/usr/bin/env python3
"""Writes tests/golden/at3p_gha.npz: the records the C restatement of the tone analysis (tests/host/at3p_gha_cpu.c) finds for the
test signals, and SHA-256 digests of its residuals and of the frames its mono pipeline writes, and the analysis' tables (twiddles, thresholds, normalisers). The signals are regenerated from
their names (tests/at3_testlib.py), so the file holds no PCM. Needs no GPU and no reference build.

With the argument `flags` it writes tests/golden/at3p_gha_flags.npz instead: SHA-256 digests of the restatement's records and
residuals for the crafted inputs of at3p_gha_lib.flag_digest_cases under the analysis flags. The committed file was written when
the restatement was still three files layered on each other (the unflagged, the gated and the shared one, each with its own entry
point, named by the keys' prefixes), from those entry points; the one file that replaced them reproduces it."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import at3p_gha_lib as G

FRAMES = 14
SIGNALS = ("tones", "burst", "stress", "mix", "noise")


def write_flags():
    out = {key: np.array(G.digests(*G.CpuToneAnalyser(bands.shape[1], fl & G.GATED, fl & G.SHARED).analyse(bands))) for key, bands, fl in G.flag_digest_cases()}
    path = os.path.join(ROOT, "tests", "golden", "at3p_gha_flags.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", len(out), "digest pairs")


def main():
    out = {"frames": np.int32(FRAMES)}
    t = G.find_tables()   # the analysis' own tables (the sine, window and amplitude tables are the decoder's: tests/golden/at3p_tonal.npz)
    for k in ("tw", "thr", "rs", "rc"):
        out["table_" + k] = np.ascontiguousarray(t[k])
    for name in SIGNALS:
        for nch in (1, 2):
            pcm = G.signal_pcm(name, FRAMES, nch)
            blocks, resid = G.CpuToneAnalyser(nch).analyse(G.pqf_bands(pcm))
            key = f"{name}_{nch}"
            out[key + "_blocks"] = blocks.view(np.uint8).reshape(FRAMES, -1)
            out[key + "_resid_sha256"] = np.array(hashlib.sha256(resid.tobytes()).hexdigest())
            if nch == 1:
                out[key + "_frames_sha256"] = np.array(hashlib.sha256(G.pipeline(pcm)[0].tobytes()).hexdigest())
            print(key, "waves per frame", [G.n_waves(b) for b in blocks])
    path = os.path.join(ROOT, "tests", "golden", "at3p_gha.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    write_flags() if sys.argv[1:] == ["flags"] else main()
