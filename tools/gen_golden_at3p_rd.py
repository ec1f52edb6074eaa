#!/usr/bin/env python3
"""Writes tests/golden/at3p_rd.npz from the restatement tests/host/at3p_rd_cpu.c (include/at3phip.h, RATE-DISTORTION WORD LENGTHS): per
case of tests/at3p_writer_lib.py's RD_GOLDEN_CASES (`noise`, `tones` and `mix`, mono and stereo, 376 and 2048 bytes, 3 frames) the frames, the
choices (j*, k*, N, which allocation the guard wrote), the word lengths and both T. tests/test_at3p_rd_cpu.py holds the restatement
to it: everything rate-distortion is pinned to the restatement, and this file pins the restatement."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import at3p_writer_lib as W

if __name__ == "__main__":
    out = {}
    for name, nch, fb in W.RD_GOLDEN_CASES:
        e = W.rd_golden_entry(name, nch, fb)
        for k, v in e.items():
            out[f"{name}_{nch}_{fb}_{k}"] = v
        print(name, nch, fb, e["choice"].tolist())
    np.savez_compressed(W.RD_GOLDEN, **out)
    print("wrote", W.RD_GOLDEN, os.path.getsize(W.RD_GOLDEN), "bytes")
