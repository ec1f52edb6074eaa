#!/usr/bin/env python3
"""Writes tests/golden/at3p_psy.npz from the restatement tests/host/at3p_psy_cpu.c (include/at3phip.h, MASKING-WEIGHTED WORD LENGTHS): per
case of tests/at3p_psy_lib.py's PSY_GOLDEN_CASES (`noise`, `tones` and `mix`, mono and stereo, 376 and 2048 bytes, 3 frames) the frames, the
choices (j*, k*, N, which allocation the guard wrote, O), the offsets, the word lengths and both Tw. tests/test_at3p_psy_cpu.py holds the
restatement to it: everything masking-weighted is pinned to the restatement, and this file pins the restatement."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import at3p_psy_lib as P

if __name__ == "__main__":
    out = {}
    for name, nch, fb in P.PSY_GOLDEN_CASES:
        e = P.psy_golden_entry(name, nch, fb)
        for k, v in e.items():
            out[f"{name}_{nch}_{fb}_{k}"] = v
        print(name, nch, fb, e["choice"].tolist())
    np.savez_compressed(P.PSY_GOLDEN, **out)
    print("wrote", P.PSY_GOLDEN, os.path.getsize(P.PSY_GOLDEN), "bytes")
