#!/usr/bin/env python3
"""Writes tests/golden/at3p_rd.npz or, with --mode psy, tests/golden/at3p_psy.npz from the restatement tests/host/at3p_rd_cpu.c
(include/at3phip.h, RATE-DISTORTION WORD LENGTHS and MASKING-WEIGHTED WORD LENGTHS): per case of tests/at3p_writer_lib.py's
RD_GOLDEN_CASES or tests/at3p_psy_lib.py's PSY_GOLDEN_CASES (`noise`, `tones` and `mix`, mono and stereo, 376 and 2048 bytes, 3 frames)
the frames, the choices (j*, k*, N, which allocation the guard wrote, and for psy O), for psy the offsets, the word lengths and both T or
Tw. tests/test_at3p_rd_cpu.py and tests/test_at3p_psy_cpu.py hold the restatement to them: everything rate-distortion and masking-weighted
is pinned to the restatement, and these files pin the restatement.

    gen_golden_at3p_rd.py [--mode rd|psy]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import at3p_psy_lib as Y
import at3p_writer_lib as W

MODES = {"rd": (W.RD_GOLDEN_CASES, W.rd_golden_entry, W.RD_GOLDEN), "psy": (Y.PSY_GOLDEN_CASES, Y.psy_golden_entry, Y.PSY_GOLDEN)}

if __name__ == "__main__":
    cases, entry, path = MODES[sys.argv[sys.argv.index("--mode") + 1] if "--mode" in sys.argv else "rd"]
    out = {}
    for name, nch, fb in cases:
        e = entry(name, nch, fb)
        for k, v in e.items():
            out[f"{name}_{nch}_{fb}_{k}"] = v
        print(name, nch, fb, e["choice"].tolist())
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
