#!/usr/bin/env python3
"""Writes tests/golden/at3p_alloc.npz from the restatement tests/host/at3p_writer_cpu.c (include/at3phip.h, ADAPTIVE WORD
LENGTHS): per case of tests/at3p_writer_lib.py's ALLOC_GOLDEN_CASES the choices (t*, k*, N) per frame and the SHA-256 of the frames."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import at3p_writer_lib as W

if __name__ == "__main__":
    out = {}
    for name, nch in W.ALLOC_GOLDEN_CASES:
        choice, digest = W.alloc_golden_entry(name, nch)
        out[f"{name}_{nch}_choice"], out[f"{name}_{nch}_sha256"] = choice, np.array(digest)
        print(name, nch, choice.tolist(), digest[:16])
    np.savez_compressed(W.ALLOC_GOLDEN, **out)
    print("wrote", W.ALLOC_GOLDEN, os.path.getsize(W.ALLOC_GOLDEN), "bytes")
