#!/usr/bin/env python3
"""Writes tests/golden/at3p_alloc.npz from the restatement tests/host/at3p_alloc_cpu.c (include/at3phip.h, ADAPTIVE WORD
LENGTHS): per case of tests/at3p_alloc_lib.py's GOLDEN_CASES the choices (t*, k*, N) per frame and the SHA-256 of the frames."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import at3p_alloc_lib as L

if __name__ == "__main__":
    out = {}
    for name, nch in L.GOLDEN_CASES:
        choice, digest = L.golden_entry(name, nch)
        out[f"{name}_{nch}_choice"], out[f"{name}_{nch}_sha256"] = choice, np.array(digest)
        print(name, nch, choice.tolist(), digest[:16])
    np.savez_compressed(L.GOLDEN, **out)
    print("wrote", L.GOLDEN, os.path.getsize(L.GOLDEN), "bytes")
