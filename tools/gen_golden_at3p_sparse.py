#!/usr/bin/env python3
"""Writes tests/golden/at3p_sparse.npz from the restatement tests/host/at3p_writer_cpu.c (include/at3phip.h, SPARSE WORD LENGTHS): per
case of tests/at3p_writer_lib.py's SPARSE_GOLDEN_CASES (`noise` and `tones`, mono and stereo, 376 and 2048 bytes, 3 frames) the frames, the
choices (t*, k*, N), the word lengths and the SHA-256 of the sparse decoder's PCM. tests/test_at3p_sparse_cpu.py holds the
restatement to it: everything sparse is pinned to the restatement, and this file pins the restatement."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import at3p_writer_lib as W

if __name__ == "__main__":
    out = {}
    for name, nch, fb in W.SPARSE_GOLDEN_CASES:
        e = W.sparse_golden_entry(name, nch, fb)
        for k, v in e.items():
            out[f"{name}_{nch}_{fb}_{k}"] = v
        print(name, nch, fb, e["choice"].tolist())
    np.savez_compressed(W.SPARSE_GOLDEN, **out)
    print("wrote", W.SPARSE_GOLDEN, os.path.getsize(W.SPARSE_GOLDEN), "bytes")
