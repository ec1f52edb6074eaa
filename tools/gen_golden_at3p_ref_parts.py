#!/usr/bin/env python3
"""Writes tests/golden/at3p_ref_parts.npz: adaptive and sparse ATRAC3plus frames written by the REFERENCE's part coders
(TWordLenEncoder, TSfIdxEncoder, TQuantUnitsEncoder, TTonalComponentEncoder) through the driver of tests/at3p_ref_parts_lib.py, under
the allocation (N, word lengths) the restatement tests/host/at3p_writer_cpu.c chooses. Runs only where the reference and
oracle/_ref/libat3ref.so are. Per cell of at3p_ref_parts_lib.cells() - mono at 176, 376 and 2048 bytes, stereo at 224, 376 and
2048, and one cell with tonal blocks and window flags per channel count, each adaptive and sparse; 3 streams x 4 frames - the file
holds the frames, N, the word lengths and the reference's bit count, and in one JSON string the cells' parameters and the SHA-256 of
their inputs, which the tests regenerate from the seeded builders. tests/test_at3p_ref_parts_cpu.py holds the three restatements to
the file and tests/test_at3p_ref_parts_gpu.py the GPU writers."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import at3p_ref_parts_lib as P

if __name__ == "__main__":
    if not P.have_ref():
        sys.exit("the reference's sources and oracle/_ref/libat3ref.so are needed")
    out = P.golden_build()
    for key, nch, fb, sparse, tonal in P.cells():
        print(key, "N", out[f"{key}_n"].reshape(-1).tolist())
    np.savez_compressed(P.GOLDEN, **out)
    print("wrote", P.GOLDEN, os.path.getsize(P.GOLDEN), "bytes")
