#!/usr/bin/env python3
"""Writes tests/golden/at3p_writer_fold.npz from the restatement tests/host/at3p_rd_cpu.c and the files it includes: per channel
count the labels and SHA-256 digests of tests/at3p_writer_lib.py's fold_entries - the cross-pin inputs written at 2048 bytes, 376
and the smallest size and decoded plain and with flipped bits, the crafted malformed frames, the first 100 random cost tables
allocated, and the sparse and rate-distortion special cases. The committed file was written at the last commit that had the six
restatements at3p_{decode,tonal,alloc,rate,sparse,rd}_cpu.c stating the writer and the decoder's unpack side by side, from their
entry points (has that script); this tool makes the same arrays from the one restatement they were folded
into, and with --check compares them with the file instead of writing it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import at3p_writer_lib as W

if __name__ == "__main__":
    out = W.fold_file_arrays()
    if "--check" in sys.argv[1:]:
        gold = np.load(W.FOLD_GOLDEN)
        assert sorted(gold.files) == sorted(out) and all(np.array_equal(gold[k], out[k]) for k in out), "the arrays differ from the file's"
        print("equal to", W.FOLD_GOLDEN, {k: v.shape for k, v in out.items()})
    else:
        np.savez_compressed(W.FOLD_GOLDEN, **out)
        print("wrote", W.FOLD_GOLDEN, os.path.getsize(W.FOLD_GOLDEN), "bytes")
