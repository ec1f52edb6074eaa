#!/usr/bin/env python3
"""Writes tests/golden/at3p_rd_fold.npz: the labels and SHA-256 digests of tests/at3p_psy_lib.py's rd_fold_entries - on 2000 random
tables in hundreds and on the signals' cells, what the restatement and the two host allocators give with rate-distortion and with
masking-weighted word lengths, field by field. The committed file was written at the last commit that had the two as separate stacks
(host_allocate_rd and host_allocate_psy, at3p_rd_cpu.c and at3p_psy_cpu.c), from their entry points (has that
script); this tool makes the same arrays from the code they were folded into, and with --check compares them with the file instead of
writing it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import at3p_psy_lib as Y

if __name__ == "__main__":
    out = Y.rd_fold_file_arrays()
    if "--check" in sys.argv[1:]:
        gold = np.load(Y.RD_FOLD_GOLDEN)
        assert sorted(gold.files) == sorted(out) and all(np.array_equal(gold[k], out[k]) for k in out), "the arrays differ from the file's"
        print("equal to", Y.RD_FOLD_GOLDEN, {k: v.shape for k, v in out.items()})
    else:
        np.savez_compressed(Y.RD_FOLD_GOLDEN, **out)
        print("wrote", Y.RD_FOLD_GOLDEN, os.path.getsize(Y.RD_FOLD_GOLDEN), "bytes")
