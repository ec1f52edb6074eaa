#!/usr/bin/env python3
"""Generate tests/golden/at1_decode.npz from the REAL reference's ATRAC1 decoder (TAtrac1Decoder of oracle/_ref/libat3ref.so,
built from the unmodified sources by `make -C oracle ref`), driven per 512-sample block through its lambda by a small program
that binds the library's exported symbols (tests/at1_decode_lib.py: ref_decode).

Run where oracle/_ref exists:  python tools/gen_golden_at1_decode.py
Per case the fixture holds the unit sequence the reference read (its AEA writer zeroes the first unit), the SHA-256 of the
reference's float PCM (bit patterns and shape, at3_testlib.pin_digest) and the 'Skipping invalid ATRAC1 frame' lines it printed
per reason. The float PCM itself is stored only for the malformed cases (FULL_PCM), where most samples clamp and it compresses:
four seconds of decoded audio as float32 do not, and the digest pins the other cases exactly as well. No reference source is
stored."""
import os
import platform
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from at1_decode_lib import crafted_units, random_modes, ref_decode, set_block_modes  # noqa: E402
from at3_testlib import ROOT, SIGNALS, at1_blocks, at1_ref_encode, have_ref, pcm_stress, pin_digest  # noqa: E402

NBLOCKS = 3          # ATRAC3-sized blocks -> 6 ATRAC1 sound units per channel
STRESS_BLOCKS = 8    # -> 16 sound units per channel
FULL_PCM = ("crafted_", "random_")


def cases():
    """(name, units [N][C][212]) in a fixed order"""
    gens = dict(SIGNALS)
    gens["stress"] = pcm_stress
    for name, gen in gens.items():
        pcm = gen(STRESS_BLOCKS if name == "stress" else NBLOCKS)
        for nch in (2, 1):
            blocks = at1_blocks(pcm, nch)
            for mode in ("auto", "short", "mask5", "auto_bfu3"):
                if name == "silence" and mode != "auto":
                    continue
                if nch == 1 and mode not in ("auto", "mask5"):
                    continue
                yield f"{name}_ch{nch}_{mode}", at1_ref_encode(blocks, mode)
    # reference-encoded units with the block-size fields rewritten: every long / short / two-block / four-block combination
    rng = np.random.default_rng(11)
    for nch in (2, 1):
        units = at1_ref_encode(at1_blocks(pcm_stress(STRESS_BLOCKS), nch), "auto")
        yield f"mixed_windows_ch{nch}", set_block_modes(units, random_modes(units.shape[:2], rng))
    for nch in (2, 1):
        yield f"crafted_ch{nch}", crafted_units(nch, seed=5 + nch)
    for nch, seed in ((2, 21), (1, 22)):
        r = np.random.default_rng(seed)
        yield f"random_ch{nch}", r.integers(0, 256, (24, nch, 212), dtype=np.uint8)


def main():
    if not have_ref():
        raise SystemExit("oracle/_ref/libat3ref.so missing: run `make -C oracle ref` where the reference sources exist")
    d = dict(meta=np.array(repr(dict(glibc=platform.libc_ver()[1], machine=platform.machine()))))
    names = []
    for name, units in cases():
        seq, pcm, reasons = ref_decode(np.ascontiguousarray(units))
        d[f"{name}_units"] = seq
        d[f"{name}_pcm_sha256"] = pin_digest(pcm)
        if name.startswith(FULL_PCM):
            d[f"{name}_pcm"] = pcm
        d[f"{name}_rejected"] = np.array([sum("block size" in r for r in reasons), sum("past the end" in r for r in reasons)], np.int64)
        assert len(reasons) == int(d[f"{name}_rejected"].sum()), reasons
        names.append(name)
    d["cases"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "at1_decode.npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
