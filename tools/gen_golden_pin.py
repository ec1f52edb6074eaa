#!/usr/bin/env python3
"""Generate tests/golden/pin.npz from the REAL reference (oracle/_ref/libat3ref.so, built from the unmodified
reference sources by `make -C oracle ref`): the outputs tests/test_pin_on_box.py compares the oracle with on the
machine that measures, which has no reference build of its own.

Run where the reference build exists:  python tools/gen_golden_pin.py
The fixture is data: digests of the regenerated PCM, the reference's frames, digests of its stage taps and the
inputs and outputs of its two libm-dependent stage functions; no reference source is stored."""
import os
import platform
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from at3_testlib import PIN_PATH, have_ref, pin_libm_inputs, pin_outputs, ref  # noqa: E402


def main():
    if not have_ref():
        raise SystemExit("oracle/_ref/libat3ref.so missing: run `make -C oracle ref` where the reference sources exist")
    flatness_in, log2f_in = pin_libm_inputs()
    d = pin_outputs(ref(), flatness_in, log2f_in)
    d.update(flatness_in=flatness_in, log2f_in=log2f_in,
             meta=np.array(repr(dict(glibc=platform.libc_ver()[1], machine=platform.machine(),
                                     fma="fma" in open("/proc/cpuinfo").read()))))
    np.savez_compressed(PIN_PATH, **d)
    print(PIN_PATH, os.path.getsize(PIN_PATH), "bytes,", len(d), "arrays")


if __name__ == "__main__":
    main()
