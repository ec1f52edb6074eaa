"""The 16-bit instantiations of the kernels that first touch PCM (ATRAC1's front, ATRAC3plus's filter bank, the resampler's
convolution, the meter's hop, carry, peak and scale kernels: SOURCES compiled for the host), run lane by lane through the SIMT
harness of tools/emu and compared bit for bit with the float instantiations on the widened input ((float)s * 0x1p-15f): ATRAC1
at 2 streams x 2 blocks, ATRAC3plus at 1 x 2 frames, the resampler at 48000 -> 44100 with 300 samples, the meter at 2 hops + 7
samples, mono and stereo, the two kinds of call alternating on one context. The cases also run with guard pages around every
device allocation (EMU_FENCE=high / low): caller-owned buffers hold exactly the 16-bit input, rows of odd length and rows that
are only 2-byte aligned among them, so a sample-pair load that reaches past a row's end or before its start is a fault. Every
case is a case of tools/emu/run_emu_s16.py, run in a child process."""
import os

import pytest

from simt_harness_lib import CLANG, Children, assert_clean, build_strict

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")

CASES = {"at1:1": 3, "at1:2": 3, "at3p:1": 2, "at3p:2": 2, "resample:1": 3, "resample:2": 3, "loudness:1": 5, "loudness:2": 5}   # comparisons per case
ENV = {"default": {}, "high": {"EMU_FENCE": "high"}, "low": {"EMU_FENCE": "low"}}
JOBS = [(m, c) for c in CASES for m in ENV]


@pytest.fixture(scope="module")
def children():
    build_strict()
    c = Children({job: ("run_emu_s16.py", ["--nobuild", job[1]], ENV[job[0]]) for job in JOBS})
    yield c
    c.close()


def check(children, mode, case):
    out = children.output((mode, case))
    assert f"\n{case} done" in out, out[-4000:]
    assert_clean(out, CASES[case])


@pytest.mark.parametrize("case", list(CASES))
def test_s16_bit_identical_to_float_on_widened_input(children, case):
    check(children, "default", case)


@pytest.mark.parametrize("fence", ["high", "low"])
@pytest.mark.parametrize("case", list(CASES))
def test_s16_guard_pages(children, fence, case):
    check(children, fence, case)
