"""The look-ahead limiter's kernel SOURCES (atracdenc_amd/csrc/loudness_limit.hpp: k_limit_detect, k_limit_gain, k_limit_carry,
k_limit_init), compiled for the host and run lane by lane through the SIMT harness of tools/emu: samples and statistics
bit-equal to the C restatement tests/host/limiter_cpu.c, mono and stereo, both detectors, one call, the cuts of
limiter_lib.cuts_for and 16-bit input. As tests/test_loudness_simt_harness.py does for the meter, the cases also run with guard
pages around every device allocation (EMU_FENCE=high / low; caller-owned buffers of exact size among them) and with the
wavefronts of a workgroup in descending order (EMU_ORDER=reverse: k_limit_gain's doubling and prefix sums hand values between
wavefronts behind barriers). Every case is a case of tools/emu/run_emu_limiter.py, run in a child process."""
import os

import pytest

from simt_harness_lib import CLANG, Children, assert_clean, build_strict

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")

CASES = {"parity:1:0": 3, "parity:1:1": 3, "parity:2:0": 3, "parity:2:1": 3, "edges": 2}   # comparisons per case
ENV = {"default": {}, "high": {"EMU_FENCE": "high"}, "low": {"EMU_FENCE": "low"}, "reverse": {"EMU_ORDER": "reverse"}}
# tests/float_domain_lib.py's streams: NaN, infinities, +-FLT_MAX, overflow, subnormals; 3 ceilings x 2 detectors x 2 call patterns
DOMAIN = {"domain:1": 12, "domain:2": 12}
JOBS = [(m, c) for c in DOMAIN for m in ("high", "reverse")] + [(m, c) for c in CASES for m in ENV]
CASES_ALL = dict(CASES, **DOMAIN)


@pytest.fixture(scope="module")
def children():
    build_strict()
    c = Children({job: ("run_emu_limiter.py", ["--nobuild", job[1]], ENV[job[0]]) for job in JOBS})
    yield c
    c.close()


def check(children, mode, case):
    out = children.output((mode, case))
    assert f"\n{case} done" in out, out[-4000:]
    assert_clean(out, CASES_ALL[case])


@pytest.mark.parametrize("case", list(CASES))
def test_bit_identical_to_restatement(children, case):
    """parity:C:TP: limiter_lib.batch() in one call, in cuts (an empty call, calls of 1 and 71 samples, both sides of a tile
    edge) and from 16-bit input. edges: exact-size device buffers for input, output and flush."""
    check(children, "default", case)


@pytest.mark.parametrize("fence", ["high", "low"])
@pytest.mark.parametrize("case", list(CASES))
def test_guard_pages(children, fence, case):
    check(children, fence, case)


@pytest.mark.parametrize("case", list(CASES))
def test_reversed_wavefront_order(children, case):
    check(children, "reverse", case)


@pytest.mark.parametrize("mode", ["high", "reverse"])
@pytest.mark.parametrize("case", list(DOMAIN))
def test_float_domain(children, mode, case):
    """domain:C: one stream per pattern of tests/float_domain_lib.py and per gain side by side (float_domain_lib.LIMITER_PAIRS:
    gains 0, 2, FLT_MAX and the smallest subnormal at -1 dBFS; gain 2 under the smallest subnormal and under FLT_MAX as the
    ceiling), both detectors, one call and three: samples (floats as bit patterns, a NaN against a NaN) and statistics against
    the restatement of each stream alone."""
    check(children, mode, case)
