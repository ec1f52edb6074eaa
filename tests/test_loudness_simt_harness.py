"""The loudness meter's kernel SOURCES (atracdenc_amd/csrc/loudness.hip: k_hops, k_carry, k_true_peak, k_scale), compiled for
the host and run lane by lane through the SIMT harness of tools/emu: hop sums, every field of the results (peaks included) and
scaled samples bit-equal to the C restatement tests/host/loudness_cpu.c, for mono and stereo, one call, random cuts and a
reset() mid-stream. As tests/test_decoders_simt_harness.py does for the decoders, the cases also run with guard pages around
every device allocation (EMU_FENCE=high / low; caller-owned buffers of exact size among them) and with the wavefronts of a
workgroup in descending order (EMU_ORDER=reverse: k_hops hands tiles from its staging wavefronts to its computing wavefront
behind one barrier per tile). Every case is a case of tools/emu/run_emu_loudness.py, run in a child process."""
import os

import pytest

from simt_harness_lib import CLANG, Children, assert_clean, build_strict

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")

CASES = {"meter:1": 8, "meter:2": 8, "edges": 7, "scale": 1}   # comparisons per case
ENV = {"default": {}, "high": {"EMU_FENCE": "high"}, "low": {"EMU_FENCE": "low"}, "reverse": {"EMU_ORDER": "reverse"}}
DOMAIN = {"domain:1": 6, "domain:2": 6}   # tests/float_domain_lib.py's streams: NaN, infinities, +-FLT_MAX, overflow, subnormals
JOBS = [(m, c) for c in DOMAIN for m in ("high", "reverse")] + [(m, c) for c in CASES for m in ENV]
CASES_ALL = dict(CASES, **DOMAIN)


@pytest.fixture(scope="module")
def children():
    build_strict()
    c = Children({job: ("run_emu_loudness.py", ["--nobuild", job[1]], ENV[job[0]]) for job in JOBS})
    yield c
    c.close()


def check(children, mode, case):
    out = children.output((mode, case))
    assert f"\n{case} done" in out, out[-4000:]
    assert_clean(out, CASES_ALL[case])


@pytest.mark.parametrize("case", list(CASES))
def test_bit_identical_to_restatement(children, case):
    """meter:C: the five signal kinds side by side, 7 hops and a partial one, true peak on: one call, random cuts (hop
    boundaries among them), reset() mid-stream; then without true peak. edges: exact-size device input, calls shorter than the
    converter's filter, empty calls, a stream shorter than a hop, an empty finish, 23 mono streams (a second, partly filled
    workgroup of k_hops). scale: apply against numpy's float32 multiply, host and device buffers, in place."""
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
    """domain:C: one stream per pattern of tests/float_domain_lib.py side by side, 1.2 s each, true peak on, one call and three:
    hop sums, every field of the results and apply's samples against the restatement of each stream alone (floats as bit
    patterns, a NaN against a NaN), with a guard page after every buffer, and in reversed wavefront order."""
    check(children, mode, case)
