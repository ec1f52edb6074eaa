"""The HOST code of every engine (at3hip.hip, at1hip.hip, at3phip.hip, resample.hip, loudness.hip over at3_host_util.hpp and
at3_decoder_host.hpp) makes the runtime calls it made before it was put on the shared engine core and the shared host
staging: which call, in which order, on which stream, with which event, byte count and launch geometry, and which
allocations with how many bytes - each destroy releases exactly what was allocated. The sources are compiled for the host and run through the SIMT harness of tools/emu with its call
trace on (EMU_TRACE); tools/emu/run_emu_trace.py runs one fixed script of calls per case and compares the trace with
tests/golden/host_trace/<case>.txt, which were written from the sources of the commit before each change. How streams land on
the few hardware queues, and with that the pipelined rates, depends on the order they are created in; the overlap of
consecutive calls on which event is recorded and waited for where. The traces pin that graph as it is;
tests/test_stream_order_simt_harness.py tests that the graph suffices."""
import os
import re

import pytest

from simt_harness_lib import CLANG, Children, assert_clean, build_strict

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the host sources")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_trace")
CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".txt"))


@pytest.fixture(scope="module")
def children():
    build_strict()
    c = Children({case: ("run_emu_trace.py", ["--nobuild", case], {}) for case in CASES})
    yield c
    c.close()


def test_every_case_has_a_golden():
    """the ATRAC3 variants (LP2 / LP4, with and without gain control, one channel, the priming call), ATRAC1, ATRAC3plus; the
    three decoders, the resampler, the meter without and with the true peak, the limiter, the ATRAC3plus tone analysis and
    the ATRAC3 stage-level entry points (mdct, gain_energy_scale, the quant tap's early release)"""
    assert len(CASES) == 18, CASES


@pytest.mark.parametrize("case", CASES)
def test_same_calls_as_before(children, case):
    out = children.output(case)
    assert len(re.findall(r"bad \d+", out)) == 1, out[-4000:]
    assert_clean(out, 1)


@pytest.mark.parametrize("case,expected", [
    ("at3_lp2_gain", ["flags=1 priority=0", "flags=1 priority=-1", "flags=1 priority=-1", "flags=1 priority=default"]),
    ("at3_lp2_nogain", ["flags=1 priority=0", "flags=1 priority=-1", "flags=1 priority=default"])])
def test_at3hip_creates_its_streams_first_and_in_order(children, case, expected):
    """front stream at the low priority (0 of the harness's range 0 .. -1), back half high, light stage high (only with gain
    control), copy stream with default priority; all non-blocking (flags=1), all before the first event"""
    begins = re.search(rf"^{case}: begins with (.*); then (\w+)$", children.output(case), re.M)
    assert begins, children.output(case)[-4000:]
    assert [re.sub(r"stream_create s\d+ ", "", ln) for ln in begins.group(1).split("; ")] == expected
    assert begins.group(2) == "event_create"
