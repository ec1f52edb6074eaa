"""The SIMT harness's deferred-stream mode (EMU_STREAMS, tools/emu/hip/hip_runtime.h) can fail, and fails only where a wait is
missing: tests/host/emu_streams_selftest.cpp, a stand-alone toy program without product code, runs each ordering pattern in an
unguarded and a guarded form. Eagerly (EMU_STREAMS unset) every operation runs at its call, in program order. Under `lazy`
and under two seeds every unguarded form must give another result than it gives eagerly, and every guarded form the same.
tests/test_stream_order_simt_harness.py relies on this when it reads a clean run of the product's pipelines as "no wait is
missing". The program is built under -fsanitize=address,undefined with the runtimes linked statically and run as a child
process; nothing sanitized is loaded into Python."""
import os
import subprocess

import pytest

from simt_harness_lib import CLANG, ROOT

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the harness for the host")

EMU = os.path.join(ROOT, "tools", "emu")
MODES = ["lazy", "lazy:1", "lazy:2"]
UNGUARDED = ["producer_consumer", "two_slots", "host_source", "blocking_copy_nonblocking_stream"]
GUARDED = ["producer_consumer", "two_slots", "host_source", "pageable_d2h_complete_at_return_1", "pageable_d2h_complete_at_return_2", "wait_before_rerecord_first",
           "wait_before_rerecord_second", "blocking_copy_blocking_stream", "blocking_copy_after_sync", "arguments_by_value"]


def run(exe, mode, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=%d:abort_on_error=0" % (not args), UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in ("EMU_TRACE", "EMU_FENCE", "EMU_ORDER", "EMU_STRICT", "EMU_STREAMS", "EMU_STREAMS_LOG"):
        env.pop(k, None)
    if mode:
        env["EMU_STREAMS"] = mode
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu_streams") / "emu_streams_selftest")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libsan", "-I", EMU, "-x", "c++", os.path.join(ROOT, "tests", "host", "emu_streams_selftest.cpp"),
                           os.path.join(EMU, "emu_runtime.cpp"), "-o", exe, "-ldl", "-lpthread"])
    out = {"exe": exe}
    for mode in [""] + MODES:
        r = run(exe, mode)
        assert "SELFTEST DONE" in r.stdout and "still holds" not in r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
        lines = [ln.split() for ln in r.stdout.splitlines() if len(ln.split()) == 3]
        out[mode] = {(name, form): value for name, form, value in lines}
        assert len(out[mode]) == len(lines)   # no (name, form) twice with two values
    return out


def test_program_order_gives_the_same_result_in_both_forms(results):
    """eagerly the unguarded form of a pattern computes what the guarded form does: the forms differ in their waits alone"""
    for name in ("producer_consumer", "two_slots"):
        assert results[""][name, "unguarded"] == results[""][name, "guarded"]
    assert results[""]["host_source", "unguarded"] == results[""]["host_source", "guarded"]
    assert results[""]["blocking_copy_nonblocking_stream", "unguarded"] == results[""]["blocking_copy_blocking_stream", "guarded"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", UNGUARDED)
def test_unguarded_pattern_differs_from_program_order(results, mode, name):
    assert results[mode][name, "unguarded"] != results[""][name, "unguarded"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", GUARDED)
def test_guarded_pattern_equals_program_order(results, mode, name):
    assert results[mode][name, "guarded"] == results[""][name, "guarded"]


def test_lazy_runs_no_more_than_a_wait_needs(results):
    """after the wait for the event's first record, the second fill, the second record and the record of the other event are
    still queued on the producer's stream under `lazy`; eagerly nothing ever is"""
    assert results[""]["wait_before_rerecord_left_on_a", "count"] == "0"
    assert results["lazy"]["wait_before_rerecord_left_on_a", "count"] == "3"
    for mode in MODES[1:]:
        assert 0 <= int(results[mode]["wait_before_rerecord_left_on_a", "count"]) <= 3


def test_operations_left_at_exit_are_reported(results):
    r = run(results["exe"], "lazy", "--leave-queued")
    assert "left queued 1" in r.stdout
    assert "at exit stream s0 still holds 1 operations, the first one: launch k_fill" in r.stderr
    r = run(results["exe"], "", "--leave-queued")
    assert "left queued 0" in r.stdout and "still holds" not in r.stderr


def test_unknown_mode_is_refused(results):
    env = dict(os.environ, EMU_STREAMS="eager")
    r = subprocess.run([results["exe"]], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode != 0 and "EMU_STREAMS must be lazy or lazy:SEED" in r.stderr
