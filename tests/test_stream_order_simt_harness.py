"""Every engine's stream pipeline under legal schedules that are not program order: the SIMT harness's deferred-stream mode
(EMU_STREAMS, tools/emu/hip/hip_runtime.h). The harness otherwise executes every launch and copy at its call, so the GPU-less
suite passes whether a wait between two streams is present or not, and tests/test_host_call_trace.py pins the waits that exist,
not that they are enough. Here each stream is a queue; `lazy` runs nothing until the host waits and then the least that wait
needs, `lazy:SEED` lets a seeded scheduler run streams ahead of and behind each other. A hazard the product does not guard
shows as a result that differs from the oracle or the restatement in one of the modes; tests/test_emu_streams_selftest.py is
the proof that the mode shows such a hazard on toy programs.

Every case is a case of tools/emu/run_emu_streams.py (the engines through the public binding classes with lib_path= the
harness, one `bad N` line per comparison), run in child processes under EMU_STREAMS unset, lazy, lazy:1, lazy:2 and lazy:3:

  * ATRAC3 encoder, LP2 with gain control (three streams and the copy stream), LP2 without (the fused kernel), LP4 with: queued
    device calls of 3, 1, 1, 3, 1, 2 blocks; the host-buffer pipeline at depths 2 and 4 with inputs poisoned and outputs
    overwritten at the earliest legal moment (16-bit once); a caller's stream whose queued copy produces each call's PCM over a
    decoy; timing events in the queues once.
  * ATRAC3plus encoder: queued calls of 2, 1, 3, 1 frames, mono and stereo; the tonal path, gated and shared, across three
    queued calls; write_frames_tonal behind a queued call.
  * ATRAC1 encoder: queued calls of unequal size.
  * The three decoders (ATRAC3plus with tones), the resampler with its flush, the meter (process, finish; apply) and the limiter
    (limit_start, limit, limit_flush): a caller's stream with a queued producer over poison and a queued copy of the result, two
    queued host-memory calls that share the one staging slot, two queued device calls, reset() between the rounds.

The mode explores orders, not timing, and knows nothing of hardware queues; tests/test_stream_order_gpu.py is its counterpart
on the device."""
import os

import pytest

from simt_harness_lib import CLANG, Children, assert_clean, build_strict

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")

MODES = {"eager": {}, "lazy": {"EMU_STREAMS": "lazy"}, "lazy:1": {"EMU_STREAMS": "lazy:1"}, "lazy:2": {"EMU_STREAMS": "lazy:2"},
         "lazy:3": {"EMU_STREAMS": "lazy:3"}}
# case -> comparisons it prints
CASES = {"at3enc:lp2_gain": 6, "at3enc:lp2_nogain": 4, "at3enc:lp4_gain": 4, "at3penc:1": 1, "at3penc:2": 1, "at3penc_tonal": 3,
         "at1enc": 1, "dec_at1": 3, "dec_at3": 3, "dec_at3p": 3, "resampler": 9, "meter": 9, "apply": 3, "limiter": 12}
ORDER = sorted(CASES, key=lambda c: not c.startswith("at3enc"))   # the long ones first
JOBS = [(m, c) for c in ORDER for m in MODES]


@pytest.fixture(scope="module")
def children():
    build_strict()
    c = Children({job: ("run_emu_streams.py", ["--nobuild", job[1]], MODES[job[0]]) for job in JOBS})
    yield c
    c.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_pipeline_equals_restatement_in_every_order(children, case, mode):
    out = children.output((mode, case))
    assert f"\n{case} done" in out, out[-4000:]
    assert f"streams mode: {'seeded' if ':' in mode else mode}" in out, out[:400]
    assert "still holds" not in out, out[-4000:]   # nothing is left queued when the process ends
    assert_clean(out, CASES[case])
