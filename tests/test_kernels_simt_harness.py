"""The kernel SOURCES of the product, compiled for the host and run lane by lane through the SIMT harness of tools/emu,
against the oracle - the parity gate that exists without a GPU (the `-m gpu` tests are the parity tests proper).

The harness is test infrastructure like the oracle: the product library never contains or loads it. It is built in its
strict form here (-O0 + EMU_STRICT): besides comparing results it aborts when the lanes of a wavefront reach a cross-lane
exchange (ballot, readlane, ds_bpermute, DPP, wave-level rendezvous) from two DIFFERENT calls, i.e. when such a read
sits inside divergent control flow - a class of mistake the GPU tolerates until the compiler or the data change.

The decoders and the resampler go through the same harness in tests/test_decoders_simt_harness.py. The default runs of the
encoders' drivers are repeated at the end of this module with the wavefronts of every workgroup visited in descending order
(EMU_ORDER=reverse): a missing __syncthreads() between a producer and a consumer wavefront shows in one of the two orders.
"""
import os
import re
import sys

import pytest

from simt_harness_lib import Children, assert_clean, build_strict, run_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")


def _run(script, *args, timeout=900):
    rc, out = run_script(script, args, timeout=timeout)
    assert rc == 0, out[-4000:]
    return out


_assert_clean = assert_clean


@pytest.fixture(scope="module")
def harness():
    return build_strict()   # (once per session: tests/test_decoders_simt_harness.py uses the same library)


def test_atrac3_kernels(harness):
    """Six signals x LP2 / LP4 x (all tools, no gain, no gain + no tonal), two streams, two calls (carried state)."""
    _assert_clean(_run("run_emu.py", "--strict", "--nobuild"), 72)   # (frames and overflow counters per case)


def test_atrac3_overflow_counters(harness):
    """Input above full scale: frames and at3hip_get_counters (TScaler::Scale's "Scale error" / "clipping" diagnostics,
    atrac_scale.cpp:150-167, counted by k_psy) against the oracle, which tests/test_oracle_vs_ref.py pins to the lines the
    reference prints."""
    out = _run("run_emu.py", "--strict", "--nobuild", "hot")
    _assert_clean(out, 12)
    assert re.search(r"overflow counters [1-9]\d+, [1-9]\d+ ", out), out[-2000:]


def test_atrac3_dense_tonal_material(harness):
    """Every BFU tonal, runs continuing across BFU boundaries (at3_testlib.pcm_dense_tonal): k_psy's wavefront-parallel tonal
    extraction and mapping with both halves of its position list in use, under the emulator's rendezvous checks."""
    _assert_clean(_run("run_emu.py", "--strict", "--nobuild", "dense"), 12)


def test_gain_curve_select_walk(harness):
    """cell_divisors_packed - the gain curve's point list walked by selects, as k_gain_energy_scale, k_mdct_sub and k_gain_curve's score use it -
    against curve_divisor, the sample-by-sample restatement of TGainProcessor::Modulate (gain_processor.h:93-112), for 20 000 curves of
    ARBITRARY bytes per field (0 .. 7 points, levels 0 .. 15, locations 0 .. 31 in any order, repeated, adjacent): all 256 divisors, bit patterns."""
    import ctypes
    import numpy as np
    sys.path.insert(0, ROOT)
    from atracdenc_amd import binding as B
    lib = ctypes.CDLL(harness)
    enc = B.At3Hip(n_streams=1, max_blocks=2, lib_path=harness)
    rng = np.random.RandomState(5)
    n = 20000
    cv = np.zeros((n, 16), np.uint8)
    cv[:, 0] = rng.randint(0, 8, n)
    cv[:, 1:8] = rng.randint(0, 16, (n, 7))
    loc = rng.randint(0, 32, (n, 7))
    srt = rng.rand(n) < 0.6                                  # most as the encoder makes them: ascending
    loc[srt] = np.sort(loc[srt], axis=1)
    cv[:, 8:15] = loc
    cv[: n // 10, 1:8] = rng.randint(0, 256, (n // 10, 7))   # and bytes no encoder writes: the walk masks what it must
    a = np.zeros((n, 256), np.float32)
    b = np.zeros((n, 256), np.float32)
    fn = lib.at3hip_debug_cell_divisors
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    lv = cv[: n // 10, 1:8]
    lv[lv > 15] &= 15                                         # (levels are four bits in the bitstream and in both walks' tables)
    assert fn(enc.ctx, cv.ctypes.data, n, a.ctypes.data, b.ctypes.data) == 0
    enc.close()
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert bad.size == 0, (bad[:5].tolist(), cv[bad[0, 0]].tolist())
    assert (a != 1.0).any(axis=1).sum() > n // 2


def test_atrac3_gain_analysis_one_wavefront_form(harness):
    """AT3HIP_OPT_GAIN_FORM = AT3HIP_GAIN_FORM_ONE_WAVE (k_gain_analysis1, incl. the restated v_permlane32/16_swap, which tools/ubench/permlane_check
    compares with the hardware): the signals with gain curves x LP2 / LP4 x three option sets."""
    _assert_clean(_run("run_emu.py", "--strict", "--nobuild", "--gain-form=1", "burst", "stress"), 24)


def test_atrac3_literal_forms(harness):
    """AT3HIP_OPT_LITERAL_FORMS: the flatness measure per line and k_gain_spec's energy sums as the reference's chains."""
    _assert_clean(_run("run_emu.py", "--strict", "--nobuild", "--literal", "mix", "stress"), 24)


def test_atrac3_s16_entry_point(harness):
    """at3hip_encode_s16 (k_s16_to_f32 + the unchanged pipeline), calls of both kinds alternating on one context."""
    _assert_clean(_run("run_emu.py", "--strict", "--nobuild", "--s16", "mix"), 12)


def test_atrac1_kernels(harness):
    _assert_clean(_run("run_emu_at1.py", "--nobuild"), 24 * 4)


def test_atrac3plus_front_kernels(harness):
    _assert_clean(_run("run_emu_at3p.py", "--nobuild"), 12)


def test_atrac3plus_frame_kernels(harness):
    _assert_clean(_run("run_emu_at3p_write.py", "--nobuild"), 26)


# ---- the same default runs with the wavefronts of a workgroup in descending order ------------------------------------------------
AT3_SIGNALS = ("noise", "burst", "tones", "silence", "mix", "stress")   # run_emu.py's default list, one child per signal


@pytest.fixture(scope="module")
def reversed_runs(harness):
    rev = {"EMU_ORDER": "reverse"}
    jobs = {name: ("run_emu.py", ["--strict", "--nobuild", name], rev) for name in AT3_SIGNALS}
    for script in ("run_emu_at1.py", "run_emu_at3p.py", "run_emu_at3p_write.py"):
        jobs[script] = (script, ["--nobuild"], rev)
    c = Children(jobs)
    yield c
    c.close()


def test_atrac3_kernels_reversed_wavefront_order(reversed_runs):
    for name in AT3_SIGNALS:
        _assert_clean(reversed_runs.output(name), 12)   # (72 in all, as test_atrac3_kernels)


def test_atrac1_kernels_reversed_wavefront_order(reversed_runs):
    _assert_clean(reversed_runs.output("run_emu_at1.py"), 24 * 4)


def test_atrac3plus_front_kernels_reversed_wavefront_order(reversed_runs):
    _assert_clean(reversed_runs.output("run_emu_at3p.py"), 12)


def test_atrac3plus_frame_kernels_reversed_wavefront_order(reversed_runs):
    _assert_clean(reversed_runs.output("run_emu_at3p_write.py"), 26)


# ---- the edges of the float domain --------------------------------------------------------------------------------------------
# tests/float_domain_lib.py's streams (NaN, infinities, +-FLT_MAX, samples whose energy sums overflow f32, subnormals in block 3 of
# 12), one stream per pattern side by side, each against the oracle's encode of that stream alone. The harness converts float to
# int as the hardware does (tools/emu/hip/hip_runtime.h), and every buffer ends at a guard page (EMU_FENCE=high) in the first
# order: an index that leaves its table ends the child with a signal here, not a GPU. tests/test_float_domain_gpu.py runs what
# has passed here.
DOMAIN_AT3 = ("domain:clean,nan1,inf_pair,max1", "domain:nan_block,max_alt,inf_left,mixed", "domain:nan_bits,e19_alt,e15,subnormal")
DOMAIN_MODES = {"fence": {"EMU_FENCE": "high"}, "reverse": {"EMU_ORDER": "reverse"}}


@pytest.fixture(scope="module")
def domain_runs(harness):
    jobs = {}
    for mode, env in DOMAIN_MODES.items():
        jobs[mode, "run_emu_at1.py"] = ("run_emu_at1.py", ["--nobuild", "domain"], env)
        for part in DOMAIN_AT3:
            jobs[mode, part] = ("run_emu.py", ["--strict", "--nobuild", part], env)
        for script in ("run_emu_at3p.py", "run_emu_at3p_write.py"):
            jobs[mode, script] = (script, ["--nobuild", "domain"], env)
    c = Children(jobs)
    yield c
    c.close()


@pytest.mark.parametrize("mode", list(DOMAIN_MODES))
def test_atrac3_float_domain(domain_runs, mode):
    """LP2 and LP4, every tool and none, whole and as 5 + 1 + 6 blocks: frames and overflow counters; the one-channel joint-stereo
    context on clean, nan1 and max_alt (a subband sample above FLT_MAX / 2 must not pass through the M/S matrixing)."""
    n = 0
    for part in DOMAIN_AT3:
        out = domain_runs.output((mode, part))
        _assert_clean(out, 16)
        n += len(re.findall(r"ch=1 split", out))
    assert n == 4   # (both parts that hold one of the one-channel patterns ran that case, whole and split)


@pytest.mark.parametrize("mode", list(DOMAIN_MODES))
def test_atrac1_float_domain(domain_runs, mode):
    """auto and short windows x 1 and 2 channels, whole and as 10 + 2 + 12 blocks: sound units and the loudness tap"""
    _assert_clean(domain_runs.output((mode, "run_emu_at1.py")), 16)


@pytest.mark.parametrize("mode", list(DOMAIN_MODES))
def test_atrac3plus_float_domain(domain_runs, mode):
    """subbands and spectra of pqf_mdct, and the frames of encode_frames whole and as 2 + 1 + 3, mono and stereo"""
    _assert_clean(domain_runs.output((mode, "run_emu_at3p.py")), 4)
    _assert_clean(domain_runs.output((mode, "run_emu_at3p_write.py")), 4)
