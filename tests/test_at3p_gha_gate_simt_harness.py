"""The tone analysis kernels with AT3PHIP_TONES_GATED (at3p_gha.hpp: k_at3p_tone_find<true>, k_at3p_tone_select, k_at3p_tone_sub,
k_at3p_tone_state) run lane by lane through the CPU SIMT harness against the C restatement tests/host/at3p_gha_cpu.c; and the
analysis under every flag combination on tests/float_domain_lib.py's streams (NaN, infinities, +-FLT_MAX, overflowing and
subnormal samples)."""
import os

import pytest

from simt_harness_lib import CLANG, Children, assert_clean, build_strict

needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")


@needs_clang
def test_harness_driver_equals_the_gated_restatement():
    """tools/emu/run_emu_at3p_gha.py gated under the strict harness: records and residuals of the crafted onsets and offsets (mono and
    stereo, in one call and in calls of 1, 2 and 3 frames) and of 8 frames of stereo `burst`, the frames of its pipeline in one call
    and in three, and the host gate function equal the restatement's - in ascending and in descending wavefront order, and with
    every device buffer ending at a guard page."""
    build_strict()
    modes = {"plain": {}, "reverse": {"EMU_ORDER": "reverse"}, "fence": {"EMU_FENCE": "high"}}
    runs = Children({m: ("run_emu_at3p_gha.py", ["gated", "--nobuild"], env) for m, env in modes.items()})
    try:
        for m in modes:
            out = runs.output(m)
            assert_clean(out, 12 * 3 + 3 + 2)
            assert out.count("onset") == 6 and out.count("offset") == 6 and out.count("encode burst nch=2") == 2
            assert "points [0, 0, 6, 0, 0, 0]" in out   # the stereo crafted cases: three bands of two channels in the record of slot 2
    finally:
        runs.close()


DOMAIN = {"domain:1": 3 * 2 * 3, "domain:2": 4 * 2 * 3}   # flag combinations x call patterns x (records, residuals, frames)
DOMAIN_ENV = {"high": {"EMU_FENCE": "high"}, "reverse": {"EMU_ORDER": "reverse"}}


@pytest.fixture(scope="module")
def domain_children():
    build_strict()
    c = Children({(m, case): ("run_emu_at3p_gha.py", [case, "--nobuild"], env) for case in DOMAIN for m, env in DOMAIN_ENV.items()})
    yield c
    c.close()


@needs_clang
@pytest.mark.parametrize("mode", list(DOMAIN_ENV))
@pytest.mark.parametrize("case", list(DOMAIN))
def test_float_domain(domain_children, mode, case):
    """domain:C: one stream per pattern of tests/float_domain_lib.py (NaN, infinities, +-FLT_MAX, overflowing and subnormal samples
    in frame 1 of 6) side by side, plain, gated, shared and gated + shared (mono: sharing once, where it changes nothing), whole
    and split 2 + 1 + 3: the records of analyse_tones byte for byte, its residuals as bit patterns (a NaN against a NaN) and the
    frames of encode_frames_tonal against the restatement of each stream alone - with every device buffer ending at a guard
    page, and with the wavefronts of a workgroup in descending order."""
    out = domain_children.output((mode, case))
    assert_clean(out, DOMAIN[case])
    assert out.count(f"domain nch={case[-1]}") == DOMAIN[case] // 3
