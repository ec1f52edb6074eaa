"""The look-ahead limiter's definition (include/at3hip_loudness.h, "The look-ahead limiter") as restated by
tests/host/limiter_cpu.c, without a GPU: the properties the definition promises, the true-peak bound measured with the meter's
own restatement, inputs that are limited but not everywhere, the levelling example, and the new symbols."""
import os
import re

import numpy as np
import pytest

import limiter_lib as LM
import loudness_lib as L

SIGNALS = ("clicks", "burst", "noise", "fs4", "tone40")
GAINS = (4.0, 16.0)
# The output's true peak (loudness_cpu.c's, all 4T converter outputs) over the ceiling, true-peak detector, worst of the ten
# cases below: 0.0052 dB (clicks at g = 16; DESIGN.md section 18 lists all ten), rounded up to the next 0.01 dB.
TRUE_PEAK_BOUND_DB = 0.01

_runs = {}


def run(kind, g, true_peak):
    key = (kind, g, true_peak)
    if key not in _runs:
        x = LM.signal(kind)
        _runs[key] = (x,) + LM.restate(x, g, LM.CEIL, true_peak)
    return _runs[key]


@pytest.mark.parametrize("g", GAINS)
@pytest.mark.parametrize("kind", SIGNALS)
def test_restatement_properties(kind, g):
    x, y, S, r, (min_s, n_lim) = run(kind, g, False)
    assert (S.astype(np.float64) / LM.FULL <= r).all()          # the smoothed gain never exceeds the required one
    assert S.min() >= 0 and S.max() <= LM.FULL and min_s == S.min() and n_lim == int((S < LM.FULL).sum())
    assert (np.abs(y) <= LM.CEIL).all()                         # |y| <= c exactly
    scaled = x * np.float32(g)
    assert scaled.dtype == np.float32
    free = S == LM.FULL                                         # not limited: the float multiply, bit for bit (unless it exceeds c)
    want = np.clip(scaled, -LM.CEIL, LM.CEIL)
    assert L.bits_equal(y[free], want[free])
    assert n_lim > 0 and float(np.abs(scaled).max()) > LM.CEIL  # every case does limit


@pytest.mark.parametrize("true_peak", [False, True])
@pytest.mark.parametrize("kind", SIGNALS)
def test_a_gain_that_needs_no_limiting_gives_apply(kind, true_peak):
    x = LM.signal(kind, 20000)
    g = np.float32(0.5)   # sample peak <= 0.5, true peak of full-scale noise < 1.7: nothing reaches -1 dBFS
    y, S, r, st = LM.restate(x, g, LM.CEIL, true_peak)
    assert st == (LM.FULL, 0) and (S == LM.FULL).all()
    assert L.bits_equal(y, x * g)


@pytest.mark.parametrize("g", GAINS)
@pytest.mark.parametrize("kind", SIGNALS)
def test_true_peak_bound(kind, g):
    """with the true-peak detector the output's true peak, measured by the meter's restatement, stays within
    TRUE_PEAK_BOUND_DB of the ceiling; with the sample detector it does not (which is why the mode exists)"""
    x, y, S, r, st = run(kind, g, True)
    assert (S.astype(np.float64) / LM.FULL <= r).all() and (np.abs(y) <= LM.CEIL).all()
    tp = max(L.measure(y, True).true_peak[:2])
    over = 20.0 * np.log10(float(tp) / float(LM.CEIL))
    print(f"true-peak detector: {kind} g={g}: output true peak {over:+.4f} dB against the ceiling, limited share {st[1] / len(S):.3f}")
    assert over <= TRUE_PEAK_BOUND_DB, over
    if kind == "noise":
        ys = run(kind, g, False)[1]
        over_s = 20.0 * np.log10(float(max(L.measure(ys, True).true_peak[:2])) / float(LM.CEIL))
        print(f"sample detector: {kind} g={g}: output true peak {over_s:+.2f} dB against the ceiling")
        assert over_s > 1.0


@pytest.mark.parametrize("kind", ["clicks", "burst"])
def test_parity_inputs_are_not_vacuous(kind):
    """the inputs of the parity tests are limited, and not everywhere"""
    for true_peak in (False, True):
        S = run(kind, 4.0, true_peak)[2]
        share = float((S < LM.FULL).mean())
        print(f"{kind} g=4 true_peak={true_peak}: limited share {share:.3f}")
        assert 0.1 < share < 0.95
        for channels in (1, 2):
            st = LM.expect(channels, true_peak)[1]
            assert 0.1 < st[0][1] / LM.T_GPU < 0.95 and 0.1 < st[2][1] / LM.T_GPU < 0.95 and st[1][1] == 0, st


def test_levelling_example():
    """A quiet tone with a full-scale click every three seconds, target -16 LUFS, ceiling -1 dBFS: the gain to the target plus the limiter
    lands within 0.5 LU of the target under the restated meter; the one constant gain capped by the peak lands many LU below."""
    x = LM.leveling_example()
    target = -16.0
    r = L.measure(x, True)
    capped = L.gain(r, target, -1.0)
    to_target = L.gain(r, target, 400.0)       # (a ceiling that never binds: the gain to the target alone)
    assert to_target > 2 * capped
    constant = L.measure(x * capped, True).integrated
    y, S, _, st = LM.restate(x, to_target, LM.CEIL, True)
    limited = L.measure(y, True)
    print(f"levelling: input {r.integrated:.2f} LUFS; capped constant gain {20 * np.log10(capped):.2f} dB -> {constant:.2f} LUFS; "
          f"gain to target {20 * np.log10(to_target):.2f} dB + limiter -> {limited.integrated:.2f} LUFS, "
          f"true peak {20 * np.log10(max(limited.true_peak)):.3f} dBFS, limited share {st[1] / len(S):.3f}")
    assert abs(limited.integrated - target) < 0.5
    assert constant < target - 5.0
    assert 20 * np.log10(max(limited.true_peak) / float(LM.CEIL)) <= TRUE_PEAK_BOUND_DB


def test_symbols():
    """the new symbols are exported, declared in the header, listed in at3hip.h's version notes and in binding.SYMBOLS"""
    import subprocess
    import atracdenc_amd
    names = ["at3hip_loudness_limit_start", "at3hip_loudness_limit", "at3hip_loudness_limit_s16", "at3hip_loudness_limit_flush",
             "at3hip_loudness_limit_stats", "at3hip_loudness_limit_delay"]
    if not os.path.exists(atracdenc_amd.LIB_PATH):
        atracdenc_amd.build_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", atracdenc_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(L.HEADER).read()
    notes = open(os.path.join(L.ROOT, "include", "at3hip.h")).read()
    for n in names:
        assert n in exported and n in atracdenc_amd.binding.SYMBOLS, n
        assert re.search(r"\b" + n + r"\s*\(", header) and re.search(r"\b" + n + r"\s*\(", notes), n
    lib = atracdenc_amd.load_library()
    assert lib.at3hip_loudness_limit_delay(0) == 220 and lib.at3hip_loudness_limit_delay(1) == 292
    assert re.search(r"#define AT3HIP_LIMIT_LOOKAHEAD 220\b", header) and re.search(r"#define AT3HIP_LIMIT_HOLD 2205\b", header)
