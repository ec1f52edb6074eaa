"""The loudness meter's definition (include/at3hip_loudness.h) without a GPU: its outside anchors - the ITU coefficient table
and the EBU Tech 3341 test signals -, the restart form against a never-restarted filter, the edge cases of gating, gain and
peaks, all on the C restatement tests/host/loudness_cpu.c; and the library's host-only functions against that restatement."""
import numpy as np
import pytest

import loudness_lib as L

# ITU-R BS.1770-4, table 1 and table 2 (48 kHz), as printed: {b0, b1, b2, a1, a2}
ITU_48K = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
                    [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]])


# ---- coefficients -------------------------------------------------------------------------------------------------------------
def test_prototype_gives_the_itu_table_at_48k():
    """14 printed decimals: 1e-13 leaves room for their rounding and nothing else"""
    assert np.abs(L.prototype(48000) - ITU_48K).max() <= 1e-13


def test_prototype_gives_the_header_literals_at_44k1():
    assert np.abs(L.prototype(44100) - L.header_coeffs()).max() <= 1e-12


def test_header_literals_equal_the_restatements():
    assert L.bits_equal(L.header_coeffs(), L.coeffs())
    # the same literals stand in the header's comment
    text = open(L.HEADER).read()
    for v in ("1.5308412300503478", "-2.6509799951547297", "1.169079079921587", "-1.6636551132560204", "0.7125954280732254",
              "-1.989169673629796", "0.9891990357870393"):
        assert text.count(v) >= 2, v


# ---- EBU Tech 3341 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(5), ids=[f"case{i + 1}" for i in range(5)])
def test_ebu_tech_3341(case):
    """Cases 1 - 5 as float32 in-phase stereo 1 kHz sines, within the EBU's own tolerance of +-0.1 LU."""
    segments, want = L.EBU_3341[case]
    x = L.tone_segments(segments)
    r = L.measure(x)
    print(f"case {case + 1}: integrated {r.integrated:.4f} LUFS (target {want}), {r.n_blocks_kept} blocks kept of {r.n_hops - 3}")
    assert abs(r.integrated - want) <= 0.1
    assert r.n_samples == x.shape[0] and r.n_hops == x.shape[0] // 4410


def test_ebu_case_3_needs_the_relative_gate():
    x = L.tone_segments(L.EBU_3341[2][0])
    z = L.hops(x)
    without = L.gate(z, relative=False).integrated
    print(f"case 3 without the relative gate: {without:.4f} LUFS")
    assert abs(without - (-23.0)) > 0.1
    assert abs(L.gate(z).integrated - (-23.0)) <= 0.1


def test_ebu_case_1_momentary_and_short_term():
    """a steady tone: every 400 ms block and every 3 s window reads what the whole programme reads"""
    r = L.measure(L.tone_segments(L.EBU_3341[0][0]))
    assert abs(r.momentary_max - (-23.0)) <= 0.1 and abs(r.short_term_max - (-23.0)) <= 0.1


# ---- the restart form ---------------------------------------------------------------------------------------------------------
def restart_signal(hops=100):
    rng = np.random.RandomState(1)
    n = hops * 4410
    t = np.arange(n)
    x = 0.3 * rng.uniform(-1, 1, (n, 2)) + 0.3 * np.sin(2 * np.pi * 440 * t / 44100)[:, None] + 0.2
    return x.astype(np.float32)


def test_restart_form_equals_a_never_restarted_filter():
    x = restart_signal()
    zc = L.hops_continuous(x)
    rel = np.abs(L.hops(x) / zc - 1).max()
    print(f"largest relative difference of z, 2 hops of warm-up: {rel:.3e}")
    assert rel <= 1e-12
    # the first three hops have no restart at all
    assert L.bits_equal(L.hops(x)[:3], zc[:3])


def test_one_hop_of_warm_up_would_not_do():
    x = restart_signal()
    rel = np.abs(L.hops(x, warm=1) / L.hops_continuous(x) - 1).max()
    print(f"largest relative difference of z, 1 hop of warm-up: {rel:.3e}")
    assert rel > 1e-12


# ---- edge cases ---------------------------------------------------------------------------------------------------------------
def test_silence():
    r = L.measure(np.zeros((44100, 2), np.float32), true_peak=True)
    assert r.integrated == -np.inf and r.momentary_max == -np.inf and r.n_blocks_kept == 0 and r.n_hops == 10
    assert list(r.sample_peak) == [0.0, 0.0] and list(r.true_peak) == [0.0, 0.0]
    assert L.gain(r, -16.0) == np.float32(1.0)


def test_fewer_than_four_hops():
    x = L.signal("noise", 4 * 4410 - 1, 2, 3)
    r = L.measure(x)
    assert r.n_hops == 3 and r.integrated == -np.inf and r.momentary_max == -np.inf and r.short_term_max == -np.inf
    assert L.gain(r, -16.0) == np.float32(1.0)
    r = L.measure(L.signal("noise", 4 * 4410, 2, 3))
    assert r.n_hops == 4 and np.isfinite(r.integrated) and r.n_blocks_kept == 1 and r.short_term_max == -np.inf
    assert np.isfinite(L.measure(L.signal("noise", 30 * 4410, 1, 3)).short_term_max)


def test_gain_rule():
    r = L.measure(L.tone_segments([(-23.0, 5.0)]))
    peak = max(r.sample_peak)
    assert abs(peak - 10 ** (-23 / 20)) < 1e-6
    # target-bound: -16 LUFS needs about +7 dB, the peak then sits near -16 dBFS, far under the ceiling
    g = L.gain(r, -16.0, -1.0)
    assert g == np.float32(10.0 ** ((-16.0 - r.integrated) / 20.0))
    # ceiling-bound: -3 LUFS would need +20 dB and put the peak at -3 dBFS; the ceiling of -6 dBFS holds it
    g = L.gain(r, -3.0, -6.0)
    assert g == np.float32(10.0 ** (-6.0 / 20.0) / np.float64(peak))
    assert abs(20 * np.log10(np.float64(g) * peak) - (-6.0)) < 1e-5
    # a measured true peak takes the sample peak's place
    r.true_peak[0] = 2 * peak
    assert L.gain(r, -3.0, -6.0) == np.float32(10.0 ** (-6.0 / 20.0) / np.float64(np.float32(2 * peak)))


def test_true_peak_of_a_quarter_rate_sine():
    """fs/4 at 45 degrees: every sample is +-0.70711 while the crest, which the 4x grid hits, is 1. The tone fades in and out
    over 50 ms (raised cosine): an abrupt start is a wide-band event whose band-limited version overshoots (1.011 here), which
    is a true peak too, but not the one this test is about; the converter's passband is flat within 0.001 dB at 11 kHz."""
    n, k = 44100, 2205
    env = np.ones(n)
    ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(k) / k)
    env[:k], env[-k:] = ramp, ramp[::-1]
    x = (env * np.sin(2 * np.pi * np.arange(n) / 4 + np.pi / 4)).astype(np.float32)[:, None]
    r = L.measure(x, true_peak=True)
    print(f"sample peak {r.sample_peak[0]:.6f}, true peak {r.true_peak[0]:.6f} ({20 * np.log10(r.true_peak[0]):+.5f} dB)")
    assert abs(r.sample_peak[0] - 0.70711) < 1e-5
    assert abs(20 * np.log10(r.true_peak[0])) <= 0.01
    assert L.measure(x).true_peak[0] == 0.0   # not measured


def test_true_peak_is_never_below_the_sample_peak():
    x = L.signal("noise", 3000, 2, 8)
    x[1500, 1] = 1.5   # a lone sample the interpolation does not exceed
    r = L.measure(x, true_peak=True)
    assert all(r.true_peak[c] >= r.sample_peak[c] for c in range(2)) and r.sample_peak[1] == np.float32(1.5)


# ---- the library's host-only functions ----------------------------------------------------------------------------------------
def test_library_gate_and_gain_equal_the_restatement():
    import atracdenc_amd
    from atracdenc_amd import loudness_gain, loudness_gate
    if not __import__("os").path.exists(atracdenc_amd.LIB_PATH):
        atracdenc_amd.build_library()
    cases = [L.tone_segments(s) for s, _ in L.EBU_3341[2:]]
    cases += [L.signal(k, 40 * 4410 + 17, c, 20 + i) for i, k in enumerate(L.KINDS) for c in (1, 2)]
    cases += [L.signal("noise", n, 2, 5) for n in (0, 4409, 3 * 4410, 4 * 4410, 29 * 4410, 30 * 4410)]
    for x in cases:
        z = L.hops(x)
        want = L.gate(z)
        got = loudness_gate(z)
        for n in ("integrated", "momentary_max", "short_term_max", "n_hops", "n_blocks_kept"):
            assert L.result_bits(got)[n] == L.result_bits(want)[n], (n, getattr(got, n), getattr(want, n))
        for peaks in (False, True) if x.shape[0] < 200000 else (False,):   # (the restated true peak of a minute takes one)
            want = L.measure(x, true_peak=peaks)
            for target, ceiling in ((-16.0, -1.0), (-23.0, -1.0), (0.0, -0.1), (-3.0, -6.0)):
                assert L.bits_equal(loudness_gain(want, target, ceiling), L.gain(want, target, ceiling)), (target, ceiling)
    lib = atracdenc_amd.load_library()
    assert lib.at3hip_loudness_gate(None, 4, 2, None) == -1 and lib.at3hip_loudness_gain(None, 0.0, 0.0, None) == -1
    z = np.zeros((4, 2))
    r = atracdenc_amd.binding.LoudnessResult()
    import ctypes
    assert lib.at3hip_loudness_gate(z.ctypes.data, 4, 3, ctypes.byref(r)) == -1   # channels 3
