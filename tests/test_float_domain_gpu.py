"""Every float-PCM engine at the edges of the float domain, on the GPU: NaN, infinities, +-FLT_MAX, samples whose squares
overflow f32, and subnormals (tests/float_domain_lib.py), one stream per pattern side by side in ONE context, each stream
compared with the oracle's (or the C restatement's) result for that stream ALONE. That one comparison is parity (the GPU
and x86 convert and propagate non-finite values differently: v_cvt_i32_f32 saturates and answers 0 for a NaN where
cvtss2si answers INT_MIN), isolation (a poisoned stream's neighbours are compared too) and recovery (the blocks after the
bad one) at once.

Byte outputs (frames, sound units, 16-bit samples) are compared exactly, float outputs by float_domain_lib.floats_match
(bit patterns; a NaN must meet a NaN, sign and payload not compared). Every output is filled with a sentinel before the
call. An (engine, pattern) pair listed in float_domain_lib.EXCEPTIONS is held to the weaker contract stated there instead;
the table is empty. The limiter and the ATRAC3plus tone analysis, which take any float by their headers' word, are held to
their C restatements in the same way.

The same inputs go through the kernel sources on the CPU first (the `domain` family of the tools/emu drivers, with guard
pages around every buffer: tests/test_*_simt_harness.py), so an index that leaves its table shows there, not here.
"""
import numpy as np
import pytest

import float_domain_lib as FD

pytestmark = pytest.mark.gpu


def _clean(exp, names):
    return exp[names.index("clean")]


def test_exception_table():
    assert not any(p in FD.COMPULSORY for _, p in FD.EXCEPTIONS)
    assert all(isinstance(r, str) and r for r in FD.EXCEPTIONS.values())
    assert all(e in ("at3", "at1", "at3p", "resample", "loudness", "limiter", "tones") and p in FD.NAMES for e, p in FD.EXCEPTIONS)


@pytest.mark.parametrize("br,ng,nt,nch,names", FD.AT3_CASES,
                         ids=[f"{'lp2' if c[0] == 132300 else 'lp4'}_{'plain' if c[1] else 'gain_tonal'}_ch{c[3]}" for c in FD.AT3_CASES])
def test_atrac3(oracle, br, ng, nt, nch, names):
    """12 streams x 12 blocks (3 streams from one channel in the joint-stereo container): frames bit for bit the oracle's,
    at3hip_get_counters equal to at3o_diag_counts, in one call and fed as 5 + 1 + 6 blocks."""
    exp, counts = FD.at3_expect(br, ng, nt, nch, names)
    whole, c_whole = FD.at3_run(None, br, ng, nt, nch, names)
    split, c_split = FD.at3_run(None, br, ng, nt, nch, names, FD.AT3_SPLIT)
    again, _ = FD.at3_run(None, br, ng, nt, nch, names)
    assert np.array_equal(whole, split) and np.array_equal(whole, again), "the frames depend on the call pattern or the run"
    bad = FD.rows_bad(whole, exp, "at3", names, _clean(exp, names))
    assert not bad, f"streams whose frames differ from the oracle's: {bad}"
    if not any(("at3", n) in FD.EXCEPTIONS for n in names):
        assert c_whole == c_split == tuple(counts.sum(0).tolist())
    assert counts.sum() > 0   # (the overflowing patterns make TScaler::Scale's diagnostics count)


@pytest.mark.parametrize("mode,nch", FD.AT1_CASES, ids=[f"{m}_ch{c}" for m, c in FD.AT1_CASES])
def test_atrac1(oracle, mode, nch):
    """12 streams x 24 blocks: sound units and the loudness tap are the oracle's, in one call and as 10 + 2 + 12 blocks."""
    exp, eloud = FD.at1_expect(mode, nch)
    whole, loud = FD.at1_run(None, mode, nch)
    split, loud_s = FD.at1_run(None, mode, nch, split=FD.AT1_SPLIT)
    assert np.array_equal(whole, split), "the sound units depend on the call pattern"
    assert np.array_equal(loud.view(np.uint32), loud_s.view(np.uint32)), "the loudness tap depends on the call pattern"
    bad = FD.rows_bad(whole, exp, "at1", FD.NAMES, _clean(exp, FD.NAMES))
    assert not bad, f"streams whose sound units differ from the oracle's: {bad}"
    for i, n in enumerate(FD.NAMES):
        if ("at1", n) not in FD.EXCEPTIONS:
            FD.assert_floats_match(loud[i], eloud[i], f"loudness tap of stream {n}")


@pytest.mark.parametrize("nch", [1, 2], ids=["mono", "stereo"])
def test_atrac3plus(oracle, nch):
    """12 streams x 6 frames: encode_frames equals the oracle's PQF -> MDCT -> writer, in one call and as 2 + 1 + 3 frames."""
    exp = FD.at3p_expect(nch)
    whole = FD.at3p_run(None, nch)
    split = FD.at3p_run(None, nch, split=FD.AT3P_SPLIT)
    assert np.array_equal(whole, split), "the frames depend on the call pattern"
    bad = FD.rows_bad(whole, exp, "at3p", FD.NAMES, _clean(exp, FD.NAMES))
    assert not bad, f"streams whose frames differ from the oracle's: {bad}"


@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
@pytest.mark.parametrize("nch", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("pair", FD.RESAMPLE_PAIRS, ids=[f"{a}_{b}" for a, b in FD.RESAMPLE_PAIRS])
def test_resampler(oracle, pair, nch, s16):
    """T = 3001 per stream, the bad block inside: the converted streams (one call + flush, and three calls + flush) are
    tests/host/resample_cpu.c's; 16-bit output is its float output through lrintf(clamp(x, -1, 1) * 32767), a NaN giving 0."""
    exp = FD.resample_expect(pair, nch)
    assert np.isnan(exp).any() and np.isinf(exp).any()   # (the patterns reach the output)
    whole = FD.resample_run(None, pair, nch, s16)
    cut = FD.resample_run(None, pair, nch, s16, cuts=FD.RESAMPLE_CUTS)
    assert not FD.resample_bad(whole, exp, s16), FD.resample_bad(whole, exp, s16)
    assert not FD.resample_bad(cut, exp, s16), FD.resample_bad(cut, exp, s16)


@pytest.mark.parametrize("nch", [1, 2], ids=["mono", "stereo"])
def test_meter(oracle, nch):
    """1.2 s per stream, true peak on: hop sums, every field of the results and apply's samples are
    tests/host/loudness_cpu.c's (apply: the float32 product), in one call and in three."""
    exp = FD.meter_expect(nch)
    assert any(np.isnan(r.true_peak[0]) for r in exp[1])   # (the patterns reach the results)
    for cuts in ((FD.METER_T,), FD.METER_CUTS):
        bad = FD.meter_bad(FD.meter_run(None, nch, cuts=cuts), exp)
        assert not any(bad.values()), (cuts, bad)


def _same_floats(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("nch", [1, 2], ids=["mono", "stereo"])
def test_limiter(oracle, nch):
    """6000 samples per stream, one stream per pattern and per gain of float_domain_lib.LIMITER_PAIRS (gains 0, 2, FLT_MAX and
    the smallest subnormal at -1 dBFS; gain 2 under the smallest subnormal and under FLT_MAX as the ceiling), both detectors:
    samples and statistics are tests/host/limiter_cpu.c's (step 8 of the limiter's definition in include/at3hip_loudness.h), in
    one call and in three, and a second run gives the bits of the first, NaN payloads included."""
    for ceiling in FD.LIMITER_CEILINGS:
        for tp in (False, True):
            exp = FD.limiter_expect(nch, tp, ceiling)
            assert np.isnan(exp[0]).any()                                      # (the patterns reach the output)
            assert ceiling != FD.LIMITER_CEIL or (0 < exp[1][len(FD.NAMES)][1] < FD.LIMITER_T and min(st[0] for st in exp[1]) == 0)
            for cuts in ((FD.LIMITER_T,), FD.LIMITER_CUTS):
                got = FD.limiter_run(None, nch, tp, ceiling, cuts=cuts)
                again = FD.limiter_run(None, nch, tp, ceiling, cuts=cuts)
                assert _same_floats(got[0], again[0]) and got[1] == again[1], "the result does not repeat"
                bad = FD.limiter_bad(got, exp, nch, ceiling)
                assert not bad, (float(ceiling), tp, cuts, bad)


@pytest.mark.parametrize("nch", [1, 2], ids=["mono", "stereo"])
def test_tones(oracle, nch):
    """12 streams x 6 frames, plain, gated, shared and gated + shared (mono: sharing once, where it changes nothing): the records
    of analyse_tones are tests/host/at3p_gha_cpu.c's byte for byte and its residuals bit for bit (a NaN against a NaN), the
    frames of encode_frames_tonal are those of at3p_gha_lib.pipeline, whole and split 2 + 1 + 3, and a second run repeats the
    first ("Any float is accepted", include/at3phip.h)."""
    for gated, shared in FD.tones_modes(nch):
        exp = FD.tones_expect(None, nch, gated, shared)
        assert np.isnan(exp[1]).any() and exp[0]["band"]["n_waves"].sum(axis=(2, 3)).max() == 48   # (NaN residuals; the budget binds)
        for split in (None, FD.TONES_SPLIT):
            got = FD.tones_run(None, nch, gated, shared, split=split)
            again = FD.tones_run(None, nch, gated, shared, split=split)
            assert got[0].tobytes() == again[0].tobytes() and _same_floats(got[1], again[1]) and np.array_equal(got[2], again[2]), \
                "the result does not repeat"
            bad = FD.tones_bad(got, exp)
            assert not any(bad.values()), (gated, shared, split, bad)
