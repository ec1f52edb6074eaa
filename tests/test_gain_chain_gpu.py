"""The light stage of the gain path (k_gain_tail, k_gain_scan, k_gain_curve) and k_psy on tiny batches, bit for bit against the
CPU oracle: 2 streams x 3 frames, LP2 and LP4, on `noise`, `burst` and `tones`.

  * GAIN_ANALYSIS tap: highFreqRatio of every (frame, channel, band < 3) item, and for the items at or above the 5 % gate the 32
    sub-frame RMS values, both quartile lists and their mean - recomputed from the PCM with the oracle's QMF, upsampler and
    AnalyzeGain (the 512 samples of an item are the frame's block and a quarter block on either side: atrac3denc.cpp:299-330);
  * CURVES tap: point counts, levels and locations against the oracle's taps;
  * PSY tap: scale-factor indices, BFU energies, loudness, tonal blocks (every field) against the oracle's taps;
  * the frames.
"""
import numpy as np
import pytest

from at3_testlib import LP2, LP4, SIGNALS

pytestmark = pytest.mark.gpu

NB = 4   # blocks per call: three frames

# two streams per signal: the suite's seeded signal and a second member of its family
STREAMS = {
    "noise": lambda: [SIGNALS["noise"](NB), SIGNALS["noise"](NB, seed=2, amp=2048)],
    "burst": lambda: [SIGNALS["burst"](NB), SIGNALS["burst"](NB, period=1100, lo=0.01, hi=0.7, freq=5000.0, phase=400)],
    "tones": lambda: [SIGNALS["tones"](NB), SIGNALS["tones"](NB, freqs=(700.0, 5200.0, 9000.0), amp=0.25)],
}


@pytest.fixture(scope="module")
def hip():
    import atracdenc_amd
    return atracdenc_amd


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def expected_gain_analysis(oracle, pcm, js):
    """per frame index 1 .. NB - 1: hfr [2][3], gain / lo / hi [2][3][32], mean gain [2][3] as the oracle's pieces give them"""
    nb = pcm.shape[0]
    sub = np.stack([oracle.qmf((pcm[:, :, ch] / np.float32(4.0)).astype(np.float32).reshape(-1)) for ch in range(2)])   # [2][4][nb * 256]
    sub = np.concatenate([np.zeros((2, 4, 128), np.float32), sub], axis=2)                                             # stream index -128 first
    hfr = np.zeros((nb, 2, 3), np.float32)
    vals = np.zeros((nb, 2, 3, 3, 32), np.float32)
    mean = np.zeros((nb, 2, 3), np.float32)
    for f in range(1, nb):
        win = sub[:, :, (f - 1) * 256:(f - 1) * 256 + 512]
        if js:
            win = np.stack([(win[0] + win[1]) * np.float32(0.5), (win[0] - win[1]) * np.float32(0.5)])
        for ch in range(2):
            for b in range(3):
                sig, hfr[f, ch, b] = oracle.upsample(win[ch, b])
                vals[f, ch, b] = oracle.analyze_gain(sig[1024:3072], 32)
                acc = np.float32(0.0)
                for g in vals[f, ch, b, 0]:
                    acc = np.float32(acc + g)
                mean[f, ch, b] = acc / np.float32(32.0)
    return hfr, vals, mean


def run_case(lib, oracle, name, br):
    """encode the two streams of `name` at `br` with `lib` and compare the three taps and the frames with the oracle; returns the oracle's taps"""
    from atracdenc_amd import binding as B
    pcm = np.stack(STREAMS[name]())
    S, F = pcm.shape[0], NB - 1
    enc = lib.At3Hip(n_streams=S, max_blocks=NB, bitrate=br)
    got = enc.encode(pcm)
    js = bool(enc.joint_stereo) if hasattr(enc, "joint_stereo") else br == LP4
    rec = enc.read_tap(B.TAP_GAIN_ANALYSIS, np.uint32, (S, NB, 2, 3, 104))
    curves = enc.read_tap(B.TAP_CURVES, np.uint8, (S, NB, 2, 4, 16))
    psy = enc.read_tap(B.TAP_PSY, B.At3Hip.PSY_DTYPE, (S, F, 2))
    enc.close()
    taps = []
    for i in range(S):
        frames, tap = oracle.encode(pcm[i], br, taps=True)
        taps.append(tap)
        # GAIN_ANALYSIS
        hfr, vals, mean = expected_gain_analysis(oracle, pcm[i], js)
        assert np.array_equal(rec[i, 1:, :, :, 0], u32(hfr[1:])), (name, br, i, "hfr")
        on = hfr[1:] >= np.float32(0.05)
        for k in range(3):   # gain, lo, hi at words 8, 40, 72
            assert np.array_equal(rec[i, 1:, :, :, 8 + 32 * k:40 + 32 * k][on], u32(vals[1:, :, :, k])[on]), (name, br, i, ("gain", "lo", "hi")[k])
        assert np.array_equal(rec[i, 1:, :, :, 2][on], u32(mean[1:])[on]), (name, br, i, "mean gain")
        # CURVES (frame f at index f; band 3 never has a curve)
        assert np.array_equal(curves[i, 1:, :, :, 0], tap["n_points"].astype(np.uint8)), (name, br, i)
        for f in range(F):
            for ch in range(2):
                for b in range(4):
                    n = int(tap["n_points"][f, ch, b])
                    assert np.array_equal(curves[i, f + 1, ch, b, 1:1 + n], tap["level"][f, ch, b, :n].astype(np.uint8)), (name, br, i, f, ch, b)
                    assert np.array_equal(curves[i, f + 1, ch, b, 8:8 + n], tap["loc"][f, ch, b, :n].astype(np.uint8)), (name, br, i, f, ch, b)
                    assert not curves[i, f + 1, ch, b, 1 + n:8].any() and not curves[i, f + 1, ch, b, 8 + n:].any()
        # PSY
        assert np.array_equal(psy[i]["sfi"], tap["sfi"].astype(np.uint8)), (name, br, i)
        assert np.array_equal(u32(psy[i]["energy"]), u32(tap["energy"])), (name, br, i)
        assert np.array_equal(u32(psy[i]["loud_ch"]), u32(tap["loudness_ch"])), (name, br, i)
        assert np.array_equal(psy[i]["n_tonal"], tap["n_tonal"]), (name, br, i)
        for f in range(F):
            for ch in range(2):
                n = int(tap["n_tonal"][f, ch])
                blk = psy[i, f, ch]["tonal"][:n]
                assert np.array_equal(blk["pos"], tap["tonal_pos"][f, ch, :n]), (name, br, i, f, ch)
                assert np.array_equal(blk["len"], tap["tonal_len"][f, ch, :n]), (name, br, i, f, ch)
                assert np.array_equal(blk["sfi"], tap["tonal_sfi"][f, ch, :n]), (name, br, i, f, ch)
                assert np.array_equal(u32(blk["values"]), u32(tap["tonal_values"][f, ch, :n, :7])), (name, br, i, f, ch)
        # frames
        assert np.array_equal(got[i], frames), (name, br, i)
    return taps, rec


@pytest.mark.parametrize("br", [LP2, LP4])
@pytest.mark.parametrize("name", ["noise", "burst", "tones"])
def test_taps_and_frames(hip, oracle, name, br):
    taps, rec = run_case(hip, oracle, name, br)
    hfr = rec[:, 1:, :, :, 0].view(np.float32)
    assert (hfr >= 0.05).any()                                       # the light stage has items to work on
    if name == "burst":
        assert sum(int(t["n_points"].sum()) for t in taps) > 0       # and the material does end in gain curves
    if name == "tones":
        assert sum(int(t["n_tonal"].sum()) for t in taps) > 0
