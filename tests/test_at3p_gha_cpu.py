"""The ATRAC3plus tone analysis (include/at3phip.h, FINDING TONES) without a GPU: the C restatement tests/host/at3p_gha_cpu.c on
single sines, on noise and in the round trip that anchors the definition; its records against the writer's contract; the host
mirror's TAt3PToneAnalyser and TAt3PEncoder against it (tests/host/test_host_shim_at3p_gha.cpp on the host-compiled kernels);
the four kernels through the CPU SIMT harness (strict checks, both wavefront orders, guard pages); the host tables."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import at3p_gha_lib as G
import at3p_tonal_lib as T
from at3_testlib import _vp, at3p_signal
from simt_harness_lib import CLANG, ROOT, Children, assert_clean, build_strict

needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")
NF = 14


# ---- one stationary sine in one subband ------------------------------------------------------------------------------------------
def _sine_frames(f, amp, phase, n=3):
    t = np.arange(128 * n)
    return (amp * np.sin(2 * np.pi * f * t / 2048 + phase)).astype(np.float32).reshape(n, 128)


# bin centres (8k), bin edges (8k + 4) from the lowest to the highest whose two bins are both candidate bins (1 and 2, 125 and 126),
# neighbours of an edge, and both ends
@pytest.mark.parametrize("f", [1, 8, 12, 100, 103, 104, 108, 500, 511, 512, 516, 1004, 1008, 1023])
def test_one_sine_is_found_as_one_wave(f):
    """A stationary sine of amplitude 1000 in subband 5 of a mono stream: once both frames of a pair hold it, one wave and no other;
    the frequency index exact or +-1, AmpSf within one step of 4 log2(A) + 3, the phase within one step of the sine's at the
    pair's sample 128 (phases in steps of 2 pi / 32).

    At both ends the coarse spectrum peaks in bin 0 or 128 and the sine's mirror image lies a quarter of a bin away, inside the Hann
    main lobe: the end bins of step 3 and the normalisers rs, rc of steps 4 and 5 are what finds these two."""
    amp, ph0 = 1000.0, 0.7
    bands = np.zeros((3, 1, 16, 128), np.float32)
    bands[:, 0, 5] = _sine_frames(f, amp, ph0)
    blocks, resid = G.CpuToneAnalyser(1).analyse(bands)
    for slot in (1, 2):   # the pairs (frame 0, frame 1) and (frame 1, frame 2)
        waves = G.band_waves(blocks[slot], 1)[0]
        assert G.n_waves(blocks[slot]) == 1 and len(waves[5]) == 1, (slot, waves)
        fq, sf, ph = waves[5][0]
        assert abs(fq - f) <= 1, (fq, f)
        assert abs(sf - (4 * np.log2(amp) + 3)) <= 1.0, sf
        want_ph = (ph0 + 2 * np.pi * f * (128 * slot) / 2048) % (2 * np.pi) / (2 * np.pi / 32)   # the sine's phase at sample 128 of the pair
        d = (ph - want_ph + 16) % 32 - 16
        assert abs(d) <= 1.0, (ph, want_ph, fq)
        assert int(blocks[slot]["num_tone_bands"]) == 6
    # the stationary part is removed: frame 1's residual (both its blocks know the sine) is far below the sine
    assert np.abs(resid[2, 0, 5]).max() < 0.12 * amp, np.abs(resid[2, 0, 5]).max()
    assert np.array_equal(resid[2, 0, :5], bands[1, 0, :5]) and np.array_equal(resid[2, 0, 6:], bands[1, 0, 6:])


# ---- noise: no wave ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
def test_noise_has_no_wave_and_the_plain_frames(nch):
    """`noise`, 14 frames: no wave in any frame (the ratio 16 of step 3 caps false positives), every residual is its frame, and
    the frames are the plain encode's, one frame later."""
    pcm = G.signal_pcm("noise", NF, nch)
    frames, blocks, resid = G.pipeline(pcm)
    assert [G.n_waves(b) for b in blocks] == [0] * NF and not blocks.tobytes().strip(b"\0")
    bands = G.pqf_bands(pcm)
    assert np.array_equal(resid[1:].view(np.uint32), bands[:-1].view(np.uint32)) and not resid[0].any()
    plain = G.write_residual(bands)
    assert np.array_equal(frames[1:], plain[:-1])


# ---- the round trip that anchors the definition ---------------------------------------------------------------------------------------
_rt = {}


def _round_trip(name, scale=1.0):
    """mono, channel 0 of at3p_signal, 14 frames: (SNR without tones, SNR with the analyser, SNR with the blocks one frame early /
    late, waves per frame). Restatement, at3pt_apply_filter, oracle MDCT and writer, splice_tonal, cpu_tonal_decode; frame j carries
    the spectrum of residual j and block T_{j-1} (the at3phip_encode_frames alignment, without the engine's own lag)."""
    if (name, scale) in _rt:
        return _rt[(name, scale)]
    x2 = at3p_signal(name, NF, channel=0, scale=scale)
    x = x2.reshape(-1)
    bands = G.pqf_bands(np.concatenate([x2, np.zeros((1, 2048), np.float32)])[:, :, None])   # and the flushing frame
    blocks, resid = G.CpuToneAnalyser(1).analyse(bands)
    tones = list(blocks[1:])   # T_0 .. T_13
    # step 8 through at3pt_apply_filter: ApplyFilter(T_j) on frame j, after ApplyFilter(T_{-1}) on the zero frame before the stream
    lib = T.tonal_lib()
    st = np.zeros(lib.at3pt_filter_bytes(), np.uint8)
    filt = np.ascontiguousarray(np.concatenate([np.zeros((1, 2048), np.float32), bands[:NF, 0].reshape(NF, 2048)]))
    for j, rec in enumerate(blocks):
        lib.at3pt_apply_filter(_vp(st), 1, _vp(G.rec_ints(rec, 1)), _vp(filt[j]))
    assert np.array_equal(filt.view(np.uint32), resid.reshape(NF + 1, 2048).view(np.uint32))   # the restatement's residual is ApplyFilter's
    base = G.write_residual(resid[1:])
    snr = {}
    for shift in (-1, 0, 1):
        recs = [tones[j - 1 + shift] if 0 <= j - 1 + shift < NF else None for j in range(NF)]
        pcm, rej = T.cpu_tonal_decode(G.splice_blocks(base, recs, 1), 1)   # (splicing never fails to fit: it asserts)
        assert rej.sum() == 0
        snr[shift] = G.snr_db(x, pcm[:, :, 0].reshape(-1), NF)
    pcm, _ = T.cpu_tonal_decode(G.write_residual(bands[:NF]), 1)
    out = (G.snr_db(x, pcm[:, :, 0].reshape(-1), NF), snr[0], snr[-1], snr[1], float(np.mean([G.n_waves(b) for b in tones])))
    print(f"round trip {name} x{scale}: plain {out[0]:.2f} dB, tones {out[1]:.2f} dB, blocks shifted -1 / +1 {out[2]:.2f} / {out[3]:.2f} dB, {out[4]:.2f} waves per frame")
    _rt[(name, scale)] = out
    return out


# Measured with the restatement (f32 / f64 as defined), against the f64 prototype's figures of DESIGN.md section 17 in brackets:
#   tones   plain 27.21 dB, with the analyser 50.81 dB (27.26, 51.03), 8.00 waves per frame; blocks one frame early / late: -4.07 / -4.09 dB
#   burst   26.16 -> 35.56 dB (26.34, 35.31), 1.64 waves     stress  21.53 -> 22.59 dB (21.71, 22.56), 3.43 waves
#   mix     16.17 -> 16.50 dB (15.98, 16.27), 1.21 waves     noise   12.61 -> 12.61 dB, no wave     tones x 0.05  27.13 -> 51.47 dB (51.5)
# Every figure is within 0.5 dB of the prototype's. The shifted figures differ from the prototype's 25.2 / 25.4 dB by construction:
# here the residual keeps its own blocks subtracted and only the written blocks move, so the decoder adds tones of the wrong phase.
@pytest.mark.parametrize("name,scale,floor", [("tones", 1.0, 20.0), ("burst", 1.0, 6.0), ("mix", 1.0, 0.0), ("stress", 1.0, 0.0), ("tones", 0.05, 20.0)])
def test_round_trip_gains_over_the_run_without_tones(name, scale, floor):
    plain, tones, _, _, _ = _round_trip(name, scale)
    assert tones >= plain + floor, (plain, tones)


def test_round_trip_blocks_belong_to_their_frame():
    """the blocks written one frame early or late, against a residual that has its own blocks subtracted, lose at least 20 dB on
    `tones` (the writer's pairing; an easier experiment than the next test's)"""
    _, tones, early, late, _ = _round_trip("tones")
    assert tones - early >= 20.0 and tones - late >= 20.0, (tones, early, late)


@pytest.mark.parametrize("shift", [-1, 1])
def test_round_trip_analysis_shifted_by_one_frame(shift):
    """The analysis as a whole one frame off on `tones`: the block used as T_j, subtracted from frame j and written for it, is the
    one found for the pair (frame j + shift, frame j + shift + 1). Encoder and decoder then subtract and add the same wrong block,
    so nothing cancels but nothing is gained: the round trip falls back to about the run without tones and loses at least 20 dB
    against the aligned analysis. Measured: 25.07 dB (-1) and 25.42 dB (+1) against 50.81 dB aligned; the prototype's 25.2 / 25.4."""
    _, tones, _, _, _ = _round_trip("tones")
    x2 = at3p_signal("tones", NF, channel=0)
    bands = G.pqf_bands(x2[:, :, None])                                   # [NF][1][16][128]
    pad = np.zeros((2, 1, 16, 128), np.float32)
    found, _ = G.CpuToneAnalyser(1).analyse(np.concatenate([bands, pad]))   # slot f: the block of (frame f - 1, frame f) = T_{f-1}
    zero = np.zeros((), found.dtype)
    used = [found[j + shift + 1] if 0 <= j + shift + 1 < found.shape[0] else zero for j in range(-1, NF)]   # as T_{-1} .. T_{NF-1}
    lib = T.tonal_lib()
    st = np.zeros(lib.at3pt_filter_bytes(), np.uint8)
    filt = np.ascontiguousarray(np.concatenate([np.zeros((1, 2048), np.float32), bands[:, 0].reshape(NF, 2048)]))
    for j, rec in enumerate(used):
        lib.at3pt_apply_filter(_vp(st), 1, _vp(G.rec_ints(rec, 1)), _vp(filt[j]))
    base = G.write_residual(filt[1:].reshape(NF, 1, 16, 128))
    recs = [used[j] for j in range(NF)]                                   # frame j carries T_{j-1} = used[j]
    pcm, rej = T.cpu_tonal_decode(G.splice_blocks(base, recs, 1), 1)
    assert rej.sum() == 0
    snr = G.snr_db(x2.reshape(-1), pcm[:, :, 0].reshape(-1), NF)
    print(f"analysis shifted by {shift}: {snr:.2f} dB against {tones:.2f} dB aligned")
    assert tones - snr >= 20.0, (tones, snr)


# ---- the records and the writer -------------------------------------------------------------------------------------------------------
@needs_clang
@pytest.mark.parametrize("nch", [1, 2])
def test_records_pass_the_writers_validation(nch):
    """Every record of `tones`, `burst`, `stress` and `mix` (14 frames) and of the frame budget's crafted frame passes
    at3phip_write_frames_tonal's host check (on the host-compiled library: the check needs no device); in mono the writer's frames
    are the oracle writer's with the block spliced in."""
    from atracdenc_amd.binding import At3pHip
    enc = At3pHip(n_streams=1, max_frames=NF, channels=nch, lib_path=build_strict())
    try:
        for name in ("tones", "burst", "stress", "mix"):
            blocks, resid = G.CpuToneAnalyser(nch).analyse(G.pqf_bands(G.signal_pcm(name, NF, nch)))
            assert sum(G.n_waves(b) for b in blocks) > 0
            specs = G.residual_specs(resid)
            got = enc.write_frames(specs[None], None, blocks[None])[0]
            if nch == 1:
                assert np.array_equal(got, G.splice_blocks(G.write_residual(resid), blocks, 1)), name
        if nch == 2:
            blocks, _ = G.CpuToneAnalyser(2).analyse(G.budget_bands())
            assert G.n_waves(blocks[1]) == 48
            enc.write_frames(np.zeros((1, 2, 2, 2048), np.float32), None, blocks[None])
    finally:
        enc.close()


def test_sines_next_to_both_ends_are_found():
    """G.end_sine_bands: every subband of both channels holds one sine within 9 indices of an end; in the pair of two whole frames
    each is found as one wave, at its index or next to it"""
    blocks, _ = G.CpuToneAnalyser(2).analyse(G.end_sine_bands())
    waves = G.band_waves(blocks[2], 2)
    for c in range(2):
        for b in range(16):
            assert len(waves[c][b]) == 1 and abs(waves[c][b][0][0] - G.END_FREQS[(b + 3 * c) % 8]) <= 1, (c, b, waves[c][b])


def test_frame_budget_and_ties():
    """The crafted stereo pair: 96 waves found, 48 kept: the 32 of the strongest sine, then channel 0's 16 of the second."""
    blocks, _ = G.CpuToneAnalyser(2).analyse(G.budget_bands())
    rec = blocks[1]
    assert G.n_waves(rec) == 48 and int(rec["num_tone_bands"]) == 16
    waves = G.band_waves(rec, 2)
    for b in range(16):
        assert [w[0] for w in waves[0][b]] == list(G.BUDGET_FREQS[:2]) and [w[0] for w in waves[1][b]] == list(G.BUDGET_FREQS[:1]), b
    # a mono stream of the same frames has 48 waves in all and keeps them
    blocks, _ = G.CpuToneAnalyser(1).analyse(np.ascontiguousarray(G.budget_bands()[:, :1]))
    assert [len(w) for w in G.band_waves(blocks[1], 1)[0]] == [3] * 16


# ---- the host tables -------------------------------------------------------------------------------------------------------------------
def _host_lib():
    """the host-compiled library: neither the tables nor the symbols need a device, and a build that fails must fail the test"""
    from atracdenc_amd import binding
    return binding, build_strict()


@needs_clang
def test_host_tables_equal_the_restatements_and_a_fixture():
    """at3phip_host_tone_find_tables: the decoder's tone tables, the restatement's twiddles and thresholds bit for bit; the twiddles
    and thresholds also against values that do not depend on the host's libm: the twiddles' exact entries and the thresholds
    2^((i - 3) / 2 - 1 / 4) to 1e-6 relative (exp2f's and exp2's last bits may differ between libms)."""
    B, path = _host_lib()
    t, w = B.at3p_host_tone_find_tables(path), G.find_tables()
    g = np.load(os.path.join(ROOT, "tests", "golden", "at3p_gha.npz"))   # the fixture: the tables as the golden's generator saw them
    for k in ("tw", "thr", "rs", "rc"):
        assert np.array_equal(np.ascontiguousarray(t[k]).view(np.uint8).reshape(-1), g["table_" + k].view(np.uint8).reshape(-1)), k
    for k in ("sine", "hann", "amp_sf", "thr", "rs", "rc"):
        assert np.array_equal(t[k].view(np.uint8), w[k].view(np.uint8)), k
    assert np.array_equal(t["tw"].reshape(-1).view(np.uint32), w["tw"].view(np.uint32))
    d = B.at3p_decoder_host_tone_tables(path)   # (whose fixture is tests/golden/at3p_tonal.npz, tests/test_at3p_tonal_cpu.py)
    for k in ("sine", "hann", "amp_sf"):
        assert np.array_equal(t[k].view(np.uint32), d[k].view(np.uint32)), k
    assert t["tw"][0].tolist() == [1.0, 0.0] and t["tw"][128, 0] == -1.0 and t["tw"][64, 1] == -1.0 and t["tw"][192, 1] == 1.0
    i = np.arange(256)
    assert np.abs(t["tw"][:, 0] - np.cos(2 * np.pi * i / 256)).max() < 1e-7 and np.abs(t["tw"][:, 1] + np.sin(2 * np.pi * i / 256)).max() < 1e-7
    want = 2.0 ** ((np.arange(64) - 3) / 2.0 - 0.25)
    assert np.abs(t["thr"] / want - 1).max() < 1e-6
    assert t["thr"][15] < 64.0 < t["thr"][16]   # the smallest amplitude kept (8.0) has AmpSf 15
    # the normalisers: 1 / 64 away from the ends (the Hann window sums to 128, sin^2 averages a half), far from it next to them
    assert np.abs(t["rs"][16:1009] * 64 - 1).max() < 0.01 and np.abs(t["rc"][16:1009] * 64 - 1).max() < 0.01
    assert t["rs"][1] > 10 / 64 and abs(t["rc"][1] * 128 - 1) < 0.05 and t["rs"][1023] > 10 / 64


@needs_clang
def test_symbols_and_prototypes():
    """the header declares the four entry points and the constants, the binding carries their prototypes, the library exports them"""
    B, path = _host_lib()
    hdr = open(os.path.join(ROOT, "include", "at3phip.h")).read()
    lib = B.load_library(path)
    for name in G.NEW_SYMBOLS:
        assert name + "(" in hdr and name in B.AT3P_SYMBOLS and hasattr(lib, name), name
    for macro in ("AT3PHIP_TONE_PEAK_RATIO 16.0", "AT3PHIP_TONE_MAX_BAND_WAVES 3", "AT3PHIP_TONE_FINE_SPAN 7", "AT3PHIP_TONE_MIN_AMP 8.0",
                  "AT3PHIP_TONE_FIND_TABLES_BYTES 28416"):
        assert "#define " + macro in hdr, macro
    assert B.AT3P_TONE_FIND_TABLES_DTYPE.itemsize == G.FIND_TABLES_DTYPE.itemsize == 28416


# ---- the kernels through the CPU SIMT harness ------------------------------------------------------------------------------------------
@needs_clang
def test_harness_driver_equals_the_restatement():
    """tools/emu/run_emu_at3p_gha.py under the strict harness: records, residuals and frames equal the restatement's, mono and
    stereo, in one call and in two, 16-bit input included, and the frame budget's frame - in ascending and in descending wavefront
    order, and with every device buffer ending at a guard page."""
    build_strict()
    modes = {"plain": {}, "reverse": {"EMU_ORDER": "reverse"}, "fence": {"EMU_FENCE": "high"}}
    runs = Children({m: ("run_emu_at3p_gha.py", ["--nobuild"], env) for m, env in modes.items()})
    try:
        for m in modes:
            out = runs.output(m)
            assert_clean(out, 2 * 5 + 2)
            assert "ends: bad 0; waves [" in out
            assert "waves kept 48" in out and out.count("analyse nch=") == 2
    finally:
        runs.close()


# ---- the host mirror -------------------------------------------------------------------------------------------------------------------
@needs_clang
def test_host_mirror_equals_the_restatement(tmp_path):
    """TAt3PToneAnalyser equals the restatement record for record and residual for residual; TAt3PEncoder around it, and
    TAt3PEncoder with the analysis on the device (here: the host-compiled kernels), write the frames the restatement's pipeline
    predicts. The stand-alone program tests/host/test_host_shim_at3p_gha.cpp, built against the harness library."""
    emu = build_strict()
    exe, data = str(tmp_path / "test_host_shim_at3p_gha"), str(tmp_path / "cases.bin")
    n = G.export_shim_cases(data, emu)[0][1]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "host", "test_host_shim_at3p_gha.cpp"), "-o", exe,
                           emu, f"-Wl,-rpath,{os.path.dirname(emu)}"])
    out = subprocess.run([exe, data], capture_output=True, text=True, env=dict(os.environ, EMU_STRICT="1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "HOST SHIM AT3P GHA TEST OK\n" in out.stdout, out.stdout
    assert out.stdout.count(f"{n} records compared, 0 differ; 0 residuals differ") == 2, out.stdout
    assert out.stdout.count(f"{n - 1} frames compared, 0 differ") == 8, out.stdout


# ---- the golden ----------------------------------------------------------------------------------------------------------------------------
def test_golden_records_and_frame_digests():
    """tests/golden/at3p_gha.npz (tools/gen_golden_at3p_gha.py): the restatement's records and the SHA-256 digests of its residuals
    and of its mono pipeline's frames for the stored signal names: the definition does not drift"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "at3p_gha.npz"))
    for key in [k[:-7] for k in g.files if k.endswith("_blocks")]:
        name, nch = key.rsplit("_", 1)
        pcm = G.signal_pcm(name, int(g["frames"]), int(nch))
        blocks, resid = G.CpuToneAnalyser(int(nch)).analyse(G.pqf_bands(pcm))
        assert blocks.tobytes() == g[key + "_blocks"].tobytes(), key
        assert hashlib.sha256(resid.tobytes()).hexdigest() == str(g[key + "_resid_sha256"]), key
        if int(nch) == 1:
            assert hashlib.sha256(G.pipeline(pcm)[0].tobytes()).hexdigest() == str(g[key + "_frames_sha256"]), key
