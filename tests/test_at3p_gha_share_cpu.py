"""The ATRAC3plus tone analysis with shared bands (include/at3phip.h, FINDING TONES, SHARING S1-S5) without a GPU: the C restatement
tests/host/at3p_gha_cpu.c on the crafted twin bands, with one band that differs, with gates, where the budget does not bind
and in the round trip that measures the gain; its records against the writer's contract and the restated decoder; the kernels
through the CPU SIMT harness and the host mirror's TAt3PToneAnalyser with Shared against it (on the host-compiled kernels); the
flag, the symbol and the command line's argument check."""
import os
import subprocess

import numpy as np
import pytest

import at3p_gha_lib as G
import at3p_tonal_lib as T
from at3_testlib import _vp
from simt_harness_lib import CLANG, ROOT, Children, assert_clean, build_strict

needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")
NF = 14


def _unflagged_is_the_parent(name, bands, gated, got):
    """the restatement without AT3PHIP_TONES_SHARED computes what the unflagged (pg) or the gated (pgg) restatement computed before
    sharing was merged into its file: the digests tests/golden/at3p_gha_flags.npz recorded from those files' own entry points"""
    G.assert_flag_digests(f"pgg_{name}_2_{G.GATED}" if gated else f"pg_{name}_2_0", bands, got)


@pytest.mark.parametrize("key", [k for k, _, _ in G.flag_digest_cases() if k.startswith("pgs_")])
def test_every_flag_combination_is_the_layered_restatements(key):
    """CASES at 6 frames and the host mirror's four crafted gate cases under none, either and both of AT3PHIP_TONES_GATED and
    AT3PHIP_TONES_SHARED: records and residuals have the SHA-256 digests tests/golden/at3p_gha_flags.npz recorded from the shared
    restatement's entry point when the restatement was three files layered on each other
    (tools/gen_golden_at3p_gha.py flags)"""
    bands = {k: b for k, b, _ in G.flag_digest_cases()}[key]
    G.assert_flag_digests(key, bands)


# ---- 1: the budget -----------------------------------------------------------------------------------------------------------------------
def test_twin_bands_are_counted_and_written_once():
    """G.budget_bands(): the same three sines in all 16 bands of both channels. Without the flag 96 waves are found and 48 kept, two
    of every band's three in channel 0 and one in channel 1. With it every band is a twin: the record of slot 1 shares all 16
    bands, channel 1 is all zero, and channel 0 holds all three sines of every band, 48 waves; the writer emits the "all" code."""
    bands = G.budget_bands()
    ana = G.CpuToneAnalyser(2, shared=True)
    blocks, resid = ana.analyse(bands)
    plain = G.CpuToneAnalyser(2, shared=False)
    ub, ur = plain.analyse(bands)
    _unflagged_is_the_parent("budget_pair", bands, False, (ub, ur))
    assert ana.found[1] == plain.found[1] == 96 and G.n_waves(ub[1]) == 48 and int(ub[1]["tone_sharing"]) == 0
    rec = blocks[1]
    assert int(rec["tone_sharing"]) == 0xffff and int(rec["num_tone_bands"]) == 16 and int(rec["second_is_leader"]) == 0
    assert not rec["band"][1].tobytes().strip(b"\0")
    assert G.n_waves(rec) == 48
    waves = G.band_waves(rec, 2)
    for b in range(16):
        assert [w[0] for w in waves[0][b]] == list(G.BUDGET_FREQS) and waves[1][b] == [], b
    bits = T.tonal_bits(2, G.block_dict(rec, 2))
    assert bits[2:4] == [(1, 1), (0, 1)]   # after the amplitude mode and the band count: sharing present, all bands
    # S5: channel 1 subtracts channel 0's waves: the channels' input is the same, and so are their residuals
    assert np.array_equal(resid[:, 0].view(np.uint32), resid[:, 1].view(np.uint32))
    assert np.abs(resid[1]).max() > 0 and not np.array_equal(resid, ur)


# ---- 2: one band differs -----------------------------------------------------------------------------------------------------------------
def test_a_band_that_differs_is_not_shared():
    """The same input, but the sine at index 808 of channel 1's band 5 has amplitude 3750 instead of 2500 (2.3 AmpSf steps). Bit 5
    is clear and every other bit set; channel 1 holds band 5's three waves itself. The population of S3 is 48 + 3 = 51, so three
    go. By hand: the order is A2 descending, then channel, band, frequency index. The 3750 sine is first; then come the waves of
    amplitude 3000 and 2750 (17 each); last the 16 of amplitude 2500, all in channel 0 and of equal A2, ordered by band: ranks 35
    to 50. Ranks 48, 49 and 50 go: the index-808 waves of channel 0's bands 13, 14 and 15."""
    bands = G.budget_bands(2, differ=True)
    ana = G.CpuToneAnalyser(2, shared=True)
    blocks, _ = ana.analyse(bands)
    rec = blocks[1]
    assert ana.found[1] == 96
    assert int(rec["tone_sharing"]) == 0xffff & ~(1 << G.DIFFER_BAND) and int(rec["num_tone_bands"]) == 16
    waves = G.band_waves(rec, 2)
    for b in range(16):
        assert [w[0] for w in waves[0][b]] == list(G.BUDGET_FREQS[:2 if b >= 13 else 3]), b
        assert [w[0] for w in waves[1][b]] == (list(G.BUDGET_FREQS) if b == G.DIFFER_BAND else []), b
    assert G.n_waves(rec) == 48
    mine, theirs = waves[1][G.DIFFER_BAND], waves[0][G.DIFFER_BAND]
    assert mine[2][1] - theirs[2][1] >= 2, (mine, theirs)   # AmpSf of the changed sine
    for b in range(16):
        if b != G.DIFFER_BAND:
            assert not rec["band"][1, b].tobytes().strip(b"\0"), b


# ---- 3: gates with sharing ---------------------------------------------------------------------------------------------------------------
def test_gates_with_sharing():
    """GATED | SHARED. The same onset (cell 16 of frame 2, bands 0, 7 and 15) in both channels: the record of slot 2 shares every
    band and channel 0 carries the three start points, channel 1 none. The onset in channel 1 only, channel 0 holding the sine from
    the start: in slot 2 the three bands' point pairs differ, so they are not shared and channel 1 carries its own points; once
    both channels hold the sine alike (slot 4 on) the bands are shared again."""
    both = G.stereo_onset_bands(True)
    blocks, resid = G.CpuToneAnalyser(2, True, True).analyse(both)
    ub, ur = G.CpuToneAnalyser(2, True, False).analyse(both)
    _unflagged_is_the_parent("onset_both", both, True, (ub, ur))
    rec = blocks[2]
    assert G.points(ub[2], 2) == {(ch, b): (17, 0) for ch in range(2) for b in G.GATE_BANDS}
    assert G.points(rec, 2) == {(0, b): (17, 0) for b in G.GATE_BANDS}
    assert int(rec["tone_sharing"]) == 0xffff and int(rec["num_tone_bands"]) == 16
    assert all(int(b["tone_sharing"]) == (1 << int(b["num_tone_bands"])) - 1 for b in blocks)
    assert not blocks["band"][:, 1].tobytes().strip(b"\0")
    # the budget does not bind: the same synthesis in both channels, the residuals of the unflagged run bit for bit (no pre-echo included)
    assert np.array_equal(resid.view(np.uint32), ur.view(np.uint32))
    one = G.stereo_onset_bands(False)
    blocks, resid = G.CpuToneAnalyser(2, True, True).analyse(one)
    ub, ur = G.CpuToneAnalyser(2, True, False).analyse(one)
    rec = blocks[2]
    assert G.points(rec, 2) == {(1, b): (17, 0) for b in G.GATE_BANDS} == G.points(ub[2], 2)
    assert G.shared_bands(rec) == [b for b in range(16) if b not in G.GATE_BANDS]
    assert all(G.band_waves(rec, 2)[0][b] for b in G.GATE_BANDS)
    for slot in (4, 5):
        assert int(blocks[slot]["tone_sharing"]) == 0xffff and G.n_waves(blocks[slot]) == 3 and G.n_waves(ub[slot]) == 6, slot
    assert np.array_equal(resid.view(np.uint32), ur.view(np.uint32))


# ---- 4: lossless where the budget does not bind ------------------------------------------------------------------------------------------
@needs_clang
def test_sharing_is_lossless_where_the_budget_does_not_bind():
    """`tones` at scale 0.05, channel 0 in both channels, 14 frames: 8 waves per channel, far below the budget. The records with and
    without the flag describe the same synthesis: equal residuals, and through the restatement pipeline (the library's writer, which
    prices the block) every frame keeps the same number of quant units, the restated decoder's PCM is bit-identical, and every
    flagged tonal block is shorter."""
    from atracdenc_amd.binding import At3pHip
    pcm = G.twin_pcm("tones", NF, 0.05)
    enc = At3pHip(n_streams=1, max_frames=NF, channels=2, lib_path=build_strict())
    try:
        write = lambda specs, recs: enc.write_frames(specs[None], None, recs[None])[0]
        (fs, bs, rs), (fu, bu, ru) = (G.pipeline(pcm, False, shared, write) for shared in (True, False))
    finally:
        enc.close()
    assert max(G.n_waves(b) for b in bu) == 16 and max(G.n_waves(b) for b in bs) == 8
    assert np.array_equal(rs.view(np.uint32), ru.view(np.uint32))
    nq = [(T.n_qu(a), T.n_qu(b)) for a, b in zip(fs, fu)]
    print("quant units (shared, unflagged) per frame:", nq)
    assert all(a == b for a, b in nq), nq
    ps, rej_s = T.cpu_tonal_decode(fs, 2)
    pu, rej_u = T.cpu_tonal_decode(fu, 2)
    assert rej_s.sum() == 0 and rej_u.sum() == 0
    assert np.array_equal(ps.view(np.uint32), pu.view(np.uint32))
    bits = [(G.block_bits(a, 2), G.block_bits(b, 2)) for a, b in zip(bs, bu)]
    print("tonal block bits (shared, unflagged) per record:", bits)
    assert all(a < b for a, b in bits if b) and sum(b > 0 for _, b in bits) >= NF - 1
    assert (fs != fu).any()


# ---- 5: the round trip -------------------------------------------------------------------------------------------------------------------
def _round_trip(pcm, shared):
    """(SNR of channel 0, of channel 1, mean waves per record, mean distinct waves per record): restatement, at3pt_apply_filter, oracle
    MDCT and writer, splice_tonal, cpu_tonal_decode, as test_at3p_gha_cpu._round_trip does for mono"""
    n = pcm.shape[0]
    bands = G.pqf_bands(np.concatenate([pcm, np.zeros((1, 2048, 2), np.float32)]))   # and the flushing frame
    blocks, resid = G.CpuToneAnalyser(2, shared=shared).analyse(bands)
    tones = list(blocks[1:])
    lib = T.tonal_lib()
    st = np.zeros(lib.at3pt_filter_bytes(), np.uint8)
    filt = np.ascontiguousarray(np.concatenate([np.zeros((1, 2, 2048), np.float32), bands[:n].reshape(n, 2, 2048)]))
    for j, rec in enumerate(blocks):
        lib.at3pt_apply_filter(_vp(st), 2, _vp(G.rec_ints(rec, 2)), _vp(filt[j]))
    assert np.array_equal(filt.view(np.uint32), resid.reshape(n + 1, 2, 2048).view(np.uint32))   # the restatement's residual is ApplyFilter's
    base = G.write_residual(resid[1:])
    recs = [tones[j - 1] if j >= 1 else None for j in range(n)]
    out, rej = T.cpu_tonal_decode(G.splice_blocks(base, recs, 2), 2)
    assert rej.sum() == 0
    snr = [G.snr_db(pcm[:, :, c].reshape(-1), out[:, :, c].reshape(-1), n) for c in range(2)]
    return snr[0], snr[1], float(np.mean([G.n_waves(b) for b in tones])), float(np.mean([len({(b_, w) for ch in G.band_waves(r, 2) for b_, ws in enumerate(ch) for w in ws}) for r in tones]))


# Measured with the restatement (the issue's emulation - a mono analysis, channel 1 sharing every band - in brackets):
#   10 subbands x 3 sines, amplitude 0.02, both channels alike, 14 frames:
#   unflagged 31.18 dB in both channels (31.18), 48 waves per record of the 60 found; shared 50.02 dB (50.02), 30 waves per record
def test_round_trip_gains_where_every_band_is_a_twin():
    """G.dense_pcm: today the budget keeps two of every band's three sines in each channel and the third dominates the error; shared,
    every sine is coded once and both channels get it. The floor is half the measured gain, the proportion the round-trip floors of
    test_at3p_gha_cpu.py keep."""
    pcm = G.dense_pcm(NF)
    plain = _round_trip(pcm, False)
    shared = _round_trip(pcm, True)
    print(f"round trip dense: unflagged {plain[0]:.2f} / {plain[1]:.2f} dB, {plain[2]:.2f} waves per record ({plain[3]:.2f} distinct); "
          f"shared {shared[0]:.2f} / {shared[1]:.2f} dB, {shared[2]:.2f} waves per record")
    for c in range(2):
        assert shared[c] >= plain[c] + 10.0, (c, plain, shared)


# ---- 6: the kernels through the CPU SIMT harness -----------------------------------------------------------------------------------------
@needs_clang
def test_harness_driver_equals_the_shared_restatement():
    """tools/emu/run_emu_at3p_gha.py shared under the strict harness: records and residuals of 2 streams x 4 slots stereo (stream 0: case
    2, stream 1: case 3) with GATED | SHARED and with SHARED alone, in one call and split 1 + 3, and of one mono stream with the
    flag against the run without it, equal the restatement's as bit patterns - in ascending and in descending wavefront order, and
    with every device buffer ending at a guard page."""
    build_strict()
    modes = {"plain": {}, "reverse": {"EMU_ORDER": "reverse"}, "fence": {"EMU_FENCE": "high"}}
    runs = Children({m: ("run_emu_at3p_gha.py", ["shared", "--nobuild"], env) for m, env in modes.items()})
    try:
        for m in modes:
            out = runs.output(m)
            assert_clean(out, 2 * 2 * 2 * 2 + 2)
            assert out.count("stream 0") == 4 and out.count("stream 1") == 4 and out.count("mono") == 1
            assert out.count("sharing ['0xffdf', '0xffdf', '0xffdf', '0xffdf']") == 4   # case 2: bit 5 clear
            assert out.count("sharing ['0x7f7e', '0x7f7e', '0x7f7e', '0xffff']") == 2   # case 3, the onset in channel 1 only: bands 0, 7, 15
    finally:
        runs.close()


# ---- 7: the host mirror ------------------------------------------------------------------------------------------------------------------
def _run_shim(tmp_path, extra_flags=()):
    emu = build_strict()
    exe, data = str(tmp_path / "test_host_shim_at3p_gha"), str(tmp_path / "cases.bin")
    cases = G.export_shim_cases(data, emu, "shared")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *extra_flags, os.path.join(ROOT, "tests", "host", "test_host_shim_at3p_gha.cpp"), "-o", exe,
                           emu, f"-Wl,-rpath,{os.path.dirname(emu)}"])
    out = subprocess.run([exe, data], capture_output=True, text=True, env=dict(os.environ, EMU_STRICT="1"))
    return cases, out


@needs_clang
def test_host_mirror_with_shared_equals_the_restatement(tmp_path):
    """TAt3PToneAnalyser(channels, gated, shared = true) equals the restatement record for record and residual for residual on twin
    `tones`, twin `burst` with gates, mono `tones` and the four crafted cases; TAt3PEncoder around it, and TAt3PEncoder with the
    shared analysis on the device (here: the host-compiled kernels), write the frames the restatement's pipeline predicts. The
    stand-alone program tests/host/test_host_shim_at3p_gha.cpp, built against the harness library."""
    cases, out = _run_shim(tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "HOST SHIM AT3P GHA TEST OK\n" in out.stdout, out.stdout
    for nch, n, fl, with_pcm in cases:
        assert f"channels {nch} flags {fl}: {n} records compared, 0 differ; 0 residuals differ" in out.stdout, out.stdout
    n = cases[0][1]
    assert out.stdout.count(f"{n - 1} frames compared, 0 differ") == 3 * 4, out.stdout
    assert "flags understood 96" in out.stdout


# ---- 8: validation and decode ------------------------------------------------------------------------------------------------------------
@needs_clang
def test_flagged_records_pass_the_writers_validation_and_decode():
    """Every flagged record of the crafted cases and of twin `burst`, `mix` and `tones` passes at3phip_write_frames_tonal's host
    check (on the host-compiled library: the check needs no device) - the record path k_at3p_write_tonal reads from device memory
    needs nothing new - and the frames decode with zero rejections, the sharing flags read back as written."""
    from atracdenc_amd.binding import At3pHip
    enc = At3pHip(n_streams=1, max_frames=NF, channels=2, lib_path=build_strict())
    try:
        cases = {name: (make(6), gated) for name, (make, gated) in G.CASES.items()}
        cases.update({name: (G.pqf_bands(G.twin_pcm(name, NF, 0.05)), name == "burst") for name in ("burst", "mix", "tones")})
        shared = 0
        for name, (bands, gated) in cases.items():
            blocks, resid = G.CpuToneAnalyser(2, gated, True).analyse(bands)
            shared += sum(len(G.shared_bands(b)) for b in blocks)
            frames = enc.write_frames(G.residual_specs(resid)[None], None, blocks[None])[0]
            _, _, rec, why = T.unpack_tonal(frames, 2)
            assert not why.any(), (name, why)
            for f, b in enumerate(blocks):
                assert _same_record(rec[f], b), (name, f)
            pcm, rej = T.cpu_tonal_decode(frames, 2)
            assert rej.sum() == 0 and np.isfinite(pcm).all(), name
        assert shared > 100
    finally:
        enc.close()


def _same_record(got, rec):
    """the unpacked record against the written one, the shared bands of channel 1 being channel 0's: counts, points and waves of
    every band below num_tone_bands (a band's start index is the decoder's own business)"""
    want, nb = G.rec_ints(rec, 2), int(rec["num_tone_bands"])
    if got[0] != (nb != 0):
        return False
    for k in [16 * ch + b for ch in range(2) for b in range(nb)]:
        g, w = got[1 + 6 * k:7 + 6 * k], want[1 + 6 * k:7 + 6 * k]
        if g[0] != w[0] or list(g[2:]) != list(w[2:]):
            return False
        for i in range(int(g[0])):
            if any(got[193 + 48 * j + g[1] + i] != want[193 + 48 * j + w[1] + i] for j in range(3)):
                return False
    return True


# ---- 9: the interface --------------------------------------------------------------------------------------------------------------------
@needs_clang
def test_flag_symbol_and_prototypes():
    """the header declares the flag and the capability symbol; the binding carries its prototype and the shared= arguments; the
    library exports it and answers with both analysis flags"""
    import inspect
    from atracdenc_amd import binding as B
    hdr = open(os.path.join(ROOT, "include", "at3phip.h")).read()
    path = build_strict()
    lib = B.load_library(path)
    assert "uint32_t at3phip_host_tone_flags(void);" in hdr and "at3phip_host_tone_flags" in B.AT3P_SYMBOLS and hasattr(lib, "at3phip_host_tone_flags")
    assert "#define AT3PHIP_TONES_SHARED 64u" in hdr and B.AT3PHIP_TONES_SHARED == G.SHARED == 64
    assert B.at3p_host_tone_flags(path) == G.GATED | G.SHARED
    for name in ("analyse_tones", "analyse_tones_device", "encode_frames_tonal", "encode_frames_tonal_s16", "encode_frames_tonal_device", "encode_frames_tonal_device_s16"):
        p = inspect.signature(getattr(B.At3pHip, name)).parameters
        assert p["shared"].default is False and p["gated"].default is False, name


def test_cli_refuses_share_without_tones(tmp_path):
    """at3hipenc --share without --tones is a usage error, like --gate: the argument check runs before anything touches a device"""
    from atracdenc_amd import binding as B
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "at3hipenc")
    if not os.path.exists(exe):   # (built by __graft_entry__.build(); the same recipe here)
        if not os.path.exists(B.LIB_PATH):
            B.build_library()
        libdir, exe = os.path.dirname(B.LIB_PATH), str(tmp_path / "at3hipenc")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "atracdenc_amd", "host", "at3hipenc.cpp"), "-o", exe,
                               f"-L{libdir}", "-lat3hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    wav = str(tmp_path / "in.wav")
    import wave
    with wave.open(wav, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(np.zeros((2048, 2), "<i2").tobytes())
    r = subprocess.run([exe, "-e", "atrac3plus", "-i", wav, "-o", str(tmp_path / "bad.oma"), "--nostdout", "--share"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--share" in r.stdout + r.stderr and not os.path.exists(str(tmp_path / "bad.oma"))
