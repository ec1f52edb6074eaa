"""The gated ATRAC3plus tone analysis (include/at3phip.h, FINDING TONES, GATES G1-G5) without a GPU: the C restatement
tests/host/at3p_gha_cpu.c on crafted onsets and offsets, at the edges of G1's split range, on stationary signals, through the
restated writer and decoder; its records against the writer's contract; the host gate function and the host mirror's
TAt3PToneAnalyser with Gated against it (on the host-compiled kernels)."""
import os
import subprocess

import numpy as np
import pytest

import at3p_gha_lib as G
import at3p_tonal_lib as T
from simt_harness_lib import CLANG, ROOT, build_strict

needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")
NF = 14
EVENT_FRAME = 2            # the crafted event's frame; its block is T_1 = the record of slot 2 (frame 1, frame 2)


def _both(bands, nch):
    """((blocks, residual) with AT3PHIP_TONES_GATED, (blocks, residual) without)"""
    return G.CpuToneAnalyser(nch, True).analyse(bands), G.CpuToneAnalyser(nch, False).analyse(bands)


def _ungated_is_the_parent(name, bands, nch, ungated):
    """the restatement without the flag computes what the ungated restatement computed before the gates were merged into its
    file: the digests tests/golden/at3p_gha_flags.npz recorded from that file's own entry point"""
    G.assert_flag_digests(f"pg_{name}_{nch}_0", bands, ungated)


# ---- detection: fails on the parent ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("s0", [4, 16, 28])
def test_onset_gets_a_start_point_and_no_pre_echo(s0, nch):
    """Subbands 0, 7 and 15 hold a sine at frequency index 300 that is exactly zero before cell s0 of frame 2. With the flag the
    record G2 names (slot 2: the block of frames 1 and 2) carries start = s0 + 1 for those bands and there is no other point in
    the stream; every residual sample before the onset is the input's, bit for bit (+0.0f). Without the flag the blocks fade the
    sine in over samples that do not hold it: the residual there is not zero."""
    bands = G.onset_bands(s0, nch)
    (gb, gr), (ub, ur) = _both(bands, nch)
    _ungated_is_the_parent(f"onset{s0}", bands, nch, (ub, ur))
    want = {(ch, b): (s0 + 1, 0) for ch in range(nch) for b in G.GATE_BANDS}
    assert [G.points(r, nch) for r in gb] == [want if f == EVENT_FRAME else {} for f in range(6)]
    assert all(not G.points(r, nch) for r in ub)
    assert int(gb[EVENT_FRAME]["num_tone_bands"]) == 16
    # residual slot f is frame f - 1: everything up to frame 1, and frame 2 before sample 4 s0
    before_g = np.concatenate([gr[:EVENT_FRAME + 1].reshape(-1, nch, 16, 128).transpose(1, 2, 0, 3).reshape(nch, 16, -1), gr[EVENT_FRAME + 1][:, :, :4 * s0]], axis=2)
    before_u = np.concatenate([ur[:EVENT_FRAME + 1].reshape(-1, nch, 16, 128).transpose(1, 2, 0, 3).reshape(nch, 16, -1), ur[EVENT_FRAME + 1][:, :, :4 * s0]], axis=2)
    assert not before_g.view(np.uint32).any()
    for b in G.GATE_BANDS:
        assert np.abs(before_u[:, b]).max() > 1.0, (b, np.abs(before_u[:, b]).max())
    assert sum(G.n_waves(r) for r in gb[EVENT_FRAME + 1:]) > 0   # and the sine is found once it is there


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("p0", [3, 15, 27])
def test_offset_gets_a_stop_point_and_no_post_echo(p0, nch):
    """The mirrored signal: the same sine from the stream's start, switched off after cell p0 of frame 2. The record of slot 2
    carries stop = p0 + 1 for the three bands and there is no other point; every residual sample after the offset is the input's
    (+0.0f); without the flag it is not."""
    bands = G.offset_bands(p0, nch)
    (gb, gr), (ub, ur) = _both(bands, nch)
    _ungated_is_the_parent(f"offset{p0}", bands, nch, (ub, ur))
    want = {(ch, b): (0, p0 + 1) for ch in range(nch) for b in G.GATE_BANDS}
    assert [G.points(r, nch) for r in gb] == [want if f == EVENT_FRAME else {} for f in range(6)]
    after_g = [gr[EVENT_FRAME + 1][:, :, 4 * (p0 + 1):], gr[EVENT_FRAME + 2:]]
    after_u = [ur[EVENT_FRAME + 1][:, :, 4 * (p0 + 1):], ur[EVENT_FRAME + 2:]]
    assert not any(a.view(np.uint32).any() for a in after_g)
    assert max(np.abs(a).max() for a in after_u) > 1.0
    assert sum(G.n_waves(r) for r in gb[:EVENT_FRAME]) > 0


# ---- no event at the edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("s0", [3, 29])
def test_no_event_at_the_edges(s0, nch):
    """An onset at cell 3 or 29 lies outside G1's splits MIN .. 32 - MIN: no event, records and residual equal to the unflagged
    call's. Cell 3: one live cell among the four before split 4 keeps the ratio near 3. Cell 29: split 28 has before = 0.0 and
    after > 0, but cell 28, the first of the MIN cells the loud side must hold, is empty (G1's condition on the loud side's cells)."""
    bands = G.onset_bands(s0, nch)
    (gb, gr), (ub, ur) = _both(bands, nch)
    print(f"onset at cell {s0}: gates of frame 2 {G.cpu_gates(bands)[EVENT_FRAME].tolist()}; points {[G.points(r, nch) for r in gb]}")
    assert not G.cpu_gates(bands).any()
    assert gb.tobytes() == ub.tobytes() and np.array_equal(gr.view(np.uint32), ur.view(np.uint32))


# ---- stationary signals -------------------------------------------------------------------------------------------------------------------
@needs_clang
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("name", ["tones", "noise", "silence"])
def test_stationary_signals_are_untouched(name, nch):
    """14 frames: the flagged records, residuals and frames are byte-identical to the unflagged ones. A condition on R, met by
    16, 64 and 256 alike. (The first frame of `tones` is not stationary - the signal starts at sample 0 after the filter bank's zero
    history, and the bands without a tone ring down from that click within four cells - but only two of those cells are loud: a
    burst shorter than MIN cells is no event.)"""
    from atracdenc_amd.binding import At3pHip
    pcm = G.signal_pcm(name, NF, nch)
    bands = G.pqf_bands(pcm)
    (gb, gr), (ub, ur) = _both(bands, nch)
    gates = G.cpu_gates(bands)
    print(f"{name} x{nch}: gates fired {[(int(f), int(c), int(b), hex(int(gates[f, c, b]))) for f, c, b in np.argwhere(gates)]}; "
          f"waves equal {[G.band_waves(a, nch) == G.band_waves(b, nch) for a, b in zip(gb, ub)].count(True)}/{NF}; residuals equal {np.array_equal(gr.view(np.uint32), ur.view(np.uint32))}")
    enc = At3pHip(n_streams=1, max_frames=NF, channels=nch, lib_path=build_strict())
    try:
        write = lambda specs, recs: enc.write_frames(specs[None], None, recs[None])[0]
        frames = [G.pipeline(pcm, gated, False, write)[0] for gated in (True, False)]
    finally:
        enc.close()
    assert gb.tobytes() == ub.tobytes()
    assert np.array_equal(gr.view(np.uint32), ur.view(np.uint32))
    assert np.array_equal(frames[0], frames[1])


# ---- the round trip of the envelope -------------------------------------------------------------------------------------------------------
def _keyed_bands(on_cell, off_cell, start_on):
    """[6][1][16][128]: band 7 holds the index-300 sine, switched at two cells counted from frame 2's first (32 cells a frame):
    start_on: on from the start, off after off_cell, on again at on_cell; else off, on at on_cell, off after off_cell"""
    x = G._gate_sine(6)
    cell = np.arange(6 * 32).repeat(4) - 64
    live = (cell <= off_cell) | (cell >= on_cell) if start_on else (cell >= on_cell) & (cell <= off_cell)
    bands = np.zeros((6, 1, 16, 128), np.float32)
    bands[:, 0, 7] = (x * live).astype(np.float32).reshape(6, 128)
    return bands


ROUND_TRIP = {   # name: (bands, slot, the interval G3 states for band 7 of that slot's block)
    "onset in the second frame": (lambda: G.onset_bands(10, 1), 2, (32 + 10, 63)),
    "offset in the first frame": (lambda: G.offset_bands(20, 1), 3, (0, 20)),
    "onset in the first frame, offset in the second": (lambda: _keyed_bands(12, 32 + 9, False), 3, (12, 32 + 9)),
    "offset in the first frame, onset in the second": (lambda: _keyed_bands(32 + 14, 6, True), 3, (32 + 14, 63)),
}


@pytest.mark.parametrize("case", list(ROUND_TRIP))
def test_written_envelope_decodes_to_the_interval_the_analysis_used(case):
    """The flagged records, written by the restated writer (oracle writer, block spliced in), unpacked by the restated decoder: the
    curr_env ff_atrac3p_generate_tones reconstructs for every block and band is the interval [lo, hi] the analysis fitted and
    subtracted under, for the four combinations of G3 (the fourth is the one the syntax cannot hold: the decoder keeps the later
    interval, and so does the analysis). The frames decode without a rejection, and decoding adds back what was subtracted: the
    round trip of the gated stream is no worse than that of the ungated one."""
    make, slot, want = ROUND_TRIP[case]
    bands = make()
    ana = G.CpuToneAnalyser(1, True)
    blocks, resid = ana.analyse(bands)
    assert tuple(ana.intervals[slot, 0, 7]) == want, (case, ana.intervals[:, 0, 7].tolist())
    recs = G.writer_records(blocks)                       # frame f carries the block of slot f - 1
    frames = G.splice_blocks(G.write_residual(resid), recs, 1)
    _, _, rec, why = T.unpack_tonal(frames, 1)
    assert not why.any()
    got = G.decoder_intervals(rec, 1)
    assert np.array_equal(got[1:], ana.intervals[:-1]), (case, got[1:, 0, 7].tolist(), ana.intervals[:-1, 0, 7].tolist())
    pcm, rej = T.cpu_tonal_decode(frames, 1)
    assert rej.sum() == 0 and np.isfinite(pcm).all()


# ---- the records and the writer -------------------------------------------------------------------------------------------------------------
@needs_clang
@pytest.mark.parametrize("nch", [1, 2])
def test_flagged_records_pass_the_writers_validation(nch):
    """Every flagged record of `burst`, `mix` and `stress` (14 frames) and of the crafted cases passes at3phip_write_frames_tonal's
    host check (on the host-compiled library: the check needs no device); in mono the writer's frames are the oracle writer's with
    the block, points included, spliced in."""
    from atracdenc_amd.binding import At3pHip
    enc = At3pHip(n_streams=1, max_frames=NF, channels=nch, lib_path=build_strict())
    try:
        cases = {name: G.pqf_bands(G.signal_pcm(name, NF, nch)) for name in ("burst", "mix", "stress")}
        cases.update(G.crafted_cases(nch))
        for name, bands in cases.items():
            blocks, resid = G.CpuToneAnalyser(nch, True).analyse(bands)
            assert sum(len(G.points(b, nch)) for b in blocks) > 0, name
            got = enc.write_frames(G.residual_specs(resid)[None], None, blocks[None])[0]
            if nch == 1:
                assert np.array_equal(got, G.splice_blocks(G.write_residual(resid), blocks, 1)), name
    finally:
        enc.close()


@needs_clang
@pytest.mark.parametrize("nch", [1, 2])
def test_a_record_with_points_and_no_wave_writes_and_decodes(nch):
    """points only: valid for the writer (the library's and the restated one write the same frame in mono) and for the decoder,
    which adds nothing for it: the PCM is that of the frames without the block"""
    from atracdenc_amd.binding import At3pHip
    recs = np.zeros(3, G.BLOCK_DTYPE)
    recs["num_tone_bands"][1] = 6
    recs["band"]["start"][1, 0, 2] = 5
    recs["band"]["stop"][1, nch - 1, 5] = 32
    resid = G.pqf_bands(G.signal_pcm("mix", 3, nch, scale=0.02))   # (quiet: the block's bits cost the frame no quant unit)
    specs = G.residual_specs(resid)
    enc = At3pHip(n_streams=1, max_frames=3, channels=nch, lib_path=build_strict())
    try:
        frames = enc.write_frames(specs[None], None, recs[None])[0]
        plain = enc.write_frames(specs[None])[0]
    finally:
        enc.close()
    assert not np.array_equal(frames[1], plain[1]) and np.array_equal(frames[[0, 2]], plain[[0, 2]])
    if nch == 1:
        assert np.array_equal(frames, G.splice_blocks(G.write_residual(resid), recs, 1))
    _, _, rec, why = T.unpack_tonal(frames, nch)
    assert not why.any() and rec[1, 0] == 1 and list(rec[1, 1 + 2 * 6:1 + 3 * 6]) == [0, 0, 1, 4, 0, 32]
    pcm, rej = T.cpu_tonal_decode(frames, nch)
    want, _ = T.cpu_tonal_decode(plain, nch)
    assert rej.sum() == 0 and np.array_equal(pcm.view(np.uint32), want.view(np.uint32))


# ---- the host gate function, the symbols -------------------------------------------------------------------------------------------------------
@needs_clang
def test_host_gate_function_equals_the_restatement():
    from atracdenc_amd import binding as B
    path = build_strict()
    cases = [G.pqf_bands(G.signal_pcm(name, NF, 2)) for name in ("burst", "tones", "noise")] + list(G.crafted_cases(2).values()) + [G.onset_bands(29, 1)]
    fired = 0
    for bands in cases:
        got = B.at3p_host_tone_gates(bands, path)
        assert np.array_equal(got, G.cpu_gates(bands))
        fired += int(np.count_nonzero(got))
    assert fired >= 6 * 6   # at least the crafted cases' events: three bands of two channels in each of the six
    special = np.zeros((1, 1, 16, 128), np.float32)   # a NaN energy is no event; an infinite one after silence is an onset
    special[0, 0, 0, 64:] = np.nan
    special[0, 0, 1, 64:] = np.inf
    special[0, 0, 2, 64:] = 3.0e38                    # (squares overflow to infinity)
    got = B.at3p_host_tone_gates(special, path)
    # (every split up to cell 16 has d = infinity, so the first one, 4, stays the candidate, and cells 4 .. 7 are not loud)
    assert np.array_equal(got, G.cpu_gates(special)) and not got.any()
    special[0, 0, 1:3, 16:64] = special[0, 0, 1:3, 64:112]   # infinite from cell 4 on: an onset at 4
    got = B.at3p_host_tone_gates(special, path)
    assert np.array_equal(got, G.cpu_gates(special)) and got[0, 0, :4].tolist() == [0, 4, 4, 0]


@needs_clang
def test_symbols_and_prototypes():
    """the header declares the flag, the constants and the host-only symbol; the binding carries its prototype; the library exports it"""
    from atracdenc_amd import binding as B
    hdr = open(os.path.join(ROOT, "include", "at3phip.h")).read()
    lib = B.load_library(build_strict())
    assert "at3phip_host_tone_gates(" in hdr and "at3phip_host_tone_gates" in B.AT3P_SYMBOLS and hasattr(lib, "at3phip_host_tone_gates")
    for macro in ("AT3PHIP_TONES_GATED 32u", "AT3PHIP_TONE_GATE_MIN 4", "AT3PHIP_TONE_GATE_RATIO 16.0"):
        assert "#define " + macro in hdr, macro
    assert B.AT3PHIP_TONES_GATED == G.GATED == 32


# ---- call splits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
def test_any_split_into_calls_gives_the_same_bytes(nch):
    bands = G.pqf_bands(G.signal_pcm("burst", 8, nch))
    wb, wr = G.CpuToneAnalyser(nch, True).analyse(bands)
    for split in ((1,) * 8, (3, 1, 4), (7, 1)):
        ana, at, gb, gr = G.CpuToneAnalyser(nch, True), 0, [], []
        for n in split:
            b, r = ana.analyse(bands[at:at + n])
            gb.append(b)
            gr.append(r)
            at += n
        assert np.concatenate(gb).tobytes() == wb.tobytes() and np.concatenate(gr).tobytes() == wr.tobytes(), split


# ---- the host mirror --------------------------------------------------------------------------------------------------------------------------
@needs_clang
def test_host_mirror_with_gated_equals_the_restatement(tmp_path):
    """TAt3PToneAnalyser(channels, gated = true) equals the restatement record for record and residual for residual on keyed, burst
    and four crafted cases; TAt3PEncoder around it, and TAt3PEncoder with the gated analysis on the device (here: the host-compiled
    kernels), write the frames the restatement's pipeline predicts. The stand-alone program
    tests/host/test_host_shim_at3p_gha.cpp, built against the harness library."""
    emu = build_strict()
    exe, data = str(tmp_path / "test_host_shim_at3p_gha"), str(tmp_path / "cases.bin")
    cases = G.export_shim_cases(data, emu, "gated")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "host", "test_host_shim_at3p_gha.cpp"), "-o", exe,
                           emu, f"-Wl,-rpath,{os.path.dirname(emu)}"])
    out = subprocess.run([exe, data], capture_output=True, text=True, env=dict(os.environ, EMU_STRICT="1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "HOST SHIM AT3P GHA TEST OK\n" in out.stdout, out.stdout
    for nch, n, fl, with_pcm in cases:
        assert fl == G.GATED and f"channels {nch} flags {fl}: {n} records compared, 0 differ; 0 residuals differ" in out.stdout, out.stdout
    n = cases[0][1]
    assert out.stdout.count(f"{n - 1} frames compared, 0 differ") == 8, out.stdout
