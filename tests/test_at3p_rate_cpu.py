"""ATRAC3plus at frame sizes other than 2048 bytes (include/at3phip.h, FRAME SIZE) without a GPU: the restatement
tests/host/at3p_writer_cpu.c against what the older restatements gave at 2048 bytes before they were folded into it
(tests/golden/at3p_writer_fold.npz); at3phip_host_allocate_sized against it; the two
smallest admissible sizes derived from the tables; every frame it writes at every size parsed, counted and decoded; the round trip
per standard bitrate; the kernels through the CPU SIMT harness against it; a build without the adaptive writer; the containers'
bytes and the command line's refusals."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import at3p_writer_lib as W
import at3p_decode_lib as D
import at3p_gha_lib as G
import at3p_tonal_lib as T
import at3p_tonal_write_lib as TW
from simt_harness_lib import CLANG, ROOT, Children, assert_clean, build_strict, run_alloc_modes

needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")
NF = W.SNR_FRAMES
HEADER = open(os.path.join(ROOT, "include", "at3phip.h")).read()

_specs = {}


def _sp(name, nch):
    if (name, nch) not in _specs:
        _specs[(name, nch)] = W.specs_of(name, nch, NF)
    return _specs[(name, nch)]


# ---- the new restatement against the two old ones at 2048 bytes --------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
def test_restatement_equals_the_old_ones_at_2048_bytes(nch):
    """tests/golden/at3p_writer_fold.npz holds, as SHA-256, what the restatements gave while each stated the writer and the decoder
    for itself (at3p_alloc_cpu.c, at3p_rate_cpu.c; at3p_decode_cpu.c without tones, at3p_tonal_cpu.c with them), all equal then.
    frames: on the signals, silence, full-scale noise, non-finite spectra, window flags and tonal records; PCM and rejection
    counters: of the at3pd_*, at3pt_* and at3pw_* entry points on those frames, on frames with flipped bits and on the crafted
    malformed frames of at3p_decode_lib"""
    gold = W.fold_golden(nch)
    cases = [(W.specs_of(n, nch, 4), None, None) for n in W.SIGNALS + ("silence", "fullscale")]
    cases.append((W.odd_specs(nch, 3), None, None))
    cases.append((W.specs_of("noise", nch, 2), np.array([[0x01ef] * nch, [0xffff] * nch], np.uint16), None))
    cases.append((np.concatenate([W.full_scale_noise(2, nch), _sp("mix", nch)[:1]]), None,
                  [TW.largest_block(nch), None, TW.case_blocks(f"small_{nch}")[0][0]]))

    def same(label, *got):
        assert np.array_equal(W.sha(*got), gold[label]), label

    rng = np.random.default_rng(11)
    for i, (sp, win, blocks) in enumerate(cases):
        new = W.write_adaptive(sp, 2048, False, win, blocks)
        same(f"a{i}_2048_frames", new)
        flipped = D.mutate_frames(new, rng, n_flips=2)
        same(f"a{i}_2048_flipped_in", flipped)
        for kind, frames in (("plain", new), ("flipped", flipped)):
            for tones in (False, True):
                a, ra = T.cpu_tonal_decode(frames, nch, tones=tones)
                b, rb = W.decode(frames, nch, tones)
                same(f"a{i}_2048_{kind}_tones{int(tones)}", a.view(np.uint32), ra)
                same(f"a{i}_2048_{kind}_tones{int(tones)}", b.view(np.uint32), rb)
            a, ra = D.cpu_decode(frames, nch)
            same(f"a{i}_2048_{kind}_tones0", a.view(np.uint32), ra)
    crafted, _ = D.crafted_frames(nch, 3)
    same("b_in", crafted)
    a, ra = D.cpu_decode(crafted, nch)
    b, rb = W.decode(crafted, nch, False)
    assert (ra[[0, 1, 2, 3, 4, 5]] > 0).all()
    same("b_tones0", a.view(np.uint32), ra)
    same("b_tones0", b.view(np.uint32), rb)
    a, ra = T.cpu_tonal_decode(crafted, nch, tones=True)
    b, rb = W.decode(crafted, nch, True)
    same("b_tones1", a.view(np.uint32), ra)
    same("b_tones1", b.view(np.uint32), rb)
    # the fields of every frame, accepted or not
    _, _, fo = D.unpack(crafted, nch)
    _, _, fn = W.unpack(crafted, nch)
    same("b_fields0", fo.view(np.uint8))
    same("b_fields0", fn.view(np.uint8))


# ---- at3phip_host_allocate_sized ---------------------------------------------------------------------------------------------------
def _budgets(nch):
    return (W.MIN_BYTES[nch], 376, 2048)


@needs_clang
def test_host_allocate_sized_equals_the_restatement_on_the_signals():
    from atracdenc_amd import binding as B
    path = build_strict()
    n = 0
    for name in W.SIGNALS + ("silence", "fullscale"):
        for nch in (1, 2):
            sp = W.specs_of(name, nch, 4)
            for f in (0, 3):
                sfi, bits, _ = W.cost_table(sp[f])
                for fb in _budgets(nch):
                    for tail in (8, 700, W.worst_tail(nch)):
                        wl, N, t, k, _ = W.allocate(sfi, bits, tail, fb)
                        gwl, gN, gt, gk = B.at3p_host_allocate(sfi, bits, tail, path, frame_bytes=fb)
                        assert (gN, gt, gk) == (N, t, k) and np.array_equal(gwl, wl), (name, nch, f, fb, tail)
                        n += 1
    assert n == 7 * 2 * 2 * 3 * 3


@needs_clang
def test_host_allocate_sized_equals_the_restatement_on_random_tables():
    """1000 seeded tables per budget (the channel count's smallest size, 376, 2048), non-monotone ones among them as
    tests/test_at3p_alloc_cpu.py builds them; at3phip_host_allocate is the sized call at 2048, and the old restatement's too"""
    from atracdenc_amd import binding as B
    path = build_strict()
    tables = W.random_cost_tables()
    nonmono = sum(bool((np.diff(b[:, :, 1:].astype(np.int64), axis=2) < 0).any()) for _, b, _ in tables)
    assert len(tables) == 1000 and nonmono >= 500
    differ = 0
    for i, (sfi, bits, tail) in enumerate(tables):
        nch = sfi.shape[0]
        got = {}
        for fb in _budgets(nch):
            tb = min(tail, 8 * fb - 3)
            wl, N, t, k, _ = W.allocate(sfi, bits, tb, fb)
            gwl, gN, gt, gk = B.at3p_host_allocate(sfi, bits, tb, path, frame_bytes=fb)
            assert (gN, gt, gk) == (N, t, k) and np.array_equal(gwl, wl), (i, fb)
            got[fb] = (gwl, gN, gt, gk)
        pwl, pN, pt, pk = B.at3p_host_allocate(sfi, bits, tail, path)
        assert (pN, pt, pk) == got[2048][1:] and np.array_equal(pwl, got[2048][0]), i
        owl, oN, ot, ok, _ = W.allocate(sfi, bits, tail)
        assert (oN, ot, ok) == got[2048][1:] and np.array_equal(owl, got[2048][0]), i
        differ += got[376][1:] != got[2048][1:]
    assert differ >= 500, differ   # (the budget matters on these tables)


@needs_clang
def test_host_allocate_sized_refuses_what_is_not_admissible():
    from atracdenc_amd import binding as B
    path = build_strict()
    sfi, bits, _ = W.cost_table(_sp("mix", 2)[0])
    for fb in (0, 7, 2056, W.MIN_BYTES[2] - 8, 380):
        with pytest.raises(B.At3HipError):
            B.at3p_host_allocate(sfi, bits, 8, path, frame_bytes=fb)
    with pytest.raises(B.At3HipError):
        B.at3p_host_allocate(sfi, bits, 8 * 376 - 2, path, frame_bytes=376)     # a tail beyond the budget
    B.at3p_host_allocate(sfi[:1], bits[:1], 8, path, frame_bytes=W.MIN_BYTES[1])   # (mono's minimum is below stereo's)
    with pytest.raises(B.At3HipError):
        B.at3p_host_allocate(sfi, bits, 8, path, frame_bytes=W.MIN_BYTES[1])


# ---- the smallest admissible sizes -------------------------------------------------------------------------------------------------
def test_min_frame_bytes_follow_from_the_tables():
    """front of A(63, 0) at its worst + the tail at its worst <= 8 * bytes - 3, smallest multiple of 8: the header's constants, its
    figures, the binding's constants and this module's"""
    from atracdenc_amd import binding as B
    assert (W.worst_front_one_unit(1), W.worst_tail(1), W.worst_front_one_unit(2), W.worst_tail(2)) == (77, 1320, 147, 1624)
    for nch, macro in ((1, "AT3PHIP_MIN_FRAME_BYTES_MONO"), (2, "AT3PHIP_MIN_FRAME_BYTES_STEREO")):
        m = W.min_frame_bytes(nch)
        need = W.worst_front_one_unit(nch) + W.worst_tail(nch)
        assert m % 8 == 0 and need <= 8 * m - 3 and need > 8 * (m - 8) - 3
        assert int(re.search(rf"#define {macro} (\d+)", HEADER).group(1)) == m == W.MIN_BYTES[nch] == getattr(B, macro)
    for fig in ("77 bits in mono, 147 in stereo", "1320 bits\n * in mono, 1624 in stereo", "77 + 1320 = 1397", "147 + 1624 = 1771"):
        assert fig in HEADER, fig
    # every size of the command line's table is admissible for the channel counts it serves
    assert all(fb >= W.MIN_BYTES[2] or kb == 32 for kb, fb in W.BITRATES.items()) and W.BITRATES[32] >= W.MIN_BYTES[1]


@pytest.mark.parametrize("nch", [1, 2])
def test_largest_record_on_full_scale_fits_the_smallest_frame(nch):
    """48 waves, both envelope points everywhere, (in stereo) the long sharing form, on full-scale noise, at the smallest
    admissible size: t* = 63 is never needed past its definition, the frame fits, decodes with its tones, and the record is
    found again field for field"""
    fb, big = W.MIN_BYTES[nch], TW.largest_block(nch)
    sp = W.full_scale_noise(2, nch)
    frames, rec, _ = W.write_adaptive(sp, fb, blocks=[big, big], info=True)
    tail = sum(n for _, n in W.tail_bits_list(nch, None, big))
    assert tail > 1000 and (rec["bits"] <= 8 * fb - 3).all() and (rec["t"] <= W.T_MAX).all()
    pcm, rej = W.decode(frames, nch, True)
    assert rej.sum() == 0, rej
    for f in range(2):
        assert W.terminator_pos(frames[f]) == 3 + rec["bits"][f] - 1 < 8 * fb
    padded = np.zeros((2, 2048), np.uint8)
    padded[:, :fb] = frames
    specs, win, recs, why = T.unpack_tonal(padded, nch)
    assert (why == 0).all() and all(TW.record_fields(recs[f]) == TW.expected_fields(nch, big) for f in range(2))


# ---- every frame at every size -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("name", W.SIGNALS)
def test_frames_parse_count_and_decode_at_every_size(name, nch):
    """14 frames of each signal at every test size: the independent head parser of at3p_writer_lib reads N outside 29..31 and word
    lengths 1..7; Bits(A), recounted from the parsed fields, is the restatement's figure and at most 8 * frame_bytes - 3; the
    terminator sits where the count says; the decoder restatement rejects no frame"""
    sp = _sp(name, nch)
    tail = sum(n for _, n in W.tail_bits_list(nch))
    costs = [W.cost_table(sp[f])[1] for f in range(NF)]
    for fb in W.SIZES[nch]:
        frames, rec, _ = W.write_adaptive(sp, fb, info=True)
        assert frames.shape == (NF, fb)
        assert W.decode(frames, nch)[1].sum() == 0
        for f in range(NF):
            p = W.parse_head(frames[f], nch)
            assert p["N"] not in (29, 30, 31) and p["N"] == rec["num_quant_units"][f]
            assert all(1 <= w <= 7 for row in p["wl"] for w in row)
            total, _ = W.recount_bits(p, nch, costs[f], tail)
            assert total == rec["bits"][f] <= 8 * fb - 3, (fb, f, total)
            assert W.terminator_pos(frames[f]) == 3 + total - 1 < 8 * fb


# ---- round trip per standard bitrate -------------------------------------------------------------------------------------------------
# dB per channel, encoder restatement then decoder restatement, 14 frames of at3p_gha_lib.signal_pcm at delay 2416 (DESIGN.md
# section 20 lists them; the 2048 column is section 19's). The restatement is deterministic: a cell is held at its recorded value
# minus 0.05 dB, which is the table's rounding and nothing else.
SNR = {
    ("noise", 1): {192: [0.23], 280: [0.38], 376: [4.89], 560: [9.65], 744: [14.20], 936: [18.11], 1120: [22.41], 1488: [29.97], 1864: [29.97],
                   2048: [29.97]},
    ("noise", 2): {280: [0.06, 0.06], 376: [0.06, 0.06], 560: [0.61, 0.62], 744: [4.81, 4.90], 936: [7.50, 7.30], 1120: [9.70, 9.67],
                   1488: [14.26, 14.15], 1864: [18.17, 18.19], 2048: [19.98, 20.04]},
    ("mix", 1): {192: [3.71], 280: [3.80], 376: [8.12], 560: [13.04], 744: [17.23], 936: [20.81], 1120: [23.80], 1488: [26.63], 1864: [26.63],
                 2048: [26.63]},
    ("mix", 2): {280: [3.72, 2.43], 376: [3.72, 2.43], 560: [3.72, 2.43], 744: [8.02, 7.00], 936: [10.89, 9.13], 1120: [13.30, 11.76],
                 1488: [17.49, 16.02], 1864: [20.79, 19.99], 2048: [22.39, 21.52]},
    ("stress", 1): {192: [6.39], 280: [8.30], 376: [8.44], 560: [18.06], 744: [22.64], 936: [26.32], 1120: [28.62], 1488: [30.29], 1864: [30.36],
                    2048: [30.36]},
    ("stress", 2): {280: [6.00, 5.80], 376: [6.35, 6.22], 560: [6.70, 6.56], 744: [8.81, 8.69], 936: [15.32, 15.30], 1120: [18.36, 18.54],
                    1488: [22.94, 23.18], 1864: [26.51, 27.09], 2048: [27.79, 28.16]},
    ("tones", 1): {192: [28.23], 280: [30.17], 376: [30.17], 560: [30.17], 744: [30.17], 936: [30.17], 1120: [30.17], 1488: [30.17], 1864: [30.17],
                   2048: [30.17]},
    ("tones", 2): {280: [19.45, 19.70], 376: [28.43, 28.10], 560: [30.17, 29.88], 744: [30.17, 29.88], 936: [30.17, 29.88], 1120: [30.17, 29.88],
                   1488: [30.17, 29.88], 1864: [30.17, 29.88], 2048: [30.17, 29.88]},
    ("burst", 1): {192: [25.16], 280: [25.66], 376: [25.86], 560: [25.98], 744: [26.12], 936: [26.16], 1120: [26.16], 1488: [26.17], 1864: [26.17],
                   2048: [26.17]},
    ("burst", 2): {280: [24.53, 23.48], 376: [25.23, 24.77], 560: [25.69, 25.40], 744: [25.90, 25.72], 936: [25.97, 25.84], 1120: [25.99, 25.88],
                   1488: [26.14, 26.10], 1864: [26.16, 26.15], 2048: [26.16, 26.16]},
}
# DESIGN.md section 19's adaptive column: the 2048-byte cells must equal it to 0.01 dB
SECTION_19 = {("noise", 1): [29.97], ("noise", 2): [19.98, 20.04], ("mix", 1): [26.63], ("mix", 2): [22.39, 21.52], ("stress", 1): [30.36],
              ("stress", 2): [27.79, 28.16], ("tones", 1): [30.17], ("tones", 2): [30.17, 29.88], ("burst", 1): [26.17], ("burst", 2): [26.16, 26.16]}


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("name", W.SIGNALS)
def test_round_trip_snr_per_bitrate(name, nch):
    sp, x = _sp(name, nch), G.signal_pcm(name, NF, nch)
    row = {}
    for kbit, fb in W.BITRATES.items():
        if fb < W.MIN_BYTES[nch]:
            continue     # 32 kbit/s is a mono rate
        frames, rec, _ = W.write_adaptive(sp, fb, info=True)
        y, rej = W.decode(frames, nch)
        assert rej.sum() == 0
        row[fb] = [G.snr_db(x[:, :, c].reshape(-1), y[:, :, c].reshape(-1), NF) for c in range(nch)]
        print(f"round trip {name} x{nch} {kbit} kbit/s ({fb} bytes): {' / '.join(f'{v:.2f}' for v in row[fb])} dB, mean bits {rec['bits'].mean():.0f} "
              f"of {8 * fb - 3}, units {rec['num_quant_units'].min()}..{rec['num_quant_units'].max()}")
    assert sorted(row) == sorted(SNR[(name, nch)])
    for fb, got in row.items():
        for c in range(nch):
            assert got[c] >= SNR[(name, nch)][fb][c] - 0.05, (name, nch, fb, c, got[c])
    for c in range(nch):
        assert abs(row[2048][c] - SECTION_19[(name, nch)][c]) <= 0.01, (name, nch, c, row[2048][c])
        assert SNR[(name, nch)][2048][c] == SECTION_19[(name, nch)][c]
    # what DESIGN.md section 20 reports: no cell of the table falls as the frame grows
    sizes = sorted(row)
    print(f"non-decreasing in frame size, {name} x{nch}: {all(row[a][c] <= row[b][c] + 1e-9 for a, b in zip(sizes, sizes[1:]) for c in range(nch))}")


def test_design_lists_the_round_trip_table():
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = doc[doc.index("## 20."):]
    for (name, nch), row in SNR.items():
        for fb, cells in row.items():
            assert " / ".join(f"{v:.2f}" for v in cells) in sec, (name, nch, fb)


# ---- the kernels through the CPU SIMT harness ----------------------------------------------------------------------------------------
@needs_clang
def test_harness_driver_equals_the_restatement():
    """tools/emu/run_emu_at3p_rate.py under the strict harness: both adaptive kernels and the decoder's kernels at the smallest size,
    376 and 2040 bytes, stereo and mono, on `mix`, silence, full-scale noise, the largest tonal record and non-finite spectra, in
    ascending and descending wavefront order and with a guard page directly behind (and directly before) every [S][F][frame_bytes]
    buffer: the check that no store or load still assumes 2048 bytes. Under a lazy, seeded stream schedule (and once in program
    order), at 376 bytes: a queued at3phip_encode_frames, a queued at3phip_encode_frames_tonal and a queued at3phip_decode at 2048
    bytes, each followed by its context's setter and a queued call at 376 - both adaptive kernels, the tone analysis and all three
    decoder kernels, and the wait in both setters."""
    build_strict()
    jobs = {"plain": ("run_emu_at3p_rate.py", ["--nobuild"], {}), "reverse": ("run_emu_at3p_rate.py", ["--nobuild"], {"EMU_ORDER": "reverse"}),
            "fence": ("run_emu_at3p_rate.py", ["--nobuild"], {"EMU_FENCE": "high"}),
            "fence_low": ("run_emu_at3p_rate.py", ["--nobuild", "signals", "tonal"], {"EMU_FENCE": "low"}),
            "lazy": ("run_emu_at3p_rate.py", ["--nobuild", "queued"], {"EMU_STREAMS": "lazy:7"}),
            "queued": ("run_emu_at3p_rate.py", ["--nobuild", "queued"], {})}
    runs = Children(jobs)
    try:
        for m in ("plain", "reverse", "fence"):
            assert_clean(runs.output(m), 3 * 6 * 3)
        assert_clean(runs.output("fence_low"), 2 * 6 * 3)
        assert_clean(runs.output("lazy"), 2 * 7)
        assert_clean(runs.output("queued"), 2 * 7)
    finally:
        runs.close()


@needs_clang
def test_a_build_without_the_adaptive_writer_refuses_every_call_at_another_size(tmp_path):
    """tests/host/at3p_alloc_modes_main.cpp, `none`: at3phip.hip linked without at3p_alloc.hip; the setter to 376 succeeds, all six
    frame-writing calls are refused with and without the flag and write nothing, inadmissible sizes change nothing. `alloc`: with
    at3p_alloc.hip alone the calls at 376 work with AT3PHIP_ALLOC_ADAPTIVE alone and are refused with every other combination"""
    run_alloc_modes(tmp_path, "none", "alloc")


# ---- symbols -------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_prototypes():
    import atracdenc_amd
    from atracdenc_amd import binding as B
    if not os.path.exists(atracdenc_amd.LIB_PATH):
        atracdenc_amd.build_library()
    lib = atracdenc_amd.load_library()
    for name in ("at3phip_set_frame_bytes", "at3phip_get_frame_bytes", "at3phip_decoder_set_frame_bytes", "at3phip_decoder_get_frame_bytes",
                 "at3phip_host_allocate_sized"):
        assert hasattr(lib, name) and name in B.PROTOTYPES and name + "(" in HEADER, name
    assert lib.at3hip_version() == B.AT3HIP_VERSION == (1 << 16) | 6
    assert "frame sizes other than 2048 bytes" not in HEADER and "a word length of 0 inside the coded range, psychoacoustic weighting." in HEADER


# ---- containers and the command line ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_io(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostio") / "libhost_io.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "host", "host_io_capi.cpp")])
    return ctypes.CDLL(so)


@pytest.mark.parametrize("nch", [1, 2])
def test_container_bytes_per_bitrate(host_io, tmp_path, nch):
    """the writers of at3hip_io.hpp at every table size, parsed here: the OMA codec word's (frame_bytes - 8) / 8 and channel id, the
    RIFF block_align, byte_rate, fact samples and data size, and the three files' lengths"""
    n = 3
    for kbit, fb in W.BITRATES.items():
        if fb < W.MIN_BYTES[nch]:
            continue
        frames = W.write_adaptive(_sp("mix", nch)[:n], fb)
        body = frames.tobytes()
        files = {}
        for kind, ext in ((5, "oma"), (6, "at3"), (7, "raw")):
            p = str(tmp_path / f"r{kbit}_{nch}.{ext}")
            assert host_io.at3host_write_container(kind, p.encode(), frames.ctypes.data_as(ctypes.c_void_p), n, fb, 0, n, nch) == 0
            files[ext] = open(p, "rb").read()
        oma = files["oma"]
        word = struct.unpack(">I", oma[32:36])[0]
        assert oma[:3] == b"EA3" and word >> 24 == 1 and (word & 0x3ff) * 8 + 8 == fb and (word >> 10) & 7 == nch
        assert len(oma) == 96 + n * fb and oma[96:] == body
        riff = files["at3"]
        assert riff[:4] == b"RIFF" and riff[8:12] == b"WAVE" and struct.unpack("<I", riff[4:8])[0] == len(riff) - 8
        fmt = riff.index(b"fmt ") + 8
        tag, ch, rate, byte_rate, align = struct.unpack("<HHIIH", riff[fmt:fmt + 14])
        assert (tag, ch, rate, align) == (0xFFFE, nch, 44100, fb) and byte_rate == fb * 44100 // 2048
        assert abs(byte_rate * 8 / 1000.0 - kbit) <= 0.03 * kbit + 0.2, (kbit, byte_rate)      # "bytes * 8 * 44100 / 2048 is about kbit * 1000"
        fact = riff.index(b"fact")
        assert struct.unpack("<II", riff[fact + 4:fact + 12]) == (8, n * 2048) or struct.unpack("<I", riff[fact + 8:fact + 12])[0] == n * 2048
        data = riff.index(b"data", fact)
        assert struct.unpack("<I", riff[data + 4:data + 8])[0] == n * fb and riff[data + 8:] == body
        assert files["raw"] == body


def _cli(*args):
    from atracdenc_amd.binding import LIB_PATH
    exe = os.path.join(os.path.dirname(LIB_PATH), "at3hipenc")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def _wav(path, nch, n=4096):
    x = (np.random.default_rng(3).standard_normal((n, nch)) * 3000).astype("<i2").tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(x)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, nch, 44100, 44100 * 2 * nch, 2 * nch, 16) + \
        b"data" + struct.pack("<I", len(x))
    open(path, "wb").write(hdr + x)
    return str(path)


def test_cli_refusals(tmp_path):
    """before any GPU work: --bitrate 64 without --adaptive says why; --bitrate 100 lists the table; --bitrate 32 on a stereo input
    is refused; and -d names an unknown frame size as before"""
    mono, stereo, out = _wav(tmp_path / "m.wav", 1), _wav(tmp_path / "s.wav", 2), str(tmp_path / "o.oma")
    r = _cli("-e", "atrac3plus", "-i", stereo, "-o", out, "--bitrate", "64")
    assert r.returncode != 0 and "--bitrate 64 needs --adaptive" in r.stderr and "fixed word-length table is defined for 2048-byte frames" in r.stderr
    r = _cli("-e", "atrac3plus", "-i", stereo, "-o", out, "--adaptive", "--bitrate", "100")
    assert r.returncode != 0 and all(f"{kb}" in r.stderr and f"-> {fb} bytes" in r.stderr for kb, fb in W.BITRATES.items()), r.stderr
    r = _cli("-e", "atrac3plus", "-i", stereo, "-o", out, "--adaptive", "--bitrate", "32")
    assert r.returncode != 0 and r.stderr.startswith("Fatal error: --bitrate 32 is a mono rate"), r.stderr
    assert not os.path.exists(out) or os.path.getsize(out) == 0
    frames = W.write_adaptive(_sp("mix", 2)[:2], 376)
    p = tmp_path / "odd.oma"
    p.write_bytes(D.oma_bytes(np.zeros((2, 384), np.uint8), 2, frame_bytes=384))
    r = _cli("-d", "-i", str(p), "-o", str(tmp_path / "z.wav"))
    assert r.returncode != 0 and r.stderr.startswith("Fatal error: ATRAC3plus decoding is not supported for channel id 2, frame size 384")
    p = tmp_path / "ok.oma"
    p.write_bytes(D.oma_bytes(frames, 2, frame_bytes=376))
    r = _cli("-d", "-i", str(p), "-o", str(tmp_path / "z.wav"))     # routed to the decoder, which needs a GPU from there on
    assert "Codec: ATRAC3plus, 2 channels, 64 kbit/s (376-byte frames)" in r.stdout, (r.stdout, r.stderr)
    assert r.returncode == 0 or "at3phip_decoder_create failed" in r.stderr, r.stderr
