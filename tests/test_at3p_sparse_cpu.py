"""ATRAC3plus sparse word lengths (include/at3phip.h, SPARSE WORD LENGTHS) without a GPU: the restatement
tests/host/at3p_writer_cpu.c with its flags off against what tests/host/at3p_rate_cpu.c gave before the two were folded into one
(tests/golden/at3p_writer_fold.npz); at3phip_host_allocate_sparse against it; every frame it writes parsed by an independent parser
(at3p_writer_lib.parse_head, written from the header's text), recounted and decoded;
the t = -21 property; the smallest frame sizes re-derived; crafted decoder frames; the round trip per standard bitrate beside
DESIGN.md section 20's; the kernels through the CPU SIMT harness; a build without the adaptive writer."""
import os
import re
import subprocess

import numpy as np
import pytest

import at3p_writer_lib as W
import at3p_decode_lib as D
import at3p_gha_lib as G
import at3p_tonal_write_lib as TW
from simt_harness_lib import CLANG, ROOT, Children, assert_clean, build_strict, run_alloc_modes
from test_at3p_rate_cpu import SNR as SECTION_20

needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")
NF = W.SNR_FRAMES
HEADER = open(os.path.join(ROOT, "include", "at3phip.h")).read()
SIZES = {1: (192, 280, 376, 744, 2048), 2: (280, 376, 744, 2048)}
REASON = {name: i for i, name in enumerate(D.REASONS)}

_specs = {}


def _sp(name, nch):
    if (name, nch) not in _specs:
        _specs[(name, nch)] = W.specs_of(name, nch, NF)
    return _specs[(name, nch)]


# ---- 1. flags off --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
def test_flags_off_equals_the_rate_restatement(nch):
    """tests/golden/at3p_writer_fold.npz holds, as SHA-256, what at3p_rate_cpu.c gave while it stated the writer and the decoder's
    unpack beside this restatement, equal to it with the flags off: frames, records, PCM and counters at 2048 bytes, 376 and the
    smallest size, on that file's test inputs: the signals, silence, full-scale noise, non-finite spectra, window flags, tonal
    records, flipped bits and the crafted malformed frames; and its allocations on the first 100 random cost tables"""
    gold = W.fold_golden(nch)

    def same(label, *got):
        assert np.array_equal(W.sha(*got), gold[label]), label

    cases = [(W.specs_of(n, nch, 4), None, None) for n in W.SIGNALS + ("silence", "fullscale")]
    cases.append((W.odd_specs(nch, 3), None, None))
    cases.append((W.specs_of("noise", nch, 2), np.array([[0x01ef] * nch, [0xffff] * nch], np.uint16), None))
    cases.append((np.concatenate([W.full_scale_noise(2, nch), _sp("mix", nch)[:1]]), None,
                  [TW.largest_block(nch), None, TW.case_blocks(f"small_{nch}")[0][0]]))
    rng = np.random.default_rng(11)
    for fb in (2048, 376, W.MIN_BYTES[nch]):
        for i, (sp, win, blocks) in enumerate(cases):
            new, ni, _ = W.write_adaptive(sp, fb, False, win, blocks, info=True)
            same(f"a{i}_{fb}_frames", new)
            same(f"a{i}_{fb}_info", ni.view(np.uint8))
            flipped = D.mutate_frames(new, rng, n_flips=2)
            same(f"a{i}_{fb}_flipped_in", flipped)
            for kind, frames in (("plain", new), ("flipped", flipped)):
                for tones in (False, True):
                    b, rb = W.decode(frames, nch, tones, sparse=False)
                    same(f"a{i}_{fb}_{kind}_tones{int(tones)}", b.view(np.uint32), rb)
    crafted, _ = D.crafted_frames(nch, 3)
    same("b_in", crafted)
    for tones in (False, True):
        b, rb = W.decode(crafted, nch, tones, sparse=False)
        same(f"b_tones{int(tones)}", b.view(np.uint32), rb)
    same("b_fields0", W.unpack(crafted, nch, sparse=False)[2].view(np.uint8))
    n = 0
    for i, (sfi, bits, tail) in enumerate(W.random_cost_tables()[:100]):
        if sfi.shape[0] == nch:
            same(f"c{i}_in", sfi, bits, tail)
            for fb in (W.MIN_BYTES[nch], 2048):
                tb = min(tail, 8 * fb - 3)
                wl, *rest = W.allocate(sfi, bits, tb, fb, False)
                same(f"c{i}_{fb}", wl, rest)
            n += 1
    assert n == sum(k.startswith("c") and k.endswith("_in") for k in gold) >= 30


# ---- 2. at3phip_host_allocate_sparse ---------------------------------------------------------------------------------------------------
def _same(B, path, sfi, bits, tail, fb, what):
    wl, N, t, k, total = W.allocate(sfi, bits, tail, fb, True)
    gwl, gN, gt, gk = B.at3p_host_allocate(sfi, bits, tail, path, frame_bytes=fb, sparse=True)
    assert (gN, gt, gk) == (N, t, k) and np.array_equal(gwl, wl), (what, (N, t, k), (gN, gt, gk))
    return wl, N, t, k, total


@needs_clang
def test_host_allocate_sparse_equals_the_restatement_on_the_signals():
    from atracdenc_amd import binding as B
    path = build_strict()
    n = zeros = 0
    for name in W.SIGNALS:
        for nch in (1, 2):
            sp = _sp(name, nch)
            for f in (0, 5, 13):
                sfi, bits, _ = W.cost_table(sp[f])
                for fb in SIZES[nch]:
                    wl, N, _, _, total = _same(B, path, sfi, bits, 8, fb, (name, nch, f, fb))
                    assert total <= 8 * fb - 3 and N not in (29, 30, 31) and wl[:, N - 1].any() and not wl[:, N:].any()
                    zeros += bool((wl[:, :N] == 0).any())
                    n += 1
    assert n == 5 * 3 * (5 + 4) and zeros >= n // 3


@needs_clang
def test_host_allocate_sparse_equals_the_restatement_on_random_tables():
    """1000 seeded tables, non-monotone ones among them as tests/test_at3p_alloc_cpu.py builds them, at the channel count's smallest
    size, 376 and 2048"""
    from atracdenc_amd import binding as B
    path = build_strict()
    tables = W.random_cost_tables()
    assert len(tables) == 1000
    differ = 0
    for i, (sfi, bits, tail) in enumerate(tables):
        nch = sfi.shape[0]
        for fb in (W.MIN_BYTES[nch], 376, 2048):
            tb = min(tail, 8 * fb - 3)
            got = _same(B, path, sfi, bits, tb, fb, (i, fb))
            differ += fb == 376 and not np.array_equal(got[0], W.allocate(sfi, bits, tb, fb)[0])
    assert differ >= 300, differ   # (the flag matters on these tables)


@needs_clang
def test_host_allocate_sparse_on_the_hand_built_cases():
    from atracdenc_amd import binding as B
    path = build_strict()
    cases = W.edge_tables()
    got = {name: _same(B, path, *case, name) for name, case in cases.items()}
    wl, N, t, k, _ = got["nothing_wanted"]        # no unit wanted: unit 0 of channel 0 becomes 1
    assert (N, t, k) == (1, 3, 0) and wl[0, 0] == 1 and wl.sum() == 1
    for top in (28, 29, 30):                      # highest wanted unit 28, 29 or 30: N = 32, unit 31 of channel 0 becomes 1
        wl, N, _, _, _ = got[f"top_{top}"]
        assert N == 32 and wl[0, 31] == 1 and wl[1, 31] == 0 and wl[1, top] > 0 and not wl[0, 4:31].any()
    wl, N, _, _, total = got["clone_bits"]        # channel-1 zeros under channel-0 non-zeros: the clone bits count
    sfi, bits, tail, fb = cases["clone_bits"]
    clones = int(((wl[1, :N] == 0) & (wl[0, :N] > 0)).sum())
    assert clones >= 10
    head = {"N": N, "wl": [[int(w) for w in wl[0, :N]], [int(w) for w in wl[1, :N]]]}
    assert W.count_bits(head, 2, bits, tail) == total
    for name in ("flat", "flat_mono"):            # a flat sfi: A(t*, 0) is empty, k alone extends N
        sfi, bits, tail, fb = cases[name]
        wl, N, t, k, _ = got[name]
        assert W.allocate(sfi, bits, tail, fb, True)[1:4] == (N, t, k) and k > 1 and N > 1
        w0 = np.maximum(0, np.minimum(7, (sfi.astype(int) - t) // 3))
        assert not w0.any() and int((wl > 0).sum()) == k and N == (k + sfi.shape[0] - 1) // sfi.shape[0]
    sfi, bits, tail, fb = cases["flat"]
    for bad_fb in (0, 7, 2056, W.MIN_BYTES[2] - 8):
        with pytest.raises(B.At3HipError):
            B.at3p_host_allocate(sfi, bits, tail, path, frame_bytes=bad_fb, sparse=True)


# ---- 3. every frame ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("name", W.SIGNALS)
def test_frames_parse_count_and_decode(name, nch):
    """14 frames of each signal at each size: the independent head parser reads them; Bits(A) recounted from the parsed fields is
    the restatement's figure and within the budget; the terminator sits where the count says; every clone flag is 1; the sparse
    decoder rejects none, and the decoder without the flag rejects exactly the frames with a zero inside the range, as bad_code"""
    sp = _sp(name, nch)
    tail = sum(n for _, n in W.tail_bits_list(nch))
    costs = [W.cost_table(sp[f])[1] for f in range(NF)]
    for fb in SIZES[nch]:
        frames, rec, _ = W.write_adaptive(sp, fb, True, info=True)
        assert W.decode(frames, nch, sparse=True)[1].sum() == 0
        zero_frames = 0
        for f in range(NF):
            p = W.parse_head(frames[f], nch)
            N = p["N"]
            assert N not in (29, 30, 31) and N == rec["num_quant_units"][f]
            assert all(p["wl"][c] == list(rec["wl"][f, c, :N]) for c in range(nch)) and any(p["wl"][c][N - 1] for c in range(nch))
            assert all(v == 1 for v in p["clone"].values())
            total = W.count_bits(p, nch, costs[f], tail)
            assert total == rec["bits"][f] <= 8 * fb - 3, (fb, f, total)
            assert W.terminator_pos(frames[f]) == 3 + total - 1 < 8 * fb
            zero_frames += any(0 in p["wl"][c] for c in range(nch))
        rej = W.decode(frames, nch, sparse=False)[1]
        assert rej[REASON["bad_code"]] == zero_frames == rej.sum(), (fb, rej, zero_frames)


# ---- 4. t = -21 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
def test_a_frame_that_fits_at_t_minus_21_is_the_adaptive_writers(nch):
    """at t = -21 every want is 7: where the unflagged allocation fits there (quiet mono `tones`-like material at 2048 bytes, section
    19's edge case), the sparse frame is the same bytes"""
    sp = np.concatenate([W.quiet_mono(4).repeat(nch, axis=1), W.specs_of("silence", nch, 2)])
    plain, rec, _ = W.write_adaptive(sp, 2048, info=True)
    assert (rec["t"] == W.T_MIN).sum() >= 2
    sparse = W.write_adaptive(sp, 2048, True)
    fits = rec["t"] == W.T_MIN
    assert np.array_equal(plain[fits], sparse[fits])


# ---- 5. the smallest sizes ---------------------------------------------------------------------------------------------------------------
def test_min_frame_bytes_still_follow_from_the_tables():
    """A(63, 0) under A3s is unit 0 of channel 0 at word length 1 and nothing else. In front of the tail: 5 + 1 bits, the word-length
    section for N = 1 with its code at the longest length, scale-factor index and power group per channel, the code-table section
    with one index (channel 1's unit at 0 under a coded channel-0 unit carries the clone flag), and unit 0's 16 lines under the
    cheapest-in-the-worst-case table - never more than A3's one unit per channel, so the header's 77 and 147 bits bound it and
    176 and 224 bytes still admit the largest tonal record"""
    tb = W.inc_tables()
    worst_unit = W.worst_front_one_unit(1) - (5 + 1 + 11 + (2 + 6) + 1 + (4 + 3) + 4 * tb["AT3P_SB_POWGRPS"][tb["AT3P_QU_TO_SB"][0]])
    longest_wl = max(e >> 12 for e in tb["AT3P_WL_VLC"])
    front = {}
    for nch in (1, 2):
        bits = 5 + 1 + 11 + (nch == 2) * (6 + longest_wl) + nch * (2 + 6) + 1 + nch * 4 + 3 + (nch == 2) * 1
        bits += nch * 4 * tb["AT3P_SB_POWGRPS"][tb["AT3P_QU_TO_SB"][0]] + worst_unit
        front[nch] = bits
        assert bits <= W.worst_front_one_unit(nch)
        assert bits + W.worst_tail(nch) <= 8 * W.MIN_BYTES[nch] - 3
    assert front[1] <= 77 and front[2] <= 147, front
    for nch in (1, 2):   # and in fact: the largest record on full-scale noise at the smallest size
        fb, big = W.MIN_BYTES[nch], TW.largest_block(nch)
        frames, rec, nb = W.write_adaptive(W.full_scale_noise(2, nch), fb, True, None, [big, big], info=True)
        assert (nb > 1000).all() and (rec["bits"] <= 8 * fb - 3).all() and W.decode(frames, nch, True, True)[1].sum() == 0
    assert "#define AT3PHIP_ALLOC_SPARSE 256u" in HEADER and "#define AT3PHIP_DECODE_SPARSE 32u" in HEADER


# ---- 6. crafted decoder frames -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
def test_crafted_frames(nch):
    """top unit zero in every channel and (stereo) a cleared clone flag are unsupported_syntax; without the flag both are bad_code
    (a word length of 0); a frame cut inside the code-table section is read_past_end"""
    bad = W.crafted_frames(nch, 376)
    assert len(bad) == nch
    _, _, fl = W.unpack(bad, nch, True, True)
    assert (fl["reason"] == REASON["unsupported_syntax"] + 1).all()
    _, _, fl = W.unpack(bad, nch, True, False)
    assert (fl["reason"] == REASON["bad_code"] + 1).all()
    pcm, rej = W.decode(bad, nch, True, True)
    assert rej[REASON["unsupported_syntax"]] == nch == rej.sum() and not pcm.any()
    good = W.write_adaptive(_sp("tones", nch)[:1], 376, True)[0]
    head = W.parse_head(good, nch)
    sf_end = head["pos"] - (1 + 4 * nch + 3 * sum(w > 0 for row in head["wl"] for w in row) + len(head["clone"]))
    for cut_bits in (sf_end + 8, head["pos"] - 2):
        cut = np.ascontiguousarray(good[:cut_bits // 8])
        assert 8 * len(cut) > sf_end and 8 * len(cut) < head["pos"]
        assert W.unpack(cut[None], nch, True, True)[2]["reason"][0] == REASON["read_past_end"] + 1


# ---- 7. round trip per standard bitrate ----------------------------------------------------------------------------------------------------
# dB per channel, sparse encoder restatement then sparse decoder restatement, section 20's signals, sizes and snr_db; measured from
# the restatement (deterministic) and listed in DESIGN.md section 21; a cell is held at its recorded value minus 0.05 dB (print rounding)
SNR = {
    ("noise", 1): {192: [1.67], 280: [3.03], 376: [4.90], 560: [9.65], 744: [14.20], 936: [18.11], 1120: [22.41], 1488: [29.97], 1864: [29.97],
                   2048: [29.97]},
    ("noise", 2): {280: [1.10, 1.11], 376: [1.71, 1.66], 560: [3.18, 3.00], 744: [4.85, 4.90], 936: [7.50, 7.30], 1120: [9.70, 9.67],
                   1488: [14.26, 14.15], 1864: [18.17, 18.19], 2048: [19.98, 20.04]},
    ("mix", 1): {192: [5.01], 280: [6.34], 376: [8.16], 560: [13.04], 744: [17.23], 936: [20.81], 1120: [23.80], 1488: [26.63], 1864: [26.63],
                 2048: [26.63]},
    ("mix", 2): {280: [4.62, 3.05], 376: [5.39, 3.60], 560: [6.65, 5.06], 744: [8.14, 6.99], 936: [10.97, 9.13], 1120: [13.30, 11.76],
                 1488: [17.49, 16.02], 1864: [20.79, 19.99], 2048: [22.39, 21.52]},
    ("stress", 1): {192: [9.57], 280: [12.32], 376: [14.92], 560: [19.26], 744: [22.64], 936: [26.32], 1120: [28.62], 1488: [30.29], 1864: [30.36],
                    2048: [30.36]},
    ("stress", 2): {280: [8.17, 8.14], 376: [9.07, 9.95], 560: [12.73, 12.69], 744: [15.30, 15.42], 936: [17.67, 17.31], 1120: [19.82, 19.62],
                    1488: [23.03, 23.56], 1864: [26.54, 27.14], 2048: [27.79, 28.27]},
    ("tones", 1): {192: [30.16], 280: [30.17], 376: [30.17], 560: [30.17], 744: [30.17], 936: [30.17], 1120: [30.17], 1488: [30.17], 1864: [30.17],
                   2048: [30.17]},
    ("tones", 2): {280: [29.08, 28.75], 376: [30.16, 29.87], 560: [30.17, 29.88], 744: [30.17, 29.88], 936: [30.17, 29.88], 1120: [30.17, 29.88],
                   1488: [30.17, 29.88], 1864: [30.17, 29.88], 2048: [30.17, 29.88]},
    ("burst", 1): {192: [25.28], 280: [25.69], 376: [25.88], 560: [26.02], 744: [26.12], 936: [26.16], 1120: [26.16], 1488: [26.17], 1864: [26.17],
                   2048: [26.17]},
    ("burst", 2): {280: [25.13, 23.93], 376: [25.52, 24.78], 560: [25.84, 25.38], 744: [25.98, 25.65], 936: [26.05, 25.78], 1120: [26.11, 25.91],
                   1488: [26.14, 26.09], 1864: [26.16, 26.15], 2048: [26.16, 26.16]},
}
# the cells below section 20's by more than 0.05 dB, which DESIGN.md section 21 lists with their cause
BELOW_SECTION_20 = {("burst", 2, 744, 1), ("burst", 2, 936, 1)}


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("name", W.SIGNALS)
def test_round_trip_snr_per_bitrate(name, nch):
    sp, x = _sp(name, nch), G.signal_pcm(name, NF, nch)
    row, used = {}, {}
    for kbit, fb in W.BITRATES.items():
        if fb < W.MIN_BYTES[nch]:
            continue     # 32 kbit/s is a mono rate
        frames, rec, _ = W.write_adaptive(sp, fb, True, info=True)
        y, rej = W.decode(frames, nch, sparse=True)
        assert rej.sum() == 0
        row[fb] = [G.snr_db(x[:, :, c].reshape(-1), y[:, :, c].reshape(-1), NF) for c in range(nch)]
        used[fb] = float(rec["bits"].mean())
        print(f"sparse round trip {name} x{nch} {kbit} kbit/s ({fb} bytes): {' / '.join(f'{v:.2f}' for v in row[fb])} dB, mean bits {used[fb]:.0f} "
              f"of {8 * fb - 3}, units {rec['num_quant_units'].min()}..{rec['num_quant_units'].max()}")
    assert sorted(row) == sorted(SNR[(name, nch)])
    for fb, got in row.items():
        for c in range(nch):
            assert got[c] >= SNR[(name, nch)][fb][c] - 0.05, (name, nch, fb, c, got[c])
            if got[c] < SECTION_20[(name, nch)][fb][c] - 0.05:
                assert (name, nch, fb, c) in BELOW_SECTION_20, (name, nch, fb, c, got[c])
    sizes = sorted(row)   # (a) every row is non-decreasing in the frame size
    assert all(row[a][c] <= row[b][c] + 0.005 for a, b in zip(sizes, sizes[1:]) for c in range(nch)), row
    if nch == 2 and name == "noise":   # (b), (c)
        assert all(row[376][c] > SECTION_20[("noise", 2)][376][c] for c in range(2)) and SECTION_20[("noise", 2)][376] == [0.06, 0.06]
        assert used[376] > 3005 / 2
    if nch == 2 and name == "mix":
        assert SECTION_20[("mix", 2)][376] == SECTION_20[("mix", 2)][560] == [3.72, 2.43]
        assert all(row[fb][c] > SECTION_20[("mix", 2)][fb][c] for fb in (376, 560) for c in range(2))


def test_design_lists_the_round_trip_table():
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = doc[doc.index("## 21."):]
    for (name, nch), row in SNR.items():
        for fb, cells in row.items():
            assert " / ".join(f"{v:.2f}" for v in cells) in sec, (name, nch, fb)


# ---- 8. golden -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nch,fb", W.SPARSE_GOLDEN_CASES, ids=[f"{n}_{c}_{fb}" for n, c, fb in W.SPARSE_GOLDEN_CASES])
def test_restatement_equals_the_golden_file(name, nch, fb):
    """tests/golden/at3p_sparse.npz (tools/gen_golden_at3p_sparse.py): the restatement's frames, t*, k*, N, word lengths and PCM on 3
    frames of `noise` and `tones`, mono and stereo, at 376 and 2048 bytes. Everything sparse is pinned to the restatement; this pins
    the restatement, so that an edit to it or another compiler cannot move every expectation at once."""
    gold = np.load(W.SPARSE_GOLDEN)
    got = W.sparse_golden_entry(name, nch, fb)
    for k, v in got.items():
        want = gold[f"{name}_{nch}_{fb}_{k}"]
        assert want.shape == np.asarray(v).shape and np.array_equal(want, v), (name, nch, fb, k)


def test_golden_file_holds_what_it_should():
    gold = np.load(W.SPARSE_GOLDEN)
    assert sorted(gold.files) == sorted(f"{n}_{c}_{fb}_{k}" for n, c, fb in W.SPARSE_GOLDEN_CASES for k in ("frames", "choice", "wl", "pcm_sha256"))
    assert os.path.getsize(W.SPARSE_GOLDEN) < 64 * 1024
    zeros = sum(bool((gold[f"{n}_{c}_376_wl"][f, :c, :gold[f"{n}_{c}_376_choice"][f, 2]] == 0).any()) for n, c, fb in W.SPARSE_GOLDEN_CASES if fb == 376
                for f in range(W.SPARSE_GOLDEN_FRAMES))
    assert zeros >= 6   # (the file holds word length 0 inside the coded range)


@pytest.mark.parametrize("nch", [1, 2])
def test_frozen_sparse_and_rd_edge_cases(nch):
    """tests/golden/at3p_writer_fold.npz, part d: what the sparse and the rate-distortion restatements gave, before the restatements
    were folded into one, where the definition has special cases: edge_specs written sparse and with rate-distortion word lengths at
    the smallest size and at 2048 bytes, edge_tables and guard_table allocated, crafted_frames decoded with sparse on"""
    gold, got = W.fold_golden(nch), W.fold_entries(nch, "d")
    assert len(got) >= 15 and set(got) == {k for k in gold if k.startswith("d")}
    assert [k for k in got if not np.array_equal(got[k], gold[k])] == []


def test_fold_golden_file_holds_what_it_should():
    """labels and SHA-256 digests per channel count, nothing else; every part present; and every input the digests were taken on
    (spectra and tails, flipped frames, crafted frames, cost tables) is still what this tree builds: a change in how numpy draws, or in
    a signal, shows here and not as a failure of the restatement"""
    gold = np.load(W.FOLD_GOLDEN)
    assert sorted(gold.files) == ["labels_1", "labels_2", "sha256_1", "sha256_2"] and os.path.getsize(W.FOLD_GOLDEN) < 64 * 1024
    for nch in (1, 2):
        labels, g = gold[f"labels_{nch}"].tolist(), W.fold_golden(nch)
        assert gold[f"sha256_{nch}"].shape == (len(labels), 32) and gold[f"sha256_{nch}"].dtype == np.uint8 and len(set(labels)) == len(labels)
        got = W.fold_entries(nch)
        assert list(got) == labels
        for part, least in (("a", 10 * (1 + 3 * 7)), ("b", 5), ("c", 3 * 30), ("d", 15)):
            assert sum(k.startswith(part) for k in labels) >= least, part
        inputs = [k for k in labels if k.endswith("_in")]
        assert len(inputs) >= 10 + 30 + 30 + 1 + 4 and [k for k in inputs if not np.array_equal(got[k], g[k])] == []


# ---- 9. the kernels through the CPU SIMT harness -----------------------------------------------------------------------------------------
@needs_clang
def test_harness_driver_equals_the_restatement():
    """tools/emu/run_emu_at3p_sparse.py under the strict harness: the sparse writer kernels (plain and tonal) and the sparse unpack
    kernels (2048 and sized) against the restatement, on the signals at 280 and 2048 bytes, at3p_writer_lib.edge_specs at the
    smallest frame sizes - whose restatement records the driver checks for the empty frame (A3s' first fix-up), N = 32 with unit 31
    of channel 0 at 1 above zeros (mono and stereo), the clone flags and the flat case, one `bad` line per channel count -,
    non-finite spectra and the largest tonal record at 224 bytes, in ascending and descending wavefront order and with a guard
    page behind every frame buffer"""
    build_strict()
    jobs = {"plain": ("run_emu_at3p_sparse.py", ["--nobuild"], {}), "reverse": ("run_emu_at3p_sparse.py", ["--nobuild"], {"EMU_ORDER": "reverse"}),
            "fence": ("run_emu_at3p_sparse.py", ["--nobuild"], {"EMU_FENCE": "high"})}
    runs = Children(jobs)
    try:
        for m in jobs:
            assert_clean(runs.output(m), 3 * 7 + 2)
    finally:
        runs.close()


# ---- 10. a build without the adaptive writer ---------------------------------------------------------------------------------------------
@needs_clang
def test_a_build_without_the_adaptive_writer_refuses_the_flag(tmp_path):
    """tests/host/at3p_alloc_modes_main.cpp, `none`: at3phip.hip linked without at3p_alloc.hip and at3p_sparse.hip; all six
    frame-writing calls refuse ADAPTIVE | SPARSE and SPARSE alone and write nothing, at3phip_decode refuses AT3PHIP_DECODE_SPARSE.
    `alloc+sparse+rd`: with these units each of their modes' calls is accepted at both sizes, SPARSE without ADAPTIVE is still refused"""
    run_alloc_modes(tmp_path, "none", "alloc+sparse+rd")


def test_symbols_and_flags():
    from atracdenc_amd import binding as B
    assert B.AT3PHIP_ALLOC_SPARSE == 256 == int(re.search(r"#define AT3PHIP_ALLOC_SPARSE (\d+)u", HEADER).group(1))
    assert B.AT3PHIP_DECODE_SPARSE == 32 == int(re.search(r"#define AT3PHIP_DECODE_SPARSE (\d+)u", HEADER).group(1))
    assert "at3phip_host_allocate_sparse" in B.PROTOTYPES
    with pytest.raises(ValueError):
        B._alloc_flag(False, True)
    assert B._alloc_flag(True, True) == 384 and B._alloc_flag(True) == 128 and B._alloc_flag(False) == 0
