"""Every ATRAC3plus spectrum code at every bit phase, without a GPU (at3p_decode_lib.code_corpus): the C restatement's unpack against
the spectrum computed in numpy from the mantissas the corpus was written from, the restatement's per-code hit counter on the corpus
and on the committed frames, the tables' prefix-code properties, the table generators' --check mode, and how far spectra built for
the purpose steer the fixed writer through the tables."""
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import at3p_decode_lib as D
import at3p_writer_lib as W

ROOT = os.path.dirname(D.HERE)


@pytest.fixture(scope="module", params=[1, 2], ids=["mono", "stereo"])
def corpus(request):
    return request.param, D.code_corpus(request.param)


def test_corpus_frame_sizes():
    """the largest frame of each corpus and the standard size the sized runs use; the limit frame fills that size to its last bit"""
    for nch, want in ((1, 560), (2, 1488)):
        c = D.code_corpus(nch)
        assert c["bytes"] == want and 8 * D.STANDARD_BYTES[D.STANDARD_BYTES.index(want) - 1] < c["max_bits"] <= 8 * want
        assert set(D.STANDARD_BYTES) == set(W.BITRATES.values())
        assert not c["frames"][:, :, want:].any()
        assert c["what"][-1] == "limit" and (c["frames"][:, -1, want - 1] & 3 == 3).all()
        assert c["n_codes"] == 4915


@pytest.mark.parametrize("sparse", [False, True], ids=["plain", "sparse"])
@pytest.mark.parametrize("sized", [False, True], ids=["2048", "sized"])
def test_unpack_equals_numpy_expectation(corpus, sparse, sized):
    """(float32(m) * AT3P_MANT[wl]) * AT3P_SCALE[sf] of the intended mantissas, as bit patterns; no frame rejected"""
    nch, c = corpus
    want = D.corpus_expected_spectrum(c)
    fb = c["bytes"] if sized else D.FRAME
    S, F = c["frames"].shape[:2]
    frames = np.ascontiguousarray(c["frames"][:, :, :fb]).reshape(S * F, fb)
    spec, win, fl = W.unpack(frames, nch, sparse=sparse)
    assert not fl["reason"].any(), np.flatnonzero(fl["reason"])[:8]
    assert not win.any()
    assert np.array_equal(spec.view(np.uint32), want.reshape(S * F, nch, D.FRAME).view(np.uint32))
    assert np.array_equal(fl["wl"][:, :nch], c["wl"].reshape(S * F, nch, 32))
    if not sparse and not sized:   # the decoder's own entry point (no flags, 2048 bytes)
        spec0, _, fl0 = D.unpack(frames, nch)
        assert not fl0["reason"].any() and np.array_equal(spec0.view(np.uint32), spec.view(np.uint32))


def _present():
    present = np.zeros((56, 256), bool)
    for t, s, _, _ in D.table_codes():
        present[t, s] = True
    return present


def test_corpus_hits_every_code():
    """the restatement's parser decodes each of the 4915 codes on the mono corpus, and nothing else"""
    c = D.code_corpus(1)
    lib = D.cpu_lib()
    D.hits(lib)
    _, _, fl = D.unpack(c["frames"].reshape(-1, D.FRAME), 1, lib)
    h = D.hits(lib)
    assert not fl["reason"].any()
    present = _present()
    assert present.sum() == 4915
    assert (h[present] > 0).all() and not h[~present].any()
    assert not D.hits(lib).any()   # the reset


GOLDEN_FRAME_FILES = ("at3p_decode", "at3p_frames", "at3p_rd", "at3p_ref_parts", "at3p_sparse", "at3p_tonal", "at3p_tonal_write")


def test_committed_frames_code_coverage(capsys):
    """What the committed 2048-byte frames (the `*frames*` arrays of the goldens above, and crafted_frames) reach of the 4915 codes
    through at3pd_unpack_frame: 2760, and 1014 of the 2662 codes longer than 8 bits, when the corpus was added. Printed so that the
    figures stay visible; the corpus, not these frames, is what covers the tables."""
    lib = D.cpu_lib()
    D.hits(lib)
    n_frames = 0
    for name in GOLDEN_FRAME_FILES:
        g = np.load(os.path.join(D.HERE, "golden", name + ".npz"))
        for k in g.files:
            a = g[k]
            if "frames" in k and a.dtype == np.uint8 and a.ndim >= 2 and a.shape[-1] == D.FRAME:
                a = a.reshape(-1, D.FRAME)
                for nch in (1, 2):
                    sel = a[((a[:, 0] >> 5) & 3) == nch - 1]
                    if len(sel):
                        D.unpack(sel, nch, lib)
                        n_frames += len(sel)
    for nch in (1, 2):
        D.unpack(D.crafted_frames(nch, nch)[0], nch, lib)
    h = D.hits(lib)
    codes = D.table_codes()
    long_codes = [(t, s) for t, s, _, n in codes if n > 8]
    reached = sum(1 for t, s, _, _ in codes if h[t, s])
    reached_long = sum(1 for t, s in long_codes if h[t, s])
    with capsys.disabled():
        print(f"\ncommitted frames ({n_frames} and the crafted ones): {reached} of {len(codes)} codes, {reached_long} of {len(long_codes)} "
              f"longer than 8 bits")
        worst = sorted((sum(1 for tt, s, _, _ in codes if tt == t and h[t, s]) / sum(1 for tt, *_ in codes if tt == t), t) for t in range(56))[:10]
        for _, t in worst:
            print(f"  (word length {t % 7 + 1}, table {t // 7}): {sum(1 for tt, s, _, _ in codes if tt == t and h[t, s])}/"
                  f"{sum(1 for tt, *_ in codes if tt == t)}")
    assert len(codes) == 4915 and len(long_codes) == 2662
    assert reached >= 2760


def _is_complete_prefix_code(entries):
    """entries [(code, length)]: the Kraft sum is exactly 1 and no code is a prefix of another"""
    assert all(0 < n <= 12 and code < (1 << n) for code, n in entries)
    kraft = sum(Fraction(1, 1 << n) for _, n in entries)
    words = sorted(format(code, f"0{n}b") for code, n in entries)
    return kraft == 1 and not any(b.startswith(a) for a, b in zip(words, words[1:]))


def test_tables_are_complete_prefix_codes():
    """from the table files alone: the 56 spectrum tables, the four word-length tables, the tone-band count's code"""
    spec_t, wl_t, _ = D.vlc_tables()
    for t in range(56):
        assert _is_complete_prefix_code(list(spec_t[t].values())), t
    for i in range(4):
        assert _is_complete_prefix_code(list(wl_t[i].values())), i
    text = open(os.path.join(ROOT, "atracdenc_amd", "csrc", "at3p_tone_vlc.inc")).read()
    v = [int(x, 16) for x in re.findall(r"0x[0-9a-f]+", text[text.index("AT3P_TONE_BANDS_VLC[16]"):])]
    assert len(v) == 16 and _is_complete_prefix_code([(e & 0xfff, e >> 12) for e in v])
    # the check itself tells an incomplete and a non-prefix code
    assert not _is_complete_prefix_code([(0, 1), (2, 2)]) and not _is_complete_prefix_code([(0, 1), (1, 2), (1, 1)])


@pytest.mark.skipif(not os.path.isdir(D.REF_SRC), reason="the reference's sources are not present")
@pytest.mark.parametrize("tool", ["gen_at3p_vlc.py", "gen_at3p_tone_tables.py", "gen_at3p_fir.py"])
def test_generated_tables_match_the_reference(tool):
    """each generator regenerates in memory and compares with the committed .inc files (both copies of at3p_vlc.inc)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- the writer, as far as it can be steered ------------------------------------------------------------------------------------
# codes of the 4915 that the fixed writer's frames of at3p_decode_lib.steered_spectra reach (mono, stereo, both), as the counting
# parser read them back when the construction was first run; it is deterministic, so the figures are exact
STEERED_CODES = {1: 3861, 2: 4043, "both": 4094}
# (word length, table index) pairs no steered unit was coded with: (2, 7) and (7, 7) can never be chosen
# (test_word_length_and_code_table_pairs_met); the other three carry group flags, which the writer always sends as 1, and under their
# own distribution another table of the word length is cheaper by those flags
STEERED_PAIRS_NOT_CHOSEN = {(1, 1), (1, 6), (2, 7), (6, 7), (7, 7)}


def test_steered_writer_coverage(oracle, capsys):
    from at3_testlib import at3p_write_frames
    lib = D.cpu_lib()
    both, chosen = np.zeros((56, 256), np.int64), set()
    for nch in (1, 2):
        specs, mant, target = D.steered_spectra(nch)
        n = specs.shape[0] * specs.shape[1]
        frames, info = at3p_write_frames(specs.reshape(n, nch, D.FRAME), info=True)
        assert (info["num_quant_units"] == 32).all()
        D.hits(lib)
        spec, _, fl = D.unpack(frames, nch, lib)
        h = D.hits(lib)
        assert not fl["reason"].any()
        # the writer quantised to the drawn mantissas and chose the intended scale factors
        coded = target.reshape(n, nch, 32) >= 0
        sfi = info["sfi"][:, :nch]
        assert np.array_equal(sfi, np.where(coded, np.where(np.array(D.FIXED_WL) == 1, D.STEER_SF - 1, D.STEER_SF), 0))
        assert np.array_equal(spec.view(np.uint32), D.steered_expectation(mant.reshape(n, nch, D.FRAME), sfi).view(np.uint32))
        tab = info["tab"][:, :nch]
        assert np.array_equal(fl["tab"][:, :nch], tab)
        chosen |= {(D.FIXED_WL[qu], int(tab[f, ch, qu])) for f, ch, qu in np.argwhere(coded)}
        hit = (tab == target.reshape(n, nch, 32))[coded].mean()
        with capsys.disabled():
            print(f"\nsteered writer, {nch} channel(s): {int((h > 0).sum())} of 4915 codes in {n} frames; {100 * hit:.0f} % of the units got the table aimed at")
        assert int((h > 0).sum()) == STEERED_CODES[nch]
        both += h
    every = {(w, i) for w in range(1, 8) for i in range(8)}
    with capsys.disabled():
        print(f"steered writer: {int((both > 0).sum())} codes in all; pairs never chosen: {sorted(every - chosen)}")
    assert int((both > 0).sum()) == STEERED_CODES["both"]
    assert every - chosen == STEERED_PAIRS_NOT_CHOSEN
