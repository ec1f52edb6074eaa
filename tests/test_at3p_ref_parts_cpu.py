"""The adaptive and sparse ATRAC3plus writers against the REFERENCE's part coders (tests/at3p_ref_parts_lib.py): the restatements
tests/host/at3p_writer_cpu.c, under each of its writers' names, chooses an allocation (N, word lengths) and write the frame; the
reference's TWordLenEncoder, TSfIdxEncoder, TQuantUnitsEncoder and TTonalComponentEncoder, given the same spectra and allocation,
must write the same bytes and count the same bits. Coverage of what the comparison met is asserted. The restatement's unpack is held
to the reference's integer mantissas on allocations no writer of the project chose. tests/golden/at3p_ref_parts.npz holds frames the
reference's code wrote; the restatements reproduce it without the reference. The tests that run the reference's code skip where
oracle/_ref is absent."""
import functools
import itertools

import numpy as np
import pytest

import at3p_writer_lib as W
import at3p_ref_parts_lib as P
import at3p_tonal_write_lib as TW

needs_ref = pytest.mark.skipif(not P.have_ref(), reason="oracle/_ref not built")
SIG_FRAMES = 6
SPARSE_SIZES = {nch: (W.MIN_BYTES[nch], 376, 744, 2048) for nch in (1, 2)}
EDGE_SIZES = {nch: (W.MIN_BYTES[nch], 2048) for nch in (1, 2)}
TONAL_SIZES = {nch: (W.MIN_BYTES[nch], 376, 2048) for nch in (1, 2)}


def _writers_at(fb):
    return (("alloc",) if fb == 2048 else ()) + ("rate", "sparse_on")


SIGNAL_CASES = [("signals", w, nch, fb) for nch in (1, 2) for w, sizes in (("alloc", (2048,)), ("rate", W.SIZES[nch]), ("sparse_off", SPARSE_SIZES[nch]),
                                                                           ("sparse_on", SPARSE_SIZES[nch])) for fb in sizes]
EDGE_CASES = [("edges", w, nch, fb) for nch in (1, 2) for fb in EDGE_SIZES[nch] for w in _writers_at(fb)]
TONAL_CASES = [("tonal", w, nch, fb) for nch in (1, 2) for fb in TONAL_SIZES[nch] for w in _writers_at(fb)]
TABLE7_CASES = [("table7", w, nch, P.TABLE7_BYTES[nch]) for nch in (1, 2) for w in ("rate", "sparse_on")]
ALL_CASES = SIGNAL_CASES + EDGE_CASES + TONAL_CASES + TABLE7_CASES


def _id(case):
    return "-".join(str(x) for x in case)


@functools.lru_cache(maxsize=None)
def _inputs(kind, nch):
    """(spectra [n, C, 2048], window flags [n, C] or None, blocks [n] or None)"""
    if kind == "signals":
        return np.concatenate([W.specs_of(name, nch, SIG_FRAMES) for name in W.SIGNALS]), None, None
    if kind == "edges":
        e = P.edge_spectra(nch)
        return np.concatenate([sp for sp, _ in e.values()]), None, [b for sp, bl in e.values() for b in (bl or [None] * len(sp))]
    if kind == "table7":
        return P.table7_specs(nch), None, None
    # every case of the tonal writer's tests with its window flags and blocks, then the largest block on noise and on tones
    ids = [c for c in TW.writer_case_ids() if c.endswith(f"_{nch}")]
    sp = [TW.case_specs(c).reshape(6, nch, 2048) for c in ids] + [W.specs_of("noise", nch, 1), W.specs_of("tones", nch, 1)]
    fl = [np.zeros((6, nch), np.uint16) if TW.case_flags(c) is None else TW.case_flags(c).reshape(6, nch) for c in ids] + [np.zeros((2, nch), np.uint16)]
    bl = [b for c in ids for row in TW.case_blocks(c) for b in row] + [TW.largest_block(nch), TW.largest_block(nch, 1)]
    return np.concatenate(sp), np.concatenate(fl), bl


@functools.lru_cache(maxsize=None)
def _run(case):
    """the restatement's frames and records of a case and the driver's frames and bit counts under the restatement's allocation"""
    kind, writer, nch, fb = case
    sp, fl, bl = _inputs(kind, nch)
    frames, rec = P.write_restatement(writer, sp, fb, fl, bl)
    got, bits = P.ref_write(sp, fb, rec["num_quant_units"], rec["wl"], writer == "sparse_on", fl, bl)
    return frames, rec, got, bits


def _check(case):
    frames, rec, got, bits = _run(case)
    bad = [f for f in range(len(frames)) if not np.array_equal(frames[f], got[f])]
    assert bad == [], f"{_id(case)}: frames {bad} differ from the reference's"
    assert np.array_equal(bits, rec["bits"] + 3)
    return rec


@needs_ref
@pytest.mark.parametrize("case", ALL_CASES, ids=_id)
def test_frames_equal_the_references(case):
    """five signals x 6 frames under every writer and size; the edge spectra (full scale, non-finite values, silence, 2^-12, three
    times full scale, 1e-7, the allocation's special cases with the largest tonal block beside an almost empty frame, channel 1 two
    bits under channel 0); the tonal writer's cases with window flags and blocks through the reference's tail part, and the largest
    block at every size; the spectra that choose code table 7 at word length 6"""
    _check(case)


@needs_ref
def test_an_allocation_that_does_not_fit_is_refused_not_shrunk():
    """word length 7 everywhere on noise at 376 bytes: the reference asks for a repeat, and the driver ends with its own status"""
    sp = W.specs_of("noise", 2, 1)
    with pytest.raises(P.RefRepeat):
        P.ref_write(sp, 376, [32], np.full((1, 2, 32), 7, np.uint8), False)
    P.ref_write(sp, 2048, [32], np.full((1, 2, 32), 4, np.uint8), False)


# ---- what the comparison met ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wl_code_lengths():
    return [[e >> 12 for e in W.inc_tables()["AT3P_WL_VLC"][8 * i:8 * i + 8]] for i in range(4)]


def _wl_table_indices(frame, nch, N, wl):
    """the word-length code table of each channel's list by A4's rule (the first with the fewest bits from the range the
    OR-accumulated largest delta allows), checked against the two index bits the frame holds"""
    lens = _wl_code_lengths()
    bits = np.unpackbits(frame)
    out, pos = [], 3 + 5 + 1
    for ch in range(nch):
        deltas = [int(wl[0][q]) - int(wl[0][q - 1]) for q in range(1, N)] if ch == 0 else [int(wl[1][q]) - int(wl[0][q]) for q in range(N)]
        m = functools.reduce(lambda a, d: a | abs(d), deltas, 0)
        scanned = deltas if ch == 0 else deltas[1:]          # the choice does not count the list's first entry
        cand = (2, 3) if m >= 3 else (1,) if m == 2 else (0,)
        idx = min(cand, key=lambda i: (sum(lens[i][d & 7] for d in scanned), i))
        at = pos + (6 if ch == 0 else 4)
        assert int(bits[at]) * 2 + int(bits[at + 1]) == idx
        out.append(idx)
        pos += (11 if ch == 0 else 6) + sum(lens[idx][d & 7] for d in deltas)
    return out


def _coded_pairs(cases, field):
    """{(q, wl)} or {(wl, tab)} over the coded units of the cases' records"""
    out = set()
    for case in cases:
        rec = _check(case)
        for r in rec:
            for ch in range(case[2]):
                for q in range(int(r["num_quant_units"])):
                    w = int(r["wl"][ch][q])
                    if w:
                        out.add((q, w) if field == "unit" else (w, int(r["tab"][ch][q])))
    return out


@needs_ref
@pytest.mark.parametrize("sparse", [False, True], ids=["adaptive", "sparse"])
def test_every_unit_met_every_word_length(sparse, capsys):
    """on the five signals alone: all 224 pairs (unit, word length 1..7), under the adaptive writers and again under the sparse one"""
    cases = [c for c in SIGNAL_CASES if (c[1] == "sparse_on") == sparse]
    pairs = _coded_pairs(cases, "unit")
    with capsys.disabled():
        print(f"\n(unit, word length) pairs, {'sparse' if sparse else 'adaptive'}: {len(pairs)} of 224")
    assert pairs == set(itertools.product(range(32), range(1, 8)))


@needs_ref
def test_word_length_tables_unit_counts_and_clone_flags_met():
    """each of the four word-length code tables chosen for channel 0's list and for channel 1's; N = 1, an N in 2..27 and N = 32;
    in the sparse writer a channel-1 unit at 0 under a coded channel-0 unit"""
    tables, counts, clones = [set(), set()], set(), 0
    for case in ALL_CASES:
        frames, rec, _, _ = _run(case)
        _check(case)
        for f, r in enumerate(rec):
            N = int(r["num_quant_units"])
            counts.add(N)
            for ch, idx in enumerate(_wl_table_indices(frames[f], case[2], N, r["wl"])):
                tables[ch].add(idx)
            if case[1] == "sparse_on" and case[2] == 2:
                clones += int(((r["wl"][1][:N] == 0) & (r["wl"][0][:N] > 0)).sum())
    assert tables[0] == {0, 1, 2, 3} and tables[1] == {0, 1, 2, 3}, tables
    assert 1 in counts and 32 in counts and any(2 <= n <= 27 for n in counts), counts
    assert not counts & {29, 30, 31}
    assert clones > 0


def _block_costs(wl, block):
    """[8][len(blocks)] bits of every block of `block` mantissas under the eight code tables of a word length, a table's group flags
    shared out evenly (in quarter bits, as integers x 4), and the blocks; mantissas range over what rint(v * inv_mant[wl]) gives for
    |v| <= 1"""
    tb = W.inc_tables()
    mx = int(np.rint(P.float_table("AT3P_INV_MANT")[wl]))
    blocks = list(itertools.product(range(-mx, mx + 1), repeat=block))
    out = []
    for i in range(8):
        t = wl - 1 + 7 * i
        gs, nc, nbits, signed = tb["AT3P_SPEC_TAB"][2 * t] & 15, tb["AT3P_SPEC_TAB"][2 * t] >> 4, tb["AT3P_SPEC_TAB"][2 * t + 1] & 15, tb["AT3P_SPEC_TAB"][2 * t + 1] >> 4
        lens = [e >> 12 for e in tb["AT3P_VLC"][tb["AT3P_VLC_OFF"][t]:tb["AT3P_VLC_OFF"][t + 1]]]
        row = []
        for g in blocks:
            n = 0 if gs == 1 else 4 * block // (gs * nc)      # one flag per gs codes of nc mantissas each
            for p in range(0, block, nc):
                val = 0
                for k, m in enumerate(g[p:p + nc]):
                    val |= ((m & ((1 << nbits) - 1)) if signed else abs(m)) << (nbits * k)
                    n += 0 if signed or m == 0 else 4
                assert lens[val] > 0
                n += 4 * lens[val]
            row.append(n)
        out.append(row)
    return np.array(out), blocks


@needs_ref
def test_word_length_and_code_table_pairs_met(capsys):
    """54 of the 56 pairs (word length, code-table index) occur, and the other two cannot: "the first table with the fewest bits"
    never chooses index 7 at word lengths 2 and 7, whatever the mantissas are, and the test derives that from the table data.
      * (7, 7): table 55 has table 6's code lengths, coefficient width and signedness, and a group flag per four codes on top, which
        the reference's writer always sends: it costs lines / 4 bits more than index 0.
      * (2, 7): table 50 codes four mantissas at a time like tables 1 and 29 (indices 0 and 4), with a flag per two codes. For every
        one of the 625 blocks of four mantissas in -2..2 its bits, flag share included, are at least the mean of index 0's and
        index 4's; summed over a unit, one of those two is not dearer, and a tie goes to the earlier index.
      * (6, 7) can be chosen, though the five signals never do: at3p_ref_parts_lib.table7_specs holds a unit whose mantissas make
        table 54 the cheapest by 10 bits, and the case `table7` brings it to word length 6 under both writers.
    The signals alone reach 53."""
    pairs = _coded_pairs(ALL_CASES, "tab")
    on_signals = _coded_pairs(SIGNAL_CASES, "tab")
    every = set(itertools.product(range(1, 8), range(8)))
    with capsys.disabled():
        print(f"\n(word length, code table) pairs: {len(on_signals)} on the signals, {len(pairs)} in all; never met: {sorted(every - pairs)}")
        for w in range(1, 8):
            print(f"  word length {w}: tables {sorted(i for v, i in pairs if v == w)}, on the signals {sorted(i for v, i in on_signals if v == w)}")
    c7, _ = _block_costs(7, 1)
    assert (c7[7] == c7[0] + 1).all()
    c2, _ = _block_costs(2, 4)
    assert (2 * c2[7] >= c2[0] + c2[4]).all()
    c6, blocks = _block_costs(6, 2)
    unit = np.array([blocks.index(g) for g in P.TABLE7_PAIRS])
    assert c6[:, unit].sum(axis=1).argmin() == 7 and np.sort(c6[:, unit].sum(axis=1))[1] - c6[7, unit].sum() == 4 * 10
    assert pairs == every - {(2, 7), (7, 7)}
    assert len(on_signals) >= 53


# ---- the decoder's parse against the reference's integers --------------------------------------------------------------------------
def _random_allocation(rng, n, nch, sparse):
    N = rng.choice([1, 2, 5, 17, 28, 32], n)
    wl = rng.randint(0 if sparse else 1, 6, (n, 2, 32)).astype(np.uint8)
    wl[:, :, 0] = rng.randint(0 if sparse else 1, 8, (n, 2))      # 6 and 7 too, where they are cheap
    for f in range(n):
        wl[f, :, N[f]:] = 0
        wl[f, 0, N[f] - 1] = max(1, wl[f, 0, N[f] - 1])           # the highest coded unit carries a word length
    if nch == 1:
        wl[:, 1] = 0
    return N, wl


@needs_ref
@pytest.mark.parametrize("sparse", [False, True], ids=["adaptive", "sparse"])
@pytest.mark.parametrize("nch", [1, 2])
def test_unpack_gives_the_references_mantissas(nch, sparse):
    """frames the driver wrote under random allocations, which no writer of the project chose: every line of every coded unit unpacks
    to (float)m * atrac3p_mant_tab[wl] * ScaleTable[sf] (step 2 of the decoder's definition, left to right in float) with m the
    reference's integer mantissa and sf ScaleFrame's index; a unit at 0 and every line from unit N on is +0.0f"""
    n = 8
    sp = np.concatenate([W.specs_of("mix", nch, n // 2), W.specs_of("burst", nch, n // 2)])
    N, wl = _random_allocation(np.random.RandomState(11 + nch + 2 * sparse), n, nch, sparse)
    frames, bits, mant, sf = P.ref_write(sp, 2048, N, wl, sparse, mant=True)
    MANT, SCALE = P.float_table("AT3P_MANT"), P.float_table("AT3P_SCALE")
    want = np.zeros((n, nch, 2048), np.float32)
    for f in range(n):
        for ch in range(nch):
            for q in range(N[f]):
                a, b = W.QU_START[q], W.QU_START[q + 1]
                if wl[f, ch, q]:
                    want[f, ch, a:b] = (mant[f, ch, a:b].astype(np.float32) * MANT[wl[f, ch, q]]) * SCALE[sf[f, ch, q]]
    assert np.abs(mant).max() >= 20 and (np.abs(mant).reshape(n, -1).max(axis=1) > 0).all()
    got, win, fields = W.unpack(frames, nch, sparse=sparse)
    assert (fields["reason"] == 0).all() and np.array_equal(fields["n_qu"], N)
    for f in range(n):
        assert np.array_equal(fields["wl"][f, :nch, :N[f]], wl[f, :nch, :N[f]]) and np.array_equal(fields["sf"][f, :nch, :N[f]], sf[f, :, :N[f]])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if sparse:
        assert any((wl[f, :nch, :N[f]] == 0).any() for f in range(n))


# ---- the golden file ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", P.cells(), ids=lambda c: c[0])
def test_restatements_reproduce_the_golden_frames(cell):
    """tests/golden/at3p_ref_parts.npz holds frames the reference's code wrote (tools/gen_golden_at3p_ref_parts.py); the inputs are
    regenerated and their hash checked; at3p_writer_cpu.c with the flag on for the sparse cells, and with it off under every writer name
    for the adaptive ones, gives the same frames, N, word lengths and bit counts"""
    key, nch, fb, sparse, tonal = cell
    g, meta = P.golden_load()
    sp, fl, bl, sha = P.cell_inputs(nch, tonal)
    assert meta[key] == {"channels": nch, "frame_bytes": fb, "sparse": sparse, "tonal": tonal, "inputs_sha256": sha}
    n = P.G_S * P.G_F
    flat, flf, blf = sp.reshape(n, nch, 2048), None if fl is None else fl.reshape(n, nch), None if bl is None else [b for row in bl for b in row]
    for writer in (("sparse_on",) if sparse else ("sparse_off", "rate") + (("alloc",) if fb == 2048 else ())):
        frames, rec = P.write_restatement(writer, flat, fb, flf, blf)
        assert np.array_equal(frames, g[f"{key}_frames"].reshape(n, fb)), writer
        assert np.array_equal(rec["num_quant_units"], g[f"{key}_n"].reshape(n)) and np.array_equal(rec["wl"], g[f"{key}_wl"].reshape(n, 2, 32))
        assert np.array_equal(rec["bits"] + 3, g[f"{key}_bits"].reshape(n))


def test_golden_file_holds_arrays_and_one_metadata_string():
    import os
    g, meta = P.golden_load()
    keys = {c[0] for c in P.cells()}
    assert set(meta) == keys and set(g.files) == {f"{k}_{x}" for k in keys for x in ("frames", "n", "wl", "bits")} | {"meta"}
    assert all(g[k].dtype.kind in "ui" for k in g.files if k != "meta") and g["meta"].dtype.kind == "U" and g["meta"].shape == ()
    others = [os.path.getsize(os.path.join(os.path.dirname(P.GOLDEN), f)) for f in os.listdir(os.path.dirname(P.GOLDEN))
              if f.endswith(".npz") and f != os.path.basename(P.GOLDEN)]
    assert os.path.getsize(P.GOLDEN) <= max(others)
    sparse_zero = [k for k in keys if k.startswith("sparse") and any((g[f"{k}_wl"][s, f, :meta[k]["channels"], :g[f"{k}_n"][s, f]] == 0).any()
                                                                      for s in range(P.G_S) for f in range(P.G_F))]
    assert len(sparse_zero) >= 4, sparse_zero       # the sparse cells hold zeros inside the coded range


@needs_ref
def test_generator_reproduces_the_golden_file():
    g, _ = P.golden_load()
    new = P.golden_build()
    assert set(new) == set(g.files)
    for k, v in new.items():
        assert np.array_equal(np.asarray(v), g[k]), k
