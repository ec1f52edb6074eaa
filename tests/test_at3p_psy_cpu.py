"""ATRAC3plus masking-weighted word lengths without a GPU (include/at3phip.h, MASKING-WEIGHTED WORD LENGTHS): the restatement
tests/host/at3p_rd_cpu.c with psy against its golden file, with the guard's property recomputed on every frame; at3phip_host_allocate_psy against
the restatement on the signals' tables and on random tables with random offsets; zero offsets give the rate-distortion choice; the masked
twin, the one test of behaviour; the definition's edges; the table generator; the argument checks; every frame parsed, recounted and
decoded as the sparse frame it is; and, where the reference is built, its own part coders under the chosen allocation."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import at3p_psy_lib as Y
import at3p_ref_parts_lib as P
import at3p_writer_lib as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "at3phip.h")).read()
needs_ref = pytest.mark.skipif(not P.have_ref(), reason="oracle/_ref not built")
N_FRAMES = 3
CELLS = Y.CELLS

_cache = {}


def _written(name, nch, fb):
    """(spectra, frames, records, tail bits) of the restatement on 3 frames of a signal"""
    key = (name, nch, fb)
    if key not in _cache:
        sp = W.specs_of(name, nch, N_FRAMES)
        _cache[key] = (sp,) + Y.write_psy(sp, fb, info=True)
    return _cache[key]


_random_tables = Y.random_tables


def _same(host, wl, N, rec):
    hw, hN, hj, hk, hp, ho = host
    nch = hw.shape[0]
    return (np.array_equal(hw, wl) and (hN, hj, hk, hp) == (N, int(rec["j"]), int(rec["k"]), bool(rec["chose"]))
            and np.array_equal(ho, rec["o"][:nch]))


# ---- 1. golden -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nch,fb", Y.PSY_GOLDEN_CASES, ids=[f"{n}_{c}_{fb}" for n, c, fb in Y.PSY_GOLDEN_CASES])
def test_restatement_equals_the_golden_file(name, nch, fb):
    """tests/golden/at3p_psy.npz (tools/gen_golden_at3p_rd.py --mode psy): frames, j*, k*, N, the guard's outcome, O, the offsets, word lengths and
    both Tw, bit for bit; and on each of its frames the guard's property, Tw recomputed here from the tables and the offsets, themselves
    recomputed here from M1-M3's text: the written allocation's never exceeds the sparse allocation's"""
    gold = np.load(Y.PSY_GOLDEN)
    got = Y.psy_golden_entry(name, nch, fb)
    for k, v in got.items():
        want = gold[f"{name}_{nch}_{fb}_{k}"]
        assert want.shape == np.asarray(v).shape and np.array_equal(want, v), (name, nch, fb, k)
    sp = W.specs_of(name, nch, Y.PSY_GOLDEN_FRAMES)
    nbits = Y.write_psy(sp, fb, info=True)[2]
    for f in range(Y.PSY_GOLDEN_FRAMES):
        sfi, bits, dist = W.tables(sp[f])
        _, o, O = Y.offsets_py(sfi, dist)
        assert np.array_equal(o, got["o"][f][:nch]) and O == got["choice"][f, 4]
        wl_a = W.allocate(sfi, bits, nbits[f], fb, True)[0]
        t_written, t_sparse = Y.weighted_total(sfi, dist, got["wl"][f][:nch], o), Y.weighted_total(sfi, dist, wl_a, o)
        assert t_written <= t_sparse
        assert t_sparse == got["Tw"][f, 1] and t_written == (got["Tw"][f, 0] if got["choice"][f, 3] else t_sparse)


def test_golden_file_holds_what_it_should():
    gold = np.load(Y.PSY_GOLDEN)
    assert sorted(gold.files) == sorted(f"{n}_{c}_{fb}_{k}" for n, c, fb in Y.PSY_GOLDEN_CASES for k in ("frames", "choice", "o", "wl", "Tw"))
    assert os.path.getsize(Y.PSY_GOLDEN) < 64 * 1024
    O = np.concatenate([gold[f"{n}_{c}_{fb}_choice"][:, 4] for n, c, fb in Y.PSY_GOLDEN_CASES])
    assert O.min() > 0 and O.max() <= Y.O_MAX   # every frame is weighted


# ---- 2. the host function ----------------------------------------------------------------------------------------------------------------
def test_host_allocate_psy_equals_the_restatement_on_the_signals():
    from atracdenc_amd.binding import at3p_host_allocate_psy
    for name, nch, fb in CELLS:
        sp, frames, rec, nbits = _written(name, nch, fb)
        for f in range(N_FRAMES):
            sfi, bits, dist = W.tables(sp[f])
            wl, N, r = Y.allocate_psy(sfi, bits, dist, nbits[f], fb)
            assert _same(at3p_host_allocate_psy(sfi, bits, dist, nbits[f], fb), wl, N, r), (name, nch, fb, f)
            assert np.array_equal(wl, rec["wl"][f][:nch]) and N == rec["num_quant_units"][f] and np.array_equal(r["o"], rec["o"][f])
            mu, o, O = Y.offsets_py(sfi, dist)
            assert np.array_equal(mu, r["mu"][:nch]) and np.array_equal(o, r["o"][:nch]) and O == r["O"], (name, nch, fb, f)
            wl_a = W.allocate(sfi, bits, nbits[f], fb, True)[0]
            assert Y.weighted_total(sfi, dist, wl, o) <= Y.weighted_total(sfi, dist, wl_a, o)


def test_guard_property_and_host_function_on_2000_random_tables_with_random_offsets():
    """at3phip_host_allocate_psy with the offsets given: the restatement's choice, and the allocation it returns never has more weighted
    distortion than the sparse allocation of the same tables (Tw recomputed here); both outcomes of the guard occur"""
    from atracdenc_amd.binding import at3p_host_allocate, at3p_host_allocate_psy
    fell = 0
    for i, (sfi, bits, dist, tail, off, fb) in enumerate(_random_tables()):
        host = at3p_host_allocate_psy(sfi, bits, dist, tail, fb, offsets=off)
        wl, N, r = Y.allocate_psy(sfi, bits, dist, tail, fb, off)
        assert _same(host, wl, N, r) and np.array_equal(host[5], off) and r["O"] == off.max(), i
        wl_a = at3p_host_allocate(sfi, bits, tail, frame_bytes=fb, sparse=True)[0]
        t_w, t_a = Y.weighted_total(sfi, dist, host[0], off), Y.weighted_total(sfi, dist, wl_a, off)
        assert t_w <= t_a, i
        assert t_a == r["T_sparse"] and (t_w == r["T"] if host[4] else np.array_equal(host[0], wl_a)), i
        assert W.J_MIN - int(off.max()) <= host[2] <= W.J_MAX
        fell += not host[4]
    assert 0 < fell < 2000
    # and with the offsets left to M1-M3, on every fourth table
    for i, (sfi, bits, dist, tail, _, fb) in enumerate(_random_tables()[::4]):
        host = at3p_host_allocate_psy(sfi, bits, dist, tail, fb)
        wl, N, r = Y.allocate_psy(sfi, bits, dist, tail, fb)
        assert _same(host, wl, N, r) and np.array_equal(Y.offsets_py(sfi, dist)[1], host[5]), i


# ---- 3. zero offsets ---------------------------------------------------------------------------------------------------------------------
def test_zero_offsets_give_the_rate_distortion_choice():
    """the consequence the header states: with every offset 0, wl, N, j*, k* and the outcome are at3phip_host_allocate_rd's, on the 2000
    tables and on the signals' tables"""
    from atracdenc_amd.binding import at3p_host_allocate_psy, at3p_host_allocate_rd
    cases = [(sfi, bits, dist, tail, fb) for sfi, bits, dist, tail, _, fb in _random_tables()]
    for name, nch, fb in CELLS:
        sp, _, _, nbits = _written(name, nch, fb)
        cases += [W.tables(sp[f]) + (int(nbits[f]), fb) for f in range(N_FRAMES)]
    for i, (sfi, bits, dist, tail, fb) in enumerate(cases):
        got = at3p_host_allocate_psy(sfi, bits, dist, tail, fb, offsets=np.zeros(sfi.shape, np.uint8))
        want = at3p_host_allocate_rd(sfi, bits, dist, tail, fb)
        assert np.array_equal(got[0], want[0]) and got[1:5] == want[1:5] and not got[5].any(), i
        wl, N, r = Y.allocate_psy(sfi, bits, dist, tail, fb, np.zeros(sfi.shape, np.uint8))
        wr, Nr, rr = W.allocate_rd(sfi, bits, dist, tail, fb)
        assert np.array_equal(wl, wr) and N == Nr and (r["j"], r["k"], r["chose"], r["T"], r["T_sparse"]) == (
            rr["j"], rr["k"], rr["chose"], rr["T"], rr["T_sparse"]), i


# ---- 4. the masked twin --------------------------------------------------------------------------------------------------------------------
def test_the_masked_twin_gets_fewer_bits_than_its_unmasked_copy():
    """at3p_psy_lib.masked_twin: unit 1 loud, units 2 and 7 line for line the same 16 values 30 dB below it; unit 2 is next to the masker,
    unit 7 six Bark up. Three units fill no admissible frame, so the budget is made to bind by the tail, which is an input of the allocators:
    at 176 bytes the tail is walked up in steps of 25 bits to the first one at which the rate-distortion restatement gives the twins equal
    word lengths above 0 (their tables are equal, so it tells them apart only by the raise list's walk). There the weighted choice gives
    unit 2 less than unit 7, its offset is the larger one, and the host function agrees."""
    from atracdenc_amd.binding import at3p_host_allocate_psy
    sfi, bits, dist = W.tables(Y.masked_twin()[0])
    assert np.array_equal(bits[0, 2], bits[0, 7]) and np.array_equal(dist[0, 2], dist[0, 7]) and sfi[0, 2] == sfi[0, 7]
    found = 0
    for tail in range(905, 1300, 25):
        wr = W.allocate_rd(sfi, bits, dist, tail, 176)[0]
        if not (wr[0, 2] == wr[0, 7] > 0 and wr[0, 2] < 7):
            continue
        found += 1
        wp, N, r = Y.allocate_psy(sfi, bits, dist, tail, 176)
        print(f"tail {tail}: rd {wr[0, [1, 2, 7]].tolist()} psy {wp[0, [1, 2, 7]].tolist()} o {r['o'][0, [1, 2, 7]].tolist()}")
        assert wp[0, 2] < wp[0, 7] and r["o"][0, 2] > r["o"][0, 7] and r["chose"] == 1, tail
        assert _same(at3p_host_allocate_psy(sfi, bits, dist, tail, 176), wp, N, r)
    assert found >= 2


# ---- 5. edges and structure ------------------------------------------------------------------------------------------------------------------
def test_a_frame_with_no_live_unit_has_zero_offsets_and_is_the_smallest_frame():
    for nch, fb in ((1, 176), (2, 224), (2, 2048)):
        sp = np.zeros((1, nch, 2048), np.float32)
        frames, rec, _ = Y.write_psy(sp, fb, info=True)
        assert not rec["o"].any() and rec["O"][0] == 0 and rec["num_quant_units"][0] == 1
        assert rec["wl"][0].sum() == 1 and rec["wl"][0, 0, 0] == 1
        assert np.array_equal(frames, W.write_rd(sp, fb))


def test_a_unit_under_the_threshold_in_quiet_alone_takes_mu_from_ath():
    """one line at 2^-19, in one unit at a time: its energy, 2^-38, is index 6 of lambda, below the lowest ath entry (7), so no masker
    reaches any threshold - its own unit's least of all, 6 steps further down - and mu is the ath table in every unit; one live unit has
    offset 0"""
    _, ath = Y.psy_tables()
    for qu in (0, 13, 31):
        sp = np.zeros((1, 2048), np.float32)
        sp[0, W.QU_START[qu]] = 2.0 ** -19
        sfi, bits, dist = W.tables(sp)
        assert dist[0, qu, 0] > 0
        wl, N, r = Y.allocate_psy(sfi, bits, dist, 10, 176)
        assert np.array_equal(r["mu"][0], ath) and np.array_equal(Y.offsets_py(sfi, dist)[0][0], ath) and not r["o"].any()


def test_offsets_are_clipped_at_32_and_the_clip_is_reached():
    """M3's clip. Over the first frames of `tones`, `burst` and `stress`: wherever the spread of mu over the live units exceeds 32 the
    largest offset is 32 exactly, elsewhere it is the spread, and the clip occurred. With the committed tables it occurs on `burst`
    (frame 0) and `stress` (frame 7); `tones`, on which a sketch of this definition saw it, spreads over 28 steps."""
    clipped = []
    for name, n in (("tones", 3), ("burst", 3), ("stress", 8)):
        sp = W.specs_of(name, 1, n)
        _, rec, _ = Y.write_psy(sp, 376, info=True)
        for f in range(n):
            live = W.tables(sp[f])[2][0, :, 0] > 0
            spread = int(rec["mu"][f, 0][live].max() - rec["mu"][f, 0][live].min())
            assert rec["O"][f] == min(spread, Y.O_MAX) == rec["o"][f].max()
            if spread > Y.O_MAX:
                clipped.append((name, f, spread))
    print(clipped)
    assert clipped


def test_a_frame_that_fits_with_every_word_length_7_is_the_sparse_frame():
    sp = W.quiet_mono(2)
    frames, rec, _ = Y.write_psy(sp, 2048, info=True)
    assert (rec["wl"][:, 0] == 7).all() and (rec["j"] == W.J_MIN - rec["O"]).all() and (rec["t"] == W.T_MIN).all()
    assert np.array_equal(frames, W.write_adaptive(sp, 2048, True)) and np.array_equal(frames, W.write_adaptive(sp, 2048, False))


def test_table_generator_check_and_the_header_prints_the_tables():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_at3p_psy.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    spread, ath = Y.psy_tables()
    sec = HEADER[HEADER.index("MASKING-WEIGHTED WORD LENGTHS (AT3PHIP_ALLOC_PSY"):HEADER.index("#define AT3PHIP_ALLOC_PSY")]
    rows = [[int(x) for x in ln.strip(" *").split()] for ln in sec.splitlines() if re.fullmatch(r" \*(\s+\d+){32}", ln)]
    assert np.array_equal(np.array(rows[:32]), spread) and rows[32] == ath.tolist() and len(rows) == 33
    assert ((spread <= 63) | (spread == 255)).all() and (np.diag(spread) == 6).all() and ath.max() <= Y.MU_HI
    # lambda_73 is the largest lambda_i not above 2^47
    assert Y.lam(Y.MU_HI) <= 2.0 ** 47 < Y.lam(Y.MU_HI + 1)


def test_host_allocate_psy_checks_its_arguments():
    from atracdenc_amd.binding import At3HipError, at3p_host_allocate_psy
    sfi, bits, dist, tail, fb = W.guard_table()
    big = dist.copy()
    big[0, 5, 2] = (1 << 47) + 1
    off = np.zeros((1, 32), np.uint8)
    off[0, 9] = 33
    for bad in ((sfi, bits, big, tail, fb, None), (sfi, bits, dist, tail, 168, None), (sfi, bits, dist, -1, fb, None), (sfi + 64, bits, dist, tail, fb, None),
                (sfi, bits, dist, tail, fb, off)):
        with pytest.raises(At3HipError):
            at3p_host_allocate_psy(*bad)
    off[0, 9] = 32
    assert at3p_host_allocate_psy(sfi, bits, dist, tail, fb, off)[5][0, 9] == 32
    # the guard's table with zero offsets: the fallback, as at3phip_host_allocate_rd falls back
    wl, N, j, k, psy, o = at3p_host_allocate_psy(sfi, bits, dist, tail, fb, np.zeros((1, 32), np.uint8))
    assert not psy and wl[0, 0] == 3


def test_symbols_and_flags():
    from atracdenc_amd import binding as B
    assert B.AT3PHIP_ALLOC_PSY == 1024 == int(re.search(r"#define AT3PHIP_ALLOC_PSY (\d+)u", HEADER).group(1))
    assert "at3phip_host_allocate_psy" in B.PROTOTYPES and "at3phip_host_allocate_psy(" in HEADER
    assert hasattr(B.load_library(), "at3phip_host_allocate_psy")
    for bad in ((False, False, False, True), (True, True, False, True), (True, False, True, True), (False, True, True, True)):
        with pytest.raises(ValueError):
            B._alloc_flag(*bad)
    assert B._alloc_flag(True, True, True, True) == 1920 and B._alloc_flag(True, True, True) == 896
    import inspect
    for name in ("write_frames", "encode_frames", "encode_frames_s16", "encode_frames_tonal", "encode_frames_tonal_s16", "encode_frames_device",
                 "encode_frames_device_s16", "encode_frames_tonal_device", "encode_frames_tonal_device_s16"):
        assert inspect.signature(getattr(B.At3pHip, name)).parameters["psy"].default is False, name


# ---- 6. the frames are sparse frames -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
def test_frames_parse_recount_and_decode_as_sparse_frames(nch):
    """every frame of the signals at four sizes: the head read back by at3p_writer_lib.parse_head holds the record's allocation,
    count_bits of it equals the reported bits, which fit; the sparse restatement decoder rejects none"""
    for name, c, fb in CELLS:
        if c != nch:
            continue
        sp, frames, rec, nbits = _written(name, nch, fb)
        for f in range(N_FRAMES):
            head = W.parse_head(frames[f], nch)
            N = int(rec["num_quant_units"][f])
            assert head["N"] == N and all(head["wl"][ch] == rec["wl"][f][ch][:N].tolist() for ch in range(nch)), (name, fb, f)
            unit_bits = W.tables(sp[f])[1]
            assert W.count_bits(head, nch, unit_bits, int(nbits[f])) == rec["bits"][f] <= 8 * fb - 3, (name, fb, f)
        assert W.decode(frames, nch, False, True)[1].sum() == 0, (name, fb)


@needs_ref
@pytest.mark.parametrize("nch,fb", [(1, 176), (1, 376), (2, 376), (2, 744), (2, 2048)])
def test_the_references_part_coders_write_the_same_bytes(nch, fb):
    """the reference's TWordLenEncoder, TSfIdxEncoder, TQuantUnitsEncoder's units and tail under the allocation M6 wrote, put together
    by at3p_ref_parts_lib's driver as for sparse frames: the frames byte for byte, Bits + 3 bits long"""
    for name in ("noise", "tones", "mix"):
        sp, frames, rec, _ = _written(name, nch, fb)
        ref, bits = P.ref_write(sp, fb, rec["num_quant_units"], rec["wl"], True)
        assert np.array_equal(ref, frames), name
        assert np.array_equal(bits, rec["bits"] + 3), name
