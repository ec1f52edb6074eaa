"""Adaptive ATRAC3plus word lengths (include/at3phip.h, ADAPTIVE WORD LENGTHS) without a GPU: the C restatement
tests/host/at3p_writer_cpu.c writes frames the restated decoder decodes, fills the frame, gains what the definition's prototype
measured over the fixed word-length table, and holds at its edges; at3phip_host_allocate (the host-compiled library) equals its
steps A3-A5 on real and on random cost tables; the golden pins (t*, k*, N) and the frames; the kernel runs through the CPU SIMT
harness against it."""
import os

import numpy as np
import pytest

import at3p_writer_lib as W
import at3p_gha_lib as G
import at3p_tonal_lib as T
import at3p_tonal_write_lib as TW
from at3_testlib import at3p_signal, at3p_write_frames
from simt_harness_lib import CLANG, ROOT, Children, assert_clean, build_strict, run_alloc_modes

needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")
NF = W.SNR_FRAMES
# adaptive minus fixed, dB per channel: the floors the definition's prototype set (DESIGN.md section 19 lists what is measured)
SNR_FLOORS = {"noise": 12.0, "mix": 8.0, "stress": 6.0, "tones": 2.0, "burst": -0.1}

_frames = {}


def _written(name, nch):
    """(specs, frames, per-frame records) of the restatement for a signal, computed once"""
    if (name, nch) not in _frames:
        sp = W.specs_of(name, nch, NF)
        _frames[(name, nch)] = (sp,) + W.write_adaptive(sp, info=True)[:2]
    return _frames[(name, nch)]


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("name", W.SIGNALS)
def test_restatement_writes_decodable_full_frames(name, nch):
    """14 frames of each signal: the restated decoder rejects none; every frame parses to N outside 29..31 and word lengths 1..7;
    the terminator lies inside the frame; Bits(A), recounted from the parsed fields with the oracle's at3po_wordlen_bits for the
    word-length section, is the restatement's own figure, at most 16381, and the frame ends where it says."""
    sp, frames, rec = _written(name, nch)
    pcm, rej = T.cpu_tonal_decode(frames, nch)
    assert rej.sum() == 0, rej
    tail = sum(n for _, n in W.tail_bits_list(nch))
    for f in range(NF):
        p = W.parse_head(frames[f], nch)
        assert p["N"] not in (29, 30, 31) and p["N"] == rec["num_quant_units"][f]
        assert all(1 <= w <= 7 for row in p["wl"] for w in row), p["wl"]
        assert [list(rec["wl"][f][ch][:p["N"]]) for ch in range(nch)] == p["wl"]
        assert [list(rec["sfi"][f][ch][:p["N"]]) for ch in range(nch)] == p["sf"]
        _, bits, tab = W.cost_table(sp[f])
        assert p["tab"] == [[int(tab[ch][q][p["wl"][ch][q]]) for q in range(p["N"])] for ch in range(nch)]
        total, _ = W.recount_bits(p, nch, bits, tail)
        assert total == rec["bits"][f] and total <= W.SIZE_BITS, (total, rec["bits"][f])
        assert W.terminator_pos(frames[f]) == 3 + total - 1 < 2048 * 8


@pytest.mark.parametrize("name", W.SIGNALS)
def test_round_trip_snr_over_the_fixed_table(name):
    """encoder and restated decoder, adaptive against the fixed-table writer on the same spectra, per channel"""
    for nch in (1, 2):
        sp, frames, rec = _written(name, nch)
        x = G.signal_pcm(name, NF, nch)
        a, ra = T.cpu_tonal_decode(frames, nch)
        f, rf = T.cpu_tonal_decode(at3p_write_frames(sp), nch)
        assert ra.sum() == 0 and rf.sum() == 0
        sa = [G.snr_db(x[:, :, c].reshape(-1), a[:, :, c].reshape(-1), NF) for c in range(nch)]
        sf = [G.snr_db(x[:, :, c].reshape(-1), f[:, :, c].reshape(-1), NF) for c in range(nch)]
        print(f"round trip {name} x{nch}: fixed {' / '.join(f'{v:.2f}' for v in sf)} dB, adaptive {' / '.join(f'{v:.2f}' for v in sa)} dB, "
              f"mean bits {rec['bits'].mean():.0f}, units {rec['num_quant_units'].min()}..{rec['num_quant_units'].max()}")
        for c in range(nch):
            assert sa[c] >= sf[c] + SNR_FLOORS[name], (name, nch, c, sf[c], sa[c])


def test_tones_with_adaptive_word_lengths():
    """`tones`, mono, with the tone analysis: the tonal block's bits count in A4, the block is written by the adaptive writer's
    tail, and the round trip is not below the fixed table's (50.8 dB) by more than 0.1 dB"""
    x2 = at3p_signal("tones", NF, channel=0)
    x = x2.reshape(-1)
    bands = G.pqf_bands(np.concatenate([x2, np.zeros((1, 2048), np.float32)])[:, :, None])   # and the flushing frame
    blocks, resid = G.CpuToneAnalyser(1).analyse(bands)
    tones = list(blocks[1:])
    assert sum(G.n_waves(b) for b in tones) > 0
    # frame j carries the spectrum of residual j and block T_{j-1}: the alignment of tests/test_at3p_gha_cpu.py's round trip
    specs, recs = G.residual_specs(resid[1:]), [tones[j - 1] if j else None for j in range(NF)]
    fixed = G.splice_blocks(at3p_write_frames(specs), recs, 1)
    adaptive = W.write_adaptive(specs, blocks=[None if r is None else G.block_dict(r, 1) for r in recs])
    out = []
    for fr in (fixed, adaptive):
        y, rej = T.cpu_tonal_decode(fr, 1)
        assert rej.sum() == 0
        out.append(G.snr_db(x, y[:, :, 0].reshape(-1), NF))
    print(f"tones with the tone analysis: fixed {out[0]:.2f} dB, adaptive {out[1]:.2f} dB")
    assert out[0] > 50.0 and out[1] >= out[0] - 0.1, out


# ---- edge frames ----------------------------------------------------------------------------------------------------------------
def test_silence_takes_every_bit_of_word_length():
    frames, rec, _ = W.write_adaptive(np.zeros((1, 2, 2048), np.float32), info=True)
    assert rec["t"][0] == W.T_MIN and rec["num_quant_units"][0] == 32 and (rec["wl"][0] == 7).all()
    assert W.parse_head(frames[0], 2)["wl"] == [[7] * 32] * 2


def test_quiet_mono_frame_leaves_bits_unused():
    frames, rec, _ = W.write_adaptive(W.quiet_mono(), info=True)
    assert rec["t"][0] == W.T_MIN and rec["k"][0] == 0 and rec["bits"][0] < W.SIZE_BITS and (rec["wl"][0][0] == 7).all()


def test_full_scale_stereo_noise_fills_the_frame():
    frames, rec, _ = W.write_adaptive(W.full_scale_noise(3, 2), info=True)
    assert (rec["t"] > W.T_MIN).all(), rec["t"]
    assert ((rec["bits"] >= W.SIZE_BITS - 200) & (rec["bits"] <= W.SIZE_BITS)).all(), rec["bits"]
    assert T.cpu_tonal_decode(frames, 2)[1].sum() == 0


@pytest.mark.parametrize("nch", [1, 2])
def test_largest_tonal_record_still_fits(nch):
    """48 waves, both envelope points everywhere, (in stereo) the long sharing form, on full-scale noise and on silence: the frame
    decodes with its tones, the block's bits are counted, the stereo frame is full on the loud spectrum"""
    big = TW.largest_block(nch)
    part = TW.case_blocks("share_a_2")[0][2] if nch == 2 else TW.case_blocks("small_1")[1][0]   # partial sharing / 15 waves in a band
    sp = np.concatenate([W.full_scale_noise(2, nch), np.zeros((1, nch, 2048), np.float32)])
    frames, rec, _ = W.write_adaptive(sp, blocks=[big, part, big], info=True)
    tails = [sum(n for _, n in W.tail_bits_list(nch, None, b)) for b in (big, part, big)]
    assert tails[0] > 1000
    pcm, rej = T.cpu_tonal_decode(frames, nch, tones=True)
    assert rej.sum() == 0, rej
    for f in range(3):
        p = W.parse_head(frames[f], nch)
        total, _ = W.recount_bits(p, nch, W.cost_table(sp[f])[1], tails[f])
        assert total == rec["bits"][f] <= W.SIZE_BITS and W.terminator_pos(frames[f]) == 3 + total - 1
    assert nch == 1 or rec["bits"][0] >= W.SIZE_BITS - 200   # (a mono frame of full-scale noise fits at t = -21 even with the block)
    specs, win, recs, why = T.unpack_tonal(frames, nch)
    assert (why == 0).all() and (recs[:, 0] == 1).all()
    for f, b in enumerate((big, part, big)):
        assert TW.record_fields(recs[f]) == TW.expected_fields(nch, b)


# ---- at3phip_host_allocate ---------------------------------------------------------------------------------------------------------
def _host():
    from atracdenc_amd import binding
    return binding, build_strict()


@needs_clang
def test_host_allocate_equals_the_restatement_on_the_signals():
    B, path = _host()
    n = 0
    for name in W.SIGNALS + ("silence", "fullscale"):
        for nch in (1, 2):
            sp = W.specs_of(name, nch, 4)
            for f in (0, 3):
                sfi, bits, _ = W.cost_table(sp[f])
                for tail in (8, 700, 1624):
                    wl, N, t, k, _ = W.allocate(sfi, bits, tail)
                    gwl, gN, gt, gk = B.at3p_host_allocate(sfi, bits, tail, path)
                    assert (gN, gt, gk) == (N, t, k) and np.array_equal(gwl, wl), (name, nch, f, tail)
                    n += 1
    assert n == 7 * 2 * 2 * 3


@needs_clang
def test_host_allocate_equals_the_restatement_on_random_tables():
    """1000 seeded tables; among them tables that are not monotone in the word length and tables whose totals fit, fail to fit and
    fit again as t rises (counted here: the case exists in the set), where the full scan and a bisection differ"""
    B, path = _host()
    refit = nonmono = 0
    for i, (sfi, bits, tail) in enumerate(W.random_cost_tables()):
        wl, N, t, k, total = W.allocate(sfi, bits, tail)
        gwl, gN, gt, gk = B.at3p_host_allocate(sfi, bits, tail, path)
        assert (gN, gt, gk) == (N, t, k) and np.array_equal(gwl, wl), i
        nonmono += bool((np.diff(bits[:, :, 1:].astype(np.int64), axis=2) < 0).any())
        if i % 4 >= 2 and i < 400:   # the fit pattern over t, from the restatement's own pieces
            fits = [_fits(sfi, bits, tail, tt) for tt in range(W.T_MIN, W.T_MAX + 1)]
            first = fits.index(True)
            refit += not all(fits[first:])
            assert t == W.T_MIN + first
    assert nonmono >= 500 and refit >= 5, (nonmono, refit)


def _fits(sfi, bits, tail, t):
    """whether A(t, 0) fits, recounted in Python from A3 and A4"""
    nch = sfi.shape[0]
    want = np.clip((sfi.astype(np.int64) - t) // 3, 0, 7)
    top = np.nonzero(want.max(axis=0))[0]
    N = int(top[-1]) + 1 if len(top) else 1
    N = 32 if N in (29, 30, 31) else N
    wl = np.maximum(want[:, :N], 1)
    p = {"N": N, "wl": [list(map(int, wl[ch])) for ch in range(nch)]}
    return W.recount_bits(p, nch, bits, tail)[0] <= W.SIZE_BITS


def test_host_allocate_symbol_and_flag():
    from atracdenc_amd import binding as B
    hdr = open(os.path.join(ROOT, "include", "at3phip.h")).read()
    assert "#define AT3PHIP_ALLOC_ADAPTIVE 128u" in hdr and "at3phip_host_allocate(" in hdr and "ADAPTIVE WORD LENGTHS" in hdr
    assert B.AT3PHIP_ALLOC_ADAPTIVE == 128 and "at3phip_host_allocate" in B.PROTOTYPES
    for flag in ("AT3HIP_PCM_ON_DEVICE", "AT3HIP_OUT_ON_DEVICE", "AT3HIP_ASYNC", "AT3PHIP_TONES_GATED", "AT3PHIP_TONES_SHARED"):
        assert getattr(B, flag) & 128 == 0


@needs_clang
def test_a_build_without_the_adaptive_writer_refuses_the_flag(tmp_path):
    """tests/host/at3p_alloc_modes_main.cpp, `none`: at3phip.hip linked without at3p_alloc.hip (the weak symbol's other case, which
    the stand-alone host programs with their own source lists have): all six calls refuse the flag with AT3HIP_EINVAL, write
    nothing and move no state; without the flag the context works"""
    run_alloc_modes(tmp_path, "none")


# ---- the golden -------------------------------------------------------------------------------------------------------------------
def test_golden_choices_and_frame_digests():
    """tests/golden/at3p_alloc.npz (tools/gen_golden_at3p_alloc.py): (t*, k*, N) per frame and the SHA-256 of the restatement's
    frames: the definition does not drift"""
    g = np.load(W.ALLOC_GOLDEN)
    assert os.path.getsize(W.ALLOC_GOLDEN) < 100 * 1024
    for name, nch in W.ALLOC_GOLDEN_CASES:
        choice, digest = W.alloc_golden_entry(name, nch)
        assert np.array_equal(choice, g[f"{name}_{nch}_choice"]), (name, nch, choice.tolist())
        assert digest == str(g[f"{name}_{nch}_sha256"]), (name, nch)


# ---- the kernel through the CPU SIMT harness ----------------------------------------------------------------------------------------
@needs_clang
def test_harness_driver_equals_the_restatement():
    """tools/emu/run_emu_at3p_alloc.py under the strict harness: k_at3p_write_adaptive and k_at3p_write_adaptive_tonal, stereo and
    mono, signals, window flags, the largest record and non-finite spectra, in ascending and descending wavefront order and with
    every device buffer ending at a guard page"""
    build_strict()
    modes = {"plain": {}, "reverse": {"EMU_ORDER": "reverse"}, "fence": {"EMU_FENCE": "high"}}
    runs = Children({m: ("run_emu_at3p_alloc.py", ["--nobuild"], env) for m, env in modes.items()})
    try:
        for m in modes:
            assert_clean(runs.output(m), 8)
    finally:
        runs.close()
