"""ATRAC3plus rate-distortion word lengths without a GPU (include/at3phip.h, RATE-DISTORTION WORD LENGTHS): the restatement
tests/host/at3p_rd_cpu.c against its golden file; the guard's property on every golden frame and on random tables;
at3phip_host_allocate_rd against the restatement; both outcomes of the guard, one of them on a table built for it; the frame that
fits with every word length 7; the J_MAX bound from the code tables; the flag's refusals; every frame parsed, recounted and decoded as
the sparse frame it is; and, where the reference is built, its own part coders under the chosen allocation; the kernels' properties."""
import os
import re
import subprocess

import numpy as np
import pytest

import at3p_writer_lib as W
import at3p_ref_parts_lib as P
import simt_harness_lib as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "at3phip.h")).read()
needs_ref = pytest.mark.skipif(not P.have_ref(), reason="oracle/_ref not built")
SIZES = {1: (176, 376, 744, 2048), 2: (224, 376, 744, 2048)}
N_FRAMES = 3

_cache = {}


def _written(name, nch, fb):
    """(spectra, frames, records, tail bits) of the restatement on 3 frames of a signal"""
    key = (name, nch, fb)
    if key not in _cache:
        sp = W.specs_of(name, nch, N_FRAMES)
        _cache[key] = (sp,) + W.write_rd(sp, fb, info=True)
    return _cache[key]


CELLS = [(name, nch, fb) for name in W.SIGNALS for nch in (1, 2) for fb in SIZES[nch]]


# ---- 1. golden -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nch,fb", W.RD_GOLDEN_CASES, ids=[f"{n}_{c}_{fb}" for n, c, fb in W.RD_GOLDEN_CASES])
def test_restatement_equals_the_golden_file(name, nch, fb):
    """tests/golden/at3p_rd.npz (tools/gen_golden_at3p_rd.py): frames, j*, k*, N, the guard's outcome, word lengths and both T, bit for
    bit; and on each of its frames the guard's property, T recomputed here from the tables: the written allocation's never exceeds the
    sparse allocation's"""
    gold = np.load(W.RD_GOLDEN)
    got = W.rd_golden_entry(name, nch, fb)
    for k, v in got.items():
        want = gold[f"{name}_{nch}_{fb}_{k}"]
        assert want.shape == np.asarray(v).shape and np.array_equal(want, v), (name, nch, fb, k)
    sp = W.specs_of(name, nch, W.RD_GOLDEN_FRAMES)
    nbits = W.write_rd(sp, fb, info=True)[2]
    for f in range(W.RD_GOLDEN_FRAMES):
        sfi, bits, dist = W.tables(sp[f])
        wl_a = W.allocate(sfi, bits, nbits[f], fb, True)[0]
        t_written, t_sparse = W.total_distortion(sfi, dist, got["wl"][f][:nch]), W.total_distortion(sfi, dist, wl_a)
        assert t_written <= t_sparse
        assert t_sparse == got["T"][f, 1] and t_written == (got["T"][f, 0] if got["choice"][f, 3] else t_sparse)


def test_golden_file_holds_what_it_should():
    gold = np.load(W.RD_GOLDEN)
    assert sorted(gold.files) == sorted(f"{n}_{c}_{fb}_{k}" for n, c, fb in W.RD_GOLDEN_CASES for k in ("frames", "choice", "wl", "T"))
    assert os.path.getsize(W.RD_GOLDEN) < 64 * 1024
    chose = np.concatenate([gold[f"{n}_{c}_{fb}_choice"][:, 3] for n, c, fb in W.RD_GOLDEN_CASES])
    assert (chose == 1).sum() >= 6 and (chose == 0).sum() >= 3   # both outcomes of the guard


def test_restatement_and_host_functions_equal_what_they_gave_before_the_fold():
    """tests/golden/at3p_rd_fold.npz, written before the rate-distortion and the masking-weighted stack became one (DESIGN.md, section
    24.1): on at3p_psy_lib.random_tables in hundreds and on the signals' cells, every named field of the restatement and of
    at3phip_host_allocate_rd and at3phip_host_allocate_psy - rate-distortion, masking-weighted with the offsets given and with M1-M3's -
    and the frames of write_rd and write_psy, digest for digest; the inputs' digests among them"""
    import at3p_psy_lib as Y
    gold = np.load(Y.RD_FOLD_GOLDEN)
    want = dict(zip(gold["labels"].tolist(), gold["sha256"]))
    got = Y.rd_fold_entries()
    assert list(got) == list(want)
    differ = [k for k in got if not np.array_equal(got[k], want[k])]
    assert not differ, differ


def test_fold_golden_file_holds_what_it_should():
    import at3p_psy_lib as Y
    gold = np.load(Y.RD_FOLD_GOLDEN)
    assert sorted(gold.files) == ["labels", "sha256"] and os.path.getsize(Y.RD_FOLD_GOLDEN) < 64 * 1024
    labels = [f"t{g:02d}_{k}" for g in range(20) for k in ("in", "rd_rest", "rd_host", "psy_rest", "psy_host", "m_rest", "m_host")]
    labels += [f"{n}_{c}_{fb}_{k}" for n, c, fb in Y.CELLS for k in ("in", "rd", "psy")]
    assert gold["labels"].tolist() == labels and gold["sha256"].shape == (len(labels), 32) and gold["sha256"].dtype == np.uint8
    # (a cell's spectra do not depend on its frame size: the 32 cells' `in` digests are 8 different ones; all others differ)
    assert len({bytes(d) for d in gold["sha256"]}) == len(labels) - 24


# ---- 2. the host function, the guard ---------------------------------------------------------------------------------------------------
def _same(host, wl, N, rec):
    hw, hN, hj, hk, hrd = host
    return np.array_equal(hw, wl) and (hN, hj, hk, hrd) == (N, int(rec["j"]), int(rec["k"]), bool(rec["chose"]))


def test_host_allocate_rd_equals_the_restatement_on_the_signals():
    from atracdenc_amd.binding import at3p_host_allocate_rd
    seen = set()
    for name, nch, fb in CELLS:
        sp, frames, rec, nbits = _written(name, nch, fb)
        for f in range(N_FRAMES):
            sfi, bits, dist = W.tables(sp[f])
            wl, N, r = W.allocate_rd(sfi, bits, dist, nbits[f], fb)
            assert _same(at3p_host_allocate_rd(sfi, bits, dist, nbits[f], fb), wl, N, r), (name, nch, fb, f)
            assert np.array_equal(wl, rec["wl"][f][:nch]) and N == rec["num_quant_units"][f]
            seen.add(int(r["chose"]))
    assert seen == {0, 1}   # R(j*, k*) and the fallback are both reached on the signals


def test_guard_property_and_host_function_on_2000_random_tables():
    """at3phip_host_allocate_rd on random cost and distortion tables: the restatement's choice, and the allocation it returns never
    has more distortion than the sparse allocation of the same tables (T recomputed here)"""
    from atracdenc_amd.binding import at3p_host_allocate, at3p_host_allocate_rd
    fell = 0
    for i, (sfi, bits, dist, tail) in enumerate(W.random_dist_tables(W.random_cost_tables(2000))):
        nch = sfi.shape[0]
        fb = SIZES[nch][i % 4]
        tail = min(tail, 8 * fb - 3)   # (the argument's range)
        host = at3p_host_allocate_rd(sfi, bits, dist, tail, fb)
        wl, N, r = W.allocate_rd(sfi, bits, dist, tail, fb)
        assert _same(host, wl, N, r), i
        wl_a = at3p_host_allocate(sfi, bits, tail, frame_bytes=fb, sparse=True)[0]
        t_w, t_a = W.total_distortion(sfi, dist, host[0]), W.total_distortion(sfi, dist, wl_a)
        assert t_w <= t_a, i
        assert t_a == r["T_sparse"] and (t_w == r["T"] if host[4] else np.array_equal(host[0], wl_a)), i
        fell += not host[4]
    assert fell > 0


def test_the_guard_fires_on_the_table_built_for_it():
    from atracdenc_amd.binding import at3p_host_allocate, at3p_host_allocate_rd
    sfi, bits, dist, tail, fb = W.guard_table()
    wl, N, r = W.allocate_rd(sfi, bits, dist, tail, fb)
    assert r["chose"] == 0 and r["T"] > r["T_sparse"] and wl[0, 0] == 3 and not wl[0, 1:].any() and N == 1
    assert _same(at3p_host_allocate_rd(sfi, bits, dist, tail, fb), wl, N, r)
    assert np.array_equal(wl, at3p_host_allocate(sfi, bits, tail, frame_bytes=fb, sparse=True)[0])
    # R(j*, k*) itself: the empty frame, whose closing rule gives unit 0 word length 1
    assert r["T"] == W.total_distortion(sfi, dist, np.eye(1, 32, dtype=np.uint8))


def test_host_allocate_rd_checks_its_arguments():
    from atracdenc_amd.binding import At3HipError, at3p_host_allocate_rd
    sfi, bits, dist, tail, fb = W.guard_table()
    big = dist.copy()
    big[0, 5, 2] = (1 << 47) + 1
    for bad in ((sfi, bits, big, tail, fb), (sfi, bits, dist, tail, 168), (sfi, bits, dist, -1, fb), (sfi + 64, bits, dist, tail, fb)):
        with pytest.raises(At3HipError):
            at3p_host_allocate_rd(*bad)


# ---- 3. properties of the definition ---------------------------------------------------------------------------------------------------
def test_a_frame_that_fits_with_every_word_length_7_is_the_sparse_frame():
    """quiet white noise in 2048 bytes fits at t = -21 and at J_MIN, both rules give word length 7 everywhere: byte for byte the frame
    AT3PHIP_ALLOC_SPARSE writes (and AT3PHIP_ALLOC_ADAPTIVE alone)"""
    sp = W.quiet_mono(2)
    frames, rec, _ = W.write_rd(sp, 2048, info=True)
    assert (rec["j"] == W.J_MIN).all() and (rec["t"] == W.T_MIN).all() and (rec["wl"][:, 0] == 7).all() and (rec["chose"] == 1).all()
    assert np.array_equal(frames, W.write_adaptive(sp, 2048, True)) and np.array_equal(frames, W.write_adaptive(sp, 2048, False))


def test_j_max_bound_from_the_code_tables():
    """R3: at J_MAX every unit picks 0. Re-derived from at3p_vlc.inc: the fewest bits of a 16-line chunk under any table, then the
    smallest j with lambda_j / 2^40 >= lines / (chunks * that + 3) for every unit size; and the header's weaker premise (one bit per
    chunk) gives J_MAX itself. Then the scan on the tables at their worst: full-scale distortion at w = 0, none above, the cheapest bits."""
    cmin = W.min_chunk_bits()
    assert cmin >= 1 and W.j_max_bound() <= W.J_MAX
    sc = W.scale_table().astype(np.float64)
    assert all(sc[i + 3] == 2 * sc[i] for i in range(61)) and sc[63] == 1.0
    lam = lambda j: sc[j % 3] ** 2 * 4.0 ** (j // 3)
    need = max(n / (n // 16 + 3) for n in (16, 32, 64, 128))
    assert lam(W.J_MAX) >= need > lam(W.J_MAX - 1)
    assert (W.J_MAX - W.J_MIN + 1) % 4 == 0
    from atracdenc_amd.binding import at3p_host_allocate_rd
    sfi = np.full((2, 32), 63, np.uint8)
    bits = np.zeros((2, 32, 8), np.uint16)
    bits[:, :, 1:] = (W.LINES // 16 * cmin)[None, :, None]
    dist = np.zeros((2, 32, 8), np.uint64)
    dist[:, :, 0] = W.LINES.astype(np.uint64)[None, :] << np.uint64(40)
    wl, N, j, k, rd = at3p_host_allocate_rd(sfi, bits, dist, 1624, 224)   # the largest stereo tail at the smallest stereo size
    # 165 bits are left: nothing but R's smallest frame fits, and the scan finds it first where the bound says every pick is 0 (what
    # is written is A(t*, k*): the guard prefers its one coded unit to none)
    assert (j, k) == (W.j_max_bound(), 0) and not rd and N >= 1


def test_symbols_and_flags():
    from atracdenc_amd import binding as B
    assert B.AT3PHIP_ALLOC_RD == 512 == int(re.search(r"#define AT3PHIP_ALLOC_RD (\d+)u", HEADER).group(1))
    assert "at3phip_host_allocate_rd" in B.PROTOTYPES and "at3phip_host_allocate_rd(" in HEADER
    assert hasattr(B.load_library(), "at3phip_host_allocate_rd")
    for bad in ((False, False, True), (True, False, True), (False, True, True)):
        with pytest.raises(ValueError):
            B._alloc_flag(*bad)
    assert B._alloc_flag(True, True, True) == 896 and B._alloc_flag(True, True) == 384 and B._alloc_flag(True) == 128 and B._alloc_flag(False) == 0


@pytest.mark.skipif(not os.path.exists(H.CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")
def test_a_build_without_the_rate_distortion_writer_refuses_the_flag(tmp_path):
    """tests/host/at3p_alloc_modes_main.cpp, `alloc+sparse`: at3phip.hip linked with at3p_alloc.hip and at3p_sparse.hip but not
    at3p_rd.hip; the adaptive and the sparse calls work at both sizes, all six calls refuse ADAPTIVE | SPARSE | RD because the build
    has no rate-distortion writer, write nothing and move no state"""
    H.run_alloc_modes(tmp_path, "alloc+sparse")


# ---- 4. the frames are sparse frames -------------------------------------------------------------------------------------------------
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
    """the reference's TWordLenEncoder, TSfIdxEncoder, TQuantUnitsEncoder's units and tail under the allocation R4 wrote, put together
    by at3p_ref_parts_lib's driver as for sparse frames: the frames byte for byte, Bits + 3 bits long"""
    for name in ("noise", "tones", "mix"):
        sp, frames, rec, _ = _written(name, nch, fb)
        ref, bits = P.ref_write(sp, fb, rec["num_quant_units"], rec["wl"], True)
        assert np.array_equal(ref, frames), name
        assert np.array_equal(bits, rec["bits"] + 3), name


# ---- 5. the kernels' properties -------------------------------------------------------------------------------------------------------
def _device_asm(src):
    return subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "--cuda-device-only",
                           "-S", "-o", "-", os.path.join(ROOT, "atracdenc_amd", "csrc", src)], capture_output=True, text=True, check=True).stdout


def _writer_kernels(asm, marks):
    out = {}
    for mark in marks:
        m = re.search(r"^(_ZN4at3p\d+k_at3p_write_adaptive_withINS_\d+" + mark + r"E\w*):[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M)
        assert m, mark
        meta = re.search(r"\.amdhsa_kernel " + re.escape(m.group(1)) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S)
        out[mark] = (m.group(2), meta.group(1))
    return out


def test_rd_kernels_have_no_fma_division_or_scratch_of_their_own():
    """DESIGN.md section 12's properties for the two new kernels. A1's sixteen float divisions per thread are the reference's and are
    in every adaptive writer kernel as IEEE division sequences (v_div_*, v_fma_f32 inside them): the new kernels hold exactly as many
    of those as the sparse kernels and nothing else of the kind - no fused or contracted multiply-add in f32 beyond them, none at all
    in f64, no f64 division, no scratch. R1-R4 show as ds_add_u64, v_mul_f64 and v_add_f64."""
    rd = _writer_kernels(_device_asm("at3p_rd.hip"), ("WriteParamsRd", "WriteParamsTonalRd"))
    sparse = _writer_kernels(_device_asm("at3p_sparse.hip"), ("WriteParamsSparse", "WriteParamsTonalSparse"))
    count = lambda body, pat: len(re.findall(pat, body))
    for mark, ref in (("WriteParamsRd", "WriteParamsSparse"), ("WriteParamsTonalRd", "WriteParamsTonalSparse")):
        body, meta = rd[mark]
        for pat in (r"\bv_(?:pk_)?fmac?_\w+", r"\bv_div_\w+", r"\bv_rcp_\w+", r"\bv_mad_\w*f\d+\w*"):
            assert count(body, pat) == count(sparse[ref][0], pat), (mark, pat)
        assert count(body, r"\bv_div_\w+") == 16 * 4   # div_scale twice, div_fmas, div_fixup per division
        assert not re.findall(r"\bv_(?:fma|fmac|div_\w+|rcp|mad)_f64", body), mark
        assert not re.findall(r"\bscratch_\w+|\bbuffer_(?:load|store)_\w+", body), mark
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta), mark
        assert "ds_add_u64" in body and "v_mul_f64" in body and "v_add_f64" in body, mark
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
        assert lds <= 40 * 1024 and vgpr <= 128, (mark, lds, vgpr)   # four workgroups per CU by LDS, two waves per SIMD by registers
