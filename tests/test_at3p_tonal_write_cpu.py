"""at3phip_write_frames_tonal without a GPU: the goldens against the reference where it is built, the kernel's instantiation with
tonal records through the CPU SIMT harness (strict checks, both wavefront orders, guard pages) against the goldens, the written
blocks parsed back, the host-side contract rule by rule, the bound that makes the reference's abort() branch unreachable, and
the exported symbol."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import at3p_tonal_lib as T
import at3p_tonal_write_lib as L
from simt_harness_lib import CLANG, ROOT, Children, assert_clean, build_strict

needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")
needs_ref = pytest.mark.skipif(not L.have_ref(), reason="needs oracle/_ref and the reference sources")


@pytest.fixture(scope="module")
def golden():
    return np.load(L.GOLDEN)


# ---- the goldens are the reference's ------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("cid", L.writer_case_ids())
def test_writer_goldens_equal_the_reference(golden, cid):
    """Spectra from the stored seed, blocks from the stored ints: the reference's WriteFrame writes the stored frames; through
    at3p_tonal_lib.ref_write_tonal where the case has no window flags, through the same driver with flags where it has."""
    nch = int(cid.rsplit("_", 1)[1])
    specs = L.case_specs(cid, int(golden[f"{cid}_seed"]))
    blocks = L.blocks_from_ints(nch, golden[f"{cid}_blocks"])
    assert np.array_equal(golden[f"{cid}_blocks"], L.block_ints(nch, L.case_blocks(cid)))   # the stored blocks are the case's
    for s in range(L.STREAMS):
        if f"{cid}_flags" in golden:
            got = L.ref_write_tonal_win(specs[s], blocks[s], golden[f"{cid}_flags"][s])
        else:
            got = T.ref_write_tonal(specs[s], blocks[s])
        assert np.array_equal(got, golden[f"{cid}_frames"][s]), (cid, s)


@needs_ref
def test_loud_blocks_lower_the_unit_count_in_the_reference(golden):
    """The case "loud": with the largest block the reference keeps fewer quant units than for the same spectra without a block."""
    specs = L.case_specs("loud_2", int(golden["loud_2_seed"]))
    blocks = L.blocks_from_ints(2, golden["loud_2_blocks"])
    seen = 0
    for s in range(L.STREAMS):
        none = T.ref_write_tonal(specs[s], [None] * L.FRAMES)
        for f in range(L.FRAMES):
            if blocks[s][f] is not None and blocks[s][f]["nb"] == 16:
                assert T.n_qu(golden["loud_2_frames"][s, f]) < T.n_qu(none[f])
                seen += 1
    assert seen >= 2


@needs_ref
@pytest.mark.parametrize("nch,use_gha", L.SCHEDULE_CASES)
def test_schedule_goldens_equal_the_reference(golden, nch, use_gha):
    """The reference's own TAt3PEnc around the stand-in analyser writes the stored schedule frames; under GHA_WRITE_TONAL they carry
    blocks one call late: analyses 0 and 1 find one, 2 does not, ... and frame k holds analysis k - 1's."""
    fr = L.ref_schedule(nch, use_gha)
    assert np.array_equal(fr, golden[f"schedule_{nch}_{use_gha}"])
    present = [int(r[0]) for r in T.unpack_tonal(fr, nch)[2]]
    want = [int(bool(use_gha & 2) and k >= 1 and (k - 1) % 3 != 2) for k in range(L.SCHEDULE_CALLS - 1)]
    assert present == want


def test_schedule_goldens_differ_by_flag(golden):
    """Without GHA_WRITE_RESIUDAL (UseGha = 0, 1) and without GHA_WRITE_TONAL every frame is the silent frame, whatever
    GHA_PASS_INPUT says; UseGha = 5 and 7 are two more streams, different from it and from each other (a mirror that ignored one
    of these flags would be seen)."""
    g = {f: golden[f"schedule_2_{f}"] for f in L.SCHEDULE_FLAGS}
    assert (g[0] == g[0][0]).all() and np.array_equal(g[0], g[1])
    assert not np.array_equal(g[5], g[0]) and not np.array_equal(g[7], g[0]) and not np.array_equal(g[5], g[7])
    assert np.array_equal(g[5][0], g[0][0])   # (the first frame written is PrevBuf's zeros)


# ---- the kernel through the CPU SIMT harness ------------------------------------------------------------------------------------
@needs_clang
def test_harness_driver_equals_the_goldens():
    """tools/emu/run_emu_at3p_tonal_write.py under the strict harness: every writer case equals its golden, random blocks equal
    the restated writer's splice, zero records equal the writer without records - in ascending and in descending wavefront order,
    and with every device buffer ending at a guard page."""
    build_strict()
    modes = {"plain": {}, "reverse": {"EMU_ORDER": "reverse"}, "fence": {"EMU_FENCE": "high"}}
    runs = Children({m: ("run_emu_at3p_tonal_write.py", ["--nobuild"], env) for m, env in modes.items()})
    try:
        for m in modes:
            out = runs.output(m)
            assert_clean(out, len(L.writer_case_ids()) + 6)
            assert out.count("golden ") == len(L.writer_case_ids())
    finally:
        runs.close()


# ---- what was written reads back ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", L.writer_case_ids())
def test_golden_frames_parse_back_to_the_input_fields(golden, cid):
    """The restated unpacker (tests/host/at3p_tonal_cpu.c) accepts every golden frame and returns the block that went in: per channel
    and band the envelope points and the waves (a shared band of channel 1 as channel 0's, the channels swapped under the leader
    flag), and the window flags."""
    nch = int(cid.rsplit("_", 1)[1])
    blocks = L.blocks_from_ints(nch, golden[f"{cid}_blocks"])
    for s in range(L.STREAMS):
        _, win, rec, why = T.unpack_tonal(golden[f"{cid}_frames"][s], nch)
        assert (why == 0).all(), why
        if f"{cid}_flags" in golden:
            assert np.array_equal(win, golden[f"{cid}_flags"][s])
        for f in range(L.FRAMES):
            assert L.record_fields(rec[f]) == L.expected_fields(nch, blocks[s][f]), (cid, s, f)


# ---- the contract ----------------------------------------------------------------------------------------------------------------
def _valid(nch):
    from atracdenc_amd.binding import pack_tonal_blocks
    b = L.block(nch, [L.band(L.waves_of([10, 20, 30]), 1, 2), L.band(L.waves_of([600, 700])), L.band()], shared=[False, False, True] if nch == 2 else None)
    return pack_tonal_blocks(b, nch)


def _rule(name):
    """(channels, the violating record, what the error names)"""
    nch = 1 if name.startswith("mono") else 2
    r = _valid(nch).copy()
    if name == "bands":
        r["num_tone_bands"] = 17
    elif name == "leader":
        r["second_is_leader"] = 2
    elif name == "start":
        r["band"][0, 1]["start"] = 33
    elif name == "stop":
        r["band"][1, 0]["stop"] = 33
    elif name == "band_waves":
        r["band"][0, 2]["n_waves"] = 16
    elif name == "total_waves":
        r["num_tone_bands"] = 8
        r["tone_sharing"] = 0
        r["band"]["n_waves"][:, :8] = 3
        r["band"][1, 7]["n_waves"] = 4
        r["wave"] = np.arange(48) * 16
        r["wave"][[3 * i for i in range(16)]] = 0   # (each band's first frequency may be anything)
    elif name == "wave_range":
        r["wave"][1] |= 1 << 21
    elif name == "decreasing":
        r["wave"][4] = 599
    elif name == "shared_waves":
        r["band"][1, 2]["n_waves"] = 1
    elif name == "mono_sharing":
        r["tone_sharing"] = 1
    elif name == "mono_leader":
        r["second_is_leader"] = 1
    return nch, r


RULES = {"bands": "num_tone_bands", "leader": "second_is_leader", "start": "start", "stop": "stop", "band_waves": "n_waves",
         "total_waves": "48 waves", "wave_range": "FreqIndex 0..1023, AmpSf 0..63, PhaseIndex 0..31", "decreasing": "FreqIndex decreasing",
         "shared_waves": "shared band", "mono_sharing": "tone_sharing", "mono_leader": "second_is_leader"}


@needs_clang
@pytest.mark.parametrize("rule", list(RULES))
def test_validation_table(rule):
    """Each rule of at3phip_tonal_block's contract with one violating record, in stream 1, frame 2 of a call whose other records are
    valid: AT3HIP_EINVAL before anything is queued (the frames stay untouched), the last error naming stream, frame and field.
    The valid records alone pass. Runs on the host-compiled library: the checks need no device."""
    from atracdenc_amd.binding import At3HipError, At3pHip
    nch, bad = _rule(rule)
    enc = At3pHip(n_streams=2, max_frames=3, channels=nch, lib_path=build_strict())
    try:
        specs = np.zeros((2, 3, nch, 2048), np.float32)
        recs = np.stack([np.stack([_valid(nch)] * 3)] * 2)
        frames = np.full((2, 3, 2048), 0xA5, np.uint8)
        enc.write_frames_tonal_ptr(specs.ctypes.data, 3, None, recs.ctypes.data, frames.ctypes.data, 0)
        assert not (frames == 0xA5).all()
        recs[1, 2] = bad
        frames[:] = 0xA5
        with pytest.raises(At3HipError) as e:
            enc.write_frames_tonal_ptr(specs.ctypes.data, 3, None, recs.ctypes.data, frames.ctypes.data, 0)
        assert "(-1)" in str(e.value) and "stream 1, frame 2" in str(e.value) and RULES[rule] in str(e.value), str(e.value)
        assert (frames == 0xA5).all()
    finally:
        enc.close()


@needs_clang
def test_a_record_without_bands_is_not_read():
    """num_tone_bands = 0 means no tonal block whatever the other fields hold: the frames of the writer without records."""
    from atracdenc_amd.binding import AT3P_TONAL_BLOCK_DTYPE, At3pHip
    enc = At3pHip(n_streams=1, max_frames=2, channels=2, lib_path=build_strict())
    try:
        specs = (0.05 * np.random.RandomState(3).standard_normal((1, 2, 2, 2048))).astype(np.float32)
        recs = np.frombuffer(np.random.RandomState(4).bytes(2 * AT3P_TONAL_BLOCK_DTYPE.itemsize), AT3P_TONAL_BLOCK_DTYPE).reshape(1, 2).copy()
        recs["num_tone_bands"] = 0
        assert np.array_equal(enc.write_frames(specs, None, recs), enc.write_frames(specs))
    finally:
        enc.close()


# ---- the reference's abort() branch ------------------------------------------------------------------------------------------------
def _inc_tables():
    t = open(os.path.join(ROOT, "atracdenc_amd", "csrc", "at3p_vlc.inc")).read()
    out = {}
    for m in re.finditer(r"(AT3P_[A-Z0-9_]+)((?:\[[^\]]*\])+)\s*=\s*\{(.*?)\};", t, re.S):
        if "p+" not in m.group(3) and "p-" not in m.group(3):   # (the float tables are not needed)
            out[m.group(1)] = [int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", m.group(3))]
    return out


def test_sixteen_units_and_the_largest_tail_always_fit():
    """TTonalComponentEncoder::Encode aborts when, on a repeated pass, NumToneBands (<= 16) exceeds the quant unit count
    (at3p_bitstream.cpp:652-656): the count would have to fall below 16, that is 16 units and the tail would have to miss the
    frame's 16381 bits. Upper bounds from the tables: every unit under the cheapest-in-the-worst-case of its eight code tables
    (the writer's choice is never dearer than any one table) with every code at its table's longest length, every sign and group
    flag present; the word lengths' codes at the longest length of AT3P_WL_VLC; the tail with 18 bits per window shape, the long
    sharing form, 32 bands with both envelope points, 48 waves of 10 + 6 + 5 bits and 24 order bits. Both fit with room to spare,
    so the branch cannot be reached and the header says so."""
    tb = _inc_tables()

    def wordlen(qu):   # TConfigure::Encode's allocTable (at3p_bitstream.cpp:107-112)
        return 7 if qu < 17 else 6 if qu < 26 else 5 if qu < 28 else 32 - qu

    def qu_start(qu):  # NAt3p::TScaleTable::BlockSizeTab
        return 16 * qu if qu < 8 else 128 + 32 * (qu - 8) if qu < 16 else 384 + 64 * (qu - 16) if qu < 22 else 768 + 128 * (qu - 22)

    def unit_worst(qu):
        lines, best = qu_start(qu + 1) - qu_start(qu), None
        for i in range(8):
            t = wordlen(qu) - 1 + 7 * i
            gs, nc = tb["AT3P_SPEC_TAB"][2 * t] & 15, tb["AT3P_SPEC_TAB"][2 * t] >> 4
            signed = tb["AT3P_SPEC_TAB"][2 * t + 1] >> 4
            longest = max(e >> 12 for e in tb["AT3P_VLC"][tb["AT3P_VLC_OFF"][t]:tb["AT3P_VLC_OFF"][t + 1]])
            nsym = lines // nc
            bits = nsym * (longest + (0 if signed else nc)) + (nsym // gs if gs != 1 else 0)
            best = bits if best is None else min(best, bits)
        return best

    def front_worst(nch, n):   # everything in front of the tail, without the three leading bits (they are outside SizeBits)
        wl = max(e >> 12 for e in tb["AT3P_WL_VLC"])
        bits = 5 + 1 + (2 + 2 + 2 + 2 + 3 + (n - 1) * wl) + (nch == 2) * (2 + 2 + 2 + n * wl)
        bits += nch * (2 + 6 * n) + 1 + nch * (4 + 3 * n) + nch * 4 * tb["AT3P_SB_POWGRPS"][tb["AT3P_QU_TO_SB"][n - 1]]
        return bits + nch * sum(unit_worst(q) for q in range(n))

    def tail_worst(nch):
        blk = 1 + max(n for _, n in T.tone_vlc()) + (nch == 2) * (2 + 16 + 2 + 1)
        for ch in range(nch):
            blk += ch + 16 * 12 + (ch + 1) + 16 * 4 + ch + (ch + 1)
        blk += 48 * 10 + 24 + 48 * (6 + 5)
        return (nch == 2) * 2 + nch * 18 + nch + 1 + blk + 1 + 2

    assert all(wordlen(q) == 7 for q in range(16)) and qu_start(16) == 384
    assert (front_worst(2, 16), tail_worst(2)) == (6639, 1624)     # the figures in include/at3phip.h
    for nch in (1, 2):
        assert front_worst(nch, 16) + tail_worst(nch) <= 2048 * 8 - 3
    # the largest block of the cases is within the tail's bound, and close to it
    big = sum(n for _, n in T.tonal_bits(2, L.largest_block(2)))
    assert 1500 <= big <= tail_worst(2)
    header = open(os.path.join(ROOT, "include", "at3phip.h")).read()
    assert "6639 bits" in header and "1624 bits" in header and "cannot be reached" in header


# ---- the exported symbol ---------------------------------------------------------------------------------------------------------
def test_symbol_and_prototype():
    """libat3hip.so exports at3phip_write_frames_tonal, the header declares it, binding.PROTOTYPES carries its prototype (a status;
    context, specs, count, window flags, records, frames, flags), the reported ABI version stays 1.6, and the record is 324 bytes
    on both sides."""
    import atracdenc_amd
    from atracdenc_amd import binding as B
    if not os.path.exists(atracdenc_amd.LIB_PATH):
        atracdenc_amd.build_library()
    lib = atracdenc_amd.load_library()
    name = "at3phip_write_frames_tonal"
    assert re.fullmatch(r"at3phip_[a-z_]+", name)   # what tests/test_abi.py collects from the header
    out = subprocess.check_output(["nm", "-D", "--defined-only", atracdenc_amd.LIB_PATH], text=True)
    assert name in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert name in B.AT3P_SYMBOLS
    restype, argtypes = B.PROTOTYPES[name]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_uint32]
    fn = getattr(lib, name)
    assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert lib.at3hip_version() == (1 << 16) | 6
    header = open(os.path.join(ROOT, "include", "at3phip.h")).read()
    assert re.search(r"\bint at3phip_write_frames_tonal\s*\(", header)
    assert B.AT3P_TONAL_BLOCK_DTYPE.itemsize == 324 and "324 bytes" in header
    assert fn(None, None, 1, None, None, None, 0) == -1   # AT3HIP_EINVAL without a context
