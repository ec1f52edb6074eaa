"""The rate-distortion and the masking-weighted ATRAC3plus writer kernels (csrc/at3p_rd.hip, csrc/at3p_psy.hip) stepped lane by lane on the
CPU (tools/emu) against the restatement tests/host/at3p_rd_cpu.c, as the adaptive and sparse kernels are; through the same host-compiled
library, each flag's refusals; and the stand-alone program tests/host/at3p_alloc_modes_main.cpp in a build with and a build without the
masking-weighted unit: no GPU is needed for any of it."""
import os

import numpy as np
import pytest

import at3p_writer_lib as W
from simt_harness_lib import CLANG, Children, assert_clean, build_strict, run_alloc_modes

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")
SENTINEL = 0xA5
MODES = ("rd", "psy")
# per mode: the comparison lines its driver prints at least; the flag, the flags it needs, and the text of the refusal without them
N_LINES = {"rd": 8, "psy": 10}
FLAG = {"rd": "AT3PHIP_ALLOC_RD", "psy": "AT3PHIP_ALLOC_PSY"}
NEEDS = {"rd": ("AT3PHIP_ALLOC_ADAPTIVE", "AT3PHIP_ALLOC_SPARSE"), "psy": ("AT3PHIP_ALLOC_ADAPTIVE", "AT3PHIP_ALLOC_SPARSE", "AT3PHIP_ALLOC_RD")}
REFUSAL = {"rd": "AT3PHIP_ALLOC_RD needs AT3PHIP_ALLOC_ADAPTIVE and AT3PHIP_ALLOC_SPARSE",
           "psy": "AT3PHIP_ALLOC_PSY needs AT3PHIP_ALLOC_ADAPTIVE, AT3PHIP_ALLOC_SPARSE and AT3PHIP_ALLOC_RD"}


@pytest.mark.parametrize("mode", MODES)
def test_harness_driver_equals_the_restatement(mode):
    """tools/emu/run_emu_at3p_rd.py --mode under the strict harness: the mode's two kernels against the restatement on the signals at 376,
    2048 and 192 bytes, at3p_writer_lib.edge_specs at the smallest frame sizes (the closing rules of A3s; with psy the stereo set reaches
    the clip of the offsets at 32, which the driver checks), non-finite spectra and the largest tonal record at 224 bytes (full-scale noise
    beside it gives the guard's fallback; the driver checks that both outcomes occurred), and with psy the masked twin beside a silent
    frame, in ascending and descending wavefront order and with a guard page behind every buffer"""
    build_strict()
    args = ["--mode", mode, "--nobuild"]
    jobs = {"plain": ("run_emu_at3p_rd.py", args, {}), "reverse": ("run_emu_at3p_rd.py", args, {"EMU_ORDER": "reverse"}),
            "fence": ("run_emu_at3p_rd.py", args, {"EMU_FENCE": "high"})}
    runs = Children(jobs)
    try:
        for m in jobs:
            assert_clean(runs.output(m), N_LINES[mode])
    finally:
        runs.close()


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_the_flag_without_the_flags_it_needs_is_refused_and_writes_nothing(mode, nch):
    """AT3PHIP_ALLOC_RD without ADAPTIVE and SPARSE, AT3PHIP_ALLOC_PSY without ADAPTIVE, SPARSE and RD - alone and with every proper subset
    of them -, on all six calls of the host-compiled library: AT3HIP_EINVAL with the last-error text, and the output buffer untouched;
    with all of them, the call is served"""
    emu = build_strict()
    from atracdenc_amd import binding as B
    S, F = 1, 2
    specs = W.specs_of("mix", nch, F)[None]
    pcm = np.zeros((S, F, 2048, nch), np.float32)
    p16 = np.zeros((S, F, 2048, nch), np.int16)
    recs = np.zeros((S, F), B.AT3P_TONAL_BLOCK_DTYPE)
    out = np.full((S, F, 2048), SENTINEL, np.uint8)
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, lib_path=emu)
    needs = [getattr(B, n) for n in NEEDS[mode]]
    subsets = [sum(f for i, f in enumerate(needs) if m >> i & 1) for m in range((1 << len(needs)) - 1)]   # every proper subset
    assert len(subsets) == {"rd": 3, "psy": 7}[mode]
    try:
        for extra in subsets:
            flag = getattr(B, FLAG[mode]) | extra
            calls = [lambda: enc.write_frames_ptr(specs.ctypes.data, F, None, out.ctypes.data, flag),
                     lambda: enc.write_frames_tonal_ptr(specs.ctypes.data, F, None, recs.ctypes.data, out.ctypes.data, flag),
                     lambda: enc.encode_frames_ptr(pcm.ctypes.data, F, out.ctypes.data, flag),
                     lambda: enc.encode_frames_s16_ptr(p16.ctypes.data, F, out.ctypes.data, flag),
                     lambda: enc.encode_frames_tonal_ptr(pcm.ctypes.data, F, out.ctypes.data, flag),
                     lambda: enc.encode_frames_tonal_s16_ptr(p16.ctypes.data, F, out.ctypes.data, flag)]
            for k, call in enumerate(calls):
                with pytest.raises(B.At3HipError, match=REFUSAL[mode]):
                    call()
                assert (out == SENTINEL).all(), (extra, k)
        psy = mode == "psy"
        assert np.array_equal(enc.write_frames(specs, adaptive=True, sparse=True, rd=True, psy=psy)[0], W.write_rd(specs[0], 2048, psy=psy))
    finally:
        enc.close()


@pytest.mark.parametrize("units", ["alloc+sparse+rd", "all"])
def test_builds_with_and_without_the_masking_weighted_writer(tmp_path, units):
    """tests/host/at3p_alloc_modes_main.cpp: at3phip.hip linked with the three older units and with or without at3p_psy.hip, compiled for
    the host with the harness's runtime. All sixteen flag combinations on all six calls at two sizes: without the unit ADAPTIVE | SPARSE |
    RD | PSY is refused with "this build has no masking-weighted writer", writes nothing and moves no state, and the library has no
    at3phip_host_allocate_psy; with it the call is served"""
    run_alloc_modes(tmp_path, units)
