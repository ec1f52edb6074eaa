"""The masking-weighted ATRAC3plus writer kernels (csrc/at3p_psy.hip) stepped lane by lane on the CPU (tools/emu) against the restatement
tests/host/at3p_psy_cpu.c, as the rate-distortion kernels are; through the same host-compiled library, the flag's refusals; and the
stand-alone program tests/host/at3p_psy_modes_main.cpp in a build with and a build without the unit: no GPU is needed for any of it."""
import os
import subprocess

import numpy as np
import pytest

import at3p_psy_lib as Y
import at3p_writer_lib as W
from simt_harness_lib import CLANG, ROOT, Children, assert_clean, build_strict

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")
SENTINEL = 0xA5


def test_harness_driver_equals_the_restatement():
    """tools/emu/run_emu_at3p_psy.py under the strict harness: the two kernels against the restatement on the signals at 376, 2048 and
    192 bytes, at3p_writer_lib.edge_specs at the smallest frame sizes (the closing rules of A3s; the stereo set reaches the clip of the
    offsets at 32, which the driver checks), non-finite spectra, the largest tonal record at 224 bytes (full-scale noise beside it
    gives the guard's fallback; the driver checks that both outcomes occurred) and the masked twin beside a silent frame, in ascending
    and descending wavefront order and with a guard page behind every buffer"""
    build_strict()
    jobs = {"plain": ("run_emu_at3p_psy.py", ["--nobuild"], {}), "reverse": ("run_emu_at3p_psy.py", ["--nobuild"], {"EMU_ORDER": "reverse"}),
            "fence": ("run_emu_at3p_psy.py", ["--nobuild"], {"EMU_FENCE": "high"})}
    runs = Children(jobs)
    try:
        for m in jobs:
            assert_clean(runs.output(m), 10)
    finally:
        runs.close()


@pytest.mark.parametrize("nch", [1, 2])
def test_the_flag_without_all_three_others_is_refused_and_writes_nothing(nch):
    """AT3PHIP_ALLOC_PSY with any of ADAPTIVE, SPARSE and RD missing, on all six calls of the host-compiled library: AT3HIP_EINVAL with the
    last-error text, and the output buffer untouched; with all three, the call is served"""
    emu = build_strict()
    from atracdenc_amd import binding as B
    S, F = 1, 2
    specs = W.specs_of("mix", nch, F)[None]
    pcm = np.zeros((S, F, 2048, nch), np.float32)
    p16 = np.zeros((S, F, 2048, nch), np.int16)
    recs = np.zeros((S, F), B.AT3P_TONAL_BLOCK_DTYPE)
    out = np.full((S, F, 2048), SENTINEL, np.uint8)
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, lib_path=emu)
    A, Sp, R = B.AT3PHIP_ALLOC_ADAPTIVE, B.AT3PHIP_ALLOC_SPARSE, B.AT3PHIP_ALLOC_RD
    try:
        for extra in (0, A, Sp, R, A | Sp, A | R, Sp | R):
            flag = B.AT3PHIP_ALLOC_PSY | extra
            calls = [lambda: enc.write_frames_ptr(specs.ctypes.data, F, None, out.ctypes.data, flag),
                     lambda: enc.write_frames_tonal_ptr(specs.ctypes.data, F, None, recs.ctypes.data, out.ctypes.data, flag),
                     lambda: enc.encode_frames_ptr(pcm.ctypes.data, F, out.ctypes.data, flag),
                     lambda: enc.encode_frames_s16_ptr(p16.ctypes.data, F, out.ctypes.data, flag),
                     lambda: enc.encode_frames_tonal_ptr(pcm.ctypes.data, F, out.ctypes.data, flag),
                     lambda: enc.encode_frames_tonal_s16_ptr(p16.ctypes.data, F, out.ctypes.data, flag)]
            for k, call in enumerate(calls):
                with pytest.raises(B.At3HipError, match="AT3PHIP_ALLOC_PSY needs AT3PHIP_ALLOC_ADAPTIVE, AT3PHIP_ALLOC_SPARSE and AT3PHIP_ALLOC_RD"):
                    call()
                assert (out == SENTINEL).all(), (extra, k)
        assert np.array_equal(enc.write_frames(specs, adaptive=True, sparse=True, rd=True, psy=True)[0], Y.write_psy(specs[0], 2048))
    finally:
        enc.close()


_UNITS = {"rd": ("at3p_alloc.hip", "at3p_sparse.hip", "at3p_rd.hip"), "psy": ("at3p_alloc.hip", "at3p_sparse.hip", "at3p_rd.hip", "at3p_psy.hip")}


@pytest.mark.parametrize("units", ["rd", "psy"])
def test_builds_with_and_without_the_masking_weighted_writer(tmp_path, units):
    """tests/host/at3p_psy_modes_main.cpp: at3phip.hip linked with the three older units and with or without at3p_psy.hip, compiled for
    the host with the harness's runtime. All sixteen flag combinations on all six calls at two sizes: without the unit ADAPTIVE | SPARSE |
    RD | PSY is refused with "this build has no masking-weighted writer", writes nothing and moves no state, and the library has no
    at3phip_host_allocate_psy; with it the call is served"""
    csrc, emu = os.path.join(ROOT, "atracdenc_amd", "csrc"), os.path.join(ROOT, "tools", "emu")
    exe = str(tmp_path / ("at3p_psy_modes_" + units))
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I", emu, "-include", os.path.join(emu, "at3_pk_emu.hpp"),
                           "-x", "c++", os.path.join(csrc, "at3phip.hip"), *(os.path.join(csrc, u) for u in _UNITS[units]),
                           os.path.join(csrc, "at3_tables.cpp"), os.path.join(emu, "emu_runtime.cpp"),
                           os.path.join(ROOT, "tests", "host", "at3p_psy_modes_main.cpp"), "-o", exe, "-ldl", "-lpthread"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("EMU_")}
    r = subprocess.run([exe, units], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and f"MASKING-WEIGHTED MODES OK ({units})" in r.stdout, (units, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
