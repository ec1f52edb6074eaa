"""The rate-distortion ATRAC3plus writer kernels (csrc/at3p_rd.hip) stepped lane by lane on the CPU (tools/emu) against the restatement
tests/host/at3p_rd_cpu.c, as the adaptive and sparse kernels are; and, through the same host-compiled library, the flag's refusals:
no GPU is needed for either."""
import os

import numpy as np
import pytest

import at3p_writer_lib as W
from simt_harness_lib import CLANG, Children, assert_clean, build_strict

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")
SENTINEL = 0xA5


def test_harness_driver_equals_the_restatement():
    """tools/emu/run_emu_at3p_rd.py under the strict harness: the two kernels against the restatement on the signals at 376, 2048 and
    192 bytes, at3p_writer_lib.edge_specs at the smallest frame sizes (the closing rules of A3s), non-finite spectra and the largest
    tonal record at 224 bytes - both outcomes of the guard among them, which the driver checks -, in ascending and descending wavefront
    order and with a guard page behind every buffer"""
    build_strict()
    jobs = {"plain": ("run_emu_at3p_rd.py", ["--nobuild"], {}), "reverse": ("run_emu_at3p_rd.py", ["--nobuild"], {"EMU_ORDER": "reverse"}),
            "fence": ("run_emu_at3p_rd.py", ["--nobuild"], {"EMU_FENCE": "high"})}
    runs = Children(jobs)
    try:
        for m in jobs:
            assert_clean(runs.output(m), 8)
    finally:
        runs.close()


@pytest.mark.parametrize("nch", [1, 2])
def test_the_flag_without_the_other_two_is_refused_and_writes_nothing(nch):
    """AT3PHIP_ALLOC_RD alone, with ADAPTIVE only and with SPARSE only, on all six calls of the host-compiled library: AT3HIP_EINVAL
    with the last-error text, and the output buffer untouched; with both, the call is served"""
    emu = build_strict()
    from atracdenc_amd import binding as B
    S, F = 1, 2
    specs = W.specs_of("mix", nch, F)[None]
    pcm = np.zeros((S, F, 2048, nch), np.float32)
    p16 = np.zeros((S, F, 2048, nch), np.int16)
    recs = np.zeros((S, F), B.AT3P_TONAL_BLOCK_DTYPE)
    out = np.full((S, F, 2048), SENTINEL, np.uint8)
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, lib_path=emu)
    try:
        for extra in (0, B.AT3PHIP_ALLOC_ADAPTIVE, B.AT3PHIP_ALLOC_SPARSE):
            flag = B.AT3PHIP_ALLOC_RD | extra
            calls = [lambda: enc.write_frames_ptr(specs.ctypes.data, F, None, out.ctypes.data, flag),
                     lambda: enc.write_frames_tonal_ptr(specs.ctypes.data, F, None, recs.ctypes.data, out.ctypes.data, flag),
                     lambda: enc.encode_frames_ptr(pcm.ctypes.data, F, out.ctypes.data, flag),
                     lambda: enc.encode_frames_s16_ptr(p16.ctypes.data, F, out.ctypes.data, flag),
                     lambda: enc.encode_frames_tonal_ptr(pcm.ctypes.data, F, out.ctypes.data, flag),
                     lambda: enc.encode_frames_tonal_s16_ptr(p16.ctypes.data, F, out.ctypes.data, flag)]
            for k, call in enumerate(calls):
                with pytest.raises(B.At3HipError, match="AT3PHIP_ALLOC_RD needs AT3PHIP_ALLOC_ADAPTIVE and AT3PHIP_ALLOC_SPARSE"):
                    call()
                assert (out == SENTINEL).all(), (extra, k)
        assert np.array_equal(enc.write_frames(specs, adaptive=True, sparse=True, rd=True)[0], W.write_rd(specs[0], 2048))
    finally:
        enc.close()
