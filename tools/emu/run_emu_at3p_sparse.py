#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: the sparse ATRAC3plus writer kernels (k_at3p_write_adaptive_with<WriteParamsSparse>, <WriteParamsTonalSparse>)
and the sparse unpack kernels (k_at3pd_unpack_sparse_with<false>, <true>) through the CPU SIMT emulator, against the restatement
tests/host/at3p_writer_cpu.c. Driver of tests/test_at3p_sparse_cpu.py, which runs it in child processes because the harness reads
EMU_STRICT, EMU_FENCE and EMU_ORDER when the library loads.

    run_emu_at3p_sparse.py [--nobuild]

Every buffer a kernel reads frames from or writes frames to is a caller's device buffer of exactly [S][F][frame_bytes] bytes
(DevBuf): under EMU_FENCE it ends or begins at a guard page. Prints one `<what>: bad N` line per comparison (0 is a pass), and
per channel count one for at3p_writer_lib.edge_specs: N is the number of the definition's special cases (empty frame, 29..31, clone
flags, flat) that the restatement's records do not show to have occurred."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import numpy as np
import at3p_writer_lib as W
import at3p_tonal_write_lib as TW
from atracdenc_amd.binding import (AT3HIP_OUT_ON_DEVICE, AT3HIP_PCM_ON_DEVICE, AT3PHIP_ALLOC_ADAPTIVE, AT3PHIP_ALLOC_SPARSE, AT3PHIP_DECODE_SPARSE,
                                   AT3PHIP_DECODE_TONES, At3pHip, At3pHipDecoder, pack_tonal_blocks)
import run_emu
from run_emu_decode import DevBuf, bits, report

DEV = AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE
WRITE = DEV | AT3PHIP_ALLOC_ADAPTIVE | AT3PHIP_ALLOC_SPARSE
R_MIN = {1: 176, 2: 224}   # AT3PHIP_MIN_FRAME_BYTES_MONO / _STEREO


def run(name, nch, fb, specs, blocks=None):
    """specs [S][F][C][2048], blocks [S][F] dicts or None: the sparse writer against the restatement, then the sparse decoder (tones
    on) on the restatement's frames: PCM bit for bit and the rejection counters"""
    t = time.time()
    S, F = specs.shape[:2]
    enc = At3pHip(n_streams=S, max_frames=F, channels=nch, lib_path=run_emu.EMU, frame_bytes=fb)
    src, dst = DevBuf(specs.nbytes).write(specs), DevBuf(S * F * fb)
    if blocks is None:
        enc.write_frames_ptr(src.ptr, F, None, dst.ptr, WRITE)
    else:
        recs = np.stack([pack_tonal_blocks(row, nch) for row in blocks])
        enc.write_frames_tonal_ptr(src.ptr, F, None, recs.ctypes.data, dst.ptr, WRITE)
    got = dst.read(np.uint8, (S, F, fb))
    src.free(); dst.free()
    enc.close()
    exp = np.stack([W.write_adaptive(specs[s], fb, True, None, None if blocks is None else blocks[s]) for s in range(S)])
    report(f"{name} nch={nch} size={fb} writer", (got != exp).any(axis=2).sum())
    dec = At3pHipDecoder(n_streams=S, channels=nch, max_frames=F, lib_path=run_emu.EMU, frame_bytes=fb)
    src, dst = DevBuf(exp.nbytes).write(exp), DevBuf(4 * S * F * 2048 * nch)
    dec.decode_ptr(src.ptr, F, dst.ptr, DEV | AT3PHIP_DECODE_TONES | AT3PHIP_DECODE_SPARSE)
    pcm = dst.read(np.float32, (S, F, 2048, nch))
    src.free(); dst.free()
    cnt = dec.counters()
    dec.close()
    epcm, erej = W.decode_streams(exp, nch, True, True)
    report(f"{name} nch={nch} size={fb} decoder", (bits(pcm) != bits(epcm)).reshape(S, F, -1).any(axis=2).sum())
    report(f"{name} nch={nch} size={fb} counters {list(cnt.values())}", list(cnt.values()) != erej.tolist() or erej.sum() != 0, t)


def main():
    if "--nobuild" not in sys.argv: run_emu.build("--strict" in sys.argv)
    sig = lambda nch: np.stack([np.stack([W.specs_of(n, nch, 1)[0] for n in ("noise", "tones")]), np.stack([W.specs_of(n, nch, 1)[0] for n in ("mix", "burst")])])
    run("signals", 2, 280, sig(2))
    run("signals", 2, 2048, sig(2))
    run("signals", 1, 280, sig(1))
    for nch in (2, 1):   # the definition's special cases, where the budget binds; that each occurred is part of the result
        sp, blocks = W.edge_specs(nch)
        fb = R_MIN[nch]
        rec = W.write_adaptive(sp, fb, True, None, blocks, info=True)[1]
        missed = W.edge_cases_reached(rec, nch)
        report(f"edge nch={nch} size={fb} cases not reached {missed}", len(missed))
        run("edge", nch, fb, sp[None], [blocks])
    run("odd", 2, 280, np.stack([W.odd_specs(2, 2), W.specs_of("noise", 2, 2)]))
    run("tonal", 2, 224, np.stack([W.full_scale_noise(2, 2), W.specs_of("tones", 2, 2)]),
        [[TW.largest_block(2), TW.largest_block(2)], [None, TW.case_blocks("small_2")[0][0]]])


if __name__ == "__main__":
    main()
