#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: the rate-distortion ATRAC3plus writer kernels (k_at3p_write_adaptive_with<WriteParamsRd>, <WriteParamsTonalRd>)
or, with --mode psy, the masking-weighted ones (<WriteParamsPsy>, <WriteParamsTonalPsy>) through the CPU SIMT emulator, lane by lane,
against the restatement tests/host/at3p_rd_cpu.c. Driver of tests/test_at3p_rd_simt_harness.py, which runs it in child processes because
the harness reads EMU_STRICT, EMU_FENCE and EMU_ORDER when the library loads.

    run_emu_at3p_rd.py [--mode rd|psy] [--nobuild]

Every buffer a kernel reads spectra from or writes frames to is a caller's device buffer of exactly its size (DevBuf): under EMU_FENCE
it ends or begins at a guard page. Prints one `<what>: bad N` line per comparison (0 is a pass), one that counts the cases in which
the restatement's records do not show both outcomes of the guard (R4, M6), and with --mode psy one for the clip of the offsets at 32 (M3)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import numpy as np
import at3p_writer_lib as W
import at3p_psy_lib as P
import at3p_tonal_write_lib as TW
from atracdenc_amd.binding import (AT3HIP_OUT_ON_DEVICE, AT3HIP_PCM_ON_DEVICE, AT3PHIP_ALLOC_ADAPTIVE, AT3PHIP_ALLOC_PSY, AT3PHIP_ALLOC_RD,
                                   AT3PHIP_ALLOC_SPARSE, At3pHip, pack_tonal_blocks)
import run_emu
from run_emu_decode import DevBuf, report

DEV = AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE
MODE = sys.argv[sys.argv.index("--mode") + 1] if "--mode" in sys.argv else "rd"
assert MODE in ("rd", "psy"), MODE
PSY = MODE == "psy"
WRITE = DEV | AT3PHIP_ALLOC_ADAPTIVE | AT3PHIP_ALLOC_SPARSE | AT3PHIP_ALLOC_RD | (AT3PHIP_ALLOC_PSY if PSY else 0)
R_MIN = {1: 176, 2: 224}   # AT3PHIP_MIN_FRAME_BYTES_MONO / _STEREO
seen = set()               # the outcomes of the guard the restatement reported
largest = [0]              # the largest O


def run(name, nch, fb, specs, blocks=None):
    """specs [S][F][C][2048], blocks [S][F] dicts or None: the mode's writer against the restatement"""
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
    exp = []
    for s in range(S):
        fr, rec, _ = W.write_rd(specs[s], fb, None, None if blocks is None else blocks[s], info=True, psy=PSY)
        seen.update(int(c) for c in rec["chose"])
        largest[0] = max(largest[0], int(rec["O"].max()))
        exp.append(fr)
    report(f"{name} nch={nch} size={fb} writer", (got != np.stack(exp)).any(axis=2).sum(), t)


def main():
    if "--nobuild" not in sys.argv: run_emu.build("--strict" in sys.argv)
    sig = lambda nch: np.stack([np.stack([W.specs_of(n, nch, 1)[0] for n in ("noise", "tones")]), np.stack([W.specs_of(n, nch, 1)[0] for n in ("mix", "burst")])])
    run("signals", 2, 376, sig(2))
    run("signals", 2, 2048, sig(2))
    run("signals", 1, 192, sig(1))
    for nch in (2, 1):   # the special cases of A3s' closing rules, where the budget binds
        sp, blocks = W.edge_specs(nch)
        run("edge", nch, R_MIN[nch], sp[None], [blocks])
    run("odd", 2, 280, np.stack([W.odd_specs(2, 2), W.specs_of("noise", 2, 2)]))
    run("tonal", 2, 224, np.stack([W.full_scale_noise(2, 2), W.specs_of("tones", 2, 2)]),
        [[TW.largest_block(2), TW.largest_block(2)], [None, TW.case_blocks("small_2")[0][0]]])
    if PSY:
        run("twin+silence", 1, 176, np.stack([np.concatenate([P.masked_twin(), np.zeros((1, 1, 2048), np.float32)])]), [[TW.largest_block(1), None]])
    report(f"guard outcomes seen {sorted(seen)}", seen != {0, 1})
    if PSY:
        report(f"largest O {largest[0]}", largest[0] != P.O_MAX)


if __name__ == "__main__":
    main()
