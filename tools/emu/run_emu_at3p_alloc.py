#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: the adaptive ATRAC3plus frame writer (k_at3p_write_adaptive, with and without tonal records) through the
CPU SIMT emulator against the restatement tests/host/at3p_writer_cpu.c. Arguments: the cases to run (default: all), --nobuild."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import numpy as np
import at3p_writer_lib as W
import at3p_tonal_write_lib as TW
from atracdenc_amd.binding import At3pHip, pack_tonal_blocks
import run_emu

def run(name, nch, specs, win=None, blocks=None):
    """specs [2][n][C][2048] (two streams), win [2][n][C] or None, blocks [2][n] dicts or None"""
    t = time.time()
    n = specs.shape[1]
    enc = At3pHip(n_streams=2, max_frames=n, channels=nch, lib_path=run_emu.EMU)
    recs = None if blocks is None else np.stack([pack_tonal_blocks(row, nch) for row in blocks])
    got = enc.write_frames(specs, win, recs, adaptive=True)
    enc.close()
    exp = np.stack([W.write_adaptive(specs[s], win=None if win is None else win[s], blocks=None if blocks is None else blocks[s]) for s in range(2)])
    bad = (got != exp).any(axis=2)
    print(f"{name} nch={nch}: mismatching frames {int(bad.sum())}/{bad.size} {np.argwhere(bad)[:4].tolist()} ({time.time()-t:.1f}s)", flush=True)

if __name__ == "__main__":
    if "--nobuild" not in sys.argv: run_emu.build("--strict" in sys.argv)
    want = [a for a in sys.argv[1:] if not a.startswith("--")]
    for nch in (2, 1):
        if not want or "signals" in want:    # one frame each of a loud, a tonal and a silent signal beside full-scale noise
            run("signals", nch, np.stack([np.concatenate([W.specs_of("mix", nch, 1), W.specs_of("silence", nch, 1)]),
                                          np.concatenate([W.specs_of("fullscale", nch, 1), W.specs_of("tones", nch, 2)[1:]])]))
        if not want or "win" in want:
            sp = np.stack([W.specs_of("noise", nch, 2), W.full_scale_noise(2, nch, seed=3)])
            win = np.array([[[0x01ef] * nch, [0xffff] * nch], [[0] * nch, [0x8001] * nch]], np.uint16)
            run("win", nch, sp, win)
        if not want or "tonal" in want:      # the largest record on a loud frame, no record, a small one
            sp = np.stack([W.full_scale_noise(2, nch, seed=4), W.specs_of("mix", nch, 2)])
            run("tonal", nch, sp, None, [[TW.largest_block(nch), None], [TW.case_blocks(f"small_{nch}")[0][0], TW.largest_block(nch, 1)]])
        if not want or "odd" in want:
            run("odd", nch, np.stack([W.odd_specs(nch, 2), W.specs_of("noise", nch, 2)]))
