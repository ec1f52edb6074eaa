#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: the frame writer's instantiation with tonal records (k_at3p_write_with<WriteParamsTonal>, behind
at3phip_write_frames_tonal) through the CPU SIMT emulator, lane by lane, against tests/golden/at3p_tonal_write.npz (the
reference's frames) and, for blocks drawn at random, against the restated writer of tests/at3p_tonal_lib.py spliced into the
frames of the writer without records. `validation` walks the host-side contract instead (no kernel runs)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import numpy as np
import at3p_tonal_lib as T
import at3p_tonal_write_lib as L
from atracdenc_amd.binding import At3pHip, pack_tonal_blocks
import run_emu

def goldens():
    g = np.load(L.GOLDEN)
    for cid in L.writer_case_ids():
        nch = int(cid.rsplit("_", 1)[1])
        t = time.time()
        blocks = L.blocks_from_ints(nch, g[f"{cid}_blocks"])
        flags = g[f"{cid}_flags"] if f"{cid}_flags" in g else None
        enc = At3pHip(n_streams=L.STREAMS, max_frames=L.FRAMES, channels=nch, lib_path=run_emu.EMU)
        got = enc.write_frames(L.case_specs(cid, int(g[f"{cid}_seed"])), flags, pack_tonal_blocks(blocks, nch))
        enc.close()
        bad = (got != g[f"{cid}_frames"]).any(axis=2)
        print(f"golden {cid:10s}: mismatching frames {int(bad.sum())}/{bad.size} {np.argwhere(bad)[:4].tolist()} ({time.time()-t:.1f}s)", flush=True)

def spliced():
    # quiet spectra (the block does not change the unit count): the frame without records with the restated block spliced in at its tonal flag
    rng = np.random.default_rng(5)
    for nch in (2, 1):
        nf = 4
        specs = (0.01 * rng.standard_normal((2, nf, nch, 2048))).astype(np.float32)
        blocks = [[T.random_block(rng, nch) if rng.random() < 0.8 else None for _ in range(nf)] for _ in range(2)]
        t = time.time()
        enc = At3pHip(n_streams=2, max_frames=nf, channels=nch, lib_path=run_emu.EMU)
        base = enc.write_frames(specs)
        zero = enc.write_frames(specs, None, pack_tonal_blocks([[None] * nf] * 2, nch))
        got = enc.write_frames(specs, None, pack_tonal_blocks(blocks, nch))
        enc.close()
        exp = np.stack([np.stack([base[s, f] if blocks[s][f] is None else T.splice_tonal(base[s, f], T.tonal_bits(nch, blocks[s][f]))
                                  for f in range(nf)]) for s in range(2)])
        bad = (got != exp).any(axis=2)
        same_units = all(T.n_qu(got[s, f]) == T.n_qu(base[s, f]) for s in range(2) for f in range(nf))
        print(f"spliced nch={nch}: mismatching frames {int(bad.sum())}/{bad.size}; zero records differ from the writer without records: bad {int((zero != base).any())}; "
              f"unit count moved: bad {int(not same_units)} ({time.time()-t:.1f}s)", flush=True)

if __name__ == "__main__":
    if "--nobuild" not in sys.argv: run_emu.build()
    goldens()
    spliced()
