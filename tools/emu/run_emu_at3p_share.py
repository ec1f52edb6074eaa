#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: the tone analysis kernels with AT3PHIP_TONES_SHARED (k_at3p_tone_select<true>, k_at3p_tone_sub<., true>
behind at3phip_analyse_tones) through the CPU SIMT emulator, lane by lane, against the C restatement
tests/host/at3p_gha_share_cpu.c: two stereo streams side by side over 4 slots - one band of channel 1 differing in stream 0, an
onset in stream 1 -, with and without the gates, in one call and split 1 + 3; and a mono stream, where the flag changes nothing."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import numpy as np
import at3p_gha_lib as G
import at3p_gha_share_lib as GS
from atracdenc_amd.binding import At3pHip
import run_emu

NF = 4

def run(enc, bands, split, gated, shared):
    at, gb, gr = 0, [], []
    for k in split:
        b, r = enc.analyse_tones(bands[:, at:at + k], gated=gated, shared=shared)
        gb.append(b); gr.append(r); at += k
    return np.concatenate(gb, 1), np.concatenate(gr, 1)

def stereo(gated, split):
    t = time.time()
    bands = np.stack([GS.budget_bands(NF, differ=True), GS.onset_bands(not gated, NF)])
    enc = At3pHip(n_streams=2, max_frames=NF, channels=2, lib_path=run_emu.EMU)
    gb, gr = run(enc, bands, split, gated, True)
    enc.close()
    for s in range(2):
        wb, wr = GS.CpuSharedAnalyser(2, gated).analyse(bands[s])
        print(f"stream {s} gated={int(gated)} split {split}: records bad {int(gb[s].tobytes() != wb.tobytes())}; residuals bad {int(not np.array_equal(gr[s].view(np.uint32), wr.view(np.uint32)))}; "
              f"waves {[G.n_waves(b) for b in gb[s]]} sharing {[hex(int(b['tone_sharing'])) for b in gb[s]]} ({time.time()-t:.1f}s)", flush=True)

def mono():
    bands = np.ascontiguousarray(GS.budget_bands(NF)[None, :, :1])
    enc = At3pHip(n_streams=1, max_frames=NF, channels=1, lib_path=run_emu.EMU)
    gb, gr = run(enc, bands, (1, 3), False, True)
    enc.reset()
    ub, ur = run(enc, bands, (1, 3), False, False)
    enc.close()
    wb, wr = GS.CpuSharedAnalyser(1).analyse(bands[0])
    print(f"mono: against the unflagged run bad {int(gb.tobytes() != ub.tobytes() or not np.array_equal(gr.view(np.uint32), ur.view(np.uint32)))}; "
          f"against the restatement bad {int(gb[0].tobytes() != wb.tobytes() or not np.array_equal(gr[0].view(np.uint32), wr.view(np.uint32)))}; waves {[G.n_waves(b) for b in gb[0]]}", flush=True)

if __name__ == "__main__":
    if "--nobuild" not in sys.argv: run_emu.build()
    for gated in (True, False):
        for split in ((NF,), (1, 3)):
            stereo(gated, split)
    mono()
