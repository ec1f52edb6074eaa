#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: the tone analysis kernels with AT3PHIP_TONES_GATED (k_at3p_tone_find<true>, k_at3p_tone_select,
k_at3p_tone_sub, k_at3p_tone_state behind at3phip_analyse_tones and at3phip_encode_frames_tonal) through the CPU SIMT emulator,
lane by lane, against the C restatement tests/host/at3p_gha_gate_cpu.c: records and residuals of the crafted onsets and offsets in
one call and in several, 8 frames of stereo burst (records, residuals, and the frames of the restatement's pipeline in one call and
in three), and the host gate function."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import numpy as np
import at3p_gha_lib as G
import at3p_gha_gate_lib as GG
from atracdenc_amd.binding import At3pHip, at3p_host_tone_gates
import run_emu

def analyse(tag, bands, nch, split):
    t = time.time()
    n = bands.shape[0]
    enc = At3pHip(n_streams=1, max_frames=n, channels=nch, lib_path=run_emu.EMU)
    at, gb, gr = 0, [], []
    for k in split:
        b, r = enc.analyse_tones(bands[None, at:at + k], gated=True)
        gb.append(b[0]); gr.append(r[0]); at += k
    enc.close()
    gb, gr = np.concatenate(gb), np.concatenate(gr)
    wb, wr = GG.CpuGatedAnalyser(nch).analyse(bands)
    bad_g = int(not np.array_equal(at3p_host_tone_gates(bands, run_emu.EMU), GG.cpu_gates(bands)))
    print(f"{tag} nch={nch} split {split}: records bad {int(gb.tobytes() != wb.tobytes())}; residuals bad {int(not np.array_equal(gr.view(np.uint32), wr.view(np.uint32)))}; "
          f"host gates bad {bad_g}; waves {[G.n_waves(b) for b in gb]} points {[len(GG.points(b, nch)) for b in gb]} ({time.time()-t:.1f}s)", flush=True)

def burst(nch=2, nf=8):
    pcm = G.signal_pcm("burst", nf, nch)
    analyse("burst", G.pqf_bands(pcm), nch, (nf,))
    enc = At3pHip(n_streams=1, max_frames=nf, channels=nch, lib_path=run_emu.EMU)
    exp = GG.pipeline(pcm, True, lambda specs, recs: enc.write_frames(specs[None], None, recs[None])[0])[0]
    for split in ((nf,), (3, 1, 4)):
        enc.reset()
        at, got = 0, []
        for n in split:
            got.append(enc.encode_frames_tonal(pcm[None, at:at + n], gated=True)[0])
            at += n
        bad = (np.concatenate(got) != exp).any(axis=1)
        print(f"encode burst nch={nch} split {split}: mismatching frames {int(bad.sum())}/{bad.size} {np.argwhere(bad)[:4].tolist()}", flush=True)
    enc.close()

if __name__ == "__main__":
    if "--nobuild" not in sys.argv: run_emu.build()
    for nch in (1, 2):
        for name, bands in GG.crafted_cases(nch).items():
            analyse(name, bands, nch, (6,) if name.startswith("onset") else (1, 2, 3))
    burst()
