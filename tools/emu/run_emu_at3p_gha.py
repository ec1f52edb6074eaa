#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: the tone analysis kernels (k_at3p_tone_find, k_at3p_tone_select, k_at3p_tone_sub, k_at3p_tone_state behind
at3phip_analyse_tones and at3phip_encode_frames_tonal) through the CPU SIMT emulator, lane by lane, against the C restatement
tests/host/at3p_gha_cpu.c: records and residuals of three different streams side by side, the frames of the restatement's
pipeline in one call and in two, the 16-bit entry point, the frame budget's crafted frame, and sines next to both ends of a subband."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import numpy as np
import at3p_gha_lib as G
from atracdenc_amd.binding import At3pHip
import run_emu

STREAMS, NF = ("tones", "burst", "noise"), 6

def streams(nch):
    t = time.time()
    pcm = np.stack([G.signal_pcm(n, NF, nch) for n in STREAMS])
    enc = At3pHip(n_streams=3, max_frames=NF, channels=nch, lib_path=run_emu.EMU)
    one = At3pHip(n_streams=1, max_frames=NF, channels=nch, lib_path=run_emu.EMU)
    want = [G.pipeline(pcm[s], lambda specs, recs: one.write_frames(specs[None], None, recs[None])[0]) for s in range(3)]
    blocks, resid = enc.analyse_tones(enc.pqf(pcm))
    bad_b = sum(blocks[s].tobytes() != want[s][1].tobytes() for s in range(3))
    bad_r = sum(not np.array_equal(resid[s].view(np.uint32), want[s][2].view(np.uint32)) for s in range(3))
    print(f"analyse nch={nch}: records bad {bad_b}; residuals bad {bad_r}; waves {[sum(G.n_waves(b) for b in blocks[s]) for s in range(3)]} ({time.time()-t:.1f}s)", flush=True)
    exp = np.stack([w[0] for w in want])
    for split in ((NF,), (2, 4)):
        enc.reset()
        at, got = 0, []
        for n in split:
            got.append(enc.encode_frames_tonal(pcm[:, at:at + n]))
            at += n
        bad = (np.concatenate(got, 1) != exp).any(axis=2)
        print(f"encode nch={nch} split {split}: mismatching frames {int(bad.sum())}/{bad.size} {np.argwhere(bad)[:4].tolist()}", flush=True)
    s16 = np.round(pcm * 32767.0).astype(np.int16)
    enc.reset()
    a = enc.encode_frames_tonal_s16(s16)
    enc.reset()
    b = enc.encode_frames_tonal((s16.astype(np.float32) / np.float32(32768.0)).astype(np.float32))
    print(f"encode nch={nch} 16-bit against its floats: bad {int((a != b).any())}", flush=True)
    enc.close(); one.close()

def budget():
    bands = G.budget_bands()
    enc = At3pHip(n_streams=1, max_frames=2, channels=2, lib_path=run_emu.EMU)
    blocks, resid = enc.analyse_tones(bands[None])
    enc.close()
    wb, wr = G.CpuToneAnalyser(2).analyse(bands)
    bad = int(blocks[0].tobytes() != wb.tobytes()) + int(not np.array_equal(resid[0].view(np.uint32), wr.view(np.uint32)))
    print(f"budget: bad {bad}; waves kept {G.n_waves(blocks[0, 1])}", flush=True)

def ends():
    bands = G.end_sine_bands()
    enc = At3pHip(n_streams=1, max_frames=3, channels=2, lib_path=run_emu.EMU)
    blocks, resid = enc.analyse_tones(bands[None])
    enc.close()
    wb, wr = G.CpuToneAnalyser(2).analyse(bands)
    bad = int(blocks[0].tobytes() != wb.tobytes()) + int(not np.array_equal(resid[0].view(np.uint32), wr.view(np.uint32)))
    print(f"ends: bad {bad}; waves {[G.n_waves(b) for b in blocks[0]]}", flush=True)

if __name__ == "__main__":
    if "--nobuild" not in sys.argv: run_emu.build()
    for nch in (1, 2): streams(nch)
    budget()
    ends()
