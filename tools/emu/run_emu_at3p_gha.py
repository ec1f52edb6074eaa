#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: the tone analysis kernels (k_at3p_tone_find, k_at3p_tone_select, k_at3p_tone_sub, k_at3p_tone_state behind
at3phip_analyse_tones and at3phip_encode_frames_tonal) through the CPU SIMT emulator, lane by lane, against the C restatement
tests/host/at3p_gha_cpu.c.  usage: run_emu_at3p_gha.py [plain|gated|shared|domain:1|domain:2] [--nobuild]   (default: plain)
  plain   records and residuals of three different streams side by side, the frames of the restatement's pipeline in one call and in
          two, the 16-bit entry point, the frame budget's crafted frame, and sines next to both ends of a subband
  gated   AT3PHIP_TONES_GATED (k_at3p_tone_find<true>): records and residuals of the crafted onsets and offsets in one call and in
          several, 8 frames of stereo burst (records, residuals, and the frames of the restatement's pipeline in one call and in
          three), and the host gate function
  shared  AT3PHIP_TONES_SHARED (k_at3p_tone_select<true>, k_at3p_tone_sub<., true>): two stereo streams side by side over 4 slots -
          one band of channel 1 differing in stream 0, an onset in stream 1 -, with and without the gates, in one call and split
          1 + 3; and a mono stream, where the flag changes nothing
  domain:C  tests/float_domain_lib.py's 12 streams (NaN, infinities, +-FLT_MAX, overflowing and subnormal samples in frame 1) of C
          channels side by side over 6 frames, in every flag combination (mono: sharing once, where it changes nothing), whole and
          split 2 + 1 + 3: records, residuals (a NaN against a NaN) and the frames of encode_frames_tonal against the restatement of
          each stream alone"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import numpy as np
import at3p_gha_lib as G
from atracdenc_amd.binding import At3pHip, at3p_host_tone_gates
import run_emu

STREAMS, NF, SHARED_NF = ("tones", "burst", "noise"), 6, 4

def streams(nch):
    t = time.time()
    pcm = np.stack([G.signal_pcm(n, NF, nch) for n in STREAMS])
    enc = At3pHip(n_streams=3, max_frames=NF, channels=nch, lib_path=run_emu.EMU)
    one = At3pHip(n_streams=1, max_frames=NF, channels=nch, lib_path=run_emu.EMU)
    want = [G.pipeline(pcm[s], write=lambda specs, recs: one.write_frames(specs[None], None, recs[None])[0]) for s in range(3)]
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

def gated_case(tag, bands, nch, split):
    t = time.time()
    n = bands.shape[0]
    enc = At3pHip(n_streams=1, max_frames=n, channels=nch, lib_path=run_emu.EMU)
    at, gb, gr = 0, [], []
    for k in split:
        b, r = enc.analyse_tones(bands[None, at:at + k], gated=True)
        gb.append(b[0]); gr.append(r[0]); at += k
    enc.close()
    gb, gr = np.concatenate(gb), np.concatenate(gr)
    wb, wr = G.CpuToneAnalyser(nch, True).analyse(bands)
    bad_g = int(not np.array_equal(at3p_host_tone_gates(bands, run_emu.EMU), G.cpu_gates(bands)))
    print(f"{tag} nch={nch} split {split}: records bad {int(gb.tobytes() != wb.tobytes())}; residuals bad {int(not np.array_equal(gr.view(np.uint32), wr.view(np.uint32)))}; "
          f"host gates bad {bad_g}; waves {[G.n_waves(b) for b in gb]} points {[len(G.points(b, nch)) for b in gb]} ({time.time()-t:.1f}s)", flush=True)

def gated_burst(nch=2, nf=8):
    pcm = G.signal_pcm("burst", nf, nch)
    gated_case("burst", G.pqf_bands(pcm), nch, (nf,))
    enc = At3pHip(n_streams=1, max_frames=nf, channels=nch, lib_path=run_emu.EMU)
    exp = G.pipeline(pcm, True, write=lambda specs, recs: enc.write_frames(specs[None], None, recs[None])[0])[0]
    for split in ((nf,), (3, 1, 4)):
        enc.reset()
        at, got = 0, []
        for n in split:
            got.append(enc.encode_frames_tonal(pcm[None, at:at + n], gated=True)[0])
            at += n
        bad = (np.concatenate(got) != exp).any(axis=1)
        print(f"encode burst nch={nch} split {split}: mismatching frames {int(bad.sum())}/{bad.size} {np.argwhere(bad)[:4].tolist()}", flush=True)
    enc.close()

def run(enc, bands, split, gated, shared):
    at, gb, gr = 0, [], []
    for k in split:
        b, r = enc.analyse_tones(bands[:, at:at + k], gated=gated, shared=shared)
        gb.append(b); gr.append(r); at += k
    return np.concatenate(gb, 1), np.concatenate(gr, 1)

def shared_stereo(gated, split):
    t = time.time()
    bands = np.stack([G.budget_bands(SHARED_NF, differ=True), G.stereo_onset_bands(not gated, SHARED_NF)])
    enc = At3pHip(n_streams=2, max_frames=SHARED_NF, channels=2, lib_path=run_emu.EMU)
    gb, gr = run(enc, bands, split, gated, True)
    enc.close()
    for s in range(2):
        wb, wr = G.CpuToneAnalyser(2, gated, True).analyse(bands[s])
        print(f"stream {s} gated={int(gated)} split {split}: records bad {int(gb[s].tobytes() != wb.tobytes())}; residuals bad {int(not np.array_equal(gr[s].view(np.uint32), wr.view(np.uint32)))}; "
              f"waves {[G.n_waves(b) for b in gb[s]]} sharing {[hex(int(b['tone_sharing'])) for b in gb[s]]} ({time.time()-t:.1f}s)", flush=True)

def shared_mono():
    bands = np.ascontiguousarray(G.budget_bands(SHARED_NF)[None, :, :1])
    enc = At3pHip(n_streams=1, max_frames=SHARED_NF, channels=1, lib_path=run_emu.EMU)
    gb, gr = run(enc, bands, (1, 3), False, True)
    enc.reset()
    ub, ur = run(enc, bands, (1, 3), False, False)
    enc.close()
    wb, wr = G.CpuToneAnalyser(1, shared=True).analyse(bands[0])
    print(f"mono: against the unflagged run bad {int(gb.tobytes() != ub.tobytes() or not np.array_equal(gr.view(np.uint32), ur.view(np.uint32)))}; "
          f"against the restatement bad {int(gb[0].tobytes() != wb.tobytes() or not np.array_equal(gr[0].view(np.uint32), wr.view(np.uint32)))}; waves {[G.n_waves(b) for b in gb[0]]}", flush=True)

def plain():
    for nch in (1, 2): streams(nch)
    budget()
    ends()

def gated():
    for nch in (1, 2):
        for name, bands in G.crafted_cases(nch).items():
            gated_case(name, bands, nch, (6,) if name.startswith("onset") else (1, 2, 3))
    gated_burst()

def shared():
    for gated in (True, False):
        for split in ((SHARED_NF,), (1, 3)):
            shared_stereo(gated, split)
    shared_mono()

def domain(nch):
    import float_domain_lib as FD
    for gated, shared in FD.tones_modes(nch):
        want = FD.tones_expect(run_emu.EMU, nch, gated, shared)
        for split in (None, FD.TONES_SPLIT):
            t = time.time()
            bad = FD.tones_bad(FD.tones_run(run_emu.EMU, nch, gated, shared, split=split), want)
            print(f"domain nch={nch} gated={int(gated)} shared={int(shared)} split {split or 'whole'}: records bad {len(bad['records'])}; residuals bad {len(bad['residuals'])}; "
                  f"frames bad {len(bad['frames'])} {({k: v for k, v in bad.items() if v}) or ''} ({time.time()-t:.1f}s)", flush=True)

if __name__ == "__main__":
    part = {"plain": plain, "gated": gated, "shared": shared, "domain:1": lambda: domain(1), "domain:2": lambda: domain(2)}.get(next((a for a in sys.argv[1:] if not a.startswith("--")), "plain"))
    if part is None: sys.exit(__doc__)
    if "--nobuild" not in sys.argv: run_emu.build()
    part()
