#!/usr/bin/env python3
"""The measurements behind the GATES of include/at3phip.h ("Gates"), without a GPU: for each candidate ratio
R of G1 the stationary-signal condition (flagged output = unflagged output on tones, noise, silence), the crafted detection cases,
and the CPU round trip (restatement, oracle MDCT and writer, spliced block, cpu_tonal_decode, snr_db) of burst, mix, stress and
keyed, gated against ungated from the same run.  usage: at3p_gha_gate_measure.py [R ...]   (default 16 64 256)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import at3p_gha_lib as G
import at3p_tonal_lib as T
from at3_testlib import at3p_signal

NF = 14

def signal(name):
    return G.keyed_pcm(NF, 1)[:, :, 0] if name == "keyed" else at3p_signal(name, NF, channel=0)

def round_trip(name, gated, ratio):
    x2 = signal(name)
    bands = G.pqf_bands(np.concatenate([x2, np.zeros((1, 2048), np.float32)])[:, :, None])   # and the flushing frame
    blocks, resid = G.CpuToneAnalyser(1, gated, ratio=ratio).analyse(bands)
    base = G.write_residual(resid[1:])
    recs = [None] + list(blocks[1:NF])   # frame j carries the spectrum of residual j and block T_{j-1}
    pcm, rej = T.cpu_tonal_decode(G.splice_blocks(base, recs, 1), 1)
    assert rej.sum() == 0
    npts = sum(len(G.points(b, 1)) for b in blocks)
    return G.snr_db(x2.reshape(-1), pcm[:, :, 0].reshape(-1), NF), float(np.mean([G.n_waves(b) for b in blocks[1:]])), npts

def stationary(ratio):
    bad = []
    for name in ("tones", "noise", "silence"):
        for nch in (1, 2):
            bands = G.pqf_bands(G.signal_pcm(name, NF, nch))
            a, b = G.CpuToneAnalyser(nch, True, ratio=ratio).analyse(bands), G.CpuToneAnalyser(nch, False, ratio=ratio).analyse(bands)
            if a[0].tobytes() != b[0].tobytes() or a[1].tobytes() != b[1].tobytes():
                bad.append((name, nch, int(np.count_nonzero(G.cpu_gates(bands, ratio)))))
    return bad

def detection(ratio):
    out = {}
    for s0 in (3, 4, 16, 28, 29):
        on, off = G.cpu_gates(G.onset_bands(s0, 1), ratio)[2, 0], G.cpu_gates(G.offset_bands(s0 - 1, 1), ratio)[2, 0]
        out[s0] = ([int(on[b]) for b in G.GATE_BANDS], [int(off[b]) for b in G.GATE_BANDS])
    return out

if __name__ == "__main__":
    for ratio in [float(a) for a in sys.argv[1:]] or [16.0, 64.0, 256.0]:
        print(f"R = {ratio:g}: stationary condition broken by {stationary(ratio)}; gates of the crafted frames (onset, offset) {detection(ratio)}", flush=True)
        for name in ("burst", "keyed", "mix", "stress", "tones"):
            p, g = round_trip(name, False, ratio), round_trip(name, True, ratio)
            print(f"  {name:7s} ungated {p[0]:6.2f} dB ({p[1]:.2f} waves per frame)   gated {g[0]:6.2f} dB ({g[1]:.2f} waves per frame, {g[2]} points)", flush=True)
