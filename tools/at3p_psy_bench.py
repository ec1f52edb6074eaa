#!/usr/bin/env python3
"""ATRAC3plus masking-weighted word lengths (AT3PHIP_ALLOC_PSY) beside AT3PHIP_ALLOC_ADAPTIVE | AT3PHIP_ALLOC_SPARSE | AT3PHIP_ALLOC_RD alone:
what they do to the round trip, and what they cost.

  Quality (no GPU needed): the project's signals (noise, burst, tones, mix, stress), mono and stereo, 14 frames, at 48, 64, 96, 128 and
      352 kbit/s, written by the C restatements with and without the flag - the tests hold the library to them byte for byte - and decoded
      by the restatement of this project's decoder. Per channel:
        snr_db      the round-trip SNR at the codec's delay, as tools/at3p_rd_bench.py reports it;
        nmr_db      a noise-to-mask figure on the decoded PCM, independent of the encoder's spectrum: 2048-point Hann FFTs of the
                    delay-aligned original and of the error, hop 2048, without the first and last two frames; energies in 24 Bark bands
                    (z(f) = 13 atan(0.00076 f) + 3.5 atan((f / 7500)^2), band b = floor(z)); the threshold of a band is the largest of the
                    original's band energies spread by 10 dB per Bark upwards and 27 dB per Bark downwards, minus 12 dB, not below the
                    threshold in quiet (tools/gen_at3p_psy.py's curve, its minimum over the band's bins, against the same FFT's energy
                    of a full-scale 1 kHz sine); the mean over frames and bands of max(0, 10 log10(noise / threshold));
        above       the share of (frame, band) cells whose noise lies above the threshold.
  Time (GPU only): 64 streams x 128 stereo frames of `mix` and `noise` resident in HBM at 64, 128 and 352 kbit/s. The writer kernel
      alone between the library's own events (at3phip_get_write_timing of a waiting call) and the whole PCM-to-frames call on the
      host clock around the waiting call, the median of --steps calls per run, --runs runs, the flag sets (sparse, rd, psy) alternating.
      --extra-lib NAME=PATH times another build of the library (the parent commit's) on the sparse and rd calls in the same session.
No counters are collected and nothing is traced. Writes one JSON line (--out: also to that file)."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import at3p_gha_lib as G  # noqa: E402
import gen_at3p_psy as T  # noqa: E402

SIGNALS = ("noise", "burst", "tones", "mix", "stress")
KBIT = {48: 280, 64: 376, 96: 560, 128: 744, 352: 2048}   # at3hipenc's --bitrate sizes
NF = 14
T_SIGNALS, T_KBIT = ("mix", "noise"), (64, 128, 352)
N_FFT, N_BARK = 2048, 24


def _nmr_setup():
    f = np.arange(N_FFT // 2 + 1) * 44100.0 / N_FFT
    band = np.minimum(np.floor([T.bark(x) for x in f]).astype(int), N_BARK - 1)
    win = np.hanning(N_FFT + 1)[:N_FFT]
    t = np.arange(N_FFT)
    e_fs = float(np.sum(np.abs(np.fft.rfft(win * np.sin(2 * np.pi * 1000.0 * t / 44100.0))) ** 2))
    tab = T.ath_millibel()
    ath_db = np.array([T.ath_db(max(x, 10.0), tab) - 100.0 - 0.015 * (x * 1e-3) ** 2 for x in f])
    ath = np.array([e_fs * 10.0 ** (ath_db[band == b].min() / 10.0) for b in range(N_BARK)])
    dz = np.arange(N_BARK)[None, :] - np.arange(N_BARK)[:, None]                 # [masker][maskee]
    spread = 10.0 ** (-(T.SMR_DB + np.where(dz >= 0, T.SLOPE_UP * dz, T.SLOPE_DOWN * -dz)) / 10.0)
    return band, win, ath, spread


_SETUP = None


def nmr(x, y, n_frames):
    """x the input, y the decoder's output (one channel each, flat) -> (nmr_db, share of cells above the threshold)"""
    global _SETUP
    if _SETUP is None:
        _SETUP = _nmr_setup()
    band, win, ath, spread = _SETUP
    ref = x[2 * 2048:(n_frames - 2) * 2048].astype(np.float64)
    out = y[G.DELAY + 2 * 2048:G.DELAY + (n_frames - 2) * 2048].astype(np.float64)
    over = []
    for k in range(len(ref) // N_FFT):
        seg = slice(k * N_FFT, (k + 1) * N_FFT)
        S = np.abs(np.fft.rfft(win * ref[seg])) ** 2
        N = np.abs(np.fft.rfft(win * (ref[seg] - out[seg]))) ** 2
        Sb, Nb = np.bincount(band, S, N_BARK), np.bincount(band, N, N_BARK)
        thr = np.maximum((Sb[:, None] * spread).max(axis=0), ath)
        over.append(np.maximum(0.0, 10.0 * np.log10(np.maximum(Nb, 1e-300) / thr)))
    over = np.array(over)
    return round(float(over.mean()), 3), round(float((over > 0).mean()), 3)


def quality_restatement():
    import at3p_psy_lib as Y
    import at3p_writer_lib as W
    out = {}
    for name in SIGNALS:
        for nch in (1, 2):
            x = G.signal_pcm(name, NF, nch)
            sp = W.specs_of_pcm(x)
            for kbit, fb in KBIT.items():
                if fb < W.MIN_BYTES[nch]:
                    continue
                cell = {}
                for key, frames in (("rd", W.write_rd(sp, fb)), ("psy", Y.write_psy(sp, fb))):
                    y, rej = W.decode(frames, nch, sparse=True)
                    assert rej.sum() == 0
                    chans = [(x[:, :, c].reshape(-1), y[:, :, c].reshape(-1)) for c in range(nch)]
                    cell[key] = {"snr_db": [round(G.snr_db(a, b, NF), 2) for a, b in chans], "nmr_db": [nmr(a, b, NF)[0] for a, b in chans],
                                 "above": [nmr(a, b, NF)[1] for a, b in chans]}
                rec = Y.write_psy(sp, fb, info=True)[1]
                cell["frames_psy_of"] = [int(rec["chose"].sum()), NF]
                out[f"{name}_{nch}_{kbit}"] = cell
    summary = {}
    for kbit in KBIT:
        cells = [v for k, v in out.items() if k.endswith(f"_{kbit}")]
        mean = lambda key, what: round(float(np.mean([c for v in cells for c in v[key][what]])), 3)
        summary[str(kbit)] = {what: {"rd": mean("rd", what), "psy": mean("psy", what)} for what in ("snr_db", "nmr_db", "above")}
    return {"cells": out, "mean_over_signals_and_channels": summary}


def timing(B, a):
    import torch
    from at3p_rate_bench import C, F, S, staggered, timed
    libs = {"this": None}
    for spec in a.extra_lib:
        k, v = spec.split("=", 1)
        libs[k] = v
    d_pcm = {name: torch.from_numpy(staggered(G.signal_pcm(name, F + 2, C))).cuda() for name in T_SIGNALS}
    torch.cuda.synchronize()
    res = {"setup": f"{S} x {F} stereo frames in HBM, median of {a.steps} waiting calls, {a.runs} runs; write_ms between the library's events, "
                    "call_ms on the host clock", "device": torch.cuda.get_device_name(0), "cells": {}}
    for kbit in T_KBIT:
        fb = KBIT[kbit]
        out = torch.zeros((S, F, fb), dtype=torch.uint8, device="cuda")
        for lib, path in libs.items():
            keys = ("sparse", "rd", "psy") if path is None else ("sparse", "rd")
            enc = B.At3pHip(n_streams=S, max_frames=F, channels=C, lib_path=path, frame_bytes=None if fb == 2048 else fb)
            torch.cuda.synchronize()
            for name in T_SIGNALS:
                cell = {k: {"call_ms": [], "write_ms": []} for k in keys}
                for r in range(a.runs):
                    for key in (keys if r % 2 == 0 else keys[::-1]):
                        kw = dict(adaptive=True, sparse=True, rd=key != "sparse")
                        if key == "psy":
                            kw["psy"] = True
                        call = lambda: enc.encode_frames_device(d_pcm[name].data_ptr(), F, out.data_ptr(), **kw)
                        ms, wr = timed(call, a.steps, a.warmup, after=lambda: enc.timings()["write_ms"])
                        cell[key]["call_ms"].append(round(ms, 4))
                        cell[key]["write_ms"].append(round(wr, 4))
                if "psy" in keys:
                    for what in ("call_ms", "write_ms"):
                        cell[f"ratio_{what}"] = round(float(np.median(cell["psy"][what]) / np.median(cell["rd"][what])), 3)
                res["cells"][f"{lib}_{name}_{kbit}"] = cell
            enc.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--restatement", action="store_true", help="the quality table from the C restatements, without a GPU; no timing")
    ap.add_argument("--extra-lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--merge", default=None, help="a JSON file of an earlier run whose keys are kept beside this run's")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = json.load(open(a.merge)) if a.merge else {}
    if a.restatement:
        res["quality_restatement"] = quality_restatement()
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("needs an MI355X (or --restatement for the quality table alone)")
        from atracdenc_amd import binding as B
        res["time"] = timing(B, a)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
