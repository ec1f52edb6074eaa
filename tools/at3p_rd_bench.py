#!/usr/bin/env python3
"""ATRAC3plus rate-distortion word lengths (AT3PHIP_ALLOC_RD) beside AT3PHIP_ALLOC_ADAPTIVE | AT3PHIP_ALLOC_SPARSE alone: what they do
to the round trip, and what they cost.

  Quality: the project's signals (noise, burst, tones, mix, stress), mono and stereo, 14 frames, at 48, 64, 96, 128 and 352 kbit/s,
      encoded with and without the flag and decoded by this project's decoder; round-trip SNR per channel at the codec's delay. On a
      GPU both are the library's calls; with --restatement (no GPU) both are the C restatements, to which the tests hold the library
      byte for byte and bit for bit, so the numbers are the same.
  Time (GPU only): 64 streams x 128 stereo frames of `mix` and `noise` resident in HBM at 64, 128 and 352 kbit/s. The writer kernel
      alone between the library's own events (at3phip_get_write_timing of a waiting call) and the whole PCM-to-frames call on the
      host clock around the waiting call, the median of --steps calls per run, --runs runs, the two flag sets alternating.
      --extra-lib NAME=PATH times another build of the library on the same calls (a build whose kernel leaves out the guard's two
      scans shows their share).
No counters are collected and nothing is traced. Writes one JSON line (--out: also to that file)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import at3p_gha_lib as G  # noqa: E402

SIGNALS = ("noise", "burst", "tones", "mix", "stress")
KBIT = {48: 280, 64: 376, 96: 560, 128: 744, 352: 2048}   # at3hipenc's --bitrate sizes
NF = 14
T_SIGNALS, T_KBIT = ("mix", "noise"), (64, 128, 352)


def quality_restatement():
    import at3p_writer_lib as W
    from at3p_writer_lib import MIN_BYTES
    out = {}
    for name in SIGNALS:
        for nch in (1, 2):
            x = G.signal_pcm(name, NF, nch)
            sp = W.specs_of_pcm(x)
            for kbit, fb in KBIT.items():
                if fb < MIN_BYTES[nch]:
                    continue
                cell = {}
                for key, frames in (("sparse", W.write_adaptive(sp, fb, True)), ("rd", W.write_rd(sp, fb))):
                    y, rej = W.decode(frames, nch, sparse=True)
                    assert rej.sum() == 0
                    cell[key] = [round(G.snr_db(x[:, :, c].reshape(-1), y[:, :, c].reshape(-1), NF), 2) for c in range(nch)]
                rec = W.write_rd(sp, fb, info=True)[1]
                cell["frames_rd_of"] = [int(rec["chose"].sum()), NF]
                out[f"{name}_{nch}_{kbit}"] = cell
    return out


def quality_library(B):
    from at3p_writer_lib import MIN_BYTES
    out = {}
    for name in SIGNALS:
        for nch in (1, 2):
            x = np.ascontiguousarray(G.signal_pcm(name, NF, nch)[None])
            for kbit, fb in KBIT.items():
                if fb < MIN_BYTES[nch]:
                    continue
                enc = B.At3pHip(n_streams=1, max_frames=NF, channels=nch, frame_bytes=fb)
                dec = B.At3pHipDecoder(n_streams=1, channels=nch, max_frames=NF, frame_bytes=fb)
                cell = {}
                for key, rd in (("sparse", False), ("rd", True)):
                    enc.reset()
                    dec.reset()
                    y = dec.decode(enc.encode_frames(x, adaptive=True, sparse=True, rd=rd), sparse=True)[0]
                    cell[key] = [round(G.snr_db(x[0, :, :, c].reshape(-1), y[:, :, c].reshape(-1), NF), 2) for c in range(nch)]
                cell["rejected"] = int(sum(dec.counters().values()))
                enc.close()
                dec.close()
                out[f"{name}_{nch}_{kbit}"] = cell
    return out


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
            enc = B.At3pHip(n_streams=S, max_frames=F, channels=C, lib_path=path, frame_bytes=None if fb == 2048 else fb)
            torch.cuda.synchronize()
            for name in T_SIGNALS:
                cell = {"sparse": {"call_ms": [], "write_ms": []}, "rd": {"call_ms": [], "write_ms": []}}
                for r in range(a.runs):
                    for key in (("sparse", "rd") if r % 2 == 0 else ("rd", "sparse")):
                        call = lambda: enc.encode_frames_device(d_pcm[name].data_ptr(), F, out.data_ptr(), adaptive=True, sparse=True, rd=key == "rd")
                        ms, wr = timed(call, a.steps, a.warmup, after=lambda: enc.timings()["write_ms"])
                        cell[key]["call_ms"].append(round(ms, 4))
                        cell[key]["write_ms"].append(round(wr, 4))
                for what in ("call_ms", "write_ms"):
                    cell[f"ratio_{what}"] = round(float(np.median(cell["rd"][what]) / np.median(cell["sparse"][what])), 3)
                res["cells"][f"{lib}_{name}_{kbit}"] = cell
            enc.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--restatement", action="store_true", help="quality from the C restatements, without a GPU; no timing")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--extra-lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if a.restatement:
        res["quality_restatement"] = quality_restatement()
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("needs an MI355X (or --restatement for the quality table alone)")
        from atracdenc_amd import binding as B
        if not a.no_quality:
            res["quality"] = quality_library(B)
        res["time"] = timing(B, a)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
