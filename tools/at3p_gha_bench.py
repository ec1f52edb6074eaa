#!/usr/bin/env python3
"""The ATRAC3plus encoder with the tone analysis (at3phip_encode_frames_tonal, with and without AT3PHIP_TONES_GATED and
AT3PHIP_TONES_SHARED) against the one without (at3phip_encode_frames): 64 streams x 128 stereo frames, PCM and frames resident in
HBM, each call timed on the host around the (waiting) call, the median of --steps calls per run.

  Yardstick 1, the parent: --parent-lib names a libat3hip.so built from the parent commit; it and this library run alternately on
      the same PCM, --runs runs each, which of the two goes first alternating as well (--parent-first: the parent's context and
      device buffers are created before this library's): at3phip_encode_frames and the unflagged at3phip_encode_frames_tonal on
      `tones`, the gated call on `burst` and the shared call on the dense signal. Each new median of medians must lie within the
      parent's own spread (not above its slowest run), and the frames must be the same bytes.
  Yardstick 2, the cost of the analysis: at3phip_encode_frames_tonal on `tones` (waves in every frame) and on `noise` (none: the
      fine search is skipped) against this library's at3phip_encode_frames on the same PCM. Not a gate.
  The gated rows: the call with AT3PHIP_TONES_GATED on `tones` (no event after the stream's start: the cost of G1 alone) and on
      `burst` (events in most bands of most frames: the gated fit), beside the unflagged call on `burst`. Reported, not bounded.
  The shared rows: the call with AT3PHIP_TONES_SHARED beside the unflagged one on `tones` with channel 0 in both channels (16 waves
      a frame, the budget does not bind: the flag only shortens the block) and on the dense signal (three sines in each of ten
      subbands, both channels alike: the budget binds without the flag). Reported, not bounded.
  --kernel-stats name=csv ... merges kernel times from `rocprofv3 --kernel-trace --stats` runs of their own (start the tool with
      --only NAME under the profiler: it then runs that variant alone and writes nothing).
Writes one JSON line (--out: also to that file)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from atracdenc_amd import binding as B  # noqa: E402
import at3p_gha_lib as G  # noqa: E402

S, F, C = 64, 128, 2


def staggered(x):
    """x [F + 2][2048][C] -> [S][F][2048][C]: each stream starting 37 samples after the one before"""
    x = x.reshape(-1, C)
    return np.ascontiguousarray(np.stack([x[37 * s:37 * s + F * 2048].reshape(F, 2048, C) for s in range(S)]))


SIGNALS = {"tones": lambda: G.signal_pcm("tones", F + 2, C), "noise": lambda: G.signal_pcm("noise", F + 2, C), "burst": lambda: G.signal_pcm("burst", F + 2, C),
           "tones_twin": lambda: G.twin_pcm("tones", F + 2), "dense": lambda: G.dense_pcm(F + 2)}
# name: (signal, tonal, gated, shared)
VARIANTS = {"plain": ("tones", False, False, False), "tones": ("tones", True, False, False), "noise": ("noise", True, False, False),
            "burst": ("burst", True, False, False), "tones_gated": ("tones", True, True, False), "burst_gated": ("burst", True, True, False),
            "tones_twin": ("tones_twin", True, False, False), "tones_twin_shared": ("tones_twin", True, False, True),
            "dense": ("dense", True, False, False), "dense_shared": ("dense", True, False, True)}


class Encoder:
    def __init__(self, lib_path, d_frames):
        self.enc = B.At3pHip(n_streams=S, max_frames=F, channels=C, lib_path=lib_path)
        self.frames = d_frames.data_ptr()

    def call(self, d_pcm, tonal, gated=False, shared=False):
        if gated or shared:
            self.enc.encode_frames_tonal_device(d_pcm.data_ptr(), F, self.frames, gated=gated, shared=shared)
        else:
            (self.enc.encode_frames_tonal_device if tonal else self.enc.encode_frames_device)(d_pcm.data_ptr(), F, self.frames)

    def run(self, d_pcm, steps, warmup, *how):
        for _ in range(warmup):
            self.call(d_pcm, *how)
        ms = []
        for _ in range(steps):
            t = time.perf_counter()
            self.call(d_pcm, *how)    # waits for the device itself
            ms.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ms))


def kernel_stats(path):
    """{kernel name: calls, average us} of the ATRAC3plus kernels from a rocprofv3 kernel_stats csv"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        if "k_at3p" in name:
            out[name.split("(")[0]] = {"calls": int(float(row.get("Calls", 0))), "average_us": round(float(row.get("AverageNs", 0)) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-first", action="store_true", help="create the parent's context (and its device buffers) before this library's")
    ap.add_argument("--only", choices=list(VARIANTS), default=None)
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: nothing is measured without one")
    d_pcm = {name: torch.from_numpy(staggered(make())).cuda() for name, make in SIGNALS.items() if not a.only or name == VARIANTS[a.only][0]}
    d_frames = torch.zeros((S, F, 2048), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    par = Encoder(os.path.abspath(a.parent_lib), d_frames) if a.parent_lib and a.parent_first else None
    new = Encoder(None, d_frames)
    if a.only:
        name, *how = VARIANTS[a.only]
        for _ in range(a.steps + a.warmup):
            new.call(d_pcm[name], *how)
        return

    def row(variant):
        name, *how = VARIANTS[variant]
        new.enc.reset()
        runs = [new.run(d_pcm[name], a.steps, a.warmup, *how) for _ in range(a.runs)]
        return {"call_ms": round(float(np.median(runs)), 4), "runs_ms": [round(x, 4) for x in runs], "frames_per_s": round(S * F / (float(np.median(runs)) * 1e-3))}

    res = {"shape": f"{S} x {F} stereo frames, PCM and frames in HBM", "steps": a.steps, "runs": a.runs, "parent_context_first": bool(a.parent_first)}
    if a.parent_lib:
        par = par or Encoder(os.path.abspath(a.parent_lib), d_frames)
        for key, variant in (("yardstick_parent", "plain"), ("yardstick_parent_tonal", "tones"), ("yardstick_parent_gated", "burst_gated"),
                             ("yardstick_parent_shared", "dense_shared")):
            name, *how = VARIANTS[variant]
            new.enc.reset()
            par.enc.reset()
            new.call(d_pcm[name], *how)
            ref = d_frames.cpu().numpy().copy()
            d_frames.zero_()
            torch.cuda.synchronize()
            par.call(d_pcm[name], *how)
            same = bool(np.array_equal(d_frames.cpu().numpy(), ref))
            p_runs, n_runs = [], []
            for r in range(a.runs):   # (which of the two goes first alternates as well)
                for who in ((par, new) if r % 2 == 0 else (new, par)):
                    (p_runs if who is par else n_runs).append(who.run(d_pcm[name], a.steps, a.warmup, *how))
            res[key] = {"variant": variant, "same_frames_as_parent": same, "parent_call_ms": [round(x, 4) for x in p_runs],
                        "new_call_ms": [round(x, 4) for x in n_runs], "new_median_within_parent_spread": bool(np.median(n_runs) <= max(p_runs))}
        par.enc.close()
    y2 = {kind: row(kind) for kind in ("plain", "tones", "noise")}
    for kind in ("tones", "noise"):
        y2[kind]["call_ratio_to_plain"] = round(y2[kind]["call_ms"] / y2["plain"]["call_ms"], 3)
    res["yardstick_analysis"] = y2
    res["gated"] = {kind: row(kind) for kind in ("tones_gated", "burst", "burst_gated")}
    for r in res["gated"].values():
        r["call_ratio_to_plain"] = round(r["call_ms"] / y2["plain"]["call_ms"], 3)
    res["shared"] = {kind: row(kind) for kind in ("tones_twin", "tones_twin_shared", "dense", "dense_shared")}
    for name in ("tones_twin", "dense"):
        res["shared"][name + "_shared"]["call_ratio_to_unflagged"] = round(res["shared"][name + "_shared"]["call_ms"] / res["shared"][name]["call_ms"], 4)
    for item in a.kernel_stats:
        name, path = item.split("=", 1)
        res.setdefault("kernel_trace", {})[name] = kernel_stats(path)
    line = json.dumps({"metric": "at3p_gha", "results": res})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
