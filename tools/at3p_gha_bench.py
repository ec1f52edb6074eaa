#!/usr/bin/env python3
"""The ATRAC3plus encoder with the tone analysis (at3phip_encode_frames_tonal) against the one without (at3phip_encode_frames):
64 streams x 128 stereo frames, PCM and frames resident in HBM, each call timed on the host around the (waiting) call, the median
of --steps calls per run.

  Yardstick 1, the parent: --parent-lib names a libat3hip.so built from the parent commit; its at3phip_encode_frames and this
      library's run alternately on the same PCM, --runs runs each, and so do the two libraries' at3phip_encode_frames_tonal without
      a flag. Each new median of medians must lie within the parent's own spread (not above its slowest run), and the frames must
      be the same bytes.
  Yardstick 2, the cost of the analysis: at3phip_encode_frames_tonal on `tones` (waves in every frame) and on `noise` (none: the
      fine search is skipped) against this library's at3phip_encode_frames on the same PCM. Not a gate.
  The gated rows: at3phip_encode_frames_tonal with AT3PHIP_TONES_GATED on `tones` (no event after the stream's start: the cost of
      G1 alone) and on `burst` (events in most bands of most frames: the gated fit), beside the unflagged call on `burst`. Reported,
      not bounded.
  --kernel-stats name=csv ... merges kernel times from `rocprofv3 --kernel-trace --stats` runs of their own (start the tool with
      --only NAME under the profiler: it then runs that variant alone and writes nothing).
Writes one JSON line (--out: also to that file, profiles/at3p_gha_bench.json)."""
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


def signal(name):
    """[S][F][2048][C]: the signal, each stream starting 37 samples after the one before"""
    x = G.signal_pcm(name, F + 2, C).reshape(-1, C)
    return np.ascontiguousarray(np.stack([x[37 * s:37 * s + F * 2048].reshape(F, 2048, C) for s in range(S)]))


class Encoder:
    def __init__(self, lib_path, d_frames):
        self.enc = B.At3pHip(n_streams=S, max_frames=F, channels=C, lib_path=lib_path)
        self.frames = d_frames.data_ptr()

    def call(self, d_pcm, tonal, gated=False):
        if gated:
            self.enc.encode_frames_tonal_device(d_pcm.data_ptr(), F, self.frames, gated=True)
        else:
            (self.enc.encode_frames_tonal_device if tonal else self.enc.encode_frames_device)(d_pcm.data_ptr(), F, self.frames)

    def run(self, d_pcm, tonal, steps, warmup, gated=False):
        for _ in range(warmup):
            self.call(d_pcm, tonal, gated)
        ms = []
        for _ in range(steps):
            t = time.perf_counter()
            self.call(d_pcm, tonal, gated)    # waits for the device itself
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
    ap.add_argument("--only", choices=["plain", "tones", "noise", "burst", "tones_gated", "burst_gated"], default=None)
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: nothing is measured without one")
    d_pcm = {name: torch.from_numpy(signal(name)).cuda() for name in ("tones", "noise", "burst")}
    d_frames = torch.zeros((S, F, 2048), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    new = Encoder(None, d_frames)
    if a.only:
        for _ in range(a.steps + a.warmup):
            new.call(d_pcm["tones" if a.only == "plain" else a.only.split("_")[0]], a.only != "plain", a.only.endswith("_gated"))
        return
    res = {"shape": f"{S} x {F} stereo frames, PCM and frames in HBM", "steps": a.steps, "runs": a.runs}
    if a.parent_lib:
        par = Encoder(os.path.abspath(a.parent_lib), d_frames)
        new.enc.reset()
        new.call(d_pcm["tones"], False)
        ref = d_frames.cpu().numpy().copy()
        d_frames.zero_()
        torch.cuda.synchronize()
        par.call(d_pcm["tones"], False)
        res["same_frames_as_parent"] = bool(np.array_equal(d_frames.cpu().numpy(), ref))
        p_runs, n_runs = [], []
        for _ in range(a.runs):
            p_runs.append(par.run(d_pcm["tones"], False, a.steps, a.warmup))
            n_runs.append(new.run(d_pcm["tones"], False, a.steps, a.warmup))
        res["yardstick_parent"] = {"parent_call_ms": [round(x, 4) for x in p_runs], "new_call_ms": [round(x, 4) for x in n_runs],
                                   "new_median_within_parent_spread": bool(np.median(n_runs) <= max(p_runs))}
        # the same for the unflagged at3phip_encode_frames_tonal
        new.enc.reset()
        par.enc.reset()
        new.call(d_pcm["tones"], True)
        ref = d_frames.cpu().numpy().copy()
        d_frames.zero_()
        torch.cuda.synchronize()
        par.call(d_pcm["tones"], True)
        same = bool(np.array_equal(d_frames.cpu().numpy(), ref))
        p_runs, n_runs = [], []
        for _ in range(a.runs):
            p_runs.append(par.run(d_pcm["tones"], True, a.steps, a.warmup))
            n_runs.append(new.run(d_pcm["tones"], True, a.steps, a.warmup))
        res["yardstick_parent_tonal"] = {"same_frames_as_parent": same, "parent_call_ms": [round(x, 4) for x in p_runs],
                                         "new_call_ms": [round(x, 4) for x in n_runs],
                                         "new_median_within_parent_spread": bool(np.median(n_runs) <= max(p_runs))}
    y2 = {}
    for kind in ("plain", "tones", "noise"):
        new.enc.reset()
        runs = [new.run(d_pcm["noise" if kind == "noise" else "tones"], kind != "plain", a.steps, a.warmup) for _ in range(a.runs)]
        y2[kind] = {"call_ms": round(float(np.median(runs)), 4), "frames_per_s": round(S * F / (float(np.median(runs)) * 1e-3))}
        if kind != "plain":
            y2[kind]["call_ratio_to_plain"] = round(y2[kind]["call_ms"] / y2["plain"]["call_ms"], 3)
    res["yardstick_analysis"] = y2
    gated = {}
    for name, flag in (("tones", True), ("burst", False), ("burst", True)):
        new.enc.reset()
        runs = [new.run(d_pcm[name], True, a.steps, a.warmup, flag) for _ in range(a.runs)]
        row = {"call_ms": round(float(np.median(runs)), 4), "frames_per_s": round(S * F / (float(np.median(runs)) * 1e-3)),
               "call_ratio_to_plain": round(float(np.median(runs)) / y2["plain"]["call_ms"], 3)}
        gated[name + ("_gated" if flag else "")] = row
    res["gated"] = gated
    for item in a.kernel_stats:
        name, path = item.split("=", 1)
        res.setdefault("kernel_trace", {})[name] = kernel_stats(path)
    line = json.dumps({"metric": "at3p_gha", "results": res})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
