#!/usr/bin/env python3
"""The ATRAC3plus encoder with adaptive word lengths (at3phip_encode_frames with AT3PHIP_ALLOC_ADAPTIVE) against the fixed
word-length table (the same call without the flag): 64 streams x 128 stereo frames, PCM and frames resident in HBM, each call
timed on the host around the (waiting) call, the median of --steps calls per run, --runs runs. The protocol of
tools/at3p_gha_bench.py.

  Yardstick 1, the parent: --parent-lib names a libat3hip.so built from the parent commit; it and this library run the unflagged
      call alternately on the same PCM (which of the two goes first alternating as well). This library's median of medians must
      lie within the parent's own spread (not above its slowest run), and the frames must be the same bytes.
  Yardstick 2, the cost of the allocation: the flagged call against the unflagged one on `mix`, `noise` and `tones`, with the
      writer's own device time (at3phip_get_write_timing) beside the call's. Reported, not bounded.
  --kernel-stats name=csv ... merges kernel times from `rocprofv3 --kernel-trace --stats` runs of their own (start the tool with
      --only NAME under the profiler: it then runs that variant alone and writes nothing).
Not measured by this tool: host-fed calls (PCM and frames crossing the bus) and anything on more than one GPU.
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
SIGNALS = ("mix", "noise", "tones")
# name: (signal, adaptive)
VARIANTS = {f"{name}_{kind}": (name, kind == "adaptive") for name in SIGNALS for kind in ("fixed", "adaptive")}


def staggered(x):
    """x [F + 2][2048][C] -> [S][F][2048][C]: each stream starting 37 samples after the one before"""
    x = x.reshape(-1, C)
    return np.ascontiguousarray(np.stack([x[37 * s:37 * s + F * 2048].reshape(F, 2048, C) for s in range(S)]))


class Encoder:
    def __init__(self, lib_path, d_frames):
        self.enc = B.At3pHip(n_streams=S, max_frames=F, channels=C, lib_path=lib_path)
        self.frames = d_frames.data_ptr()

    def call(self, d_pcm, adaptive):
        if adaptive:
            self.enc.encode_frames_device(d_pcm.data_ptr(), F, self.frames, adaptive=True)
        else:
            self.enc.encode_frames_device(d_pcm.data_ptr(), F, self.frames)   # (the parent's binding has no such keyword)

    def run(self, d_pcm, steps, warmup, adaptive):
        """(median call ms, median writer ms on the device)"""
        for _ in range(warmup):
            self.call(d_pcm, adaptive)
        ms, wr = [], []
        for _ in range(steps):
            t = time.perf_counter()
            self.call(d_pcm, adaptive)    # waits for the device itself
            ms.append((time.perf_counter() - t) * 1e3)
            wr.append(self.enc.timings().get("write_ms", 0.0))
        return float(np.median(ms)), float(np.median(wr))


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
    ap.add_argument("--only", choices=list(VARIANTS), default=None)
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: nothing is measured without one")
    d_pcm = {name: torch.from_numpy(staggered(G.signal_pcm(name, F + 2, C))).cuda() for name in SIGNALS if not a.only or name == VARIANTS[a.only][0]}
    d_frames = torch.zeros((S, F, 2048), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    new = Encoder(None, d_frames)
    if a.only:
        name, adaptive = VARIANTS[a.only]
        for _ in range(a.steps + a.warmup):
            new.call(d_pcm[name], adaptive)
        return
    res = {"shape": f"{S} x {F} stereo frames, PCM and frames in HBM", "steps": a.steps, "runs": a.runs,
           "not_measured": ["host-fed calls (PCM and frames crossing the bus)", "more than one GPU"]}
    if a.parent_lib:
        par = Encoder(os.path.abspath(a.parent_lib), d_frames)
        for name in SIGNALS:
            new.enc.reset()
            par.enc.reset()
            new.call(d_pcm[name], False)
            ref = d_frames.cpu().numpy().copy()
            d_frames.zero_()
            torch.cuda.synchronize()
            par.call(d_pcm[name], False)
            same = bool(np.array_equal(d_frames.cpu().numpy(), ref))
            p_runs, n_runs = [], []
            for r in range(a.runs):   # (which of the two goes first alternates as well)
                for who in ((par, new) if r % 2 == 0 else (new, par)):
                    (p_runs if who is par else n_runs).append(who.run(d_pcm[name], a.steps, a.warmup, False)[0])
            res.setdefault("yardstick_parent", {})[name] = {
                "same_frames_as_parent": same, "parent_call_ms": [round(x, 4) for x in p_runs], "new_call_ms": [round(x, 4) for x in n_runs],
                "new_median_within_parent_spread": bool(np.median(n_runs) <= max(p_runs))}
        par.enc.close()
    rows = {}
    for variant, (name, adaptive) in VARIANTS.items():
        new.enc.reset()
        runs = [new.run(d_pcm[name], a.steps, a.warmup, adaptive) for _ in range(a.runs)]
        call, write = float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))
        rows[variant] = {"call_ms": round(call, 4), "runs_ms": [round(r[0], 4) for r in runs], "writer_ms": round(write, 4),
                         "frames_per_s": round(S * F / (call * 1e-3))}
    for name in SIGNALS:
        rows[f"{name}_adaptive"]["call_ratio_to_fixed"] = round(rows[f"{name}_adaptive"]["call_ms"] / rows[f"{name}_fixed"]["call_ms"], 3)
        rows[f"{name}_adaptive"]["writer_ratio_to_fixed"] = round(rows[f"{name}_adaptive"]["writer_ms"] / max(rows[f"{name}_fixed"]["writer_ms"], 1e-9), 3)
    res["yardstick_allocation"] = rows
    for item in a.kernel_stats:
        name, path = item.split("=", 1)
        res.setdefault("kernel_trace", {})[name] = kernel_stats(path)
    line = json.dumps({"metric": "at3p_alloc", "results": res})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
