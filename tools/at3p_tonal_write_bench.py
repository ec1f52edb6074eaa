#!/usr/bin/env python3
"""The ATRAC3plus frame writer with and without tonal records (at3phip_write_frames / at3phip_write_frames_tonal): 64 streams x 128
stereo frames, spectra and frames resident in HBM, each call timed on the host around the (waiting) call, the median of --steps
calls per run, and the device milliseconds at3phip_get_write_timing reports (record upload and kernel).

  Yardstick 1, the parent: --parent-lib names a libat3hip.so built from the parent commit; its at3phip_write_frames and this
      library's run alternately on the same spectra, --runs runs each. The new median of medians must lie within the parent's
      own spread (not above its slowest run).
  Yardstick 2, the untouched call: at3phip_write_frames_tonal with random blocks (4 of 5 frames carry one) and with the largest
      block on every frame, against this library's at3phip_write_frames on the same spectra.
  --kernel-stats name=csv ... merges kernel times from `rocprofv3 --kernel-trace --stats` runs of their own (start the tool with
      --only NAME under the profiler: it then runs that variant alone and writes nothing).
Writes one JSON line (--out: also to that file, profiles/at3p_tonal_write_bench.json)."""
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
import at3p_tonal_lib as T  # noqa: E402
import at3p_tonal_write_lib as L  # noqa: E402

S, F, C = 64, 128, 2


def records(kind):
    rng = np.random.default_rng(11)
    if kind == "largest":
        one = B.pack_tonal_blocks(L.largest_block(C), C)
        return np.ascontiguousarray(np.broadcast_to(one, (S, F)))
    pool = B.pack_tonal_blocks([T.random_block(rng, C) if i % 5 else None for i in range(256)], C)
    return np.ascontiguousarray(pool[rng.integers(0, pool.shape[0], (S, F))])


def block_bits(rec_kind):
    if rec_kind == "largest":
        return sum(n for _, n in T.tonal_bits(C, L.largest_block(C)))
    rng = np.random.default_rng(11)
    bl = [T.random_block(rng, C) if i % 5 else None for i in range(256)]
    return float(np.mean([sum(n for _, n in T.tonal_bits(C, b)) if b else 0 for b in bl]))


class Writer:
    def __init__(self, lib_path, d_specs, d_frames):
        self.enc = B.At3pHip(n_streams=S, max_frames=F, channels=C, lib_path=lib_path)
        self.specs, self.frames = d_specs.data_ptr(), d_frames.data_ptr()
        self.flags = B.AT3HIP_PCM_ON_DEVICE | B.AT3HIP_OUT_ON_DEVICE

    def call(self, recs):
        if recs is None:
            self.enc.write_frames_ptr(self.specs, F, None, self.frames, self.flags)
        else:
            self.enc.write_frames_tonal_ptr(self.specs, F, None, recs.ctypes.data, self.frames, self.flags)

    def run(self, recs, steps, warmup):
        for _ in range(warmup):
            self.call(recs)
        ms, dev = [], []
        for _ in range(steps):
            t = time.perf_counter()
            self.call(recs)           # waits for the device itself
            ms.append((time.perf_counter() - t) * 1e3)
            dev.append(self.enc.timings()["write_ms"])
        return float(np.median(ms)), float(np.median(dev))


def kernel_stats(path):
    """{kernel name: average ns} of the writer's kernels from a rocprofv3 kernel_stats csv"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        if "k_at3p_write" in name:
            out[name] = {"calls": int(float(row.get("Calls", 0))), "average_us": round(float(row.get("AverageNs", 0)) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", choices=["untouched", "random", "largest"], default=None)
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: nothing is measured without one")
    specs = (0.05 * np.random.RandomState(21).standard_normal((S, F, C, 2048))).astype(np.float32)
    d_specs = torch.from_numpy(specs).cuda()
    d_frames = torch.zeros((S, F, 2048), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    recs = {"untouched": None, "random": records("random"), "largest": records("largest")}
    new = Writer(None, d_specs, d_frames)
    if a.only:
        for _ in range(a.steps + a.warmup):
            new.call(recs[a.only])
        return
    res = {"shape": f"{S} x {F} stereo frames, spectra and frames in HBM", "steps": a.steps, "runs": a.runs}
    # the results first: the untouched call writes the parent's bytes, zero records write the same
    new.call(None)
    ref_frames = d_frames.cpu().numpy().copy()
    if a.parent_lib:
        par = Writer(os.path.abspath(a.parent_lib), d_specs, d_frames)
        d_frames.zero_()
        torch.cuda.synchronize()
        par.call(None)
        res["same_frames_as_parent"] = bool(np.array_equal(d_frames.cpu().numpy(), ref_frames))
        p_runs, n_runs = [], []
        for _ in range(a.runs):
            p_runs.append(par.run(None, a.steps, a.warmup))
            n_runs.append(new.run(None, a.steps, a.warmup))
        res["yardstick_parent"] = {"parent_call_ms": [round(x[0], 4) for x in p_runs], "new_call_ms": [round(x[0], 4) for x in n_runs],
                                   "parent_device_ms": [round(x[1], 4) for x in p_runs], "new_device_ms": [round(x[1], 4) for x in n_runs],
                                   "new_median_within_parent_spread": bool(np.median([x[0] for x in n_runs]) <= max(x[0] for x in p_runs))}
    y2 = {}
    for kind in ("untouched", "random", "largest"):
        runs = [new.run(recs[kind], a.steps, a.warmup) for _ in range(a.runs)]
        y2[kind] = {"call_ms": round(float(np.median([r[0] for r in runs])), 4), "device_ms": round(float(np.median([r[1] for r in runs])), 4),
                    "frames_per_s": round(S * F / (float(np.median([r[0] for r in runs])) * 1e-3))}
        if kind != "untouched":
            y2[kind]["call_ratio_to_untouched"] = round(y2[kind]["call_ms"] / y2["untouched"]["call_ms"], 3)
            y2[kind]["device_ratio_to_untouched"] = round(y2[kind]["device_ms"] / y2["untouched"]["device_ms"], 3)
            y2[kind]["mean_block_bits"] = round(block_bits(kind), 1)
            y2[kind]["record_upload_bytes"] = int(recs[kind].nbytes)
    res["yardstick_untouched"] = y2
    for item in a.kernel_stats:
        name, path = item.split("=", 1)
        res.setdefault("kernel_trace", {})[name] = kernel_stats(path)
    line = json.dumps({"metric": "at3p_tonal_write", "results": res})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
