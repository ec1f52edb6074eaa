#!/usr/bin/env python3
"""ATRAC1 decoder throughput (include/at1hip.h, the decoder section; not the headline metric - bench.py stays on the ATRAC3
north star). Sound units resident in HBM (reference-encoded units of tests/golden/at1_decode.npz, tiled), one
at1hip_decode per timed region on torch's current stream, bracketed by events; the median region is reported.
Shapes: 64 streams x 128 frames and 1 stream x 131 072 frames, stereo, float32 and 16-bit output.
CPU baseline on one core: the C restatement (tests/host/at1_decode_cpu.c) and, where oracle/_ref/libat3ref.so exists, the
reference decoder itself (its driver in tests/at1_decode_lib.py; the figure includes one process start)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from atracdenc_amd import At1HipDecoder  # noqa: E402

HBM_PEAK_GBS = 8000.0
FP32_NO_FMA_PEAK_TF = 157.3 / 2.0   # bench.py's ceiling: the fp32 vector peak counts an FMA as two flops; the contract has none
# algorithmic flops per channel-frame: synthesis 128 x 96 + 256 x 96, merges 768, frame n-1's history 12 x 96 + 70,
# IMDCT (all long) ~10 700, dequantisation 1 024, windows ~300
FLOPS_PER_CF = 128 * 96 + 256 * 96 + 768 + 12 * 96 + 70 + 10_700 + 1_024 + 300
# HBM bytes per channel-frame: unit, band record written and read, tails written and read, mode and last-writer index
# written and read, the PCM
BYTES_IN_PER_CF = 212 + 2 * 2048 + 2 * 192 + 2 * 4 + 2 * 16


def unit_pool():
    g = np.load(os.path.join(ROOT, "tests", "golden", "at1_decode.npz"))
    return np.concatenate([g[f"{n}_units"] for n in g["cases"] if "_ch2_" in n and not n.startswith(("crafted", "random"))])


def gpu_shape(streams, frames, s16, steps, warmup, pool):
    idx = np.arange(streams * frames) % pool.shape[0]
    units = torch.from_numpy(np.ascontiguousarray(pool[idx].reshape(streams, frames, 2, 212))).cuda()
    out = torch.zeros((streams, frames, 512, 2), dtype=torch.int16 if s16 else torch.float32, device="cuda")
    dec = At1HipDecoder(n_streams=streams, max_frames=frames, channels=2)
    for _ in range(warmup):
        dec.decode_device(units, out)
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dec.decode_device(units, out)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    dec.close()
    med = float(np.median(ms))
    cf = streams * frames * 2
    rate = cf / (med * 1e-3)
    gbs = rate * (BYTES_IN_PER_CF + (1024 if s16 else 2048)) / 1e9
    tf = rate * FLOPS_PER_CF / 1e12
    return {"shape": f"{streams}x{frames} stereo {'s16' if s16 else 'f32'}", "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
            "channel_frames_per_s": round(rate), "x_realtime": round(rate / 2 * 512 / 44100, 1), "GB_per_s": round(gbs, 1),
            "hbm_frac": round(gbs / HBM_PEAK_GBS, 4), "TFLOPs": round(tf, 3), "no_fma_fp32_frac": round(tf / FP32_NO_FMA_PEAK_TF, 4)}


def cpu_baselines(pool, frames):
    from at1_decode_lib import CpuDecoder, have_ref_decoder, ref_decode
    units = np.ascontiguousarray(pool[np.arange(frames) % pool.shape[0]])
    d = CpuDecoder(2)
    t = time.perf_counter()
    d.decode(units)
    out = {"restatement": {"channel_frames_per_s": round(2 * frames / (time.perf_counter() - t)), "cores": 1, "frames": frames}}
    if have_ref_decoder():
        with tempfile.TemporaryDirectory() as tmp:
            ref_decode(units[:8], tmp)   # builds the driver
            t = time.perf_counter()
            ref_decode(units, tmp)
            out["reference"] = {"channel_frames_per_s": round(2 * frames / (time.perf_counter() - t)), "cores": 1, "frames": frames,
                                "note": "one process: start-up, AEA read and writing the floats included"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-frames", type=int, default=4096)
    a = ap.parse_args()
    pool = unit_pool()
    res = [gpu_shape(s, f, s16, a.steps, a.warmup, pool) for s, f in ((64, 128), (1, 131072)) for s16 in (False, True)]
    print(json.dumps({"metric": "atrac1_decode_channel_frames_per_s", "value": res[2]["channel_frames_per_s"],
                      "target": 500e6, "shapes": res, "flops_per_channel_frame": FLOPS_PER_CF, "cpu_baseline": cpu_baselines(pool, a.cpu_frames)}))


if __name__ == "__main__":
    main()
