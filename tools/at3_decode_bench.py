#!/usr/bin/env python3
"""ATRAC3 decoder throughput (include/at3hip.h, the decoder section; not the headline metric - bench.py stays on the encoder's
north star). Frames resident in HBM (reference-encoded frames of tests/golden/at3_decode.npz, tiled), one at3hip_decode per timed
region on torch's current stream, bracketed by events; the median region is reported.
Shapes: 64 streams x 128 frames and 1 stream x 131 072 frames, on LP2 (384 bytes) and the joint-stereo LP4 row (192 bytes),
float32 and 16-bit output. CPU baseline on one core: the C restatement (tests/host/at3_decode_cpu.c); the reference has no ATRAC3
decoder."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from atracdenc_amd import At3HipDecoder  # noqa: E402

HBM_PEAK_GBS = 8000.0
FP32_NO_FMA_PEAK_TF = 157.3 / 2.0   # as tools/at1_decode_bench.py: the contract has no FMA
# algorithmic flops per channel-frame: four IMDCT-512 (128-point kissfft ~4 480, rotations 1 536, window 512 each),
# dequantisation 2 048, demodulation 3 072, two TQmf<512> (256 pairs x 96) and one TQmf<1024> (512 pairs x 96), their merges
# 4 096, frame n-1's rebuilt history ~3 000
FLOPS_PER_CF = 4 * (4480 + 1536 + 512) + 2048 + 3072 + 2 * 256 * 96 + 512 * 96 + 4096 + 3000
# HBM bytes per stereo frame: the frame, the windowed IMDCT records written and read (2 units x 4 bands x 512 floats), gain
# records; plus the PCM
BYTES_IN_PER_FRAME = 2 * 2 * 4 * 512 * 4 + 3 * 2 * 68


def frame_pool(fsz):
    g = np.load(os.path.join(ROOT, "tests", "golden", "at3_decode.npz"))
    return np.concatenate([g[f"{n}_frames"] for n in g["cases"] if int(g[f"{n}_row"][0]) == fsz and "_ch2" in str(n)])


def gpu_shape(fsz, streams, frames, s16, steps, warmup):
    pool = frame_pool(fsz)
    idx = np.arange(streams * frames) % pool.shape[0]
    src = torch.from_numpy(np.ascontiguousarray(pool[idx].reshape(streams, frames, fsz))).cuda()
    out = torch.zeros((streams, frames, 1024, 2), dtype=torch.int16 if s16 else torch.float32, device="cuda")
    dec = At3HipDecoder(n_streams=streams, frame_size=fsz, max_frames=frames)
    for _ in range(warmup):
        dec.decode_device(src, out)
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dec.decode_device(src, out)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    c = dec.counters()
    dec.close()
    assert not any(c.values()), c
    med = float(np.median(ms))
    rate = streams * frames / (med * 1e-3)
    gbs = rate * (fsz + BYTES_IN_PER_FRAME + (4096 if s16 else 8192)) / 1e9
    tf = rate * 2 * FLOPS_PER_CF / 1e12
    return {"shape": f"{streams}x{frames} {fsz}B {'s16' if s16 else 'f32'}", "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
            "stereo_frames_per_s": round(rate), "x_realtime": round(rate * 1024 / 44100, 1), "GB_per_s": round(gbs, 1),
            "hbm_frac": round(gbs / HBM_PEAK_GBS, 4), "TFLOPs": round(tf, 3), "no_fma_fp32_frac": round(tf / FP32_NO_FMA_PEAK_TF, 4)}


def cpu_baseline(fsz, frames):
    from at3_decode_lib import CpuDecoder
    pool = frame_pool(fsz)
    d = CpuDecoder(fsz, fsz in (192, 272))
    x = np.ascontiguousarray(pool[np.arange(frames) % pool.shape[0]])
    t = time.perf_counter()
    d.decode(x)
    return {"restatement": {"stereo_frames_per_s": round(frames / (time.perf_counter() - t)), "cores": 1, "frames": frames, "frame_size": fsz}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-frames", type=int, default=2048)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    res = [gpu_shape(fsz, s, f, s16, a.steps, a.warmup) for fsz in (384, 192) for s, f in ((64, 128), (1, 131072)) for s16 in (False, True)]
    line = json.dumps({"metric": "atrac3_decode_stereo_frames_per_s", "value": res[2]["stereo_frames_per_s"], "target": 20e6,
                       "shapes": res, "flops_per_channel_frame": FLOPS_PER_CF,
                       "cpu_baseline": {**cpu_baseline(384, a.cpu_frames), "reference": "none: the reference has no ATRAC3 decoder"}})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
