#!/usr/bin/env python3
"""ATRAC3plus decoder throughput (include/at3phip.h, the decoder section; not the headline metric - bench.py stays on the encoder's
north star). Frames resident in HBM (reference-written stereo frames of tests/golden/at3p_decode.npz, tiled), one at3phip_decode
per timed region on torch's current stream, bracketed by events; the median region is reported.
Shapes: 64 streams x 128 frames and 1 stream x 65 536 frames, stereo, float32 and 16-bit output. CPU baseline on one core: the C
restatement (tests/host/at3p_decode_cpu.c); the reference has no ATRAC3plus decoder."""
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
from atracdenc_amd import At3pHipDecoder  # noqa: E402

# f64 lane operations per channel-frame of the synthesis's exact DCT-IV: 151 columns x 16 outputs x 16 (multiply + add)
F64_OPS_PER_CF = 151 * 16 * 16 * 2


def frame_pool():
    g = np.load(os.path.join(ROOT, "tests", "golden", "at3p_decode.npz"))
    return np.concatenate([g[f"{n}_frames"] for n in g["cases"] if str(n).startswith(("sig_", "win_")) and str(n).endswith("_2ch")])


def gpu_shape(streams, frames, s16, steps, warmup):
    pool = frame_pool()
    idx = np.arange(streams * frames) % pool.shape[0]
    src = torch.from_numpy(np.ascontiguousarray(pool[idx].reshape(streams, frames, 2048))).cuda()
    out = torch.zeros((streams, frames, 2048, 2), dtype=torch.int16 if s16 else torch.float32, device="cuda")
    dec = At3pHipDecoder(n_streams=streams, channels=2, max_frames=frames)
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
    return {"shape": f"{streams}x{frames} {'s16' if s16 else 'f32'}", "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
            "stereo_frames_per_s": round(rate), "x_realtime": round(rate * 2048 / 44100, 1),
            "f64_Tops": round(rate * 2 * F64_OPS_PER_CF / 1e12, 3)}


def cpu_baseline(frames):
    from at3p_decode_lib import CpuDecoder
    pool = frame_pool()
    d = CpuDecoder(2)
    x = np.ascontiguousarray(pool[np.arange(frames) % pool.shape[0]])
    t = time.perf_counter()
    d.decode(x)
    return {"restatement": {"stereo_frames_per_s": round(frames / (time.perf_counter() - t)), "cores": 1, "frames": frames}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-frames", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    res = [gpu_shape(s, f, s16, a.steps, a.warmup) for s, f in ((64, 128), (1, 65536)) for s16 in (False, True)]
    line = json.dumps({"metric": "atrac3plus_decode_stereo_frames_per_s", "value": res[2]["stereo_frames_per_s"], "target": 100e3,
                       "shapes": res, "f64_ops_per_channel_frame": F64_OPS_PER_CF,
                       "cpu_baseline": {**cpu_baseline(a.cpu_frames), "reference": "none: the reference has no ATRAC3plus decoder"}})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
