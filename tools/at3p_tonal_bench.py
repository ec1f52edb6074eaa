#!/usr/bin/env python3
"""ATRAC3plus decoder throughput with tonal blocks (include/at3phip.h, TONAL BLOCKS), beside tools/at3p_decode_bench.py. Stereo
frames resident in HBM, one at3phip_decode per timed region bracketed by events, the median region reported, for three inputs:
frames with random tonal blocks decoded with AT3PHIP_DECODE_TONES, the same frames without their tonal blocks with the flag, and
the non-tonal goldens (tests/golden/at3p_decode.npz) without the flag. Shapes: 64 streams x 128 frames and 1 x 65 536."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from atracdenc_amd import At3pHipDecoder  # noqa: E402
import at3p_tonal_lib as L  # noqa: E402
from at3p_decode_lib import make_frame  # noqa: E402


def pools(n=64):
    rng = np.random.default_rng(5)
    tonal, plain = [], []
    while len(tonal) < n:
        b = L.random_block(rng, 2)
        base = make_frame(2, nqu=6, wl=[[3] * 6, [3] * 6], sf=[[30] * 6, [30] * 6], mant=lambda ch, qu, k: (k % 3) - 1)
        fr = L.splice_tonal(base, L.tonal_bits(2, b))
        if fr is not None:
            tonal.append(fr)
            plain.append(base)
    g = np.load(os.path.join(ROOT, "tests", "golden", "at3p_decode.npz"))
    golden = np.concatenate([g[f"{c}_frames"] for c in g["cases"] if str(c).startswith(("sig_", "win_")) and str(c).endswith("_2ch")])
    return {"tonal": (np.stack(tonal), True), "tonal_removed": (np.stack(plain), True), "goldens_flag_off": (golden, False)}


def shape(pool, tones, streams, frames, steps, warmup):
    idx = np.arange(streams * frames) % pool.shape[0]
    src = torch.from_numpy(np.ascontiguousarray(pool[idx].reshape(streams, frames, 2048))).cuda()
    out = torch.zeros((streams, frames, 2048, 2), dtype=torch.float32, device="cuda")
    dec = At3pHipDecoder(n_streams=streams, channels=2, max_frames=frames)
    for _ in range(warmup):
        dec.decode_device(src, out, tones=tones)
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dec.decode_device(src, out, tones=tones)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    c = dec.counters()
    dec.close()
    assert not any(c.values()), c
    med = float(np.median(ms))
    return {"median_ms": round(med, 4), "stereo_frames_per_s": round(streams * frames / (med * 1e-3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    for name, (pool, tones) in pools().items():
        for s, f in ((64, 128), (1, 65536)):
            res[f"{name} {s}x{f}"] = shape(pool, tones, s, f, a.steps, a.warmup)
    line = json.dumps({"metric": "at3p_tonal_decode", "results": res})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
