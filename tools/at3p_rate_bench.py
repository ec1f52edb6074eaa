#!/usr/bin/env python3
"""The ATRAC3plus adaptive encoder and the decoder at frame sizes other than 2048 bytes (at3phip_set_frame_bytes,
at3phip_decoder_set_frame_bytes). The protocol of tools/at3p_alloc_bench.py: everything resident in HBM, each call timed on the
host around the (waiting) call, the median of --steps calls per run, --runs runs.

  Encoder: at3phip_encode_frames with AT3PHIP_ALLOC_ADAPTIVE on `mix` and `noise`, 64 streams x 128 stereo frames, at 376, 1120 and
      2048 bytes, with the writer's own device time (at3phip_get_write_timing) beside the call's.
  Decoder: at3phip_decode (float output, tones on) on one stream of 2048 stereo frames of `mix`, at 376 and 2048 bytes; the frames
      are the encoder's own at that size.
  Yardstick, the parent: --parent-lib names a libat3hip.so built from the parent commit; it and this library alternate (which goes
      first alternating as well) on the adaptive call at 2048, the unflagged call (same bytes?) and the decoder at 2048. This
      library's median of medians must lie within the parent's own spread (not above its slowest run).
  --kernel-stats name=csv ... merges kernel times from `rocprofv3 --kernel-trace --stats` runs of their own (start the tool with
      --only NAME under the profiler: it then runs that variant alone and writes nothing).
Not measured by this tool: host-fed calls (PCM, frames or samples crossing the bus) and anything on more than one GPU.
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
DEC_F = 2048
SIGNALS = ("mix", "noise")
ENC_SIZES, DEC_SIZES = (376, 1120, 2048), (376, 2048)
VARIANTS = {**{f"enc_{name}_{fb}": ("enc", name, fb) for name in SIGNALS for fb in ENC_SIZES}, **{f"dec_{fb}": ("dec", "mix", fb) for fb in DEC_SIZES}}


def staggered(x):
    """x [F + 2][2048][C] -> [S][F][2048][C]: each stream starting 37 samples after the one before"""
    x = x.reshape(-1, C)
    return np.ascontiguousarray(np.stack([x[37 * s:37 * s + F * 2048].reshape(F, 2048, C) for s in range(S)]))


def timed(call, steps, warmup, after=None):
    """(median ms of `call`, median of after() per step or None)"""
    for _ in range(warmup):
        call()
    ms, extra = [], []
    for _ in range(steps):
        t = time.perf_counter()
        call()    # waits for the device itself
        ms.append((time.perf_counter() - t) * 1e3)
        if after:
            extra.append(after())
    return float(np.median(ms)), (float(np.median(extra)) if after else None)


class Encoder:
    def __init__(self, lib_path, frame_bytes=None):
        # (the parent's library has no setter: it is never asked for one)
        self.enc = B.At3pHip(n_streams=S, max_frames=F, channels=C, lib_path=lib_path, frame_bytes=None if frame_bytes in (None, 2048) else frame_bytes)
        self.fb = frame_bytes or 2048
        self.out = torch.zeros((S, F, self.fb), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def call(self, d_pcm, adaptive=True):
        self.enc.encode_frames_device(d_pcm.data_ptr(), F, self.out.data_ptr(), adaptive=adaptive)

    def run(self, d_pcm, steps, warmup, adaptive=True):
        return timed(lambda: self.call(d_pcm, adaptive), steps, warmup, lambda: self.enc.timings().get("write_ms", 0.0))


class Decoder:
    def __init__(self, lib_path, frame_bytes=None):
        self.dec = B.At3pHipDecoder(n_streams=1, channels=C, max_frames=DEC_F, lib_path=lib_path, frame_bytes=None if frame_bytes in (None, 2048) else frame_bytes)
        self.pcm = torch.zeros((1, DEC_F, 2048, C), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

    def call(self, d_frames):
        self.dec.decode_device(d_frames, self.pcm, ordered=False, tones=True)

    def run(self, d_frames, steps, warmup):
        return timed(lambda: self.call(d_frames), steps, warmup)[0]


def long_stream_frames(fb):
    """[1][DEC_F][fb] on the device: `mix` encoded by this library at that size, 128 frames per call"""
    x = np.ascontiguousarray(G.signal_pcm("mix", DEC_F, C)[None])
    enc = B.At3pHip(n_streams=1, max_frames=128, channels=C, frame_bytes=None if fb == 2048 else fb)
    out = np.concatenate([enc.encode_frames(x[:, f:f + 128], adaptive=True) for f in range(0, DEC_F, 128)], axis=1)
    enc.close()
    d = torch.from_numpy(out).cuda()
    torch.cuda.synchronize()
    return d


def alternate(par, new, run, runs):
    p_runs, n_runs = [], []
    for r in range(runs):
        for who in ((par, new) if r % 2 == 0 else (new, par)):
            (p_runs if who is par else n_runs).append(run(who))
    return {"parent_ms": [round(x, 4) for x in p_runs], "new_ms": [round(x, 4) for x in n_runs],
            "new_median_within_parent_spread": bool(np.median(n_runs) <= max(p_runs))}


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
    d_pcm = {name: torch.from_numpy(staggered(G.signal_pcm(name, F + 2, C))).cuda() for name in SIGNALS}
    torch.cuda.synchronize()
    if a.only:
        kind, name, fb = VARIANTS[a.only]
        if kind == "enc":
            e = Encoder(None, fb)
            for _ in range(a.steps + a.warmup):
                e.call(d_pcm[name])
        else:
            frames, d = long_stream_frames(fb), Decoder(None, fb)
            for _ in range(a.steps + a.warmup):
                d.call(frames)
        return
    res = {"shape": f"encoder {S} x {F} stereo frames, decoder 1 x {DEC_F} stereo frames, everything in HBM", "steps": a.steps, "runs": a.runs,
           "not_measured": ["host-fed calls (PCM, frames or samples crossing the bus)", "more than one GPU"]}
    rows = {}
    for name in SIGNALS:
        for fb in ENC_SIZES:
            e = Encoder(None, fb)
            runs = [e.run(d_pcm[name], a.steps, a.warmup) for _ in range(a.runs)]
            call, write = float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))
            rows[f"{name}_{fb}"] = {"call_ms": round(call, 4), "runs_ms": [round(r[0], 4) for r in runs], "writer_ms": round(write, 4),
                                    "frames_per_s": round(S * F / (call * 1e-3))}
            e.enc.close()
        for fb in ENC_SIZES[:-1]:
            rows[f"{name}_{fb}"]["call_ratio_to_2048"] = round(rows[f"{name}_{fb}"]["call_ms"] / rows[f"{name}_2048"]["call_ms"], 3)
            rows[f"{name}_{fb}"]["writer_ratio_to_2048"] = round(rows[f"{name}_{fb}"]["writer_ms"] / max(rows[f"{name}_2048"]["writer_ms"], 1e-9), 3)
    res["encoder"] = rows
    frames = {fb: long_stream_frames(fb) for fb in DEC_SIZES}
    drows = {}
    for fb in DEC_SIZES:
        d = Decoder(None, fb)
        runs = [d.run(frames[fb], a.steps, a.warmup) for _ in range(a.runs)]
        rejected = sum(d.dec.counters().values())
        drows[str(fb)] = {"call_ms": round(float(np.median(runs)), 4), "runs_ms": [round(r, 4) for r in runs],
                          "frames_per_s": round(DEC_F / (float(np.median(runs)) * 1e-3)), "rejected": int(rejected)}
        d.dec.close()
    res["decoder"] = drows
    if a.parent_lib:
        plib = os.path.abspath(a.parent_lib)
        par, new = Encoder(plib), Encoder(None)
        yard = {}
        for name in SIGNALS:
            for adaptive in (True, False):
                for who in (par, new):
                    who.enc.reset()
                    who.call(d_pcm[name], adaptive)
                same = bool(torch.equal(par.out, new.out))
                row = alternate(par, new, lambda who: who.run(d_pcm[name], a.steps, a.warmup, adaptive)[0], a.runs)
                row["same_frames_as_parent"] = same
                yard[f"{name}_{'adaptive' if adaptive else 'unflagged'}_2048"] = row
        par.enc.close()
        new.enc.close()
        pd, nd = Decoder(plib), Decoder(None)
        pd.call(frames[2048])
        nd.call(frames[2048])
        same = bool(torch.equal(pd.pcm.view(torch.int32), nd.pcm.view(torch.int32)))
        row = alternate(pd, nd, lambda who: who.run(frames[2048], a.steps, a.warmup), a.runs)
        row["same_pcm_as_parent"] = same
        yard["decoder_2048"] = row
        pd.dec.close()
        nd.dec.close()
        res["yardstick_parent"] = yard
    for item in a.kernel_stats:
        name, path = item.split("=", 1)
        res.setdefault("kernel_trace", {})[name] = kernel_stats(path)
    line = json.dumps({"metric": "at3p_rate", "results": res})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
