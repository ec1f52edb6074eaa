#!/usr/bin/env python3
"""at3phip_encode_frames_tonal with AT3PHIP_TONES_SHARED against the call without the flag, and this library against its parent:
64 streams x 128 stereo frames, PCM and frames resident in HBM, each call timed on the host around the (waiting) call, the median of
--steps calls per run. A sibling of tools/at3p_gha_bench.py.

  Yardstick, the parent: --parent-lib names a libat3hip.so built from the parent commit; its at3phip_encode_frames and
      at3phip_encode_frames_tonal (no flag) and this library's run alternately on the same PCM, --runs runs each. Each new median
      of medians must lie within the parent's own spread (not above its slowest run), and the frames must be the same bytes.
  The shared rows: the flagged call beside the unflagged one on `tones` with channel 0 in both channels (16 waves a frame, the
      budget does not bind: the flag only shortens the block) and on the dense signal (three sines in each of ten subbands, both
      channels alike: the budget binds without the flag). Reported, not bounded.
Writes one JSON line (--out: also to that file, profiles/at3p_share_bench.json)."""
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
from atracdenc_amd import binding as B  # noqa: E402
import at3p_gha_lib as G  # noqa: E402
import at3p_gha_share_lib as GS  # noqa: E402

S, F, C = 64, 128, 2


def staggered(x):
    """x [F + 2][2048][C] -> [S][F][2048][C]: each stream starting 37 samples after the one before"""
    x = x.reshape(-1, C)
    return np.ascontiguousarray(np.stack([x[37 * s:37 * s + F * 2048].reshape(F, 2048, C) for s in range(S)]))


class Encoder:
    def __init__(self, lib_path, d_frames):
        self.enc = B.At3pHip(n_streams=S, max_frames=F, channels=C, lib_path=lib_path)
        self.frames = d_frames.data_ptr()

    def call(self, d_pcm, tonal, shared=False):
        if shared:
            self.enc.encode_frames_tonal_device(d_pcm.data_ptr(), F, self.frames, shared=True)
        else:
            (self.enc.encode_frames_tonal_device if tonal else self.enc.encode_frames_device)(d_pcm.data_ptr(), F, self.frames)

    def run(self, d_pcm, tonal, steps, warmup, shared=False):
        for _ in range(warmup):
            self.call(d_pcm, tonal, shared)
        ms = []
        for _ in range(steps):
            t = time.perf_counter()
            self.call(d_pcm, tonal, shared)    # waits for the device itself
            ms.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-first", action="store_true", help="create the parent's context (and its device buffers) before this library's")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: nothing is measured without one")
    d_pcm = {"tones": torch.from_numpy(staggered(G.signal_pcm("tones", F + 2, C))).cuda(),
             "tones_twin": torch.from_numpy(staggered(GS.twin_pcm("tones", F + 2))).cuda(),
             "dense": torch.from_numpy(staggered(GS.dense_pcm(F + 2))).cuda()}
    d_frames = torch.zeros((S, F, 2048), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    par = Encoder(os.path.abspath(a.parent_lib), d_frames) if a.parent_lib and a.parent_first else None
    new = Encoder(None, d_frames)
    res = {"shape": f"{S} x {F} stereo frames, PCM and frames in HBM", "steps": a.steps, "runs": a.runs, "parent_context_first": bool(a.parent_first)}
    if a.parent_lib:
        par = par or Encoder(os.path.abspath(a.parent_lib), d_frames)
        for key, tonal in (("yardstick_parent", False), ("yardstick_parent_tonal", True)):
            new.enc.reset()
            par.enc.reset()
            new.call(d_pcm["tones"], tonal)
            ref = d_frames.cpu().numpy().copy()
            d_frames.zero_()
            torch.cuda.synchronize()
            par.call(d_pcm["tones"], tonal)
            same = bool(np.array_equal(d_frames.cpu().numpy(), ref))
            p_runs, n_runs = [], []
            for r in range(a.runs):   # (which of the two goes first alternates as well)
                for who in ((par, new) if r % 2 == 0 else (new, par)):
                    (p_runs if who is par else n_runs).append(who.run(d_pcm["tones"], tonal, a.steps, a.warmup))
            res[key] = {"same_frames_as_parent": same, "parent_call_ms": [round(x, 4) for x in p_runs], "new_call_ms": [round(x, 4) for x in n_runs],
                        "new_median_within_parent_spread": bool(np.median(n_runs) <= max(p_runs))}
        par.enc.close()
    rows = {}
    for name in ("tones_twin", "dense"):
        for shared in (False, True):
            new.enc.reset()
            runs = [new.run(d_pcm[name], True, a.steps, a.warmup, shared) for _ in range(a.runs)]
            rows[name + ("_shared" if shared else "")] = {"call_ms": round(float(np.median(runs)), 4), "runs_ms": [round(x, 4) for x in runs],
                                                          "frames_per_s": round(S * F / (float(np.median(runs)) * 1e-3))}
        rows[name + "_shared"]["call_ratio_to_unflagged"] = round(rows[name + "_shared"]["call_ms"] / rows[name]["call_ms"], 4)
    res["shared"] = rows
    line = json.dumps({"metric": "at3p_share", "results": res})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
