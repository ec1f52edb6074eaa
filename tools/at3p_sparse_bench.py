#!/usr/bin/env python3
"""ATRAC3plus sparse word lengths (AT3PHIP_ALLOC_SPARSE, AT3PHIP_DECODE_SPARSE) beside the unflagged calls, and the unflagged calls
against the parent commit's library. The setup of tools/at3p_rate_bench.py, whose pieces this tool uses: 64 x 128 stereo frames
resident in HBM, each call timed on the host around the waiting call, the median of --steps calls per run, --runs runs.

  Unflagged, against --parent-lib (a libat3hip.so built from the parent commit), the two libraries alternating, which goes first
      alternating as well: at3phip_encode_frames with AT3PHIP_ALLOC_ADAPTIVE on `mix` and `noise`, and at3phip_decode (float, tones on)
      on 2048 frames of `mix`, at 376 and 2048 bytes. Passing: this library's median of medians is not above the parent's slowest run.
  Sparse, this library alone, reported beside them: the same encode call with AT3PHIP_ALLOC_SPARSE, and at3phip_decode with
      AT3PHIP_DECODE_SPARSE on the sparse encoder's frames (and on the unflagged frames, which it decodes alike).
No counters are collected and nothing is traced. Writes one JSON line (--out: also to that file; --append: added to it, so that
the file holds one line per session, which is how profiles/at3p_sparse_bench.json was made)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from atracdenc_amd import binding as B  # noqa: E402
import at3p_gha_lib as G  # noqa: E402
from at3p_rate_bench import C, DEC_F, F, S, alternate, staggered, timed  # noqa: E402

SIGNALS, SIZES = ("mix", "noise"), (376, 2048)


class Encoder:
    def __init__(self, lib_path, fb):
        self.enc = B.At3pHip(n_streams=S, max_frames=F, channels=C, lib_path=lib_path, frame_bytes=None if fb == 2048 else fb)
        self.out = torch.zeros((S, F, fb), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def run(self, d_pcm, steps, warmup, sparse=False):
        kw = {"sparse": True} if sparse else {}   # (the parent's binding call has no such argument to give)
        return timed(lambda: self.enc.encode_frames_device(d_pcm.data_ptr(), F, self.out.data_ptr(), adaptive=True, **kw), steps, warmup)[0]


class Decoder:
    def __init__(self, lib_path, fb):
        self.dec = B.At3pHipDecoder(n_streams=1, channels=C, max_frames=DEC_F, lib_path=lib_path, frame_bytes=None if fb == 2048 else fb)
        self.pcm = torch.zeros((1, DEC_F, 2048, C), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

    def run(self, d_frames, steps, warmup, sparse=False):
        kw = {"sparse": True} if sparse else {}
        return timed(lambda: self.dec.decode_device(d_frames, self.pcm, ordered=False, tones=True, **kw), steps, warmup)[0]


def long_stream_frames(fb, sparse=False):
    """[1][DEC_F][fb] on the device: `mix` encoded by this library at that size, 128 frames per call"""
    x = np.ascontiguousarray(G.signal_pcm("mix", DEC_F, C)[None])
    enc = B.At3pHip(n_streams=1, max_frames=128, channels=C, frame_bytes=None if fb == 2048 else fb)
    out = np.concatenate([enc.encode_frames(x[:, f:f + 128], adaptive=True, sparse=sparse) for f in range(0, DEC_F, 128)], axis=1)
    enc.close()
    d = torch.from_numpy(out).cuda()
    torch.cuda.synchronize()
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--lib", default=None, help="the library measured against the parent's (default: this tree's)")
    ap.add_argument("--unflagged-only", action="store_true", help="no sparse calls: for --lib without them, e.g. a copy of the parent's "
                    "library, which shows what the pass rule gives for two builds of the same code")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add the line to --out instead of replacing the file: one line per session")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: nothing is measured without one")
    d_pcm = {name: torch.from_numpy(staggered(G.signal_pcm(name, F + 2, C))).cuda() for name in SIGNALS}
    torch.cuda.synchronize()
    res = {"setup": f"{S} x {F} stereo frames in HBM, median of {a.steps} waiting calls, {a.runs} runs; decoder: 1 x {DEC_F} frames of mix",
           "device": torch.cuda.get_device_name(0), "lib": a.lib or "this tree's", "encode": {}, "decode": {}}
    for fb in SIZES:
        par, new = Encoder(a.parent_lib, fb), Encoder(a.lib, fb)
        for name in SIGNALS:
            cell = alternate(par, new, lambda who: who.run(d_pcm[name], a.steps, a.warmup), a.runs)
            if not a.unflagged_only:
                cell["sparse_ms"] = [round(new.run(d_pcm[name], a.steps, a.warmup, sparse=True), 4) for _ in range(a.runs)]
            res["encode"][f"{name}_{fb}"] = cell
        par.enc.close()
        new.enc.close()
        plain = long_stream_frames(fb)
        par, new = Decoder(a.parent_lib, fb), Decoder(a.lib, fb)
        cell = alternate(par, new, lambda who: who.run(plain, a.steps, a.warmup), a.runs)
        if not a.unflagged_only:
            sparse = long_stream_frames(fb, True)
            cell["sparse_flag_on_unflagged_frames_ms"] = [round(new.run(plain, a.steps, a.warmup, sparse=True), 4) for _ in range(a.runs)]
            cell["sparse_flag_on_sparse_frames_ms"] = [round(new.run(sparse, a.steps, a.warmup, sparse=True), 4) for _ in range(a.runs)]
        cell["rejected_after_all_runs"] = int(sum(new.dec.counters().values()))
        res["decode"][f"mix_{fb}"] = cell
        par.dec.close()
        new.dec.close()
    res["pass"] = all(c["new_median_within_parent_spread"] for k in ("encode", "decode") for c in res[k].values())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
