#!/usr/bin/env python3
"""16-bit against float PCM input of the ATRAC1 encoder, the ATRAC3plus encoder, the resampler and the loudness meter, and the
float path of this build against the float path of a parent build. Writes profiles/s16_bench.json.

    python tools/s16_bench.py [--parent-lib PATH/libat3hip.so --parent-commit HASH] [--rounds 3] [--out profiles/s16_bench.json]

The parent library is the parent commit's sources compiled with the command of atracdenc_amd.build_library (the same flags, the
output elsewhere); its commit is recorded in the JSON.

For each engine one child process per round and library measures, with stereo streams:
  host-fed         K calls queued (AT3HIP_ASYNC) from one page-locked host buffer, outputs left in device memory, then one wait:
                   wall time per call, median of `--reps` such groups. The input crosses the bus in every call (a context has one
                   staging buffer and one stream, so a call's copy does not overlap the previous call's kernels).
  device-resident  the same K queued calls on a device buffer: wall time per call, median of `--reps` groups.
  h2d alone        a plain copy of the call's own input (the float buffer for a float call, the 16-bit buffer for a 16-bit call)
                   from the same page-locked buffer (hipMemcpyAsync through torch), as the bus's own figure: bus fraction = h2d
                   time of the call's input bytes / host-fed time of the call.
The rounds alternate between this build and the parent build (float calls only: the parent has no 16-bit entry points); the
spread of a figure is the range of its per-round medians. A child is a fresh process: the measuring process itself never opens
the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PCM_ON_DEVICE, OUT_ON_DEVICE, ASYNC = 1, 2, 4
K = 8   # queued calls per timed group


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def child(lib_path, kinds, reps):
    import numpy as np
    import torch
    from atracdenc_amd.binding import At1Hip, At3pHip, HipLoudness, HipResampler
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1)

    def timed(queue, sync):
        """median wall milliseconds per call of `reps` groups of K queued calls"""
        ms = []
        for i in range(reps + 2):
            sync()
            t0 = time.perf_counter()
            for _ in range(K):
                queue()
            sync()
            if i >= 2:
                ms.append((time.perf_counter() - t0) * 1e3 / K)
        return median(ms)

    def h2d_ms(host):
        """a plain copy of `host` (page-locked) to the device, median milliseconds"""
        dst = torch.empty(host.shape, dtype=host.dtype, device=dev)
        ms = []
        for i in range(reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                dst.copy_(host, non_blocking=True)
            torch.cuda.synchronize()
            if i >= 2:
                ms.append((time.perf_counter() - t0) * 1e3 / K)
        return median(ms)

    # engine: (context, samples per call incl. channels, units per call, unit name, {kind: queue(ptr, flags)})
    S = 64
    engines = {}
    a1 = At1Hip(n_streams=S, max_blocks=64, channels=2, lib_path=lib_path)
    a1_out = torch.zeros((S, 64, 2, 212), dtype=torch.uint8, device=dev)
    engines["at1_encode"] = (a1, S * 64 * 512 * 2, S * 64, "unit_pairs", {
        "float": lambda p, f: a1.encode_ptr(p, 64, a1_out.data_ptr(), f | OUT_ON_DEVICE | ASYNC),
        "s16": lambda p, f: a1.encode_s16_ptr(p, 64, a1_out.data_ptr(), f | OUT_ON_DEVICE | ASYNC)})
    ap = At3pHip(n_streams=S, max_frames=16, channels=2, lib_path=lib_path)
    ap_out = torch.zeros((S, 16, 2048), dtype=torch.uint8, device=dev)
    engines["at3p_encode_frames"] = (ap, S * 16 * 2048 * 2, S * 16, "frames", {
        "float": lambda p, f: ap.encode_frames_ptr(p, 16, ap_out.data_ptr(), f | OUT_ON_DEVICE | ASYNC),
        "s16": lambda p, f: ap.encode_frames_s16_ptr(p, 16, ap_out.data_ptr(), f | OUT_ON_DEVICE | ASYNC)})
    n_rs = 32768
    rs = HipResampler(48000, 44100, channels=2, n_streams=S, max_in=n_rs, lib_path=lib_path)
    rs_out = torch.zeros((S, rs.max_out, 2), dtype=torch.float32, device=dev)
    engines["resampler_48000_44100"] = (rs, S * n_rs * 2, S * n_rs, "input_samples", {
        "float": lambda p, f: rs.process_ptr(p, n_rs, rs_out.data_ptr(), f | OUT_ON_DEVICE | ASYNC),
        "s16": lambda p, f: rs.process_s16_ptr(p, n_rs, rs_out.data_ptr(), f | OUT_ON_DEVICE | ASYNC)})
    n_ld = 65536
    ld = HipLoudness(channels=2, n_streams=S, max_in=n_ld, max_hops=n_ld // 4410, true_peak=False, lib_path=lib_path)

    def meter(process_ptr):
        def queue(p, f):
            ld.reset()
            process_ptr(p, n_ld, f | ASYNC)
        return queue

    engines["loudness_process"] = (ld, S * n_ld * 2, S * n_ld, "samples", {"float": meter(ld.process_ptr), "s16": meter(ld.process_s16_ptr)})
    ld_out = torch.zeros((S, n_ld, 2), dtype=torch.float32, device=dev)
    gains = np.full(S, 0.7371, np.float32)
    engines["loudness_apply"] = (ld, S * n_ld * 2, S * n_ld, "samples", {
        "float": lambda p, f: ld.apply_ptr(p, n_ld, gains, ld_out.data_ptr(), f | OUT_ON_DEVICE | ASYNC),
        "s16": lambda p, f: ld.apply_s16_ptr(p, n_ld, gains, ld_out.data_ptr(), f | OUT_ON_DEVICE | ASYNC)})

    result = {}
    for name, (ctx, n, units, unit_name, queues) in engines.items():
        p16 = rng.randint(-20000, 20000, size=n).astype(np.int16)
        host = {"s16": torch.from_numpy(p16).pin_memory(), "float": torch.from_numpy(p16.astype(np.float32) / np.float32(32768)).pin_memory()}
        devb = {k: v.to(dev) for k, v in host.items()}
        torch.cuda.synchronize()
        r = {"samples_per_call": n, "units_per_call": units, "unit": unit_name}
        for kind in kinds:
            q = queues[kind]
            fed = timed(lambda: q(host[kind].data_ptr(), 0), ctx.sync)
            res = timed(lambda: q(devb[kind].data_ptr(), PCM_ON_DEVICE), ctx.sync)
            copy = h2d_ms(host[kind])
            r[kind] = {"host_fed_ms_per_call": round(fed, 4), "host_fed_units_per_s": round(units / fed * 1e3), "device_resident_ms_per_call": round(res, 4),
                       "h2d_alone_ms": round(copy, 4), "input_bytes": int(host[kind].numel() * host[kind].element_size()),
                       "h2d_alone_gb_per_s": round(host[kind].numel() * host[kind].element_size() / copy / 1e6, 2),
                       "bus_fraction": round(copy / fed, 3)}
        result[name] = r
    for c in (a1, ap, rs, ld):
        c.close()
    print("S16_BENCH " + json.dumps(result), flush=True)


def run_child(lib_path, kinds, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", lib_path, "--kinds", ",".join(kinds), "--reps", str(reps)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    for line in out.stdout.splitlines():
        if line.startswith("S16_BENCH "):
            return json.loads(line[len("S16_BENCH "):])
    raise SystemExit(f"child failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")


def summarise(rounds, kind):
    """per engine and figure: the median of the rounds' medians, and their range"""
    out = {}
    for name in rounds[0]:
        figs = {}
        for key in rounds[0][name][kind]:
            vals = [r[name][kind][key] for r in rounds]
            figs[key] = median(vals)
            if key.endswith("_ms_per_call"):
                figs[key.replace("_ms_per_call", "_ms_range")] = [min(vals), max(vals)]
        out[name] = figs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--kinds", default="float,s16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib")
    ap.add_argument("--parent-commit", default="", help="the commit the parent library was built from (recorded in the JSON)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s16_bench.json"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.kinds.split(","), args.reps)
    from atracdenc_amd import LIB_PATH
    mine, parent = [], []
    for i in range(args.rounds):
        mine.append(run_child(LIB_PATH, ["float", "s16"], args.reps))
        print(f"round {i}: this build done", flush=True)
        if args.parent_lib:
            parent.append(run_child(os.path.abspath(args.parent_lib), ["float"], args.reps))
            print(f"round {i}: parent build done", flush=True)
    result = {"what": "tools/s16_bench.py: 64 stereo streams per call, K = %d queued calls per group, median of %d groups per round, %d rounds "
                      "alternating between this build and the parent build; *_ms_range = [min, max] of the per-round medians" % (K, args.reps, args.rounds),
              "shape": {n: {k: mine[0][n][k] for k in ("samples_per_call", "units_per_call", "unit")} for n in mine[0]},
              "float": summarise(mine, "float"), "s16": summarise(mine, "s16")}
    if parent:
        result["parent_float"] = summarise(parent, "float")
        result["parent_build"] = {"commit": args.parent_commit,
                                  "how": "the commit's atracdenc_amd/csrc compiled with the command of atracdenc_amd.build_library "
                                         "(hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fvisibility=hidden "
                                         "-fPIC -shared, the same version script), loaded through this tree's binding"}
    cmp = {}
    for name in mine[0]:
        f, s = result["float"][name], result["s16"][name]
        c = {"host_fed_s16_over_float_speedup": round(f["host_fed_ms_per_call"] / s["host_fed_ms_per_call"], 3),
             "device_resident_s16_over_float_time": round(s["device_resident_ms_per_call"] / f["device_resident_ms_per_call"], 3)}
        if parent:
            p = result["parent_float"][name]
            for key in ("host_fed", "device_resident"):
                lo, hi = p[key + "_ms_range"]
                mlo, mhi = f[key + "_ms_range"]
                c[key + "_float_over_parent_float_time"] = round(f[key + "_ms_per_call"] / p[key + "_ms_per_call"], 3)
                c[key + "_float_ranges_overlap"] = bool(mlo <= hi and lo <= mhi)
        cmp[name] = c
    result["comparison"] = cmp
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(cmp, indent=1))


if __name__ == "__main__":
    main()
