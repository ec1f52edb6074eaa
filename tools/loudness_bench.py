"""Loudness meter benchmark: 64 stereo streams x 65 536 samples at 44.1 kHz, device-resident: one at3hip_loudness_process call
(reset before it) without and with true peak, and one at3hip_loudness_apply call, each the median of 20 calls between events on
a torch stream the meter is ordered on; and, in the same process, an ATRAC3 encode step (LP2) of 64 streams x 64 blocks (4096
frames, the encoder's own device timing, median of 20), so that the meter's share of an encode is measured, not assumed. Prints
one JSON line. The kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (k_hops,
k_carry, k_true_peak, k_scale)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from resample_bench import median_ms   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from atracdenc_amd import At3Hip, HipLoudness
    dev = torch.device("cuda:0")
    S, N, C = args.streams, args.samples, 2
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand((S, N, C), device=dev, generator=g) * 2 - 1
    out = torch.empty_like(x)
    gains = np.full(S, 0.5, np.float32)
    side = torch.cuda.Stream(dev)   # a stream of torch's own, not the default (null) stream: the calls are queued on it, between the events
    result = {"metric": "loudness_meter_stereo_44k1", "streams": S, "samples": N, "hops_per_stream": N // 4410}
    for name, true_peak in (("meter_ms", False), ("meter_true_peak_ms", True)):
        m = HipLoudness(channels=C, n_streams=S, max_in=N, max_hops=N // 4410, true_peak=true_peak)

        def meter():
            m.reset()
            m.process_device(x, asynchronous=True)

        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            result[name] = round(median_ms(meter, args.steps, args.warmup), 4)
            if not true_peak:
                result["apply_ms"] = round(median_ms(lambda: m.apply_device(x, gains, out, asynchronous=True), args.steps, args.warmup), 4)
        r = m.finish()[0]
        result["integrated_lufs_stream0"] = round(r.integrated, 3)
        m.close()
    # the encode step's device time as the encoder reports it (at3hip_get_timings: first stage start to last stage end), the
    # figure bench.py's steps add up to; the call itself waits for its work
    blocks = 64
    enc = At3Hip(n_streams=S, max_blocks=blocks)
    pcm = (torch.rand((S, blocks, 1024, C), device=dev, generator=g) - 0.5)
    frames = torch.zeros((S, blocks, enc.frame_size), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    enc_ms = []
    for i in range(args.warmup + args.steps):
        enc.encode_device(pcm.data_ptr(), blocks, frames.data_ptr())
        if i >= args.warmup:
            enc_ms.append(enc.timings()["total_ms"])
    encode_ms = sorted(enc_ms)[len(enc_ms) // 2]
    enc.close()
    result.update({"at3_encode_step_ms": round(encode_ms, 4), "encode_frames": S * blocks,
                   "ratio_to_encode_step": round(result["meter_ms"] / encode_ms, 4),
                   "true_peak_ratio_to_encode_step": round(result["meter_true_peak_ms"] / encode_ms, 4),
                   "true_peak_gflops": round(2.0 * S * N * C * 576 / (result["meter_true_peak_ms"] - result["meter_ms"]) / 1e6, 1)})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
