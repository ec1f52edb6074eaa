"""Sample-rate converter benchmark: stereo 48 -> 44.1 kHz, 64 streams x 65 536 input samples, device-resident, the median of 20
calls between events on a torch stream the converter is ordered on; and, in the same process, an ATRAC3 encode step (LP2) of 64
streams x 64 blocks (4096 frames, the encoder's own device timing, median of 20), so that the converter's share of an encode is
measured, not assumed. Prints one JSON line. The kernel's own time comes from a separate
`rocprofv3 --kernel-trace --stats` run of this script (k_resample)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.current_stream().synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from atracdenc_amd import At3Hip, HipResampler
    dev = torch.device("cuda:0")
    S, N, C = args.streams, args.samples, 2
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand((S, N, C), device=dev, generator=g) * 2 - 1
    r = HipResampler(48000, 44100, channels=C, n_streams=S, max_in=N)
    out = torch.empty((S, r.max_out, C), device=dev)
    n_out = [0]

    def convert():
        r.reset()
        n_out[0] = r.process_device(x, out, asynchronous=True)

    # a stream of torch's own, not the default (null) stream: process_device then queues k_resample on it, between the events
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        resample_ms = median_ms(convert, args.steps, args.warmup)
    r.sync()
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
    flops = 2.0 * S * n_out[0] * C * r.K
    print(json.dumps({"metric": "resample_48k_to_44k1_stereo", "streams": S, "input_samples": N, "outputs_per_stream": n_out[0],
                      "taps": r.K, "resample_ms": round(resample_ms, 4), "gflops": round(flops / resample_ms / 1e6, 1),
                      "at3_encode_step_ms": round(encode_ms, 4), "encode_frames": S * blocks,
                      "ratio_to_encode_step": round(resample_ms / encode_ms, 4)}))
    enc.close()
    r.close()


if __name__ == "__main__":
    main()
