"""Limiter benchmark: 64 stereo streams x 10 s at 44.1 kHz, device-resident. One limiter run (at3hip_loudness_limit_start, one
at3hip_loudness_limit call over the whole buffer, at3hip_loudness_limit_flush) with the sample detector and with the true-peak
detector, against at3hip_loudness_apply and at3hip_loudness_process (true peak on, reset before it) on the same buffers in the
same session; each the median of 20 between events on a torch stream the context is ordered on. A measurement, not a gate:
writes profiles/limiter_bench.json and prints the same JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from resample_bench import median_ms   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "limiter_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from atracdenc_amd import HipLoudness
    dev = torch.device("cuda:0")
    S, N, C = args.streams, int(args.seconds * 44100), 2
    # bench.py's `burst` (a 3 kHz sine toggling 0.02 / 0.6 every 3000 samples, a phase per stream): at g = 4 limited about 0.9 of the time
    t = torch.arange(N, device=dev, dtype=torch.float64)[None, :] + 97.0 * torch.arange(S, device=dev, dtype=torch.float64)[:, None]
    left = torch.where((torch.floor(t / 3000.0) % 2) == 0, 0.02, 0.6) * torch.sin(2 * np.pi * 3000.0 * t / 44100.0)
    x = torch.stack([left, 0.5 * left], dim=-1).to(torch.float32).contiguous()
    del t, left
    out = torch.empty_like(x)
    tail = torch.empty((S, 292, C), device=dev)
    gains = np.full(S, 4.0, np.float32)
    ceiling = float(np.float32(10.0 ** (-1.0 / 20.0)))
    side = torch.cuda.Stream(dev)   # a stream of torch's own, not the null stream: the calls are queued on it, between the events
    m = HipLoudness(channels=C, n_streams=S, max_in=N, max_hops=N // 4410, true_peak=True)
    result = {"metric": "limiter_stereo_44k1", "streams": S, "samples": N, "steps": args.steps}

    def limiter(true_peak):
        def run():
            m.limit_start(gains, ceiling, true_peak)
            m.limit_device(x, out, asynchronous=True)
            m.limit_flush_device(tail, asynchronous=True)
        return run

    def meter():
        m.reset()
        m.process_device(x, asynchronous=True)

    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        result["limit_sample_ms"] = round(median_ms(limiter(False), args.steps, args.warmup), 4)
        st = m.limit_stats()[0]
        result["limited_share_stream0"] = round(st.n_limited / st.n_out, 4)
        result["limit_true_peak_ms"] = round(median_ms(limiter(True), args.steps, args.warmup), 4)
        result["apply_ms"] = round(median_ms(lambda: m.apply_device(x, gains, out, asynchronous=True), args.steps, args.warmup), 4)
        result["process_true_peak_ms"] = round(median_ms(meter, args.steps, args.warmup), 4)
    m.finish()
    m.close()
    gb = 2.0 * S * N * C * 4 / 1e9   # bytes read + written by apply, and the least a limiter call moves
    result.update({"gbytes_in_plus_out": round(gb, 4),
                   "apply_gbps": round(gb / result["apply_ms"] * 1e3, 1),
                   "limit_sample_gbps": round(gb / result["limit_sample_ms"] * 1e3, 1),
                   "limit_true_peak_over_process_plus_apply": round(result["limit_true_peak_ms"] / (result["process_true_peak_ms"] + result["apply_ms"]), 4),
                   "limit_sample_over_apply": round(result["limit_sample_ms"] / result["apply_ms"], 4),
                   "true_peak_detector_gflops": round(2.0 * S * N * C * 576 / max(1e-9, result["limit_true_peak_ms"] - result["limit_sample_ms"]) / 1e6, 1)})
    line = json.dumps(result)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
