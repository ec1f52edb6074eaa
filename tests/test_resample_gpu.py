"""The batched sample-rate converter on the GPU (include/at3hip_resample.h): bit-identical to the C restatement
tests/host/resample_cpu.c for every supported pair, split and flush, device tensors and streams, the filter's effect on tones,
bad arguments, buffers past 4 GiB and on-device chaining into the ATRAC3 encoder."""
import numpy as np
import pytest

import atracdenc_amd
from atracdenc_amd import At3Hip, At3HipError, HipResampler
from atracdenc_amd.binding import AT3HIP_ASYNC, AT3HIP_OUT_ON_DEVICE, AT3HIP_PCM_ON_DEVICE, ResamplerConfig
from resample_lib import PAIRS, CpuResampler, bits_equal, n_outputs, run_split, shape, signal

pytestmark = pytest.mark.gpu

GB = 1 << 30


def restated(pair, x, channels):
    """the whole converted stream of x [n][channels]"""
    return CpuResampler(*pair, channels).whole(x)


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
@pytest.mark.parametrize("channels", [1, 2])
def test_bit_identical_to_restatement(pair, channels):
    kinds = ("noise", "sweep", "silence", "subnormal")
    T = 6000
    xs = np.stack([signal(k, T, channels, seed=i, rate=pair[0]) for i, k in enumerate(kinds)])
    exp = [restated(pair, xs[i], channels) for i in range(len(kinds))]
    rng = np.random.RandomState(pair[0] + 3 * pair[1] + channels)
    r = HipResampler(*pair, channels=channels, n_streams=len(kinds), max_in=T)
    try:
        for trial in range(2):
            cuts = [T] if trial == 0 else sorted(set(rng.randint(0, T, 5).tolist())) + [T]
            got = run_split(r, xs, cuts)
            for i, k in enumerate(kinds):
                assert bits_equal(got[i], exp[i]), (pair, channels, k, trial)
        # reset mid-stream starts over
        r.process(xs[:, :1234])
        r.reset()
        got = run_split(r, xs, [T])
        assert all(bits_equal(got[i], exp[i]) for i in range(len(kinds)))
    finally:
        r.close()


def test_max_out_and_empty_calls():
    r = HipResampler(44100, 192000, channels=2, n_streams=3, max_in=100)
    try:
        L, M, K = shape(44100, 192000)
        assert r.max_out == max(-(-100 * L // M), -(-(K // 2) * L // M))
        x = signal("noise", 100, 2, 5)
        xs = np.stack([x, x * 0.5, -x])
        assert r.process(xs[:, :0]).shape == (3, 0, 2)
        got = run_split(r, xs, [1, 1, 2, 50, 100])
        for i, s in enumerate((1.0, 0.5, -1.0)):
            assert bits_equal(got[i], restated((44100, 192000), np.float32(s) * x, 2))
        assert r.flush().shape == (3, 0, 2)   # a flush of an empty stream emits nothing
    finally:
        r.close()


@pytest.mark.parametrize("own_stream", [True, False])
def test_device_tensors_async(own_stream):
    import torch
    pair, C, S, T = (48000, 44100), 2, 5, 20000
    xs = np.stack([signal("noise", T, C, seed=40 + i) for i in range(S)])
    exp = [restated(pair, xs[i], C) for i in range(S)]
    r = HipResampler(*pair, channels=C, n_streams=S, max_in=8192)
    try:
        dev = torch.device("cuda:0")
        stream = torch.cuda.Stream(dev) if not own_stream else None
        outs, at = [], 0
        ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream(dev))
        with ctx:
            x_dev = torch.from_numpy(xs).to(dev)
            for cut in (3000, 11192, 19000, T):
                # the slice and the output stay alive (and, on the resampler's own stream, complete) until the queued call ran
                piece = x_dev[:, at:cut].contiguous()
                out = torch.full((S, r.max_out, C), float("nan"), device=dev)
                if own_stream:
                    torch.cuda.current_stream(dev).synchronize()
                    n = r.process_device(piece, out, asynchronous=True, ordered=False)
                else:
                    n = r.process_device(piece, out, asynchronous=True)
                outs.append((out, n, piece))
                at = cut
            out = torch.full((S, r.max_out, C), float("nan"), device=dev)
            if own_stream:
                torch.cuda.current_stream(dev).synchronize()
            n = r.flush_device(out, asynchronous=True, ordered=not own_stream)
            outs.append((out, n, None))
        r.sync()
        if stream is not None:
            stream.synchronize()
        got = np.concatenate([o.flatten()[: S * n * C].view(S, n, C).cpu().numpy() for o, n, _ in outs], axis=1)
        assert got.shape[1] == n_outputs(T, *pair)
        for i in range(S):
            assert bits_equal(got[i], exp[i]), i
    finally:
        r.close()


def test_sine_snr_and_stopband():
    pair = (48000, 44100)
    L, M, K = shape(*pair)
    t = np.arange(96000)
    x = np.stack([np.sin(2 * np.pi * 997 * t / 48000), 0.5 * np.sin(2 * np.pi * 23000 * t / 48000)], axis=-1).astype(np.float32)
    r = HipResampler(*pair, channels=2, n_streams=1, max_in=t.size)
    try:
        y = np.concatenate([r.process(x[None]), r.flush()], axis=1)[0]
    finally:
        r.close()
    edge = K * L // M
    n = np.arange(y.shape[0])
    ref = np.sin(2 * np.pi * 997 * n / 44100)
    err = (y[:, 0] - ref)[edge:-edge]
    snr = 10 * np.log10(np.sum(ref[edge:-edge] ** 2) / np.sum(err ** 2))
    assert snr >= 90, snr
    # 23 kHz lies above 44.1 kHz's Nyquist: what is left of it (aliased or not) is at least 95 dB below its input level
    rms_in = 0.5 / np.sqrt(2)
    rms_out = np.sqrt(np.mean(y[edge:-edge, 1].astype(np.float64) ** 2))
    assert 20 * np.log10(rms_out / rms_in) <= -95, 20 * np.log10(rms_out / rms_in)


def test_bad_arguments():
    lib = atracdenc_amd.load_library()
    for pair in ((44100, 44100), (48000, 32000), (44000, 44100), (44100, 12345)):
        with pytest.raises(At3HipError):
            HipResampler(*pair)
    for channels in (0, 3, -1):
        with pytest.raises(At3HipError):
            HipResampler(48000, 44100, channels=channels)
    for bad in (dict(n_streams=0), dict(max_in=0), dict(n_streams=65536), dict(device_id=-1)):
        with pytest.raises(At3HipError):
            HipResampler(48000, 44100, **bad)
    r = HipResampler(48000, 44100, channels=2, n_streams=2, max_in=64)
    try:
        x = np.zeros((2, 65, 2), np.float32)
        out = np.zeros((2, r.max_out, 2), np.float32)
        with pytest.raises(At3HipError):
            r.process_ptr(x.ctypes.data, 65, out.ctypes.data, 0)            # n_in > max_in
        with pytest.raises(At3HipError):
            r.process_ptr(x.ctypes.data, -1, out.ctypes.data, 0)
        with pytest.raises(At3HipError):
            r.process_ptr(x.ctypes.data, 8, out.ctypes.data, 64)            # unknown flag
        with pytest.raises(At3HipError):
            r.process_ptr(x.ctypes.data, 8, 0, 0)                           # no output
        assert lib.at3hip_resampler_create(None, None) != 0
        cfg = ResamplerConfig(48000, 44100, 3, 1, 16, 0)
        import ctypes
        h = ctypes.c_void_p()
        assert lib.at3hip_resampler_create(ctypes.byref(cfg), ctypes.byref(h)) == -1 and not h.value
        # a refused call changes nothing: the stream still converts as one call does
        xs = np.stack([signal("noise", 64, 2, 7), signal("sweep", 64, 2, 8)])
        got = run_split(r, xs, [64])
        for i in range(2):
            assert bits_equal(got[i], restated((48000, 44100), xs[i], 2))
    finally:
        r.close()


def test_past_4gib():
    """Input and output of 5.3 / 4.9 GiB (device tensors): the last stream, whose input and output start beyond 2^32 bytes, equals
    the restatement; every stream equals its replica among the first P."""
    import torch
    P, C, n_in = 7, 2, 1 << 20
    pair = (48000, 44100)
    S = 677
    free, _ = torch.cuda.mem_get_info()
    # the input, the two output tensors (each about 0.92 x the input) and 1 GiB to spare; the resampler itself holds only its
    # table and history here (its staging for host memory is allocated by the first host-memory call, and there is none)
    need = 3 * S * n_in * C * 4 + (1 << 30)
    if free < need:
        pytest.skip(f"needs {need / GB:.1f} GiB of free device memory, {free / GB:.1f} GiB free")
    assert (S - 1) * n_in * C * 4 > 4 * GB
    dev = torch.device("cuda:0")
    base = np.stack([signal("noise" if i % 2 == 0 else "sweep", n_in, C, seed=90 + i) for i in range(P)])
    x = torch.from_numpy(base).to(dev)[torch.arange(S, device=dev) % P].contiguous()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    r = HipResampler(*pair, channels=C, n_streams=S, max_in=n_in)
    try:
        out = torch.full((S, r.max_out, C), float("nan"), device=dev)
        n = r.process_device(x, out)
        tail = torch.full((S, r.max_out, C), float("nan"), device=dev)
        m = r.flush_device(tail)
        torch.cuda.synchronize()
        # device-only calls allocate no staging (it would be 10 GiB here): besides the two output tensors the context holds
        # its table and history
        held = before - torch.cuda.mem_get_info()[0] - 2 * out.numel() * 4
        assert held < 2 * GB, held / GB
        assert n + m == n_outputs(n_in, *pair)
        assert (S - 1) * n * C * 4 > 4 * GB
        head = out.flatten()[: S * n * C].view(S, n, C)
        rest = tail.flatten()[: S * m * C].view(S, m, C)
        del x
        last = S - 1
        exp = restated(pair, base[last % P], C)
        assert bits_equal(torch.cat([head[last], rest[last]]).cpu().numpy(), exp)
        for s0 in range(P):
            ref_h, ref_t = head[s0].view(torch.int32), rest[s0].view(torch.int32)
            for s in range(s0 + P, S, P):
                assert torch.equal(head[s].view(torch.int32), ref_h), s
                assert torch.equal(rest[s].view(torch.int32), ref_t), s
    finally:
        r.close()


def test_on_device_chain_into_the_encoder():
    """48 kHz PCM resampled into a torch tensor and encoded from there by the ATRAC3 encoder (AT3HIP_PCM_ON_DEVICE): the frames
    equal those of encoding the restatement's output."""
    import torch
    pair, C, T = (48000, 44100), 2, 48000
    x = signal("sweep", T, C, seed=3)
    x = np.ascontiguousarray(0.6 * x + 0.2 * signal("noise", T, C, seed=4), np.float32)
    exp_pcm = restated(pair, x, C)
    nb = exp_pcm.shape[0] // 1024
    dev = torch.device("cuda:0")
    r = HipResampler(*pair, channels=C, n_streams=1, max_in=T)
    enc = At3Hip(n_streams=1, max_blocks=nb)
    try:
        buf = torch.zeros(2 * r.max_out * C + 2048 * C, device=dev)
        n = r.process_device(torch.from_numpy(x[None]).to(dev), buf)
        m = r.flush_device(buf[n * C:])
        assert n + m == exp_pcm.shape[0]
        frames = torch.zeros((1, nb, enc.frame_size), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        nf = enc.encode_device(buf.data_ptr(), nb, frames.data_ptr())
        got = frames[:, :nf].cpu().numpy()
        enc.reset()
        exp = enc.encode(exp_pcm[: nb * 1024].reshape(1, nb, 1024, C))
        assert got.shape == exp.shape and np.array_equal(got, exp)
    finally:
        enc.close()
        r.close()
