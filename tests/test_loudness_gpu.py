"""The batched loudness and true-peak meter on the GPU (include/at3hip_loudness.h): hop sums and every field of the results
bit-identical to the C restatement tests/host/loudness_cpu.c, the true peak against the restated 44100 -> 176400 converter,
device tensors and streams, apply, the on-device chain into the ATRAC3 encoder, bad arguments and an input past 4 GiB."""
import ctypes

import numpy as np
import pytest

import atracdenc_amd
import loudness_lib as L
from atracdenc_amd import At3Hip, At3HipError, HipLoudness, loudness_gain
from atracdenc_amd.binding import LoudnessConfig, LoudnessResult
from resample_lib import CpuResampler

pytestmark = pytest.mark.gpu

GB = 1 << 30
HOP = L.HOP


def assert_equal_to_restatement(z, results, xs, true_peak, what):
    for i in range(xs.shape[0]):
        assert L.bits_equal(z[i], L.hops(xs[i])), (what, i, "z")
        want = L.measure(xs[i], true_peak)
        assert L.result_bits(results[i]) == L.result_bits(want), (what, i, {n: getattr(results[i], n) for n in L.FIELDS[:3]})


@pytest.mark.parametrize("channels", [1, 2])
def test_bit_identical_to_restatement(channels):
    """noise, sweep, silence, subnormal, tone with DC side by side; one call, random cuts, reset() mid-stream; true peak on"""
    T = 40 * HOP + 1234
    xs = np.stack([L.signal(k, T, channels, seed=10 * channels + i) for i, k in enumerate(L.KINDS)])
    rng = np.random.RandomState(50 + channels)
    m = HipLoudness(channels=channels, n_streams=len(L.KINDS), max_in=T, max_hops=40, true_peak=True)
    try:
        z, res = L.run_split(m, xs, [T])
        assert_equal_to_restatement(z, res, xs, True, "one call")
        for trial in range(2):
            cuts = L.random_cuts(rng, T, 7)
            z, res = L.run_split(m, xs, cuts)   # (finish() has returned the meter to its start state)
            assert_equal_to_restatement(z, res, xs, True, cuts)
        m.process(xs[:, :3 * HOP + 99])
        m.reset()
        z, res = L.run_split(m, xs, [5, 2 * HOP, 2 * HOP + 1, T])
        assert_equal_to_restatement(z, res, xs, True, "after reset")
        # the results say something: full-scale white noise reads about 0 LUFS, the silence has no loudness
        assert -10 < res[0].integrated < 5 and res[2].integrated == -np.inf and res[0].n_hops == 40
    finally:
        m.close()
    m = HipLoudness(channels=channels, n_streams=len(L.KINDS), max_in=T, max_hops=40, true_peak=False)
    try:
        z, res = L.run_split(m, xs, [HOP, T])
        assert_equal_to_restatement(z, res, xs, False, "without true peak")
        assert all(r.true_peak[0] == 0.0 and r.true_peak[1] == 0.0 for r in res)
    finally:
        m.close()


@pytest.mark.parametrize("channels", [1, 2])
def test_true_peak_equals_the_restated_converter(channels):
    """the larger of the samples and of EVERY output of resample_lib.CpuResampler(44100, 176400), flush included"""
    T = 9000
    xs = np.stack([L.signal(k, T, channels, seed=3 + i) for i, k in enumerate(("noise", "sweep", "tone_dc"))])
    xs[0, -1] = 1.0   # the last sample's ringing lies in the outputs that only the flush emits
    m = HipLoudness(channels=channels, n_streams=3, max_in=T, max_hops=3, true_peak=True)
    try:
        for cuts in ([T], [10, 71, 72, 73, 150, 5000, T]):
            _, res = L.run_split(m, xs, cuts)
            for i in range(3):
                u = CpuResampler(44100, 176400, channels).whole(xs[i])
                assert u.shape[0] == 4 * T
                want = np.maximum(np.abs(u).max(axis=0), np.abs(xs[i]).max(axis=0))
                assert L.bits_equal(np.array(res[i].true_peak[:channels], np.float32), want.astype(np.float32)), (cuts, i)
                assert L.bits_equal(np.array(res[i].sample_peak[:channels], np.float32), np.abs(xs[i]).max(axis=0))
    finally:
        m.close()


@pytest.mark.parametrize("own_stream", [True, False])
def test_device_tensors_async(own_stream):
    """device tensors, AT3HIP_ASYNC, on the meter's own stream or (set_stream) on a torch stream"""
    import torch
    C, S, T = 2, 6, 12 * HOP + 321
    xs = np.stack([L.signal(L.KINDS[i % 5], T, C, seed=40 + i) for i in range(S)])
    m = HipLoudness(channels=C, n_streams=S, max_in=1 << 15, max_hops=12, true_peak=True)
    try:
        dev = torch.device("cuda:0")
        stream = torch.cuda.Stream(dev) if not own_stream else None
        keep, at = [], 0
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            x_dev = torch.from_numpy(xs).to(dev)
            for cut in (3000, 3000 + (1 << 15), 40000, T):
                piece = x_dev[:, at:cut].contiguous()   # stays alive (and, on the meter's own stream, complete) until the call ran
                if own_stream:
                    torch.cuda.current_stream(dev).synchronize()
                m.process_device(piece, asynchronous=True, ordered=not own_stream)
                keep.append(piece)
                at = cut
        z = m.hops()
        res = m.finish()
        assert_equal_to_restatement(z, res, xs, True, own_stream)
    finally:
        m.close()


def test_apply_equals_float32_multiply():
    import torch
    rng = np.random.RandomState(2)
    for C, S, n in ((2, 4, 50000), (1, 3, 12345), (2, 1, 7)):
        xs = np.stack([L.signal(L.KINDS[i % 5], n, C, seed=60 + i) for i in range(S)])
        g = rng.uniform(0.05, 4.0, S).astype(np.float32)
        want = xs * g[:, None, None]
        assert want.dtype == np.float32
        m = HipLoudness(channels=C, n_streams=S, max_in=n, max_hops=1)
        try:
            assert L.bits_equal(m.apply(xs, g), want)
            x_dev = torch.from_numpy(xs).cuda()
            out = torch.full_like(x_dev, float("nan"))
            m.apply_device(x_dev, g, out)
            assert L.bits_equal(out.cpu().numpy(), want)
            m.apply_device(x_dev, g, x_dev, asynchronous=True)   # in place, queued
            m.sync()
            assert L.bits_equal(x_dev.cpu().numpy(), want)
        finally:
            m.close()


def test_on_device_chain_into_the_encoder():
    """meter -> gain -> apply -> At3Hip.encode_device, all on device tensors: the frames equal those of encoding the host-scaled
    PCM, and the gain brought an over-full-scale input under the ceiling."""
    import torch
    C, nb = 2, 48
    T = nb * 1024
    x = np.ascontiguousarray(1.4 * L.signal("tone_dc", T, C, seed=5) + 0.5 * L.signal("noise", T, C, seed=6), np.float32)
    assert np.abs(x).max() > 1.0
    dev = torch.device("cuda:0")
    m = HipLoudness(channels=C, n_streams=1, max_in=T, max_hops=T // HOP, true_peak=True)
    enc = At3Hip(n_streams=1, max_blocks=nb)
    try:
        x_dev = torch.from_numpy(x[None]).to(dev)
        m.process_device(x_dev)
        r = m.finish()[0]
        assert L.results_equal(r, L.measure(x, True))
        g = loudness_gain(r, -16.0, -1.0)
        assert g == L.gain(L.measure(x, True), -16.0, -1.0) and g < 1.0
        scaled = torch.empty_like(x_dev)
        m.apply_device(x_dev, np.array([g], np.float32), scaled)
        frames = torch.zeros((1, nb, enc.frame_size), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        nf = enc.encode_device(scaled.data_ptr(), nb, frames.data_ptr())
        got = frames[:, :nf].cpu().numpy()
        enc.reset()
        host_scaled = x * g
        exp = enc.encode(host_scaled.reshape(1, nb, 1024, C))
        assert got.shape == exp.shape and np.array_equal(got, exp)
        assert float(np.max(r.true_peak)) * float(g) <= 10 ** (-1.0 / 20) * (1 + 1e-6)
    finally:
        enc.close()
        m.close()


def test_bad_arguments():
    lib = atracdenc_amd.load_library()
    for bad in (dict(channels=3), dict(channels=0), dict(n_streams=0), dict(n_streams=65536), dict(max_in=0), dict(max_hops=0),
                dict(device_id=-1)):
        with pytest.raises(At3HipError):
            HipLoudness(**bad)
    assert lib.at3hip_loudness_create(None, None) == -1
    cfg = LoudnessConfig(3, 1, 16, 4, 0, 0)
    h = ctypes.c_void_p()
    assert lib.at3hip_loudness_create(ctypes.byref(cfg), ctypes.byref(h)) == -1 and not h.value
    cfg = LoudnessConfig(2, 1, 16, 4, 2, 0)   # true_peak is 0 or 1
    assert lib.at3hip_loudness_create(ctypes.byref(cfg), ctypes.byref(h)) == -1 and not h.value
    m = HipLoudness(channels=2, n_streams=2, max_in=3 * HOP, max_hops=4, true_peak=True)
    try:
        xs = np.stack([L.signal("noise", 5 * HOP, 2, 7), L.signal("tone_dc", 5 * HOP, 2, 8)])
        buf = np.ascontiguousarray(xs[:, :3 * HOP + 1])
        for n_in, flags in ((3 * HOP + 1, 0), (-1, 0), (8, 64), (8, 2)):   # n_in > max_in, negative, unknown flag, OUT_ON_DEVICE
            assert lib.at3hip_loudness_process(m.ctx, buf.ctypes.data, n_in, flags) == -1
        assert lib.at3hip_loudness_process(m.ctx, None, 8, 0) == -1
        assert lib.at3hip_loudness_finish(m.ctx, None) == -1                     # a null result
        assert lib.at3hip_loudness_read_hops(m.ctx, 2, None, 0) == -1            # no such stream
        assert lib.at3hip_loudness_apply(m.ctx, buf.ctypes.data, 8, None, buf.ctypes.data, 0) == -1   # no gains
        assert b"bad argument" in lib.at3hip_loudness_last_error(m.ctx)
        # hops past max_hops: 4 fit, the call that would complete the fifth is refused and changes nothing
        m.process(xs[:, :3 * HOP])
        m.process(xs[:, 3 * HOP:4 * HOP + 100])
        piece = np.ascontiguousarray(xs[:, 4 * HOP + 100:])
        assert lib.at3hip_loudness_process(m.ctx, piece.ctypes.data, piece.shape[1], 0) == -1
        assert b"max_hops" in lib.at3hip_loudness_last_error(m.ctx)
        short = np.ascontiguousarray(xs[:, :4 * HOP + 100])
        z = m.hops()
        assert lib.at3hip_loudness_read_hops(m.ctx, 0, z[0].ctypes.data, z[0].nbytes - 8) == -1   # a wrong size
        res = m.finish()
        assert_equal_to_restatement(z, res, short, True, "after refused calls")
    finally:
        m.close()


def test_past_4gib():
    """An input of 4.7 GiB (one device tensor, one call): the last stream, whose samples start beyond 2^32 bytes, equals the
    restatement in z and in every field; every stream equals its replica among the first P."""
    import torch
    P, C, n_in, S = 7, 2, 1 << 20, 600
    free, _ = torch.cuda.mem_get_info()
    # the input, what builds it (the P base streams and the index) and 1 GiB to spare; the meter itself holds the carry, z and
    # peaks only (its staging for host memory is allocated by the first host-memory call, and there is none)
    need = S * n_in * C * 4 + (1 << 30)
    if free < need:
        pytest.skip(f"needs {need / GB:.1f} GiB of free device memory, {free / GB:.1f} GiB free")
    assert (S - 1) * n_in * C * 4 > 4 * GB
    dev = torch.device("cuda:0")
    base = np.stack([L.signal(L.KINDS[i % 5] if i % 5 != 2 else "noise", n_in, C, seed=90 + i) for i in range(P)])
    x = torch.from_numpy(base).to(dev)[torch.arange(S, device=dev) % P].contiguous()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    m = HipLoudness(channels=C, n_streams=S, max_in=n_in, max_hops=n_in // HOP, true_peak=True)
    try:
        m.process_device(x)
        held = before - torch.cuda.mem_get_info()[0]
        assert held < 1 * GB, held / GB   # device-only calls allocate no staging (it would be 4.7 GiB here)
        z = m.hops()
        res = m.finish()
        last = S - 1
        assert L.bits_equal(z[last], L.hops(base[last % P]))
        assert L.result_bits(res[last]) == L.result_bits(L.measure(base[last % P], True))
        for s in range(P, S):
            assert L.bits_equal(z[s], z[s % P]), s
            assert L.result_bits(res[s]) == L.result_bits(res[s % P]), s
    finally:
        m.close()
