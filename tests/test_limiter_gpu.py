"""The look-ahead limiter on the GPU (include/at3hip_loudness.h, "The look-ahead limiter"): samples and statistics bit-identical
to the C restatement tests/host/limiter_cpu.c on limiter_lib.batch() - 3 streams of two gain-kernel tiles plus 1237 samples, a
gain per stream (one stream never limited), peaks on both sides of the tile edge and within the look-ahead of the stream's start
and end - from float and 16-bit input, in one call and in cuts; device tensors and streams, the overlap rule, independence of
the meter, bad arguments; contexts whose max_in is smaller than the filter and the carries, and k_limit_gain's scalar path behind
device pointers that are only 4-byte (16-bit input: 2-byte) aligned."""
import ctypes

import numpy as np
import pytest

import atracdenc_amd
import limiter_lib as LM
import loudness_lib as L
from atracdenc_amd import At3HipError, HipLoudness
from atracdenc_amd.binding import AT3HIP_OUT_ON_DEVICE, AT3HIP_PCM_ON_DEVICE

pytestmark = pytest.mark.gpu

MODES = [(1, False), (1, True), (2, False), (2, True)]


def meter(channels, **kw):
    return HipLoudness(channels=channels, n_streams=3, max_in=LM.T_GPU, max_hops=2, **kw)


@pytest.mark.parametrize("channels,true_peak", MODES)
def test_bit_identical_to_restatement(channels, true_peak):
    """one call and 16-bit input in two calls; the batch is limited, and not everywhere"""
    xs, (want_y, want_st) = LM.batch(channels, true_peak), LM.expect(channels, true_peak)
    for i in (0, 2):
        assert 0.1 < want_st[i][1] / LM.T_GPU < 0.95, want_st[i]
    assert want_st[1] == (LM.FULL, 0)
    m = meter(channels)
    try:
        for cuts, s16 in (([LM.T_GPU], False), ([LM.T_GPU // 3, LM.T_GPU], True)):
            y, st = LM.run_engine(m, xs, LM.GAINS, LM.CEIL, true_peak, cuts, s16)
            assert LM.bad_streams(y, st, want_y, want_st) == [], (cuts, s16, st, want_st)
    finally:
        m.close()


@pytest.mark.parametrize("channels,true_peak", MODES)
def test_call_splits(channels, true_peak):
    """cuts with an empty call, calls of 1 and 71 samples and cuts on both sides of a tile edge give the same bits; a second
    run after the flush equals the first"""
    xs, (want_y, want_st) = LM.batch(channels, true_peak), LM.expect(channels, true_peak)
    rng = np.random.RandomState(11 + channels + 2 * true_peak)
    m = meter(channels)
    try:
        for trial in range(2):
            cuts = LM.cuts_for(rng, LM.T_GPU, true_peak)
            assert 0 in cuts and 1 in cuts and 72 in cuts
            y, st = LM.run_engine(m, xs, LM.GAINS, LM.CEIL, true_peak, cuts)
            assert LM.bad_streams(y, st, want_y, want_st) == [], (trial, cuts)
    finally:
        m.close()


@pytest.mark.parametrize("side_stream", [False, True])
def test_device_tensors(side_stream):
    """limit_device on torch's current stream (ordered=True) behind a producer kernel queued just before it, on the default
    stream and on a side stream; the flush likewise"""
    import torch
    C, tp = 2, True
    xs, (want_y, want_st) = LM.batch(C, tp), LM.expect(C, tp)
    dev = torch.device("cuda:0")
    m = meter(C)
    try:
        half = torch.from_numpy(xs * np.float32(0.5)).to(dev)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(dev) if side_stream else torch.cuda.current_stream(dev)
        m.limit_start(LM.GAINS, LM.CEIL, tp)
        with torch.cuda.stream(stream):
            big = torch.ones((2048, 2048), device=dev)
            for _ in range(4):
                big = big @ big * 1e-4            # keeps the stream busy in front of the producer
            x_dev = half * 2.0                    # the producer: exact, = xs
            out = torch.full_like(x_dev, float("nan"))
            n = m.limit_device(x_dev, out, asynchronous=True)
            tail = torch.full((3, LM.delay(tp), C), float("nan"), device=dev)
            k = m.limit_flush_device(tail, asynchronous=True)
        m.sync()
        assert n == LM.T_GPU - LM.delay(tp) and k == LM.delay(tp)
        y = np.concatenate([out.cpu().numpy().reshape(-1)[: 3 * n * C].reshape(3, n, C), tail.cpu().numpy()], axis=1)
        st = [(s.min_sum, s.n_limited) for s in m.limit_stats()]
        assert LM.bad_streams(y, st, want_y, want_st) == []
    finally:
        m.close()


@pytest.mark.parametrize("true_peak", [False, True], ids=["sample", "true_peak"])
@pytest.mark.parametrize("max_in,T", [(1, 330), (71, 3000), (293, 3000)])
def test_limiter_small_max_in(max_in, T, true_peak):
    """contexts whose max_in is below the filter's half length (72), below the carried samples (292) and just above them, fed in
    calls of max_in samples: the q rows, the output staging and the carries are sized by the larger of max_in and the carry"""
    C = 2
    xs, gains = LM.seven(T, C)
    want_y, want_st = LM.restate_all(xs, gains, LM.CEIL, true_peak)
    if max_in == 293:
        assert 0.1 < want_st[0][1] / T < 0.95, want_st[0]                      # limited, and not everywhere
    assert want_st[1] == (LM.FULL, 0)
    m = HipLoudness(channels=C, n_streams=xs.shape[0], max_in=max_in, max_hops=1)
    try:
        cuts = list(range(max_in, T, max_in)) + [T]
        assert max(b - a for a, b in zip([0] + cuts, cuts)) == max_in
        m.limit_start(gains, LM.CEIL, true_peak)
        with pytest.raises(At3HipError, match="max_in"):
            m.limit(xs[:, :max_in + 1])
        m.reset()
        y, st = LM.run_engine(m, xs, gains, LM.CEIL, true_peak, cuts)
        assert LM.bad_streams(y, st, want_y, want_st) == [], (st, want_st)
    finally:
        m.close()


def _device_window(values, offset, dtype):
    """a device tensor of values.size + 4 elements filled with a sentinel, `values` at `offset`: (whole tensor, the window)"""
    import torch
    n = values.size
    sent = 0x5A5A if dtype == torch.int16 else float("nan")
    whole = torch.full((n + 4,), sent, dtype=dtype, device="cuda")
    if n:
        whole[offset:offset + n] = torch.from_numpy(np.ascontiguousarray(values).reshape(-1)).cuda()
    return whole, whole[offset:offset + n]


def _untouched(whole, offset, n):
    import torch
    rest = torch.cat([whole[:offset], whole[offset + n:]])
    return bool(torch.isnan(rest).all()) if whole.dtype == torch.float32 else bool((rest == 0x5A5A).all())


@pytest.mark.parametrize("true_peak", [False, True], ids=["sample", "true_peak"])
@pytest.mark.parametrize("case", ["in", "out", "both", "s16"])
def test_limiter_unaligned_device_buffers(case, true_peak):
    """stereo float input and / or output one float past an 8-byte boundary (k_limit_gain's scalar loads and stores instead of
    the 8-byte ones), and mono 16-bit input at an odd 2-byte offset: device buffers of exactly the call's size, the elements
    around them untouched"""
    import torch
    s16 = case == "s16"
    C = 1 if s16 else 2
    xs, (want_y, want_st) = LM.batch(C, true_peak), LM.expect(C, true_peak)
    S, T, d = xs.shape[0], LM.T_GPU, LM.delay(true_peak)
    src = np.round(xs * 32768.0).astype(np.int16) if s16 else xs
    off_in = 1 if case in ("in", "both", "s16") else 2
    off_out = 1 if case in ("out", "both") else 2
    x_all, x_dev = _device_window(src, off_in, torch.int16 if s16 else torch.float32)
    y_all, y_dev = _device_window(np.full(S * (T - d) * C, np.nan, np.float32), off_out, torch.float32)
    t_all, t_dev = _device_window(np.full(S * d * C, np.nan, np.float32), off_out, torch.float32)
    assert x_dev.data_ptr() % (4 if s16 else 8) == (2 if s16 else 4 if off_in == 1 else 0)
    assert y_dev.data_ptr() % 8 == (4 if off_out == 1 else 0) and t_dev.data_ptr() % 8 == y_dev.data_ptr() % 8
    torch.cuda.synchronize()
    m = meter(C)
    try:
        m.limit_start(LM.GAINS, LM.CEIL, true_peak)
        n = m.limit_ptr(x_dev.data_ptr(), T, y_dev.data_ptr(), AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE, s16=s16)
        k = m.limit_flush_ptr(t_dev.data_ptr(), AT3HIP_OUT_ON_DEVICE)
        assert (n, k) == (T - d, d)
        st = [(s.min_sum, s.n_limited) for s in m.limit_stats()]
    finally:
        m.close()
    y = np.concatenate([y_dev.cpu().numpy().reshape(S, n, C), t_dev.cpu().numpy().reshape(S, k, C)], axis=1)
    assert LM.bad_streams(y, st, want_y, want_st) == []
    assert _untouched(x_all, off_in, src.size) and _untouched(y_all, off_out, S * n * C) and _untouched(t_all, off_out, S * k * C)
    assert np.array_equal(x_dev.cpu().numpy().reshape(src.shape), src)        # the input is only read


def test_overlapping_device_buffers_are_refused():
    """out cannot be in (the header says why): AT3HIP_EINVAL for device buffers of one call that overlap; the run goes on"""
    import torch
    C, tp = 2, False
    xs, (want_y, want_st) = LM.batch(C, tp), LM.expect(C, tp)
    m = meter(C)
    try:
        x_dev = torch.from_numpy(xs).cuda()
        out = torch.empty_like(x_dev)
        m.limit_start(LM.GAINS, LM.CEIL, tp)
        for dst in (x_dev, x_dev.view(-1)[LM.T_GPU:]):   # in place, and partly overlapping
            with pytest.raises(At3HipError, match="overlap"):
                m.limit_ptr(x_dev.data_ptr(), LM.T_GPU, dst.data_ptr(), AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE)
        n = m.limit_device(x_dev, out)
        y = np.concatenate([out.cpu().numpy().reshape(-1)[: 3 * n * C].reshape(3, n, C), m.limit_flush()], axis=1)
        assert LM.bad_streams(y, [(s.min_sum, s.n_limited) for s in m.limit_stats()], want_y, want_st) == []
    finally:
        m.close()


def test_meter_and_limiter_do_not_touch_each_other():
    """a meter run interleaved with a limiter run on one context: hop sums, results and limited samples of the two runs alone"""
    C, tp = 2, True
    xs, (want_y, want_st) = LM.batch(C, tp), LM.expect(C, tp)
    other = np.stack([L.signal(k, LM.T_GPU, C, seed=3 + i) for i, k in enumerate(("noise", "sweep", "tone_dc"))])
    m = meter(C, true_peak=True)
    try:
        m.limit_start(LM.GAINS, LM.CEIL, tp)
        pieces, at = [], 0
        for cut in (1000, L.HOP + 3, LM.T_GPU):
            m.process(other[:, at:cut])
            pieces.append(m.limit(xs[:, at:cut]))
            at = cut
        z = m.hops()
        res = m.finish()           # (a meter call: the limiter's run stays open)
        pieces.append(m.limit_flush())
        st = [(s.min_sum, s.n_limited) for s in m.limit_stats()]
        assert LM.bad_streams(np.concatenate(pieces, axis=1), st, want_y, want_st) == []
        for i in range(3):
            assert L.bits_equal(z[i], L.hops(other[i]))
            assert L.result_bits(res[i]) == L.result_bits(L.measure(other[i], True))
        # reset ends a limiter run
        m.limit_start(LM.GAINS, LM.CEIL, tp)
        m.limit(xs[:, :500])
        m.reset()
        with pytest.raises(At3HipError, match="limit_start"):
            m.limit(xs[:, :10])
        y, st = LM.run_engine(m, xs, LM.GAINS, LM.CEIL, tp, [LM.T_GPU])
        assert LM.bad_streams(y, st, want_y, want_st) == []
    finally:
        m.close()


def test_bad_arguments():
    """each is AT3HIP_EINVAL with a message and leaves the context usable"""
    lib = atracdenc_amd.load_library()
    C, tp = 1, False
    xs, (want_y, want_st) = LM.batch(C, tp), LM.expect(C, tp)
    m = meter(C)
    try:
        out = np.zeros((3, LM.T_GPU + 1, C), np.float32)
        n = ctypes.c_int32()
        st = (atracdenc_amd.binding.LimitStats * 3)()
        assert lib.at3hip_loudness_limit_stats(m.ctx, st) == -1                                    # no run yet
        assert lib.at3hip_loudness_limit(m.ctx, xs.ctypes.data, 8, out.ctypes.data, ctypes.byref(n), 0) == -1   # before limit_start
        assert b"limit_start" in lib.at3hip_loudness_last_error(m.ctx)
        for bad in (-1.0, float("nan"), float("inf")):
            g = np.array([1.0, bad, 1.0], np.float32)
            assert lib.at3hip_loudness_limit_start(m.ctx, g.ctypes.data, ctypes.c_float(0.5), 0) == -1
            assert b"gain" in lib.at3hip_loudness_last_error(m.ctx)
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            assert lib.at3hip_loudness_limit_start(m.ctx, LM.GAINS.ctypes.data, ctypes.c_float(bad), 0) == -1
            assert b"ceiling" in lib.at3hip_loudness_last_error(m.ctx)
        assert lib.at3hip_loudness_limit_start(m.ctx, LM.GAINS.ctypes.data, ctypes.c_float(0.5), 2) == -1   # an unknown flag
        assert lib.at3hip_loudness_limit_start(m.ctx, None, ctypes.c_float(0.5), 0) == -1
        m.limit_start(LM.GAINS, LM.CEIL, tp)
        assert lib.at3hip_loudness_limit_start(m.ctx, LM.GAINS.ctypes.data, ctypes.c_float(0.5), 0) == -1   # mid-run
        assert b"open" in lib.at3hip_loudness_last_error(m.ctx)
        big = np.zeros((3, LM.T_GPU + 1, C), np.float32)
        assert lib.at3hip_loudness_limit(m.ctx, big.ctypes.data, LM.T_GPU + 1, out.ctypes.data, ctypes.byref(n), 0) == -1
        assert b"max_in" in lib.at3hip_loudness_last_error(m.ctx)
        assert lib.at3hip_loudness_limit(m.ctx, xs.ctypes.data, -1, out.ctypes.data, ctypes.byref(n), 0) == -1
        assert lib.at3hip_loudness_limit(m.ctx, xs.ctypes.data, 8, out.ctypes.data, None, 0) == -1
        assert lib.at3hip_loudness_limit(m.ctx, xs.ctypes.data, 8, out.ctypes.data, ctypes.byref(n), 64) == -1
        assert lib.at3hip_loudness_limit_flush(m.ctx, out.ctypes.data, ctypes.byref(n), AT3HIP_PCM_ON_DEVICE) == -1
        assert m.limit_delay(False) == LM.A and m.limit_delay(True) == LM.A + 72
        # none of the refused calls changed the run
        y = np.concatenate([m.limit(xs), m.limit_flush()], axis=1)
        assert LM.bad_streams(y, [(s.min_sum, s.n_limited) for s in m.limit_stats()], want_y, want_st) == []
    finally:
        m.close()
