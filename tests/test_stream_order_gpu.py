"""Stream ordering on the device, under schedules in which a missing wait has room to show: the counterpart of
tests/test_stream_order_simt_harness.py, which explores orders on the CPU and knows nothing of timing or hardware queues.

1. Unequal queued calls. The other queued-call tests issue equal, tiny calls whose stages last microseconds, so launch latency
   alone keeps consecutive calls apart. Here 64 streams (8 distinct signals, each 8 times) take calls of 64, 1, 1, 64, 1, 1, 1,
   64, 2, 1 blocks: a 64 x 64 call is the 4096-frame step, whose back half lasts many times the whole of a one-block call, so the
   small calls that follow it - reusing its parity's spectra, curves, scales and staging two calls later - are ready long before
   it is done. The replicas must equal each other and each distinct stream the oracle. DESIGN.md section 4 says, from one kernel
   trace of this module, which waits the schedule makes binding.

2. Slow producers. The input tensor first holds a different valid signal (the decoy); torch.cuda._sleep runs on the caller's
   stream, then the copy of the real input, then the ordered call, with no host synchronisation in between. A call that does
   not wait for the caller's stream reads the decoy and returns the decoy's (valid-looking) result.

   Measured on an MI355X (gfx950) at the parent commit, with events on the caller's stream: _sleep(20_000_000) lasts 8.3 ms
   (8.33 to 8.45 ms in eight runs, 9.97 ms in the process's first). The longest ordered call is the meter's process of
   2 x 4410 + 777 samples on three streams with the true-peak converter: 0.57 and 0.62 ms on the caller's stream in two runs (a context's
   first call, which makes its buffers); the others last 0.005 ms (apply) to 0.40 ms (the ATRAC3 encoder's 16-bit first stage), and
   the ATRAC3 encoder's whole call of 4 streams x 6 blocks lasts 0.24 ms from its launch to the end of sync(). 20 times
   0.62 ms is 12.4 ms, that is 30 million cycles; SLEEP_CYCLES is 60 million, a sleep of 25 ms, 40 times the longest call -
   the margin absorbs queueing on a shared device. Every test prints what it measures.

3. One control, on apply only: the same sequence with ordered=False breaks the contract on purpose (a read racing a copy on
   allocated, initialised memory, nothing more). With this module run alone it returned the decoy's result bit for bit - the
   evidence that the sequence can fail -, inside the whole suite it did not (see the test): it is a printed line."""
import numpy as np
import pytest

from at3_testlib import LP2, LP4, SIGNALS

pytestmark = pytest.mark.gpu

SLEEP_CYCLES = 60_000_000   # 25 ms on an MI355X: see the docstring

S, DISTINCT = 64, 8
BLOCKS = (64, 1, 1, 64, 1, 1, 1, 64, 2, 1)
PIPE_BLOCKS = (64, 1, 1, 64, 1)
_cache = {}


@pytest.fixture(scope="module")
def hip():
    import atracdenc_amd
    return atracdenc_amd


def at3_base(nb):
    """the 8 distinct signals of test_full_batch_config_properties, nb blocks each (computed once, never written)"""
    if ("base", nb) not in _cache:
        base = np.stack([SIGNALS["noise"](nb, seed=100 + i) for i in range(4)] + [SIGNALS["mix"](nb, seed=i) for i in range(4)])
        _cache["base", nb] = base
    return _cache["base", nb]


def at3_expect(oracle, nb, br, ng):
    if ("exp", nb, br, ng) not in _cache:
        base = at3_base(nb)
        exp = np.stack([oracle.encode(base[i], br, ng, 0)[0] for i in range(DISTINCT)])
        exp.setflags(write=False)
        _cache["exp", nb, br, ng] = exp
    return _cache["exp", nb, br, ng]


def assert_replicas_and_oracle(got, exp):
    assert got.shape == (S,) + exp.shape[1:], (got.shape, exp.shape)
    for i in range(DISTINCT, S):
        bad = np.argwhere((got[i] != got[i % DISTINCT]).any(axis=-1))
        assert bad.size == 0, f"stream {i} differs from its twin {i % DISTINCT} in frames {bad[:8].ravel().tolist()}"
    for i in range(DISTINCT):
        bad = np.argwhere((got[i] != exp[i]).any(axis=-1))
        assert bad.size == 0, f"stream {i} differs from the oracle in frames {bad[:8].ravel().tolist()}"


def packed(out, n_streams, count, frame_size):
    return out.reshape(-1)[: n_streams * count * frame_size].reshape(n_streams, count, frame_size)


# ---- 1. unequal queued calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("br,ng", [(LP2, 0), (LP2, 1), (LP4, 0)], ids=["lp2_gain", "lp2_nogain", "lp4_gain"])
def test_at3_unequal_queued_calls(hip, oracle, br, ng):
    import torch
    nb = sum(BLOCKS)
    base = at3_base(nb)
    exp = at3_expect(oracle, nb, br, ng)
    enc = hip.At3Hip(n_streams=S, max_blocks=max(BLOCKS), bitrate=br, no_gain=ng)
    dev = torch.from_numpy(base).cuda()
    ins, outs, counts, pos = [], [], [], 0
    for n in BLOCKS:
        ins.append(dev[:, pos:pos + n].repeat(S // DISTINCT, 1, 1, 1).contiguous())   # stream i holds signal i % 8
        outs.append(torch.full((S, n, enc.frame_size), 0xEE, dtype=torch.uint8, device="cuda"))
        pos += n
    torch.cuda.synchronize()
    for x, o, n in zip(ins, outs, BLOCKS):
        counts.append(enc.encode_device(x.data_ptr(), n, o.data_ptr(), asynchronous=True))
    enc.sync()
    got = np.concatenate([packed(o.cpu().numpy(), S, c, enc.frame_size) for o, c in zip(outs, counts)], axis=1)
    enc.close()
    assert counts == [BLOCKS[0] - 1] + list(BLOCKS[1:])
    assert_replicas_and_oracle(got, exp)


def test_at3_unequal_host_buffer_pipeline(hip, oracle):
    """the host-buffer pipeline at depth 3 with 64, 1, 1, 64, 1 blocks: page-locked buffers refilled (NaN) and read (then 0xEE)
    as soon as wait_input / wait_frames allow"""
    depth, nb = 3, sum(PIPE_BLOCKS)
    base = at3_base(nb)
    exp = at3_expect(oracle, nb, LP2, 0)
    piece = max(PIPE_BLOCKS)
    enc = hip.At3Hip(n_streams=S, max_blocks=piece, bitrate=LP2)
    ins = [enc.host_alloc((S, piece, 1024, 2), np.float32) for _ in range(depth)]
    outs = [enc.host_alloc((S, piece, enc.frame_size), np.uint8) for _ in range(depth)]
    got, counts, pos = [], [], 0

    def take(k):
        got.append(packed(outs[k % depth], S, counts[k], enc.frame_size).copy())
        outs[k % depth][...] = 0xEE

    for k, n in enumerate(PIPE_BLOCKS):
        q = k % depth
        if k >= depth:
            enc.wait_input(depth - 1)
        ins[q][...] = np.nan
        flat = ins[q].reshape(-1)[: S * n * 2048].reshape(S, n, 1024, 2)
        flat[...] = np.tile(base[:, pos:pos + n], (S // DISTINCT, 1, 1, 1))
        counts.append(enc.encode_host_async(flat, outs[q]))
        if k >= depth - 1:
            enc.wait_frames(depth - 1)
            take(k - (depth - 1))
        pos += n
    enc.sync()
    for k in range(len(PIPE_BLOCKS) - (depth - 1), len(PIPE_BLOCKS)):
        take(k)
    for a in ins + outs:
        enc.host_free(a)
    enc.close()
    assert_replicas_and_oracle(np.concatenate(got, axis=1), exp)


def test_at3p_unequal_queued_calls(hip):
    import torch
    from at3_testlib import at3p_signal, at3p_specs, at3p_write_frames
    nf, nch = sum(PIPE_BLOCKS), 2
    kinds = [(n, sc) for sc in (1.0, 0.5) for n in ("mix", "burst", "tones", "noise")]
    base = np.stack([np.stack([at3p_signal(n, nf, channel=c, scale=sc) for c in range(nch)], axis=-1) for n, sc in kinds])
    exp = np.stack([at3p_write_frames(at3p_specs(n, nf, nch, scale=sc)) for n, sc in kinds])
    enc = hip.At3pHip(n_streams=S, max_frames=max(PIPE_BLOCKS), channels=nch)
    dev = torch.from_numpy(base).cuda()
    ins, outs, pos = [], [], 0
    for n in PIPE_BLOCKS:
        ins.append(dev[:, pos:pos + n].repeat(S // DISTINCT, 1, 1, 1).contiguous())
        outs.append(torch.full((S, n, 2048), 0xEE, dtype=torch.uint8, device="cuda"))
        pos += n
    torch.cuda.synchronize()
    for x, o, n in zip(ins, outs, PIPE_BLOCKS):
        enc.encode_frames_device(x.data_ptr(), n, o.data_ptr(), asynchronous=True)
    enc.sync()
    got = np.concatenate([o.cpu().numpy() for o in outs], axis=1)
    enc.close()
    assert_replicas_and_oracle(got, exp)


# ---- 2. slow producers ----------------------------------------------------------------------------------------------------------
def slow_producer(real, decoy, call, what, ordered_stream=True):
    """decoy in the input tensor; on a side stream: sleep, copy of the real input, call(x) -> output tensor (or None), a clone of
    the output queued behind it; only then a wait. Returns (the clone on the host or None, x). Prints the measured durations."""
    import torch
    side = torch.cuda.Stream()
    src = torch.from_numpy(np.ascontiguousarray(real)).cuda()
    x = torch.from_numpy(np.ascontiguousarray(decoy)).cuda()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    with torch.cuda.stream(side):
        ev[0].record()
        torch.cuda._sleep(SLEEP_CYCLES)
        ev[1].record()
        x.copy_(src, non_blocking=True)
        ev[2].record()
        out = call(x)
        ev[3].record()
        res = out.clone() if out is not None else None
    side.synchronize()
    print(f"{what}: sleep of {SLEEP_CYCLES} cycles {ev[0].elapsed_time(ev[1]):.3f} ms, copy {ev[1].elapsed_time(ev[2]):.3f} ms, "
          f"what the call queued on this stream {ev[2].elapsed_time(ev[3]):.3f} ms")
    return (res.cpu().numpy() if res is not None else None), x


@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
def test_at3_encoder_caller_stream_slow_producer(hip, oracle, s16):
    """at3hip_set_stream orders the first stage behind the caller's stream; the frames are read after sync()"""
    import torch
    n_streams, nb = 4, 6
    pcm = np.stack([SIGNALS["mix"](nb, seed=41), SIGNALS["burst"](nb, phase=100), SIGNALS["noise"](nb, seed=42), SIGNALS["tones"](nb)])
    p16 = np.round(np.clip(pcm, -1.0, 32767.0 / 32768.0) * 32768.0).astype(np.int16)
    pcm = (p16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    real = p16 if s16 else pcm
    enc = hip.At3Hip(n_streams=n_streams, max_blocks=nb, bitrate=LP2)
    out = torch.full((n_streams, nb, enc.frame_size), 0xEE, dtype=torch.uint8, device="cuda")
    count = []

    def call(x):
        enc.set_stream(torch.cuda.current_stream().cuda_stream)
        count.append((enc.encode_device_s16 if s16 else enc.encode_device)(x.data_ptr(), nb, out.data_ptr(), asynchronous=True))

    slow_producer(real, real[::-1], call, f"at3 encoder set_stream s16={s16}")
    enc.sync()
    got = packed(out.cpu().numpy(), n_streams, count[0], enc.frame_size)
    enc.set_stream(None)
    # (measurement only: the same call again, from its launch to the end of sync())
    import time
    again, scratch = torch.from_numpy(np.ascontiguousarray(real)).cuda(), torch.empty_like(out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    (enc.encode_device_s16 if s16 else enc.encode_device)(again.data_ptr(), nb, scratch.data_ptr(), asynchronous=True)
    enc.sync()
    print(f"at3 encoder s16={s16}: a whole call of {n_streams} x {nb} blocks, launch to the end of sync() {(time.perf_counter() - t0) * 1e3:.3f} ms")
    enc.close()
    exp = np.stack([oracle.encode(pcm[i], LP2)[0] for i in range(n_streams)])
    assert np.array_equal(got, exp)


def test_at3p_decoder_slow_producer():
    import torch
    import at3p_tonal_lib as AT
    from atracdenc_amd.binding import At3pHipDecoder
    frames = AT.fuzz_tonal_streams(2, 4, 24, None)
    exp = np.stack([AT.cpu_tonal_decode(frames[i], 2)[0] for i in range(4)])
    dec = At3pHipDecoder(n_streams=4, channels=2, max_frames=24)
    out = torch.full(exp.shape, float("nan"), device="cuda")

    def call(x):
        dec.decode_device(x, out, asynchronous=True, tones=True)
        return out

    got, _ = slow_producer(frames, frames[::-1], call, "at3p decoder")
    dec.close()
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_resampler_slow_producer():
    import torch
    import resample_lib as RS
    from atracdenc_amd.binding import HipResampler
    pair, C, T = (48000, 44100), 2, 5000
    xs = np.stack([RS.signal(k, T, C, seed=i, rate=pair[0]) for i, k in enumerate(("noise", "sweep", "noise"))])
    exp = np.stack([RS.CpuResampler(*pair, C).process(xs[i]) for i in range(3)])
    r = HipResampler(*pair, channels=C, n_streams=3, max_in=T)
    out = torch.full((3, r.max_out, C), float("nan"), device="cuda")
    n = []

    def call(x):
        n.append(r.process_device(x, out, asynchronous=True))
        return out

    got, _ = slow_producer(xs, xs[::-1], call, "resampler")
    r.close()
    assert n == [exp.shape[1]]
    assert RS.bits_equal(packed(got, 3, n[0], C), exp)


def meter_inputs():
    import loudness_lib as L
    T = 2 * L.HOP + 777
    return np.stack([L.signal(k, T, 2, seed=60 + i) for i, k in enumerate(("noise", "tone_dc", "sweep"))])


def test_meter_process_slow_producer():
    import loudness_lib as L
    from atracdenc_amd.binding import HipLoudness
    xs = meter_inputs()
    m = HipLoudness(channels=2, n_streams=3, max_in=xs.shape[1], max_hops=2, true_peak=True)
    slow_producer(xs, xs[::-1], lambda x: m.process_device(x, asynchronous=True), "meter process")
    z, res = m.hops(), m.finish()   # (both wait for the queued call)
    m.close()
    for i in range(3):
        assert L.bits_equal(z[i], L.hops(xs[i])), i
        assert L.results_equal(res[i], L.measure(xs[i], True)), i


GAINS = np.array([0.37, 2.5, 1.25], np.float32)


def run_apply(ordered):
    import torch
    from atracdenc_amd.binding import HipLoudness
    xs = meter_inputs()
    m = HipLoudness(channels=2, n_streams=3, max_in=xs.shape[1], max_hops=1)
    out = torch.full(xs.shape, float("nan"), device="cuda")

    def call(x):
        m.apply_device(x, GAINS, out, asynchronous=True, ordered=ordered)
        if not ordered:
            m.sync()   # the call ran on the meter's own stream: its output is complete before the clone is queued
        return out

    got, _ = slow_producer(xs, xs[::-1], call, f"apply ordered={ordered}")
    m.close()
    return xs, got


def test_apply_slow_producer():
    import loudness_lib as L
    xs, got = run_apply(True)
    assert L.bits_equal(got, xs * GAINS[:, None, None])


def test_apply_unordered_control():
    """ordered=False breaks the contract on purpose: the call does not wait for the caller's stream. Run alone, the module
    returned the decoy's result bit for bit (two runs); in a run of the whole suite, whose process holds many more streams than the
    device has hardware queues, the meter's stream shared a queue with the sleeping one and the call saw the real input. The
    outcome is therefore printed, not asserted; asserted is that it is one of the two, bit for bit."""
    import loudness_lib as L
    xs, got = run_apply(False)
    decoy, real = L.bits_equal(got, xs[::-1] * GAINS[:, None, None]), L.bits_equal(got, xs * GAINS[:, None, None])
    print(f"apply ordered=False control: returned the {'decoy' if decoy else 'real input' if real else 'NEITHER'}'s result")
    assert decoy or real


def test_limiter_slow_producer():
    import torch
    import limiter_lib as LM
    from atracdenc_amd.binding import HipLoudness
    T = LM.TILE + 900
    xs, gains = LM.seven(T, 2)
    xs, gains = np.ascontiguousarray(xs[:3]), gains[:3]
    d = LM.delay(True)
    m = HipLoudness(channels=2, n_streams=3, max_in=T, max_hops=1)
    m.limit_start(gains, LM.CEIL, True)
    out = torch.full(xs.shape, float("nan"), device="cuda")
    n = []

    def call(x):
        n.append(m.limit_device(x, out, asynchronous=True))
        return out

    got, _ = slow_producer(xs, xs[::-1], call, "limiter")
    tail = m.limit_flush()
    st = [(s.min_sum, s.n_limited) for s in m.limit_stats()]
    m.close()
    assert n == [T - d]
    res = [LM.restate(xs[i], gains[i], LM.CEIL, True) for i in range(3)]
    y = np.concatenate([packed(got, 3, T - d, 2), tail], axis=1)
    assert LM.bad_streams(y, st, np.stack([r[0] for r in res]), [r[3] for r in res]) == []
