"""Every batched GPU engine past 4 GiB buffers and at its create-time limits: the largest grids the contexts accept
(gridDim.y = 65535 / 65534 (stream, channel) rows), caller and internal buffers beyond 2^32 bytes, and the decoders' frame
caps exactly where they fall, accepted and refused.

One recipe throughout. P = 7 distinct streams (an odd period: a wrapped power-of-two offset can never land one stream's data
on an identical replica) are tiled on the device over all S streams (stream s is copy s % P). Every output is filled with a
sentinel before the call (0xA5 bytes, NaN floats, 0x5A5A samples), so a region that is never written cannot pass. The same P
streams go through a small context, and that small run is itself checked against the CPU oracle or the C restatement. Then
every replica of the large output is compared with its small-run counterpart on the device, every element (floats as bit
patterns), and the counters of the large run must be the replica-weighted sum of the per-stream counts."""
import os

import numpy as np
import pytest

from atracdenc_amd import At1Hip, At1HipDecoder, At3Hip, At3HipDecoder, At3HipError, At3pHip, At3pHipDecoder, HipLoudness
from atracdenc_amd.binding import AT3HIP_OUT_ON_DEVICE, AT3HIP_PCM_ON_DEVICE
from at3_testlib import (LP2, LP4, ROOT, SIGNALS, at1_blocks, at1_oracle_encode, at3p_mdct, at3p_pqf, at3p_signal, at3p_specs,
                         at3p_write_frames, oracle_diag_counts, pcm_hot, pcm_stress)

pytestmark = pytest.mark.gpu

P = 7
GB = 1 << 30
SENTINEL_U8 = 0xA5
SENTINEL_S16 = 0x5A5A


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def _need(gbytes):
    """skip (never fail) when the device cannot hold what the test allocates"""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < gbytes * GB:
        pytest.skip(f"needs {gbytes} GiB of free device memory, {free / GB:.1f} GiB free")


class _Mem:
    """Peak device memory of a test: torch's allocations (max_memory_allocated) and the whole device's use
    (mem_get_info, which sees the library's own buffers too), sampled after each large context's creation and call."""

    def __init__(self):
        import torch
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        self.base = torch.cuda.mem_get_info()[0]
        self.peak = 0

    def probe(self):
        import torch
        torch.cuda.synchronize()
        self.peak = max(self.peak, self.base - torch.cuda.mem_get_info()[0])

    def create(self, fn, *a, **kw):
        ctx = fn(*a, **kw)
        self.probe()
        return ctx


@pytest.fixture
def mem():
    import torch
    m = _Mem()
    yield m
    torch.cuda.synchronize()
    print(f"peak device memory: torch {torch.cuda.max_memory_allocated() / 1e9:.2f} GB allocated, "
          f"{m.peak / 1e9:.2f} GB in use on the device (mem_get_info)")
    torch.cuda.empty_cache()


def _tile(small, S):
    """[P, ...] device tensor -> [S, ...], stream s = copy s % P, built on the device"""
    import torch
    big = torch.empty((S,) + tuple(small.shape[1:]), dtype=small.dtype, device=small.device)
    for r in range(P):
        big[r::P] = small[r]
    return big


def _filled(shape, dtype):
    import torch
    if dtype == torch.uint8:
        return torch.full(shape, SENTINEL_U8, dtype=dtype, device="cuda")
    if dtype == torch.int16:
        return torch.full(shape, SENTINEL_S16, dtype=dtype, device="cuda")
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_replicas(big, small, what):
    """big[s] == small[s % P] for every s, element by element (floats as bit patterns), on the device in chunks"""
    b, s = _bits(big), _bits(small)
    assert b.shape[0] >= P and tuple(b.shape[1:]) == tuple(s.shape[1:]) and s.shape[0] == P, (tuple(big.shape), tuple(small.shape))
    per = max(1, s[0].numel())
    step = max(1, (1 << 28) // per)
    for r in range(P):
        rows = b[r::P]
        for a in range(0, rows.shape[0], step):
            bad = int((rows[a:a + step] != s[r]).sum())
            assert bad == 0, f"{what}: {bad} elements of streams {r + P * a} .. (step {P}) differ from the small run's stream {r}"


def _replicas(S):
    """how many of the S streams are copies of each of the P distinct ones"""
    return np.array([len(range(r, S, P)) for r in range(P)], np.int64)


def _s16(pcm):
    """the decoders' float -> 16-bit rule: (int16_t)__float2int_rn(x * 32767.0f)"""
    return np.rint(np.asarray(pcm, np.float32) * np.float32(32767.0)).astype(np.int32).astype(np.int16)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()   # (the library's streams do not wait for torch's: the fills and the tiling first)


# ---- ATRAC3 encoder -----------------------------------------------------------------------------------------------------------
def _at3_pcm(nb):
    """P distinct stereo streams [P, nb, 1024, 2]; the hot one (above full scale) makes the overflow counters count"""
    return np.stack([SIGNALS["noise"](nb, seed=7), SIGNALS["mix"](nb, seed=8), SIGNALS["burst"](nb), SIGNALS["tones"](nb),
                     SIGNALS["silence"](nb), pcm_hot(nb, seed=5), SIGNALS["noise"](nb, seed=11)]).astype(np.float32)


def _at3_oracle(oracle, pcm, br, ng):
    """(frames [P, nb - 1, fsz], per-stream (scale_overflow, clipped_values) [P, 2]) of the oracle"""
    frames, counts = [], []
    oracle_diag_counts(reset=True)
    for i in range(pcm.shape[0]):
        frames.append(oracle.encode(pcm[i], br, ng, 0)[0])
        counts.append(oracle_diag_counts(reset=True))
    return np.stack(frames), np.array(counts, np.int64)


def _at3_encode(enc, pcm_ptr, nb, out, s16=False, host=False):
    """one synchronous call into a sentinel-filled output; returns frames per stream"""
    raw = enc.encode_s16_ptr if s16 else enc.encode_ptr
    flags = 0 if host else AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE
    outp = out.ctypes.data if host else out.data_ptr()
    return raw(pcm_ptr, nb, outp, flags)


@pytest.mark.parametrize("mode", ["lp2_gain_tonal", "lp2_no_gain", "lp4_joint_stereo"])
def test_at3_encoder_past_4gib(oracle, mem, mode):
    """LP2 stereo S = 4096 x 129 blocks: the caller's PCM and each d_specs buffer 4.33e9 bytes. Default options (gain
    control + tonal extraction: k_qmf_sub8, k_gain_*, k_mdct_sub<false>), no gain control (the fused k_qmf_mdct8), LP4
    (joint stereo, k_mdct_sub<true>)."""
    import torch
    _need(40)
    br, ng = {"lp2_gain_tonal": (LP2, 0), "lp2_no_gain": (LP2, 1), "lp4_joint_stereo": (LP4, 0)}[mode]
    S, nb = 4096, 129
    pcm = _at3_pcm(nb)
    exp, per_stream = _at3_oracle(oracle, pcm, br, ng)
    assert per_stream.sum(0).min() > 0                                    # the counters have something to count
    small_in = _dev(pcm)
    enc7 = At3Hip(n_streams=P, max_blocks=nb, bitrate=br, no_gain=ng)
    fs = enc7.frame_size
    out7 = _filled((P * nb * fs,), torch.uint8)
    _sync()
    n = _at3_encode(enc7, small_in.data_ptr(), nb, out7)
    c7 = enc7.counters()
    enc7.close()
    assert n == nb - 1
    small = out7[:P * n * fs].view(P, n, fs)
    assert np.array_equal(small.cpu().numpy(), exp)
    assert bool((out7[P * n * fs:] == SENTINEL_U8).all())                # nothing past the packed frames
    assert [c7["scale_overflow"], c7["clipped_values"]] == per_stream.sum(0).tolist()

    big_in = _tile(small_in, S)
    del small_in
    assert big_in.numel() * 4 > 2 ** 32 and S * (nb + 2) * 2048 * 4 > 2 ** 32   # caller PCM and d_specs past 4 GiB
    enc = mem.create(At3Hip, n_streams=S, max_blocks=nb, bitrate=br, no_gain=ng)
    out = _filled((S * nb * fs,), torch.uint8)
    _sync()
    try:
        n = _at3_encode(enc, big_in.data_ptr(), nb, out)
        c = enc.counters()
        mem.probe()
    finally:
        enc.close()
    assert n == nb - 1
    _assert_replicas(out[:S * n * fs].view(S, n, fs), small, f"ATRAC3 {mode} frames")
    assert bool((out[S * n * fs:] == SENTINEL_U8).all())
    assert [c["scale_overflow"], c["clipped_values"]] == (_replicas(S) @ per_stream).tolist()
    del big_in, out, out7, small


def test_at3_encoder_s16_host_past_2gib(oracle, mem):
    """at3hip_encode_s16 from a host buffer of 2.16e9 bytes (LP2 stereo, S = 4096 x 129): the staged copy's byte count
    n_in * sizeof(int16_t), the 16-bit staging buffer and k_s16_to_f32 over 1.08e9 samples."""
    import torch
    _need(40)
    S, nb = 4096, 129
    pcm16 = np.round(np.clip(_at3_pcm(nb), -1.0, 32767.0 / 32768.0) * 32768.0).astype(np.int16)
    pcm16[6, 0, :4] = [[-32768, 32767], [32767, -32768], [0, -1], [1, 0]]
    f32 = (pcm16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    exp, per_stream = _at3_oracle(oracle, f32, LP2, 0)
    enc7 = At3Hip(n_streams=P, max_blocks=nb, bitrate=LP2)
    fs = enc7.frame_size
    out7 = np.full(P * nb * fs, SENTINEL_U8, np.uint8)
    n = _at3_encode(enc7, pcm16.ctypes.data, nb, out7, s16=True, host=True)
    c7 = enc7.counters()
    enc7.close()
    assert n == nb - 1
    small = out7[:P * n * fs].reshape(P, n, fs)
    assert np.array_equal(small, exp)
    assert (out7[P * n * fs:] == SENTINEL_U8).all()
    assert [c7["scale_overflow"], c7["clipped_values"]] == per_stream.sum(0).tolist()

    big = np.empty((S, nb, 1024, 2), np.int16)
    for r in range(P):
        big[r::P] = pcm16[r]
    assert big.nbytes > 2 ** 31                                           # the host buffer and its staged copy past 2 GiB
    enc = mem.create(At3Hip, n_streams=S, max_blocks=nb, bitrate=LP2)
    out = np.full(S * nb * fs, SENTINEL_U8, np.uint8)
    try:
        n = _at3_encode(enc, big.ctypes.data, nb, out, s16=True, host=True)
        c = enc.counters()
        mem.probe()
    finally:
        enc.close()
    del big
    assert n == nb - 1
    _assert_replicas(torch.from_numpy(out[:S * n * fs].reshape(S, n, fs)).cuda(), torch.from_numpy(small).cuda(), "ATRAC3 s16 frames")
    assert (out[S * n * fs:] == SENTINEL_U8).all()
    assert [c["scale_overflow"], c["clipped_values"]] == (_replicas(S) @ per_stream).tolist()


# ---- ATRAC1 encoder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,S", [(1, 65535), (2, 32767)], ids=["mono", "stereo"])
def test_at1_encoder_full_grid(mem, nch, S):
    """S * C = 65535 / 65534 (stream, channel) rows: gridDim.y at its limit; the caller's PCM and d_specs / d_values
    S * 33 * C * 512 floats, 4.43e9 bytes."""
    import torch
    _need(30)
    nb = 33
    sig = [SIGNALS["noise"](17, seed=7), SIGNALS["mix"](17, seed=8), SIGNALS["burst"](17), SIGNALS["tones"](17),
           SIGNALS["silence"](17), pcm_stress(17), SIGNALS["noise"](17, seed=11)]
    pcm = np.stack([at1_blocks(x, nch)[:nb] for x in sig])                # [P, 33, 512, C]
    exp = np.stack([at1_oracle_encode(p, "auto") for p in pcm])            # [P, 33, C, 212]
    small_in = _dev(pcm)
    enc7 = At1Hip(n_streams=P, max_blocks=nb, channels=nch)
    small = _filled((P, nb, nch, 212), torch.uint8)
    _sync()
    enc7.encode_device(small_in.data_ptr(), nb, small.data_ptr())
    enc7.close()
    assert np.array_equal(small.cpu().numpy(), exp)

    big_in = _tile(small_in, S)
    assert S * nch in (65535, 65534) and big_in.numel() * 4 > 2 ** 32
    enc = mem.create(At1Hip, n_streams=S, max_blocks=nb, channels=nch)
    out = _filled((S, nb, nch, 212), torch.uint8)
    _sync()
    try:
        enc.encode_device(big_in.data_ptr(), nb, out.data_ptr())
        mem.probe()
    finally:
        enc.close()
    _assert_replicas(out, small, f"ATRAC1 {nch}-channel sound units")
    del big_in, out, small_in, small


# ---- ATRAC3plus encoder -------------------------------------------------------------------------------------------------------
AT3P_SIGNALS = (("mix", 1.0), ("noise", 1.0), ("burst", 1.0), ("tones", 1.0), ("silence", 1.0), ("mix", 0.25), ("stress", 1.0))


def _at3p_pcm(nf, nch):
    return np.stack([np.stack([at3p_signal(n, nf, channel=c, scale=k) for c in range(nch)], axis=-1) for n, k in AT3P_SIGNALS])


def test_at3p_encode_frames_full_grid(mem):
    """encode_frames, mono S = 65535 x 9 frames: gridDim.y = 65535; the caller's PCM and the internal subbands / spectra
    S * 9 * 2048 floats, 4.83e9 bytes each."""
    import torch
    _need(32)
    S, nf, nch = 65535, 9, 1
    pcm = _at3p_pcm(nf, nch)                                                # [P, 9, 2048, 1]
    exp = np.stack([at3p_write_frames(at3p_specs(n, nf, nch, scale=k)) for n, k in AT3P_SIGNALS])
    small_in = _dev(pcm)
    enc7 = At3pHip(n_streams=P, max_frames=nf, channels=nch)
    small = _filled((P, nf, 2048), torch.uint8)
    _sync()
    enc7.encode_frames_device(small_in.data_ptr(), nf, small.data_ptr())
    enc7.close()
    assert np.array_equal(small.cpu().numpy(), exp)

    big_in = _tile(small_in, S)
    assert S * nch == 65535 and big_in.numel() * 4 > 2 ** 32
    enc = mem.create(At3pHip, n_streams=S, max_frames=nf, channels=nch)
    out = _filled((S, nf, 2048), torch.uint8)
    _sync()
    try:
        enc.encode_frames_device(big_in.data_ptr(), nf, out.data_ptr())
        mem.probe()
    finally:
        enc.close()
    _assert_replicas(out, small, "ATRAC3plus frames")
    del big_in, out, small_in, small


def test_at3p_pqf_mdct_past_4gib(mem):
    """pqf_mdct, stereo S = 16384 x 17 frames: the caller's PCM and spectra S * 17 * 2 * 2048 floats, 4.56e9 bytes."""
    import torch
    _need(32)
    S, nf, nch = 16384, 17, 2
    pcm = _at3p_pcm(nf, nch)                                                # [P, 17, 2048, 2]
    exp = np.zeros((P, nf, nch, 2048), np.float32)
    for s in range(P):
        for c in range(nch):
            exp[s, :, c] = at3p_mdct(at3p_pqf(np.ascontiguousarray(pcm[s, :, :, c])))
    small_in = _dev(pcm)
    enc7 = At3pHip(n_streams=P, max_frames=nf, channels=nch)
    small = _filled((P, nf, nch, 2048), torch.float32)
    _sync()
    enc7.pqf_mdct_device(small_in.data_ptr(), nf, small.data_ptr())
    enc7.close()
    assert np.array_equal(small.cpu().numpy().view(np.uint32), exp.view(np.uint32))

    big_in = _tile(small_in, S)
    assert big_in.numel() * 4 > 2 ** 32 and S * nf * nch * 2048 * 4 > 2 ** 32
    enc = mem.create(At3pHip, n_streams=S, max_frames=nf, channels=nch)
    out = _filled((S, nf, nch, 2048), torch.float32)
    _sync()
    try:
        enc.pqf_mdct_device(big_in.data_ptr(), nf, out.data_ptr())
        mem.probe()
    finally:
        enc.close()
    _assert_replicas(out, small, "ATRAC3plus spectra")
    del big_in, out, small_in, small


def test_at3p_tonal_encode_full_grid(mem):
    """encode_frames_tonal, mono S = 65535 x 9 frames: gridDim.y = 65535 in k_at3p_tone_find and k_at3p_tone_sub; the caller's PCM
    and the internal subbands, residuals and spectra S * 9 * 2048 floats, 4.83e9 bytes each."""
    import torch
    import at3p_gha_lib as G
    _need(48)
    S, nf, nch = 65535, 9, 1
    pcm = _at3p_pcm(nf, nch)                                                # [P, 9, 2048, 1]
    want = [G.pipeline(p) for p in pcm]
    exp = np.stack([w[0] for w in want])
    assert sum(any(G.n_waves(b) for b in w[1]) for w in want) >= 3           # the blocks carry waves
    small_in = _dev(pcm)
    enc7 = At3pHip(n_streams=P, max_frames=nf, channels=nch)
    small = _filled((P, nf, 2048), torch.uint8)
    _sync()
    enc7.encode_frames_tonal_device(small_in.data_ptr(), nf, small.data_ptr())
    enc7.close()
    assert np.array_equal(small.cpu().numpy(), exp)

    big_in = _tile(small_in, S)
    assert S * nch == 65535 and big_in.numel() * 4 > 2 ** 32
    enc = mem.create(At3pHip, n_streams=S, max_frames=nf, channels=nch)
    out = _filled((S, nf, 2048), torch.uint8)
    _sync()
    try:
        enc.encode_frames_tonal_device(big_in.data_ptr(), nf, out.data_ptr())
        mem.probe()
    finally:
        enc.close()
    _assert_replicas(out, small, "ATRAC3plus tonal frames")
    del big_in, out, small_in, small


def test_at3p_analyse_tones_past_4gib(mem):
    """analyse_tones with AT3PHIP_TONES_GATED | AT3PHIP_TONES_SHARED on device buffers, stereo S = 32767 x 9 frames: gridDim.y =
    65534; the caller's subbands and residuals S * 9 * 2 * 2048 floats, 4.83e9 bytes each; the records of all S * 9 slots in host
    memory."""
    import torch
    import at3p_gha_lib as G
    from atracdenc_amd.binding import AT3P_TONAL_BLOCK_DTYPE
    _need(48)
    S, nf, nch = 32767, 9, 2
    flags = AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE | G.GATED | G.SHARED
    pcm = [G.twin_pcm("tones", nf), G.keyed_pcm(nf, nch), G.twin_pcm("burst", nf), G.signal_pcm("mix", nf, nch), G.signal_pcm("noise", nf, nch),
           G.signal_pcm("burst", nf, nch), G.signal_pcm("tones", nf, nch, 0.25)]
    bands = np.stack([G.pqf_bands(p) for p in pcm])                          # [P, 9, 2, 16, 128]
    want = [G.CpuToneAnalyser(nch, True, True).analyse(b) for b in bands]
    exp_recs, exp_resid = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    assert sum(len(G.shared_bands(b)) for b in exp_recs.reshape(-1)) > 0     # sharing bits ...
    assert sum(len(G.points(b, nch)) for b in exp_recs.reshape(-1)) > 0      # ... and envelope points are there
    assert sum(G.n_waves(b) for b in exp_recs.reshape(-1)) > 0

    def run(enc, d_bands, n):
        recs = np.full((n, nf, AT3P_TONAL_BLOCK_DTYPE.itemsize), SENTINEL_U8, np.uint8)
        resid = _filled((n, nf, nch, 16, 128), torch.float32)
        _sync()
        enc.analyse_tones_ptr(d_bands.data_ptr(), nf, recs.ctypes.data, resid.data_ptr(), flags)
        return recs.reshape(n, -1), resid

    small_in = _dev(bands)
    enc7 = At3pHip(n_streams=P, max_frames=nf, channels=nch)
    recs7, resid7 = run(enc7, small_in, P)
    enc7.close()
    assert recs7.tobytes() == exp_recs.tobytes()
    assert np.array_equal(resid7.cpu().numpy().view(np.uint32), exp_resid.view(np.uint32))

    big_in = _tile(small_in, S)
    assert S * nch == 65534 and big_in.numel() * 4 > 2 ** 32
    enc = mem.create(At3pHip, n_streams=S, max_frames=nf, channels=nch)
    try:
        recs, resid = run(enc, big_in, S)
        mem.probe()
    finally:
        enc.close()
    assert resid.numel() * 4 > 2 ** 32
    for r in range(P):
        bad = np.nonzero((recs[r::P] != recs7[r]).any(axis=1))[0]
        assert bad.size == 0, f"records of streams {(r + P * bad[:4]).tolist()} differ from the small run's stream {r}"
    _assert_replicas(resid, resid7, "ATRAC3plus tone residuals")
    del big_in, resid, small_in, resid7


# ---- the limiter ----------------------------------------------------------------------------------------------------------------
def _limit_large(mem, S, nch, true_peak, T, max_in, calls):
    """The recipe for the limiter: limiter_lib.seven() through a context of P streams (checked against the restatement) and, tiled,
    through one of S streams, in calls ending at `calls` and the flush: every replica's samples, limit_stats of every stream
    and n_out. Returns (bytes of the large input, bytes of its outputs without the flush)."""
    import torch
    import limiter_lib as LM
    xs, gains = LM.seven(T, nch)
    want_y, want_st = LM.restate_all(xs, gains, LM.CEIL, true_peak)
    assert 0.1 < want_st[0][1] / T < 0.95, want_st[0]                       # stream 0 is limited, and not everywhere
    assert want_st[1] == (LM.FULL, 0)                                        # stream 1 never
    d = LM.delay(true_peak)
    assert max(b - a for a, b in zip((0,) + calls, calls)) <= max_in

    def run(n, d_in, create):
        m = create(HipLoudness, channels=nch, n_streams=n, max_in=max_in, max_hops=1)
        try:
            m.limit_start(np.resize(gains, n), LM.CEIL, true_peak)
            outs, at = [], 0
            for cut in calls:
                piece = d_in[:, at:cut].contiguous() if (at, cut) != (0, T) else d_in
                out = _filled((n * (cut - at) * nch,), torch.float32)
                k = m.limit_device(piece, out)
                assert k == max(0, cut - d) - max(0, at - d)
                assert bool(torch.isnan(out[n * k * nch:]).all())            # nothing past the outputs
                outs.append(out[:n * k * nch].view(n, k, nch))
                del piece
                at = cut
            tail = _filled((n, d, nch), torch.float32)
            assert m.limit_flush_device(tail) == d
            st = m.limit_stats()
            mem.probe()
        finally:
            m.close()
        return outs, tail, st

    small_in = _dev(xs)
    outs7, tail7, st7 = run(P, small_in, lambda f, **kw: f(**kw))
    y7 = np.concatenate([o.cpu().numpy() for o in outs7] + [tail7.cpu().numpy()], axis=1)
    assert LM.bad_streams(y7, [(s.min_sum, s.n_limited) for s in st7], want_y, want_st) == []
    assert all(s.n_out == T for s in st7)

    big_in = _tile(small_in, S)
    outs, tail, st = run(S, big_in, mem.create)
    for o, o7 in zip(outs, outs7):
        if o7.shape[1]:
            _assert_replicas(o, o7, "limited samples")
    _assert_replicas(tail, tail7, "the limiter's flush")
    got = np.array([(s.min_sum, s.n_limited, s.n_out) for s in st], np.int64)
    exp = np.array([want_st[r] + (T,) for r in range(P)], np.int64)[np.arange(S) % P]
    assert np.array_equal(got, exp), np.nonzero((got != exp).any(axis=1))[0][:8]
    return big_in.numel() * 4, [o.numel() * 4 for o in outs]


def test_limiter_past_4gib(mem):
    """stereo, true-peak detector, S = 4200 x 131072 samples in one call: the caller's input and output past 4 GiB even without
    their last stream ((S - 1) * n_in * 8 and (S - 1) * (n_in - 292) * 8 bytes); two q rows of 2645 + n_in words per stream."""
    _need(20)
    S, n_in = 4200, 131072
    assert (S - 1) * n_in * 8 > 2 ** 32 and (S - 1) * (n_in - 292) * 8 > 2 ** 32
    in_bytes, out_bytes = _limit_large(mem, S, 2, True, n_in, n_in, (n_in,))
    assert in_bytes == S * n_in * 8 and out_bytes == [S * (n_in - 292) * 8]


def test_limiter_full_grid(mem):
    """mono, sample detector, S = 65535 (gridDim.y at its limit in every kernel), max_in = 3000, 3000 samples in calls of 1500"""
    _need(4)
    S = 65535
    _limit_large(mem, S, 1, False, 3000, 3000, (1500, 3000))


# ---- decoders: shared driver --------------------------------------------------------------------------------------------------
def _decode_large(mem, make, S, inputs, exp_f32, per_stream, out_shape, reasons, **kw):
    """The recipe for a decoder: `inputs` [P, F, ...] (host), `exp_f32` [P, F, ...] its restatement's PCM, `per_stream`
    [P, len(reasons)] its rejection counts. Small run (checked against the restatement, f32 and s16), then the large run
    of S streams (f32, then s16 after a reset), every replica and the counters compared."""
    import torch
    F = inputs.shape[1]
    small_in = _dev(inputs)
    dec7 = make(P, F)
    small = {}
    for dt in (torch.float32, torch.int16):
        dec7.reset()
        dec7.counters(reset=True)
        small[dt] = _filled((P,) + out_shape, dt)
        _sync()
        dec7.decode_device(small_in, small[dt], **kw)
        c = dec7.counters()
        assert [c[r] for r in reasons] == per_stream.sum(0).tolist()
    dec7.close()
    assert np.array_equal(small[torch.float32].cpu().numpy().view(np.uint32), exp_f32.view(np.uint32))
    assert np.array_equal(small[torch.int16].cpu().numpy(), _s16(exp_f32))
    assert per_stream.sum() > 0                                         # some frames are rejected: the counters mean something

    big_in = _tile(small_in, S)
    del small_in
    dec = mem.create(make, S, F)
    want = (_replicas(S) @ per_stream).tolist()
    try:
        for dt in (torch.float32, torch.int16):
            dec.reset()
            dec.counters(reset=True)
            out = _filled((S,) + out_shape, dt)
            _sync()
            dec.decode_device(big_in, out, **kw)
            dec.sync()
            c = dec.counters()
            mem.probe()
            _assert_replicas(out, small[dt], f"{type(dec).__name__} {dt} output")
            assert [c[r] for r in reasons] == want, (c, want)
            del out
    finally:
        dec.close()
    del big_in, small


def _pick(pool, F, rng):
    return pool[rng.integers(0, pool.shape[0], F)]


# ---- ATRAC1 decoder -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def at1_cpu(tmp_path_factory):
    from at1_decode_lib import cpu_lib
    return cpu_lib(str(tmp_path_factory.mktemp("at1_decode_cpu")))


@pytest.mark.parametrize("nch,S,F", [(1, 65535, 64), (2, 16384, 128)], ids=["mono_full_grid", "stereo_at_frame_cap"])
def test_at1_decoder_large(mem, at1_cpu, nch, S, F):
    """mono: S * C = 65535 rows, F * S * C 64 below the cap; stereo: F * S * C = 2^22, exactly the cap. d_raw / d_out and the
    float output S * C * F * 512 floats (8.6e9 bytes)."""
    from at1_decode_lib import CpuDecoder, crafted_units, random_modes, set_block_modes
    _need(36)
    assert F * S * nch <= 2 ** 22 and (S * nch == 65535 or F * S * nch == 2 ** 22)
    assert S * nch * F * 512 * 4 > 2 ** 32
    rng = np.random.default_rng(11 + nch)
    g = np.load(os.path.join(ROOT, "tests", "golden", "at1_decode.npz"))
    pool = np.concatenate([g[f"{n}_units"] for n in g["cases"] if f"_ch{nch}" in n and not n.startswith("random")])
    crafted = crafted_units(nch, 5 + nch)
    units = []
    for k in range(P):
        u = _pick(pool, F, rng)
        if k % 2:
            u = set_block_modes(u, random_modes(u.shape[:2], rng))
        if k >= 4:   # malformed units, and in the last stream random bytes too
            u[rng.integers(0, F, 6)] = crafted[rng.integers(0, crafted.shape[0], 6)]
        if k == 6:
            u[rng.integers(0, F, 5)] = rng.integers(0, 256, (5, nch, 212), dtype=np.uint8)
        units.append(u)
    units = np.stack(units)                                               # [P, F, C, 212]
    exp, rej = [], []
    for s in range(P):
        d = CpuDecoder(nch, at1_cpu)
        exp.append(d.decode(units[s]))
        rej.append(d.rejected.astype(np.int64))
    _decode_large(mem, lambda n, f: At1HipDecoder(n_streams=n, max_frames=f, channels=nch), S, units, np.stack(exp), np.stack(rej),
                  (F, 512, nch), ("bad_block_size", "read_past_end"))


# ---- ATRAC3 decoder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fsz,S,F", [(384, 32767, 14), (192, 4096, 126)], ids=["lp2_full_grid", "lp4_at_frame_cap"])
def test_at3_decoder_large(mem, fsz, S, F):
    """LP2: 2 S = 65534 rows (gridDim.y); LP4 (joint stereo): (F + 2) S = 2^19, exactly the cap. d_raw (F + 2) * S * 2 * 2048
    floats, 8.6e9 bytes."""
    from at3_decode_lib import REASONS, CpuDecoder, crafted_frames, mutate_frames
    _need(30)
    js = fsz == 192
    assert (F + 2) * S <= 2 ** 19 and (2 * S == 65534 or (F + 2) * S == 2 ** 19)
    assert (F + 2) * S * 2 * 2048 * 4 > 2 ** 32
    rng = np.random.default_rng(fsz)
    g = np.load(os.path.join(ROOT, "tests", "golden", "at3_decode.npz"))
    pool = np.concatenate([g[f"{c}_frames"] for c in g["cases"] if int(g[f"{c}_row"][0]) == fsz and not str(c).startswith("random")])
    crafted = crafted_frames(fsz, js, seed=fsz + 1)
    frames = []
    for k in range(P):
        f = _pick(pool, F, rng)
        if k >= 2:
            f = mutate_frames(f, rng, n_flips=k - 1)
        if k >= 4:
            f[rng.integers(0, F, min(F, 6))] = crafted[rng.integers(0, crafted.shape[0], min(F, 6))]
        if k == 6:
            f[rng.integers(0, F, 2)] = rng.integers(0, 256, (2, fsz), dtype=np.uint8)
        frames.append(f)
    frames = np.stack(frames)                                             # [P, F, fsz]
    exp, rej = [], []
    for s in range(P):
        d = CpuDecoder(fsz, js)
        exp.append(d.decode(frames[s]))
        rej.append(d.rejected.astype(np.int64))
    _decode_large(mem, lambda n, f: At3HipDecoder(n_streams=n, frame_size=fsz, max_frames=f), S, frames, np.stack(exp), np.stack(rej),
                  (F, 1024, 2), REASONS)


# ---- ATRAC3plus decoder -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,S,F,tones", [(1, 65535, 4, False), (2, 2048, 129, True)], ids=["mono_full_grid", "stereo_tonal"])
def test_at3p_decoder_large(mem, nch, S, F, tones):
    """mono: S * C = 65535 rows, d_raw (F + 2) * S * 4096 floats (6.4e9 bytes); stereo with tonal blocks: d_raw 8.7e9 bytes
    and the float output S * F * 2048 * 2 floats, 4.33e9 bytes."""
    from at3p_decode_lib import REASONS, crafted_frames, cpu_decode, mutate_frames
    import at3p_tonal_lib as L
    _need(36)
    assert S * nch == 65535 or (S * F * 2048 * nch * 4 > 2 ** 32 and tones)
    assert (F + 2) * S * nch * 4096 * 4 > 6 * 10 ** 9
    rng = np.random.default_rng(100 + nch)
    name = "at3p_tonal.npz" if tones else "at3p_decode.npz"
    g = np.load(os.path.join(ROOT, "tests", "golden", name))
    pool = np.concatenate([g[f"{c}_frames"] for c in g["cases"] if int(g[f"{c}_channels"]) == nch and not str(c).startswith("random")])
    crafted = crafted_frames(nch, seed=60 + nch)[0]
    frames = []
    for k in range(P):
        f = _pick(pool, F, rng)
        if k >= 3:
            f = mutate_frames(f, rng, n_flips=k - 2, span=600 if k % 2 else None)
        if k >= 5:
            f[rng.integers(0, F, min(F, 3))] = crafted[rng.integers(0, crafted.shape[0], min(F, 3))]
        frames.append(f)
    frames = np.stack(frames)                                             # [P, F, 2048]
    exp, rej = [], []
    for s in range(P):
        pcm, r = L.cpu_tonal_decode(frames[s], nch) if tones else cpu_decode(frames[s], nch)
        exp.append(pcm)
        rej.append(np.asarray(r, np.int64))
    _decode_large(mem, lambda n, f: At3pHipDecoder(n_streams=n, channels=nch, max_frames=f), S, frames, np.stack(exp), np.stack(rej),
                  (F, 2048, nch), REASONS, tones=tones)


# ---- the refusing side of the frame caps --------------------------------------------------------------------------------------
def test_frame_caps_refused():
    """One frame past each decoder's cap (or its row of the grid) is refused at create, before anything is allocated."""
    import torch
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for make, kw, what in (
            (At1HipDecoder, dict(n_streams=16384, max_frames=129, channels=2), (129 * 16384 * 2, 2 ** 22)),
            (At1HipDecoder, dict(n_streams=65535, max_frames=65, channels=1), (65 * 65535, 2 ** 22)),
            (At3HipDecoder, dict(n_streams=4096, frame_size=192, max_frames=127), ((127 + 2) * 4096, 2 ** 19)),
            (At3pHipDecoder, dict(n_streams=32767, channels=2, max_frames=2047), ((2047 + 2) * 32767 * 2, 2 ** 27))):
        assert what[0] > what[1]
        with pytest.raises(At3HipError):
            make(**kw)
    # (no allocation: a few GB would have shown; the smallest refused configuration's buffers are 8.7e9 bytes)
    assert before - torch.cuda.mem_get_info()[0] < GB
