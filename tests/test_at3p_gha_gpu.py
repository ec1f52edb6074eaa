"""The ATRAC3plus tone analysis on the GPU (include/at3phip.h, FINDING TONES): at3phip_analyse_tones against the C restatement
tests/host/at3p_gha_cpu.c record for record and residual bit for bit, at3phip_encode_frames_tonal against the restatement's
pipeline byte for byte, the carried state, the frame budget, the buffer and queueing flags, and one decode of the frames."""
import numpy as np
import pytest

import at3p_gha_lib as G
import at3p_tonal_lib as T
from at3p_decode_lib import DELAY

pytestmark = pytest.mark.gpu

STREAMS = ("tones", "burst", "noise")
NF = 6


@pytest.fixture(scope="module")
def B():
    from atracdenc_amd import binding
    for name in G.NEW_SYMBOLS:   # a library without the analysis fails every test here
        binding._need(binding.load_library(), name)
    return binding


_cache = {}


def _writer(B, nch, max_frames):
    """the pipeline's frame writer: at3phip_write_frames_tonal with the records in host memory, the entry point that
    tests/test_at3p_tonal_write_gpu.py pins to the reference's frames (it prices the block, which a loud stereo frame needs)"""
    enc = B.At3pHip(n_streams=1, max_frames=max_frames, channels=nch)
    return enc, lambda specs, recs: enc.write_frames(specs[None], None, recs[None])[0]


def _case(B, nch):
    """(pcm [3][NF][2048][C], per stream the restatement pipeline's (frames, blocks, residual)), computed once"""
    if nch not in _cache:
        pcm = np.stack([G.signal_pcm(name, NF, nch) for name in STREAMS])
        enc, write = _writer(B, nch, NF)
        try:
            _cache[nch] = (pcm, [G.pipeline(pcm[s], write=write) for s in range(len(STREAMS))])
        finally:
            enc.close()
        if nch == 1:   # where the block leaves the frame its quant units the oracle's writer with the block spliced in says the same
            for s in range(len(STREAMS)):
                assert np.array_equal(G.pipeline(pcm[s])[0], _cache[nch][1][s][0])
    return _cache[nch]


def _enc(B, nch, streams=len(STREAMS), max_frames=NF):
    return B.At3pHip(n_streams=streams, max_frames=max_frames, channels=nch)


def _same_blocks(got, want):
    return got.tobytes() == np.ascontiguousarray(want, got.dtype).tobytes()


@pytest.mark.parametrize("nch", [1, 2])
def test_analyse_tones_equals_restatement(B, nch):
    pcm, want = _case(B, nch)
    enc = _enc(B, nch)
    try:
        bands = enc.pqf(pcm)
        blocks, resid = enc.analyse_tones(bands)
    finally:
        enc.close()
    for s, name in enumerate(STREAMS):
        assert np.array_equal(bands[s].view(np.uint32), G.pqf_bands(pcm[s]).view(np.uint32)), name
        assert _same_blocks(blocks[s], want[s][1]), (name, [G.band_waves(b, nch) for b in blocks[s]], [G.band_waves(b, nch) for b in want[s][1]])
        assert np.array_equal(resid[s].view(np.uint32), want[s][2].view(np.uint32)), name
    found = [sum(G.n_waves(b) for b in blocks[s]) for s in range(3)]
    assert found[0] > 0 and found[1] > 0 and found[2] == 0, found   # tones and burst have waves, noise has none


@pytest.mark.parametrize("nch", [1, 2])
def test_encode_frames_tonal_equals_restatement_pipeline(B, nch):
    pcm, want = _case(B, nch)
    enc = _enc(B, nch)
    try:
        got = enc.encode_frames_tonal(pcm)
        enc.reset()
        s16 = np.round(pcm * 32767.0).astype(np.int16)
        got16 = enc.encode_frames_tonal_s16(s16)
        enc.reset()
        as_float = enc.encode_frames_tonal((s16.astype(np.float32) / np.float32(32768.0)).astype(np.float32))
    finally:
        enc.close()
    for s, name in enumerate(STREAMS):
        bad = (got[s] != want[s][0]).any(axis=1)
        assert not bad.any(), (name, np.nonzero(bad)[0].tolist())
    assert np.array_equal(got16, as_float)


@pytest.mark.parametrize("nch", [1, 2])
def test_carried_state_any_split_gives_the_same(B, nch):
    """6 frames in one call, as 2 + 4 and as six calls of 1: records, residuals and frames; after at3phip_reset the stream starts over"""
    pcm, want = _case(B, nch)
    enc = _enc(B, nch)
    try:
        bands = enc.pqf(pcm)
        for split in ((6,), (2, 4), (1,) * 6):
            enc.reset()
            at, blocks, resid, frames = 0, [], [], []
            for n in split:
                b, r = enc.analyse_tones(bands[:, at:at + n])
                blocks.append(b)
                resid.append(r)
                at += n
            enc.reset()
            at = 0
            for n in split:
                frames.append(enc.encode_frames_tonal(pcm[:, at:at + n]))
                at += n
            blocks, resid, frames = np.concatenate(blocks, 1), np.concatenate(resid, 1), np.concatenate(frames, 1)
            for s in range(len(STREAMS)):
                assert _same_blocks(blocks[s], want[s][1]), (split, s)
                assert np.array_equal(resid[s].view(np.uint32), want[s][2].view(np.uint32)), (split, s)
                assert np.array_equal(frames[s], want[s][0]), (split, s)
        # without a reset the stream goes on: the first slot pairs the last frame with the new first one
        b2, _ = enc.analyse_tones(bands[:, :2])
        cont = G.CpuToneAnalyser(nch)
        cont.analyse(bands[0])
        assert _same_blocks(b2[0], cont.analyse(bands[0, :2])[0])
        assert not _same_blocks(b2[0], want[0][1][:2])
    finally:
        enc.close()


def test_async_queued_calls_and_device_pointers(B):
    """Two queued calls (AT3HIP_ASYNC) on device buffers, host and device PCM / frames in the synchronous call: the same bytes.
    The tensors are complete (torch.cuda.synchronize) before they are handed over: the context's streams wait for no other."""
    import torch
    nch = 2
    pcm, want = _case(B, nch)
    exp = np.stack([w[0] for w in want])
    enc = _enc(B, nch)
    try:
        d_pcm = [torch.from_numpy(np.ascontiguousarray(pcm[:, a:b])).cuda() for a, b in ((0, 2), (2, 6))]
        d_out = [torch.zeros((3, n, 2048), dtype=torch.uint8, device="cuda") for n in (2, 4)]
        torch.cuda.synchronize()
        for p, o in zip(d_pcm, d_out):
            enc.encode_frames_tonal_device(p.data_ptr(), p.shape[1], o.data_ptr(), asynchronous=True)
        enc.sync()
        assert np.array_equal(np.concatenate([o.cpu().numpy() for o in d_out], 1), exp)
        d_all = torch.from_numpy(pcm).cuda()
        d_s16 = torch.from_numpy(np.round(pcm * 32767.0).astype(np.int16)).cuda()
        d_fr = torch.zeros((3, NF, 2048), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for in_dev in (False, True):
            for out_dev in (False, True):
                enc.reset()
                h_out = np.zeros((3, NF, 2048), np.uint8)
                d_fr.zero_()
                torch.cuda.synchronize()
                enc.encode_frames_tonal_ptr(d_all.data_ptr() if in_dev else pcm.ctypes.data, NF, d_fr.data_ptr() if out_dev else h_out.ctypes.data,
                                            (B.AT3HIP_PCM_ON_DEVICE if in_dev else 0) | (B.AT3HIP_OUT_ON_DEVICE if out_dev else 0))
                assert np.array_equal(d_fr.cpu().numpy() if out_dev else h_out, exp), (in_dev, out_dev)
        enc.reset()
        host16 = enc.encode_frames_tonal_s16(d_s16.cpu().numpy())
        enc.reset()
        enc.encode_frames_tonal_device_s16(d_s16.data_ptr(), NF, d_fr.data_ptr())
        assert np.array_equal(d_fr.cpu().numpy(), host16)
        # the stage tap on device buffers
        enc.reset()
        d_bands = torch.from_numpy(enc.pqf(pcm)).cuda()
        d_res = torch.zeros_like(d_bands)
        torch.cuda.synchronize()
        blocks = enc.analyse_tones_device(d_bands.data_ptr(), NF, d_res.data_ptr())
        for s in range(3):
            assert _same_blocks(blocks[s], want[s][1])
            assert np.array_equal(d_res[s].cpu().numpy().view(np.uint32), want[s][2].view(np.uint32))
    finally:
        enc.close()


def test_frame_budget_keeps_48_of_96_with_the_ties_as_defined(B):
    """A stereo frame pair with the same three strong sines in each of the 16 subbands of both channels: 96 waves are found, 32
    of equal A2 for each sine. The 32 of the strongest stay, then of the second sine's the 16 that go first by channel, then
    band: channel 0's. Every band of channel 0 holds two waves, every band of channel 1 one."""
    bands = G.budget_bands()[None]
    enc = _enc(B, 2, streams=1, max_frames=2)
    try:
        blocks, resid = enc.analyse_tones(bands)
    finally:
        enc.close()
    wb, wr = G.CpuToneAnalyser(2).analyse(bands[0])
    assert _same_blocks(blocks[0], wb) and np.array_equal(resid[0].view(np.uint32), wr.view(np.uint32))
    rec = blocks[0, 1]
    assert G.n_waves(rec) == 48 and int(rec["num_tone_bands"]) == 16
    waves = G.band_waves(rec, 2)
    for b in range(16):
        assert [w[0] for w in waves[0][b]] == list(G.BUDGET_FREQS[:2]), (b, waves[0][b])
        assert [w[0] for w in waves[1][b]] == list(G.BUDGET_FREQS[:1]), (b, waves[1][b])


def test_more_stream_channel_pairs_than_a_quarter_of_the_grid_limit(B):
    """16400 mono streams, one frame: at3phip_create admits n_streams * channels up to 65535, and the analysis must launch for all
    of them ((stream, channel) is gridDim.y as in every other kernel; four times that would pass the limit from 16384 on). The
    streams repeat four signals; each equals the restatement, records, residual and frame, the last stream included."""
    names, S = ("tones", "burst", "noise", "mix"), 16400
    one = np.stack([G.signal_pcm(n, 1, 1) for n in names])                      # [4][1][2048][1]
    pcm = np.ascontiguousarray(np.tile(one, (S // 4, 1, 1, 1)))
    enc = _enc(B, 1, streams=S, max_frames=1)
    try:
        bands = enc.pqf(pcm)
        blocks, resid = enc.analyse_tones(bands)
        enc.reset()
        frames = enc.encode_frames_tonal(pcm)
    finally:
        enc.close()
    for i, name in enumerate(names):
        wf, wb, wr = G.pipeline(one[i])
        for s in (i, S - 4 + i):
            assert _same_blocks(blocks[s], wb) and np.array_equal(resid[s].view(np.uint32), wr.view(np.uint32)), (name, s)
            assert np.array_equal(frames[s], wf), (name, s)
    assert blocks.tobytes() == np.tile(blocks[:4, 0], S // 4).tobytes()
    assert np.array_equal(frames.reshape(S // 4, 4, 2048), np.tile(frames[:4, 0], (S // 4, 1, 1)))
    assert sum(G.n_waves(b) for b in blocks[:4, 0]) > 0


def test_sines_next_to_both_ends_equal_restatement(B):
    """sines within 9 indices of either end of a subband (step 3's end bins, the normalisers of steps 4 and 5)"""
    bands = G.end_sine_bands()
    enc = _enc(B, 2, streams=1, max_frames=3)
    try:
        blocks, resid = enc.analyse_tones(bands[None])
    finally:
        enc.close()
    wb, wr = G.CpuToneAnalyser(2).analyse(bands)
    assert _same_blocks(blocks[0], wb) and np.array_equal(resid[0].view(np.uint32), wr.view(np.uint32))
    assert G.n_waves(blocks[0, 2]) == 32


@pytest.mark.parametrize("nch", [1, 2])
def test_noise_gives_the_plain_frames_one_frame_later(B, nch):
    pcm = G.signal_pcm("noise", 14, nch)[None]
    enc = _enc(B, nch, streams=1, max_frames=14)
    try:
        plain = enc.encode_frames(pcm)
        enc.reset()
        tonal = enc.encode_frames_tonal(pcm)
    finally:
        enc.close()
    assert np.array_equal(tonal[0, 1:], plain[0, :-1])


def test_tones_decode_reaches_the_cpu_round_trip(B):
    """`tones`, mono, 14 frames and the flushing frame of silence through at3phip_encode_frames_tonal and At3pHipDecoder(tones=True):
    the SNR of the CPU round trip (the restatement's pipeline through the decoder's restatement) to 0.01 dB"""
    nf = 14
    pcm = np.concatenate([G.signal_pcm("tones", nf, 1), np.zeros((1, 2048, 1), np.float32)])
    x = pcm[:nf, :, 0].reshape(-1)
    enc = _enc(B, 1, streams=1, max_frames=nf + 1)
    dec = B.At3pHipDecoder(n_streams=1, channels=1, max_frames=nf + 1)
    try:
        frames = enc.encode_frames_tonal(pcm[None])
        out = dec.decode(frames, tones=True)
        assert sum(dec.counters().values()) == 0
    finally:
        enc.close()
        dec.close()
    want_frames = G.pipeline(pcm)[0]   # (mono: the oracle's writer with the block spliced in)
    assert np.array_equal(frames[0], want_frames)
    cpu, rej = T.cpu_tonal_decode(want_frames, 1)
    assert rej.sum() == 0
    # the analysis lags one frame: the decoder's output is one frame later than at3phip_encode_frames'
    snr_gpu = G.snr_db(x, out[0, :, :, 0].reshape(-1)[2048:], nf)
    snr_cpu = G.snr_db(x, cpu[:, :, 0].reshape(-1)[2048:], nf)
    print(f"tones round trip: GPU {snr_gpu:.3f} dB, CPU {snr_cpu:.3f} dB")
    assert abs(snr_gpu - snr_cpu) <= 0.01, (snr_gpu, snr_cpu)
    assert DELAY == 2416
