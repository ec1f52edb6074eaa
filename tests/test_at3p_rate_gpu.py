"""ATRAC3plus at frame sizes other than 2048 bytes on the GPU (at3phip_set_frame_bytes, at3phip_decoder_set_frame_bytes; include/
at3phip.h, FRAME SIZE): the adaptive writers' frames and the decoder's PCM equal the restatement tests/host/at3p_writer_cpu.c bit for
bit at every test size through every call, from host and device buffers, queued and waiting, however the stream is split; the
fixed table is refused at any size but 2048; the setter refuses what is not admissible; a context that never changes its size, or
changes back, gives the bytes it always gave; the command line writes and reads the standard bitrates.
3 streams x 4 frames unless said otherwise; what does not depend on the frame size (spectra, tone analysis) is computed once."""
import ctypes
import os
import struct
import subprocess
import wave

import numpy as np
import pytest

import at3p_writer_lib as W
import at3p_gha_lib as G
import at3p_tonal_write_lib as TW
from at3_testlib import at3p_mdct, at3p_pqf, at3p_write_frames

pytestmark = pytest.mark.gpu
S, F = 3, 4
CASES = [(nch, fb) for nch in (1, 2) for fb in W.SIZES[nch]]
IDS = [f"{'mono' if nch == 1 else 'stereo'}_{fb}" for nch, fb in CASES]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def B():
    from atracdenc_amd import binding
    return binding


def _as16(pcm):
    """(int16 samples, the floats the device widens them to): both calls of a pair then see the same signal"""
    p16 = np.clip(np.rint(pcm * 32767.0), -32768, 32767).astype(np.int16)
    return p16, (p16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def _specs_of_pcm(pcm):
    """pcm [n, 2048, C] of one stream from its start -> [n, C, 2048]: what at3phip_encode_frames hands its writer"""
    out = np.zeros((pcm.shape[0], pcm.shape[2], 2048), np.float32)
    for c in range(pcm.shape[2]):
        bands = at3p_pqf(np.ascontiguousarray(pcm[:, :, c]))
        out[:, c] = at3p_mdct((bands.astype(np.float64) / G.SCALE).astype(np.float32))
    return out


_cache = {}


def _plain(nch, n=F):
    """(int16 PCM [S, n, 2048, C], the same as float, the spectra the writer sees [S, n, C, 2048]) of mix, noise and tones"""
    if ("plain", nch, n) not in _cache:
        p16, pcm = _as16(np.stack([G.signal_pcm(name, n, nch) for name in ("mix", "noise", "tones")]))
        _cache[("plain", nch, n)] = (p16, pcm, np.stack([_specs_of_pcm(pcm[s]) for s in range(S)]))
    return _cache[("plain", nch, n)]


def _tonal(nch):
    """(int16 PCM, float PCM, residual spectra [S, F, C, 2048], the writer's records [S, F]) of the tone analysis with gates and
    sharing on tones, keyed and mix (stereo: both channels alike, so that there are bands to share)"""
    if ("tonal", nch) not in _cache:
        raw = [G.twin_pcm("tones", F), G.keyed_pcm(F, 2), G.twin_pcm("mix", F)] if nch == 2 else \
            [G.signal_pcm("tones", F, 1), G.keyed_pcm(F, 1), G.signal_pcm("mix", F, 1)]
        p16, pcm = _as16(np.stack(raw))
        specs, recs = [], []

        def grab(sp, rc):
            specs.append(sp)
            recs.append(rc)
            return np.zeros((sp.shape[0], 2048), np.uint8)
        waves = 0
        for s in range(S):
            _, blocks, _ = G.pipeline(pcm[s], True, True, grab)
            waves += sum(G.n_waves(b) for b in blocks[:-1])
        assert waves > 0
        _cache[("tonal", nch)] = (p16, pcm, np.stack(specs), np.stack(recs))
    return _cache[("tonal", nch)]


WIN = np.array([[[0x01ef, 0x8001], [0xffff, 0xffff], [0, 0x00ff], [0, 0]], [[0x0010, 0], [0xfeff, 0x1234], [0xffff, 0], [1, 2]],
                [[0, 0], [0, 0], [0x8000, 0x0001], [0xffff, 0x7fff]]], np.uint16)


def _records(nch):
    """[S][F] dicts / None: the largest record, small ones and frames without"""
    small, rnd = TW.case_blocks(f"small_{nch}")[0][0], TW.case_blocks(f"random_{nch}")[0][0]
    return [[TW.largest_block(nch), None, small, TW.largest_block(nch, 1)], [rnd, TW.largest_block(nch), None, None], [None, small, rnd, None]]


# ---- the writers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,fb", CASES, ids=IDS)
def test_six_calls_equal_the_restatement(B, nch, fb):
    """at3phip_write_frames, at3phip_write_frames_tonal (window flags, records beside frames without one, the largest record on
    full-scale noise), at3phip_encode_frames(_short) and at3phip_encode_frames_tonal(_short) with gates and sharing, host buffers"""
    p16, pcm, specs = _plain(nch)
    t16, tpcm, tspecs, trecs = _tonal(nch)
    win, blocks = np.ascontiguousarray(WIN[:, :, :nch]), _records(nch)
    wspecs = np.stack([W.full_scale_noise(F, nch, seed=4), W.specs_of("mix", nch, F), W.specs_of("silence", nch, F)])
    recs = np.stack([B.pack_tonal_blocks(row, nch) for row in blocks])
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, frame_bytes=fb)
    try:
        assert enc.frame_bytes == fb
        got_w = enc.write_frames(wspecs, win, adaptive=True)
        got_t = enc.write_frames(wspecs, win, recs, adaptive=True)
        got_e = enc.encode_frames(pcm, adaptive=True)
        enc.reset()
        got_e16 = enc.encode_frames_s16(p16, adaptive=True)
        enc.reset()
        got_a = enc.encode_frames_tonal(tpcm, gated=True, shared=True, adaptive=True)
        enc.reset()
        got_a16 = enc.encode_frames_tonal_s16(t16, gated=True, shared=True, adaptive=True)
    finally:
        enc.close()
    for g in (got_w, got_t, got_e, got_e16, got_a, got_a16):
        assert g.shape == (S, F, fb)
    assert np.array_equal(got_w, W.write_streams(wspecs, fb, win=win))
    assert np.array_equal(got_t, np.stack([W.write_adaptive(wspecs[s], fb, win=win[s], blocks=blocks[s]) for s in range(S)]))
    want_e = W.write_streams(specs, fb)
    assert np.array_equal(got_e, want_e) and np.array_equal(got_e16, want_e)
    want_a = np.stack([W.write_adaptive(tspecs[s], fb, blocks=trecs[s]) for s in range(S)])
    assert np.array_equal(got_a, want_a) and np.array_equal(got_a16, want_a)


@pytest.mark.parametrize("nch,fb", CASES, ids=IDS)
def test_device_buffers_queued_calls_and_splits(B, nch, fb):
    """device buffers waiting and queued for all six calls, one call of 4 frames against calls of 1 + 3 for all six; the bytes
    directly behind every [S][F][frame_bytes] output stay what they were"""
    import torch
    p16, pcm, specs = _plain(nch)
    want = W.write_streams(specs, fb)
    n = S * F * fb
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, frame_bytes=fb)
    try:
        d_pcm, d_specs = torch.from_numpy(pcm).cuda(), torch.from_numpy(specs).cuda()
        outs = [torch.full((n + 4096,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(7)]
        torch.cuda.synchronize()
        enc.encode_frames_device(d_pcm.data_ptr(), F, outs[0].data_ptr(), adaptive=True)
        enc.reset()
        enc.encode_frames_device(d_pcm.data_ptr(), F, outs[1].data_ptr(), asynchronous=True, adaptive=True)
        enc.sync()
        enc.write_frames_ptr(d_specs.data_ptr(), F, None, outs[2].data_ptr(), B.AT3HIP_PCM_ON_DEVICE | B.AT3HIP_OUT_ON_DEVICE | B.AT3PHIP_ALLOC_ADAPTIVE)
        t16, tpcm, tspecs, trecs = _tonal(nch)
        d_t16 = torch.from_numpy(t16).cuda()
        torch.cuda.synchronize()
        enc.reset()
        enc.encode_frames_tonal_device_s16(d_t16.data_ptr(), F, outs[3].data_ptr(), asynchronous=True, gated=True, shared=True, adaptive=True)
        enc.sync()
        # the other three: the float tonal call waiting, the 16-bit encode queued, the tonal writer from device spectra (its
        # records are host memory by its contract)
        d_tpcm, d_p16 = torch.from_numpy(tpcm).cuda(), torch.from_numpy(p16).cuda()
        blocks = _records(nch)
        recs = np.stack([B.pack_tonal_blocks(row, nch) for row in blocks])
        torch.cuda.synchronize()
        enc.reset()
        enc.encode_frames_tonal_device(d_tpcm.data_ptr(), F, outs[4].data_ptr(), gated=True, shared=True, adaptive=True)
        enc.reset()
        enc.encode_frames_device_s16(d_p16.data_ptr(), F, outs[5].data_ptr(), asynchronous=True, adaptive=True)
        enc.sync()
        enc.write_frames_tonal_ptr(d_specs.data_ptr(), F, None, recs.ctypes.data, outs[6].data_ptr(),
                                   B.AT3HIP_PCM_ON_DEVICE | B.AT3HIP_OUT_ON_DEVICE | B.AT3PHIP_ALLOC_ADAPTIVE)
        # 1 + 3 for each of the six
        def split(call, x, **kw):
            enc.reset()
            return np.concatenate([call(x[:, :1], **kw), call(x[:, 1:], **kw)], axis=1)
        parts = split(enc.encode_frames, pcm, adaptive=True)
        parts16 = split(enc.encode_frames_s16, p16, adaptive=True)
        t_parts = split(enc.encode_frames_tonal, tpcm, gated=True, shared=True, adaptive=True)
        t_parts16 = split(enc.encode_frames_tonal_s16, t16, gated=True, shared=True, adaptive=True)
        w_parts = np.concatenate([enc.write_frames(specs[:, :1], adaptive=True), enc.write_frames(specs[:, 1:], adaptive=True)], axis=1)
        wt_parts = np.concatenate([enc.write_frames(specs[:, :1], None, recs[:, :1], adaptive=True),
                                   enc.write_frames(specs[:, 1:], None, recs[:, 1:], adaptive=True)], axis=1)
    finally:
        enc.close()
    got = [o.cpu().numpy() for o in outs]
    for g in got:
        assert (g[n:] == SENTINEL).all()
    for k in range(3):
        assert np.array_equal(got[k][:n].reshape(S, F, fb), want), k
    t_want = np.stack([W.write_adaptive(tspecs[s], fb, blocks=trecs[s]) for s in range(S)])
    wt_want = np.stack([W.write_adaptive(specs[s], fb, blocks=blocks[s]) for s in range(S)])
    assert np.array_equal(got[3][:n].reshape(S, F, fb), t_want) and np.array_equal(got[4][:n].reshape(S, F, fb), t_want)
    assert np.array_equal(got[5][:n].reshape(S, F, fb), want) and np.array_equal(got[6][:n].reshape(S, F, fb), wt_want)
    assert np.array_equal(parts, want) and np.array_equal(parts16, want) and np.array_equal(w_parts, want)
    assert np.array_equal(t_parts, t_want) and np.array_equal(t_parts16, t_want) and np.array_equal(wt_parts, wt_want)


def test_odd_stride_mono_192_from_device_buffers(B):
    """mono, 5 streams x 3 frames of 192 bytes: frame offsets that are no multiple of 2048 or 256"""
    import torch
    S5, F3, fb = 5, 3, 192
    specs = np.ascontiguousarray(W.specs_of("mix", 1, S5 * F3).reshape(S5, F3, 1, 2048))
    enc = B.At3pHip(n_streams=S5, max_frames=F3, channels=1, frame_bytes=fb)
    dec = B.At3pHipDecoder(n_streams=S5, channels=1, max_frames=F3, frame_bytes=fb)
    try:
        d_specs = torch.from_numpy(specs).cuda()
        d_out = torch.full((S5 * F3 * fb + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_pcm = torch.zeros((S5, F3, 2048, 1), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        enc.write_frames_ptr(d_specs.data_ptr(), F3, None, d_out.data_ptr(), B.AT3HIP_PCM_ON_DEVICE | B.AT3HIP_OUT_ON_DEVICE | B.AT3PHIP_ALLOC_ADAPTIVE)
        frames = d_out[:S5 * F3 * fb].reshape(S5, F3, fb).contiguous()
        dec.decode_device(frames, d_pcm, ordered=False)
        got, pcm = d_out.cpu().numpy(), d_pcm.cpu().numpy()
        assert sum(dec.counters().values()) == 0
    finally:
        enc.close()
        dec.close()
    want = W.write_streams(specs, fb)
    assert (got[S5 * F3 * fb:] == SENTINEL).all() and np.array_equal(got[:S5 * F3 * fb].reshape(S5, F3, fb), want)
    epcm, _ = W.decode_streams(want, 1)
    assert np.array_equal(pcm.view(np.uint32), epcm.view(np.uint32))


# ---- the fixed table, the setter, the default --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
def test_unflagged_calls_are_refused_at_376_and_write_nothing(B, nch):
    """all six calls without AT3PHIP_ALLOC_ADAPTIVE on a context set to 376 bytes: AT3HIP_EINVAL, the reason in the last error, a
    sentinel-filled output untouched; and no stream state moved: the next flagged call gives a fresh context's bytes"""
    p16, pcm, specs = _plain(nch)
    recs = np.zeros((S, F), B.AT3P_TONAL_BLOCK_DTYPE)
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, frame_bytes=376)
    try:
        out = np.full((S, F, 2048), SENTINEL, np.uint8)
        calls = [lambda: enc.write_frames_ptr(specs.ctypes.data, F, None, out.ctypes.data, 0),
                 lambda: enc.write_frames_tonal_ptr(specs.ctypes.data, F, None, recs.ctypes.data, out.ctypes.data, 0),
                 lambda: enc.encode_frames_ptr(pcm.ctypes.data, F, out.ctypes.data, 0),
                 lambda: enc.encode_frames_s16_ptr(p16.ctypes.data, F, out.ctypes.data, 0),
                 lambda: enc.encode_frames_tonal_ptr(pcm.ctypes.data, F, out.ctypes.data, B.AT3PHIP_TONES_GATED),
                 lambda: enc.encode_frames_tonal_s16_ptr(p16.ctypes.data, F, out.ctypes.data, 0)]
        for k, call in enumerate(calls):
            with pytest.raises(B.At3HipError, match=r"\(-1\).*the fixed table is defined for 2048-byte frames only"):
                call()
            enc.sync()
            assert (out == SENTINEL).all(), k
        got = enc.encode_frames(pcm, adaptive=True)
    finally:
        enc.close()
    assert np.array_equal(got, W.write_streams(specs, 376))


@pytest.mark.parametrize("nch", [1, 2])
def test_setter_refuses_inadmissible_sizes(B, nch):
    enc = B.At3pHip(n_streams=1, max_frames=1, channels=nch, frame_bytes=376)
    dec = B.At3pHipDecoder(n_streams=1, channels=nch, max_frames=1, frame_bytes=376)
    try:
        for obj in (enc, dec):
            for bad in (0, 7, 2056, W.MIN_BYTES[nch] - 8, -8, 380):
                with pytest.raises(B.At3HipError, match=r"\(-1\).*frame_bytes"):
                    obj.set_frame_bytes(bad)
                assert obj.frame_bytes == 376
            obj.set_frame_bytes(W.MIN_BYTES[nch])
            assert obj.frame_bytes == W.MIN_BYTES[nch]
        lib = enc.lib
        assert lib.at3phip_set_frame_bytes(None, 376) == -1 and lib.at3phip_decoder_set_frame_bytes(None, 376) == -1
        v = ctypes.c_int32(5)
        assert lib.at3phip_get_frame_bytes(None, ctypes.byref(v)) == -1 and lib.at3phip_get_frame_bytes(enc.ctx, None) == -1 and v.value == 5
    finally:
        enc.close()
        dec.close()


@pytest.mark.parametrize("nch", [1, 2])
def test_explicit_2048_equals_an_untouched_context(B, nch):
    """flagged and unflagged, write and encode: the same bytes, and the unflagged ones are the oracle writer's"""
    p16, pcm, specs = _plain(nch)
    a = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    b = B.At3pHip(n_streams=S, max_frames=F, channels=nch, frame_bytes=2048)
    try:
        assert a.frame_bytes == b.frame_bytes == 2048
        got = [[e.write_frames(specs), e.write_frames(specs, adaptive=True), e.encode_frames(pcm), e.encode_frames_tonal(pcm, adaptive=True)] for e in (a, b)]
    finally:
        a.close()
        b.close()
    for x, y in zip(*got):
        assert np.array_equal(x, y)
    assert np.array_equal(got[1][0], np.stack([at3p_write_frames(specs[s]) for s in range(S)]))
    assert np.array_equal(got[1][1], np.stack([W.write_adaptive(specs[s]) for s in range(S)]))


@pytest.mark.parametrize("nch", [1, 2])
def test_a_stream_may_change_its_size_between_calls(B, nch):
    """2048 -> 376 -> 2048 between calls of 2, 1 and 2 frames (the first queued: the setter waits for it): per call the bytes of
    fresh contexts at those sizes fed the same stream, which are the restatement's"""
    import torch
    n = 5
    p16, pcm, specs = _plain(nch, n)
    enc = B.At3pHip(n_streams=S, max_frames=n, channels=nch)
    fresh = {fb: B.At3pHip(n_streams=S, max_frames=n, channels=nch, frame_bytes=fb) for fb in (2048, 376)}
    try:
        d_pcm = torch.from_numpy(np.ascontiguousarray(pcm[:, :2])).cuda()
        d_out = torch.zeros((S, 2, 2048), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        enc.encode_frames_device(d_pcm.data_ptr(), 2, d_out.data_ptr(), asynchronous=True, adaptive=True)
        enc.set_frame_bytes(376)
        first = d_out.cpu().numpy()
        second = enc.encode_frames(pcm[:, 2:3], adaptive=True)
        enc.set_frame_bytes(2048)
        third = enc.encode_frames(pcm[:, 3:], adaptive=True)
        whole = {fb: e.encode_frames(pcm, adaptive=True) for fb, e in fresh.items()}
    finally:
        enc.close()
        for e in fresh.values():
            e.close()
    assert second.shape == (S, 1, 376) and third.shape == (S, 2, 2048)
    assert np.array_equal(first, whole[2048][:, :2]) and np.array_equal(second, whole[376][:, 2:3]) and np.array_equal(third, whole[2048][:, 3:])
    assert np.array_equal(whole[376], W.write_streams(specs, 376)) and np.array_equal(whole[2048], W.write_streams(specs, 2048))


@pytest.mark.parametrize("nch", [1, 2])
def test_non_finite_spectra_stay_in_their_stream_at_376(B, nch):
    normal = W.specs_of("noise", nch, F)
    specs = np.stack([W.odd_specs(nch, F), normal, W.specs_of("mix", nch, F)])
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, frame_bytes=376)
    try:
        got = enc.write_frames(specs, adaptive=True)
        alone = enc.write_frames(np.stack([normal, normal, normal]), adaptive=True)
    finally:
        enc.close()
    assert np.array_equal(got[1], alone[0]) and np.array_equal(got[1], W.write_adaptive(normal, 376))
    assert np.array_equal(got, W.write_streams(specs, 376))


# ---- the decoder -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,fb", CASES, ids=IDS)
def test_decoder_equals_the_restatement(B, nch, fb):
    """the frames of the writer tests (records among them) through at3phip_decode: float and int16, tones on and off (off: the
    frames with a block are rejected and counted), one call against 1 + 3"""
    win, blocks = np.ascontiguousarray(WIN[:, :, :nch]), _records(nch)
    wspecs = np.stack([W.full_scale_noise(F, nch, seed=4), W.specs_of("mix", nch, F), W.specs_of("silence", nch, F)])
    frames = np.stack([W.write_adaptive(wspecs[s], fb, win=win[s], blocks=blocks[s]) for s in range(S)])
    dec = B.At3pHipDecoder(n_streams=S, channels=nch, max_frames=F, frame_bytes=fb)
    try:
        assert dec.frame_bytes == fb
        for tones in (True, False):
            want, rej = W.decode_streams(frames, nch, tones)
            dec.reset()
            got = dec.decode(frames, tones=tones)
            cnt = dec.counters(reset=True)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), tones
            assert list(cnt.values()) == rej.tolist(), (tones, cnt, rej)
            assert (rej.sum() == 0) if tones else (rej[2] == sum(b is not None for row in blocks for b in row))
            dec.reset()
            parts = np.concatenate([dec.decode(frames[:, :1], tones=tones), dec.decode(frames[:, 1:], tones=tones)], axis=1)
            assert np.array_equal(parts.view(np.uint32), want.view(np.uint32))
            dec.reset()
            s16 = dec.decode(frames, s16=True, tones=tones)
            assert np.array_equal(s16, np.rint(want * np.float32(32767.0)).astype(np.int16))
    finally:
        dec.close()


@pytest.mark.parametrize("nch", [1, 2])
def test_decoder_may_change_its_size_between_queued_calls(B, nch):
    """a queued at3phip_decode at 2048 bytes, at3phip_decoder_set_frame_bytes(376) - which waits for it -, a queued decode at 376 on
    the same streams, and back: the restatement's PCM for the stream as a whole (the synthesis state carries over the changes)"""
    import torch
    specs = np.stack([W.specs_of(name, nch, 6) for name in ("mix", "noise", "tones")])
    parts = [W.write_streams(specs[:, :2], 2048), W.write_streams(specs[:, 2:4], 376), W.write_streams(specs[:, 4:], 2048)]
    dec = B.At3pHipDecoder(n_streams=S, channels=nch, max_frames=2)
    try:
        d_in = [torch.from_numpy(p).cuda() for p in parts]
        d_out = [torch.zeros((S, 2, 2048, nch), dtype=torch.float32, device="cuda") for _ in parts]
        torch.cuda.synchronize()
        for k, fb in enumerate((2048, 376, 2048)):
            if k:
                dec.set_frame_bytes(fb)
            dec.decode_ptr(d_in[k].data_ptr(), 2, d_out[k].data_ptr(), B.AT3HIP_PCM_ON_DEVICE | B.AT3HIP_OUT_ON_DEVICE | B.AT3HIP_ASYNC)
        dec.sync()
        got = np.concatenate([o.cpu().numpy() for o in d_out], axis=1)
        assert sum(dec.counters().values()) == 0
    finally:
        dec.close()
    for s in range(S):
        ref = W.Decoder(nch)
        want = np.concatenate([ref.decode(p[s]) for p in parts])
        assert np.array_equal(got[s].view(np.uint32), want.view(np.uint32)), s


@pytest.mark.parametrize("nch", [1, 2])
def test_decoder_at_376_on_the_first_bytes_of_2048_byte_frames(B, nch):
    """frames written at 2048 bytes, cut to their first 376: the rejection counters per reason and the PCM equal the restatement's
    (full frames run past the end; a frame that ends early enough still decodes)"""
    specs = np.stack([W.specs_of("mix", nch, F), W.specs_of("silence", nch, F), W.quiet_mono(F).repeat(nch, axis=1) * np.float32(2.0 ** -6)])
    full = W.write_streams(specs, 2048)
    cut = np.ascontiguousarray(full[:, :, :376])
    dec = B.At3pHipDecoder(n_streams=S, channels=nch, max_frames=F, frame_bytes=376)
    try:
        got = dec.decode(cut, tones=True)
        cnt = dec.counters()
    finally:
        dec.close()
    want, rej = W.decode_streams(cut, nch, True)
    assert list(cnt.values()) == rej.tolist() and rej[4] >= F, (cnt, rej)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def _wav_in(path, pcm16, nch):
    with wave.open(path, "wb") as w:
        w.setnchannels(nch)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(pcm16.tobytes())


def _run(*args):
    return subprocess.run(list(args), capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("container", ["oma", "riff"])
def test_cli_bitrate_64(B, tmp_path, container):
    """-e atrac3plus --adaptive --bitrate 64, then -d: the header fields and file size, the frames of the library path, and the
    decoded WAV equal to the library's decoder on those frames"""
    NF, nch, fb = 6, 2, 376
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "at3hipenc")
    pcm16 = np.clip(np.rint(G.signal_pcm("mix", NF, nch) * 32767.0), -32768, 32767).astype("<i2")
    wav_in, out, wav_out = str(tmp_path / "in.wav"), str(tmp_path / ("a.oma" if container == "oma" else "a.at3")), str(tmp_path / "y.wav")
    _wav_in(wav_in, pcm16, nch)
    r = _run(exe, "-e", "atrac3plus", "-i", wav_in, "-o", out, "--adaptive", "--bitrate", "64", "--batch", "4", "--container", container)
    assert r.returncode == 0 and "Bitrate: 64 kbit/s (376-byte frames)" in r.stdout, r.stdout + r.stderr
    data = open(out, "rb").read()
    if container == "oma":
        word = struct.unpack(">I", data[32:36])[0]
        assert data[:3] == b"EA3" and word >> 24 == 1 and (word >> 10) & 7 == nch and (word & 0x3ff) * 8 + 8 == fb and len(data) == 96 + NF * fb
        body = data[96:]
    else:
        fmt, pos = data.index(b"fmt ") + 8, data.index(b"data")
        tag, ch, rate, byte_rate, align = struct.unpack("<HHIIH", data[fmt:fmt + 14])
        assert (tag, ch, rate, byte_rate, align) == (0xFFFE, nch, 44100, fb * 44100 // 2048, fb)
        assert struct.unpack("<I", data[pos + 4:pos + 8])[0] == NF * fb and len(data) == pos + 8 + NF * fb and struct.unpack("<I", data[4:8])[0] == len(data) - 8
        body = data[pos + 8:]
    got = np.frombuffer(body, np.uint8).reshape(NF, fb)
    x = (pcm16.astype(np.float32) / np.float32(32768.0)).reshape(NF, 2048, nch)
    want = np.concatenate([W.write_adaptive(np.zeros((1, nch, 2048), np.float32), fb), W.write_adaptive(_specs_of_pcm(x), fb)[:NF - 1]])
    assert np.array_equal(got, want)
    r = _run(exe, "-d", "-i", out, "-o", wav_out)
    assert r.returncode == 0 and "Skipped" not in r.stdout + r.stderr, r.stdout + r.stderr
    assert "Codec: ATRAC3plus, 2 channels, 64 kbit/s (376-byte frames)" in r.stdout
    dec = B.At3pHipDecoder(n_streams=1, channels=nch, max_frames=NF, frame_bytes=fb)
    try:
        lib_pcm = dec.decode(want[None], s16=True, tones=True)[0]
    finally:
        dec.close()
    with wave.open(wav_out, "rb") as w:
        assert (w.getnchannels(), w.getframerate(), w.getnframes()) == (nch, 44100, NF * 2048)
        assert np.array_equal(np.frombuffer(w.readframes(NF * 2048), "<i2").reshape(NF, 2048, nch), lib_pcm)


def test_cli_bitrate_with_tones_gate_share(B, tmp_path):
    """--bitrate 96 composes with --tones --gate --share as --adaptive does: the tone analysis' pipeline with the restatement at
    560 bytes as its frame writer; and 32 kbit/s mono"""
    NF, nch, fb = 5, 2, 560
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "at3hipenc")
    pcm16 = np.clip(np.rint(G.keyed_pcm(NF, nch) * 32767.0), -32768, 32767).astype("<i2")
    wav_in, oma, wav_out = str(tmp_path / "in.wav"), str(tmp_path / "a.oma"), str(tmp_path / "y.wav")
    _wav_in(wav_in, pcm16, nch)
    r = _run(exe, "-e", "atrac3plus", "-i", wav_in, "-o", oma, "--nostdout", "--adaptive", "--bitrate", "96", "--tones", "--gate", "--share", "--batch", "3")
    assert r.returncode == 0, r.stderr
    x = (pcm16.astype(np.float32) / np.float32(32768.0)).reshape(NF, 2048, nch)
    want, blocks, _ = G.pipeline(x, True, True, lambda specs, recs: W.write_adaptive(specs, fb, blocks=recs))
    assert sum(G.n_waves(b) for b in blocks[:-1]) > 0
    data = open(oma, "rb").read()
    assert len(data) == 96 + NF * fb and np.array_equal(np.frombuffer(data[96:], np.uint8).reshape(NF, fb), want)
    r = _run(exe, "-d", "-i", oma, "-o", wav_out)
    assert r.returncode == 0 and "Skipped" not in r.stdout + r.stderr, r.stdout + r.stderr
    mono16 = np.ascontiguousarray(pcm16.reshape(-1, nch)[:, 0])
    _wav_in(wav_in, mono16, 1)
    r = _run(exe, "-e", "atrac3plus", "-i", wav_in, "-o", oma, "--nostdout", "--adaptive", "--bitrate", "32")
    assert r.returncode == 0, r.stderr
    xm = (mono16.astype(np.float32) / np.float32(32768.0)).reshape(NF, 2048, 1)
    wm = np.concatenate([W.write_adaptive(np.zeros((1, 1, 2048), np.float32), 192), W.write_adaptive(_specs_of_pcm(xm), 192)[:NF - 1]])
    data = open(oma, "rb").read()
    assert len(data) == 96 + NF * 192 and np.array_equal(np.frombuffer(data[96:], np.uint8).reshape(NF, 192), wm)
    r = _run(exe, "-d", "-i", oma, "-o", wav_out)
    assert r.returncode == 0 and "32 kbit/s (192-byte frames)" in r.stdout and "Skipped" not in r.stdout + r.stderr, r.stdout + r.stderr
