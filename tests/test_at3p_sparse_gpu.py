"""ATRAC3plus sparse word lengths on the GPU (AT3PHIP_ALLOC_SPARSE, AT3PHIP_DECODE_SPARSE; include/at3phip.h, SPARSE WORD LENGTHS):
the six frame-writing calls with ADAPTIVE | SPARSE and at3phip_decode with the decoder flag equal the restatement
tests/host/at3p_writer_cpu.c bit for bit - host and device buffers, queued and waiting, however the stream is split -; SPARSE
without ADAPTIVE is refused and moves nothing; crafted frames are counted as the restatement counts them; a context that wrote
sparse frames writes the unflagged ones it always wrote; the command line composes --sparse with --bitrate and the tone analysis.
3 streams x 5 frames; what does not depend on the frame size (spectra, tone analysis) is computed once."""
import os
import subprocess
import wave

import numpy as np
import pytest

import at3p_writer_lib as W
import at3p_gha_lib as G
import at3p_tonal_write_lib as TW
from at3_testlib import at3p_mdct, at3p_pqf

pytestmark = pytest.mark.gpu
S, F = 3, 5
CASES = [(1, 176), (1, 376), (1, 2048), (2, 224), (2, 376), (2, 2048)]
IDS = [f"{'mono' if nch == 1 else 'stereo'}_{fb}" for nch, fb in CASES]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def B():
    from atracdenc_amd import binding
    return binding


def _as16(pcm):
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


def _plain(nch):
    """(int16 PCM [S, F, 2048, C], the same as float, the writer's spectra [S, F, C, 2048]) of noise (k extends N), tones (zeros
    between coded units) and mix"""
    if ("plain", nch) not in _cache:
        p16, pcm = _as16(np.stack([G.signal_pcm(name, F, nch) for name in ("noise", "tones", "mix")]))
        _cache[("plain", nch)] = (p16, pcm, np.stack([_specs_of_pcm(pcm[s]) for s in range(S)]))
    return _cache[("plain", nch)]


def _tonal(nch):
    """(int16 PCM, float PCM, residual spectra, the writer's records) of the tone analysis with gates and sharing"""
    if ("tonal", nch) not in _cache:
        raw = [G.twin_pcm("tones", F), G.keyed_pcm(F, 2), G.twin_pcm("mix", F)] if nch == 2 else \
            [G.signal_pcm("tones", F, 1), G.keyed_pcm(F, 1), G.signal_pcm("mix", F, 1)]
        p16, pcm = _as16(np.stack(raw))
        specs, recs = [], []

        def grab(sp, rc):
            specs.append(sp)
            recs.append(rc)
            return np.zeros((sp.shape[0], 2048), np.uint8)
        for s in range(S):
            G.pipeline(pcm[s], True, True, grab)
        _cache[("tonal", nch)] = (p16, pcm, np.stack(specs), np.stack(recs))
    return _cache[("tonal", nch)]


def _wspecs(nch):
    """spectra for the writer calls: noise, a stream with NaN, infinities and FLT_MAX beside normal ones, tones"""
    return np.stack([W.specs_of("noise", nch, F), np.concatenate([W.odd_specs(nch, 3), W.specs_of("mix", nch, F - 3)]), W.specs_of("tones", nch, F)])


def _records(nch):
    small = TW.case_blocks(f"small_{nch}")[0][0]
    return [[TW.largest_block(nch), None, small, None, small], [None, TW.largest_block(nch), None, None, small], [None, small, None, None, None]]


def _sparse_frames(nch, fb):
    """the frames of the writer call on _wspecs with records, from the restatement; zeros inside the coded range among them"""
    key = ("frames", nch, fb)
    if key not in _cache:
        w, blocks = _wspecs(nch), _records(nch)
        out = [W.write_adaptive(w[s], fb, True, None, blocks[s], info=True) for s in range(S)]
        _cache[key] = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]))
    return _cache[key]


# ---- the writers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,fb", CASES, ids=IDS)
def test_six_calls_equal_the_restatement(B, nch, fb):
    """host buffers: at3phip_write_frames, at3phip_write_frames_tonal, at3phip_encode_frames(_short), at3phip_encode_frames_tonal(_short)"""
    p16, pcm, specs = _plain(nch)
    t16, tpcm, tspecs, trecs = _tonal(nch)
    wspecs, blocks = _wspecs(nch), _records(nch)
    recs = np.stack([B.pack_tonal_blocks(row, nch) for row in blocks])
    kw = dict(adaptive=True, sparse=True)
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, frame_bytes=fb)
    try:
        got_w = enc.write_frames(wspecs, **kw)
        got_t = enc.write_frames(wspecs, None, recs, **kw)
        got_e = enc.encode_frames(pcm, **kw)
        enc.reset()
        got_e16 = enc.encode_frames_s16(p16, **kw)
        enc.reset()
        got_a = enc.encode_frames_tonal(tpcm, gated=True, shared=True, **kw)
        enc.reset()
        got_a16 = enc.encode_frames_tonal_s16(t16, gated=True, shared=True, **kw)
    finally:
        enc.close()
    want_w, info = W.write_streams(wspecs, fb, True), _sparse_frames(nch, fb)[1]
    assert np.array_equal(got_w, want_w)
    assert np.array_equal(got_t, _sparse_frames(nch, fb)[0])
    want_e = W.write_streams(specs, fb, True)
    assert np.array_equal(got_e, want_e) and np.array_equal(got_e16, want_e)
    want_a = np.stack([W.write_adaptive(tspecs[s], fb, True, None, trecs[s]) for s in range(S)])
    assert np.array_equal(got_a, want_a) and np.array_equal(got_a16, want_a)
    if fb < 2048:   # the flag matters at these sizes: the frames are not the adaptive writer's, and hold zeros inside the range
        assert not np.array_equal(want_e, W.write_streams(specs, fb))
        assert any((info["wl"][s, f, c, :info["num_quant_units"][s, f]] == 0).any() for s in range(S) for f in range(F) for c in range(nch))


@pytest.mark.parametrize("nch,fb", CASES, ids=IDS)
def test_device_buffers_queued_calls_and_splits(B, nch, fb):
    """device buffers waiting and queued, one call of 5 frames against calls of 2 + 3; the bytes behind every output stay"""
    import torch
    p16, pcm, specs = _plain(nch)
    t16, tpcm, tspecs, trecs = _tonal(nch)
    want = W.write_streams(specs, fb, True)
    t_want = np.stack([W.write_adaptive(tspecs[s], fb, True, None, trecs[s]) for s in range(S)])
    n = S * F * fb
    DEV = B.AT3HIP_PCM_ON_DEVICE | B.AT3HIP_OUT_ON_DEVICE | B.AT3PHIP_ALLOC_ADAPTIVE | B.AT3PHIP_ALLOC_SPARSE
    kw = dict(adaptive=True, sparse=True)
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch, frame_bytes=fb)
    try:
        d_pcm, d_specs, d_t16 = torch.from_numpy(pcm).cuda(), torch.from_numpy(specs).cuda(), torch.from_numpy(t16).cuda()
        outs = [torch.full((n + 4096,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        enc.encode_frames_device(d_pcm.data_ptr(), F, outs[0].data_ptr(), **kw)
        enc.reset()
        enc.encode_frames_device(d_pcm.data_ptr(), F, outs[1].data_ptr(), asynchronous=True, **kw)
        enc.sync()
        enc.write_frames_ptr(d_specs.data_ptr(), F, None, outs[2].data_ptr(), DEV)
        enc.reset()
        enc.encode_frames_tonal_device_s16(d_t16.data_ptr(), F, outs[3].data_ptr(), asynchronous=True, gated=True, shared=True, **kw)
        enc.sync()

        def split(call, x, **k2):
            enc.reset()
            return np.concatenate([call(x[:, :2], **k2), call(x[:, 2:], **k2)], axis=1)
        parts = split(enc.encode_frames, pcm, **kw)
        t_parts = split(enc.encode_frames_tonal, tpcm, gated=True, shared=True, **kw)
        w_parts = np.concatenate([enc.write_frames(specs[:, :2], **kw), enc.write_frames(specs[:, 2:], **kw)], axis=1)
    finally:
        enc.close()
    got = [o.cpu().numpy() for o in outs]
    for g in got:
        assert (g[n:] == SENTINEL).all()
    for k in range(3):
        assert np.array_equal(got[k][:n].reshape(S, F, fb), want), k
    assert np.array_equal(got[3][:n].reshape(S, F, fb), t_want)
    assert np.array_equal(parts, want) and np.array_equal(w_parts, want) and np.array_equal(t_parts, t_want)


@pytest.mark.parametrize("nch", [1, 2])
def test_special_cases_of_the_allocation(B, nch):
    """at3p_writer_lib.edge_specs at the smallest frame size: the empty frame (unit 0 of channel 0 takes 1), N = 32 with unit 31 of
    channel 0 at 1 above zeros, clone flags, the flat case - each checked to have occurred in the restatement's record - written
    by at3phip_write_frames_tonal and decoded by at3phip_decode, against the restatement"""
    fb = W.MIN_BYTES[nch]
    sp, blocks = W.edge_specs(nch)
    want, rec, _ = W.write_adaptive(sp, fb, True, None, blocks, info=True)
    assert W.edge_cases_reached(rec, nch) == []
    enc = B.At3pHip(n_streams=1, max_frames=4, channels=nch, frame_bytes=fb)
    dec = B.At3pHipDecoder(n_streams=1, channels=nch, max_frames=4, frame_bytes=fb)
    try:
        got = enc.write_frames(sp[None], None, B.pack_tonal_blocks(blocks, nch)[None], adaptive=True, sparse=True)
        pcm = dec.decode(want[None], tones=True, sparse=True)
        cnt = dec.counters()
    finally:
        enc.close()
        dec.close()
    assert np.array_equal(got[0], want)
    wpcm, rej = W.decode(want, nch, True, True)
    assert rej.sum() == 0 == sum(cnt.values()) and np.array_equal(pcm[0].view(np.uint32), wpcm.view(np.uint32))


@pytest.mark.parametrize("nch", [1, 2])
def test_sparse_alone_is_refused_and_moves_nothing(B, nch):
    """AT3PHIP_ALLOC_SPARSE without AT3PHIP_ALLOC_ADAPTIVE on all six calls: AT3HIP_EINVAL with a last-error text, the output untouched,
    and the next valid call gives the bytes of a fresh context (no filter-bank or analysis state moved)"""
    p16, pcm, specs = _plain(nch)
    recs = np.zeros((S, F), B.AT3P_TONAL_BLOCK_DTYPE)
    out = np.full((S, F, 2048), SENTINEL, np.uint8)
    flag = B.AT3PHIP_ALLOC_SPARSE
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    try:
        calls = [lambda: enc.write_frames_ptr(specs.ctypes.data, F, None, out.ctypes.data, flag),
                 lambda: enc.write_frames_tonal_ptr(specs.ctypes.data, F, None, recs.ctypes.data, out.ctypes.data, flag),
                 lambda: enc.encode_frames_ptr(pcm.ctypes.data, F, out.ctypes.data, flag),
                 lambda: enc.encode_frames_s16_ptr(p16.ctypes.data, F, out.ctypes.data, flag),
                 lambda: enc.encode_frames_tonal_ptr(pcm.ctypes.data, F, out.ctypes.data, flag),
                 lambda: enc.encode_frames_tonal_s16_ptr(p16.ctypes.data, F, out.ctypes.data, flag)]
        for k, call in enumerate(calls):
            with pytest.raises(B.At3HipError, match="AT3PHIP_ALLOC_SPARSE needs AT3PHIP_ALLOC_ADAPTIVE"):
                call()
            assert (out == SENTINEL).all(), k
        with pytest.raises(ValueError):
            enc.encode_frames(pcm, sparse=True)
        got = enc.encode_frames(pcm, adaptive=True, sparse=True)
        got_t = None
        enc.reset()
        got_t = enc.encode_frames_tonal(pcm, adaptive=True, sparse=True)
    finally:
        enc.close()
    fresh = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    try:
        want_t = fresh.encode_frames_tonal(pcm, adaptive=True, sparse=True)
    finally:
        fresh.close()
    assert np.array_equal(got, W.write_streams(specs, 2048, True)) and np.array_equal(got_t, want_t)


@pytest.mark.parametrize("nch", [1, 2])
def test_unflagged_frames_after_sparse_ones_equal_a_fresh_context(B, nch):
    p16, pcm, specs = _plain(nch)
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    try:
        enc.set_frame_bytes(376)
        enc.encode_frames(pcm, adaptive=True, sparse=True)
        enc.set_frame_bytes(2048)
        enc.reset()
        fixed = enc.encode_frames(pcm)
        enc.reset()
        adaptive = enc.encode_frames(pcm, adaptive=True)
        w_fixed, w_adaptive = enc.write_frames(specs), enc.write_frames(specs, adaptive=True)
    finally:
        enc.close()
    fresh = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    try:
        assert np.array_equal(fixed, fresh.encode_frames(pcm))
        fresh.reset()
        assert np.array_equal(adaptive, fresh.encode_frames(pcm, adaptive=True))
        assert np.array_equal(w_fixed, fresh.write_frames(specs)) and np.array_equal(w_adaptive, fresh.write_frames(specs, adaptive=True))
    finally:
        fresh.close()
    assert np.array_equal(adaptive, W.write_streams(specs, 2048))


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,fb", CASES, ids=IDS)
def test_decoder_equals_the_restatement(B, nch, fb):
    """the sparse frames (records among them) through at3phip_decode with AT3PHIP_DECODE_SPARSE: float and int16, with and without
    tones, one call against 2 + 3; without the flag the same frames are rejected with the restatement's counters"""
    frames = _sparse_frames(nch, fb)[0]
    dec = B.At3pHipDecoder(n_streams=S, channels=nch, max_frames=F, frame_bytes=fb)
    try:
        for tones in (True, False):
            for sparse in (True, False):
                want, rej = W.decode_streams(frames, nch, tones, sparse)
                dec.reset()
                got = dec.decode(frames, tones=tones, sparse=sparse)
                cnt = dec.counters(reset=True)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tones, sparse)
                assert list(cnt.values()) == rej.tolist(), (tones, sparse, cnt, rej)
                if sparse and tones:
                    assert rej.sum() == 0
                if not sparse and fb < 2048:
                    assert rej[3] > 0   # bad_code: a word length of 0
            want, _ = W.decode_streams(frames, nch, tones, True)
            dec.reset()
            parts = np.concatenate([dec.decode(frames[:, :2], tones=tones, sparse=True), dec.decode(frames[:, 2:], tones=tones, sparse=True)], axis=1)
            assert np.array_equal(parts.view(np.uint32), want.view(np.uint32))
            dec.reset()
            s16 = dec.decode(frames, s16=True, tones=tones, sparse=True)
            assert np.array_equal(s16, np.rint(want * np.float32(32767.0)).astype(np.int16))
    finally:
        dec.close()


@pytest.mark.parametrize("nch", [1, 2])
def test_crafted_frames_beside_good_ones(B, nch):
    """clone flag 0 (stereo) and top unit zero in every channel: counters and PCM of the restatement, beside good frames in the same
    call. (The frame cut inside the code-table section of tests/test_at3p_sparse_cpu.py needs a frame of under 100 bytes, which
    at3phip_decoder_set_frame_bytes does not admit.)"""
    fb = 376
    good = _sparse_frames(nch, fb)[0][0]
    bad = W.crafted_frames(nch, fb)
    frames = np.stack([good, np.concatenate([bad, good[:F - len(bad)]])[:F], good[::-1].copy()])
    want, rej = W.decode_streams(frames, nch, True, True)
    dec = B.At3pHipDecoder(n_streams=S, channels=nch, max_frames=F, frame_bytes=fb)
    try:
        got = dec.decode(frames, tones=True, sparse=True)
        cnt = dec.counters()
    finally:
        dec.close()
    assert list(cnt.values()) == rej.tolist() and rej[1] == len(bad) and rej.sum() == len(bad), (cnt, rej)
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


def test_cli_sparse(B, tmp_path):
    """on a 0.5 s WAV: --adaptive --sparse --bitrate 64, then -d, equals the binding's path; --sparse alone is a usage error that says
    why; --tones --gate --share --adaptive --sparse --bitrate 96 runs and decodes with no rejected frame"""
    NF, nch, fb = 11, 2, 376
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "at3hipenc")
    pcm16 = np.clip(np.rint(G.signal_pcm("noise", NF, nch) * 32767.0), -32768, 32767).astype("<i2")
    wav_in, oma, wav_out = str(tmp_path / "in.wav"), str(tmp_path / "a.oma"), str(tmp_path / "y.wav")
    _wav_in(wav_in, pcm16, nch)
    r = _run(exe, "-e", "atrac3plus", "-i", wav_in, "-o", oma, "--sparse", "--bitrate", "352")
    assert r.returncode != 0 and "--sparse needs --adaptive" in r.stderr and not os.path.exists(oma), r.stdout + r.stderr
    r = _run(exe, "-e", "atrac3plus", "-i", wav_in, "-o", oma, "--adaptive", "--sparse", "--bitrate", "64", "--batch", "4")
    assert r.returncode == 0 and "Bitrate: 64 kbit/s (376-byte frames)" in r.stdout, r.stdout + r.stderr
    data = open(oma, "rb").read()
    assert len(data) == 96 + NF * fb
    got = np.frombuffer(data[96:], np.uint8).reshape(NF, fb)
    x = (pcm16.astype(np.float32) / np.float32(32768.0)).reshape(1, NF, 2048, nch)
    enc = B.At3pHip(n_streams=1, max_frames=NF, channels=nch, frame_bytes=fb)
    dec = B.At3pHipDecoder(n_streams=1, channels=nch, max_frames=NF, frame_bytes=fb)
    try:
        lib_frames = enc.encode_frames(x, adaptive=True, sparse=True)[0]
        want = np.concatenate([W.write_adaptive(np.zeros((1, nch, 2048), np.float32), fb, True), lib_frames[:NF - 1]])   # the host's one-frame lead-in
        assert np.array_equal(got, want)
        assert W.decode(want, nch, True, False)[1][3] > 0   # the file holds word length 0 inside the range
        lib_pcm = dec.decode(want[None], s16=True, tones=True, sparse=True)[0]
    finally:
        enc.close()
        dec.close()
    r = _run(exe, "-d", "-i", oma, "-o", wav_out)
    assert r.returncode == 0 and "Skipped" not in r.stdout + r.stderr, r.stdout + r.stderr
    with wave.open(wav_out, "rb") as w:
        assert np.array_equal(np.frombuffer(w.readframes(NF * 2048), "<i2").reshape(NF, 2048, nch), lib_pcm)
    r = _run(exe, "-e", "atrac3plus", "-i", wav_in, "-o", oma, "--nostdout", "--tones", "--gate", "--share", "--adaptive", "--sparse", "--bitrate", "96")
    assert r.returncode == 0 and len(open(oma, "rb").read()) == 96 + NF * 560, r.stderr
    r = _run(exe, "-d", "-i", oma, "-o", wav_out)
    assert r.returncode == 0 and "Skipped" not in r.stdout + r.stderr, r.stdout + r.stderr
