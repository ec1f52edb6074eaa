"""Adaptive ATRAC3plus word lengths on the GPU (AT3PHIP_ALLOC_ADAPTIVE; include/at3phip.h, ADAPTIVE WORD LENGTHS): the frames of
k_at3p_write_adaptive and k_at3p_write_adaptive_tonal equal the restatement tests/host/at3p_writer_cpu.c bit for bit through
every call that takes the flag, however the stream is split into calls, from host and device buffers, waiting and queued;
without the flag the calls give the fixed writer's bytes; non-finite spectra stay in their stream; the decoder decodes the
frames; the command-line tool writes them. 2 streams x 3 frames unless said otherwise."""
import os
import subprocess
import wave

import numpy as np
import pytest

import at3p_writer_lib as W
import at3p_gha_lib as G
import at3p_tonal_lib as T
import at3p_tonal_write_lib as TW
from at3_testlib import at3p_mdct, at3p_pqf, at3p_write_frames

pytestmark = pytest.mark.gpu
S, F = 2, 3


@pytest.fixture(scope="module")
def B():
    from atracdenc_amd import binding
    return binding


def _specs(name, nch):
    """[S, F, C, 2048]: six frames of a signal's spectra, three per stream"""
    return np.ascontiguousarray(W.specs_of(name, nch, S * F).reshape(S, F, nch, 2048))


def _expect(specs, win=None, blocks=None):
    return np.stack([W.write_adaptive(specs[s], win=None if win is None else win[s], blocks=None if blocks is None else blocks[s]) for s in range(specs.shape[0])])


def _pcm(names, nch, n=F):
    """[len(names), n, 2048, C]"""
    return np.stack([G.signal_pcm(name, n, nch) for name in names])


def _specs_of_pcm(pcm):
    """pcm [n, 2048, C] of one stream from its start -> [n, C, 2048]: what at3phip_encode_frames hands its writer (oracle PQF, the
    division by 32768 / 1.122018, oracle MDCT with sine windows)"""
    out = np.zeros((pcm.shape[0], pcm.shape[2], 2048), np.float32)
    for c in range(pcm.shape[2]):
        bands = at3p_pqf(np.ascontiguousarray(pcm[:, :, c]))
        out[:, c] = at3p_mdct((bands.astype(np.float64) / G.SCALE).astype(np.float32))
    return out


WIN = np.array([[[0x01ef, 0x8001], [0xffff, 0xffff], [0, 0x00ff]], [[0x0010, 0], [0xfeff, 0x1234], [0xffff, 0]]], np.uint16)


@pytest.mark.parametrize("with_win", [False, True], ids=["sine", "win"])
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("name", ["noise", "mix", "tones", "silence", "fullscale"])
def test_write_frames_equal_the_restatement(B, name, nch, with_win):
    specs = _specs(name, nch)
    win = np.ascontiguousarray(WIN[:, :, :nch]) if with_win else None
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    try:
        got = enc.write_frames(specs, win, adaptive=True)
    finally:
        enc.close()
    assert np.array_equal(got, _expect(specs, win))


@pytest.mark.parametrize("nch", [1, 2])
def test_write_frames_tonal_equal_the_restatement(B, nch):
    """records beside frames without one, the largest record on full-scale noise among them, with window flags"""
    blocks = [[TW.largest_block(nch), None, TW.case_blocks(f"small_{nch}")[0][0]], [TW.case_blocks(f"random_{nch}")[0][0], TW.largest_block(nch, 1), None]]
    specs = np.stack([W.full_scale_noise(F, nch, seed=4), W.specs_of("mix", nch, F)])
    win = np.ascontiguousarray(WIN[:, :, :nch])
    recs = np.stack([B.pack_tonal_blocks(row, nch) for row in blocks])
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    try:
        got = enc.write_frames(specs, win, recs, adaptive=True)
        plain = enc.write_frames(specs, win, recs)
    finally:
        enc.close()
    assert np.array_equal(got, _expect(specs, win, blocks))
    assert (got != plain).any(axis=2).all()
    pcm, rej = T.cpu_tonal_decode(got[0], nch, tones=True)
    assert rej.sum() == 0


@pytest.mark.parametrize("nch", [1, 2])
def test_encode_frames_and_s16_equal_the_restatement(B, nch):
    pcm = _pcm(("mix", "noise"), nch)
    p16 = np.clip(np.rint(pcm * 32767.0), -32768, 32767).astype(np.int16)
    as_float = (p16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    try:
        got = enc.encode_frames(pcm, adaptive=True)
        enc.reset()
        got16 = enc.encode_frames_s16(p16, adaptive=True)
    finally:
        enc.close()
    assert np.array_equal(got, np.stack([W.write_adaptive(_specs_of_pcm(pcm[s])) for s in range(S)]))
    assert np.array_equal(got16, np.stack([W.write_adaptive(_specs_of_pcm(as_float[s])) for s in range(S)]))


@pytest.mark.parametrize("gated,shared", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("nch", [1, 2])
def test_encode_frames_tonal_equal_the_restatement(B, nch, gated, shared):
    """the tone analysis' pipeline (tests/at3p_gha_lib.py) with the restatement as its frame writer; stereo: both channels alike, so
    that sharing has bands to share"""
    pcm = np.stack([G.twin_pcm("tones", F), G.keyed_pcm(F, 2)]) if nch == 2 else np.stack([G.signal_pcm("tones", F, 1), G.keyed_pcm(F, 1)])
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    try:
        got = enc.encode_frames_tonal(pcm, gated=gated, shared=shared, adaptive=True)
    finally:
        enc.close()
    waves = 0
    for s in range(S):
        frames, blocks, _ = G.pipeline(pcm[s], gated, shared, write=lambda specs, recs: W.write_adaptive(specs, blocks=recs))
        waves += sum(G.n_waves(b) for b in blocks[:-1])
        assert np.array_equal(got[s], frames), s
    assert waves > 0


@pytest.mark.parametrize("nch", [1, 2])
def test_call_splits_device_buffers_and_queued_calls(B, nch):
    """one call of 3 frames = three calls of 1 frame; host buffers = device buffers; a queued call = a waiting call"""
    import torch
    pcm = _pcm(("mix", "burst"), nch)
    specs = _specs("noise", nch)
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    try:
        whole = enc.encode_frames(pcm, adaptive=True)
        enc.reset()
        parts = np.concatenate([enc.encode_frames(pcm[:, f:f + 1], adaptive=True) for f in range(F)], axis=1)
        w_whole = enc.write_frames(specs, adaptive=True)
        w_parts = np.concatenate([enc.write_frames(specs[:, f:f + 1], adaptive=True) for f in range(F)], axis=1)
        d_pcm, d_out, d_q = torch.from_numpy(pcm).cuda(), torch.zeros((S, F, 2048), dtype=torch.uint8, device="cuda"), torch.zeros((S, F, 2048), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        enc.reset()
        enc.encode_frames_device(d_pcm.data_ptr(), F, d_out.data_ptr(), adaptive=True)
        enc.reset()
        enc.encode_frames_device(d_pcm.data_ptr(), F, d_q.data_ptr(), asynchronous=True, adaptive=True)
        enc.sync()
    finally:
        enc.close()
    assert np.array_equal(whole, parts) and np.array_equal(w_whole, w_parts)
    assert np.array_equal(d_out.cpu().numpy(), whole) and np.array_equal(d_q.cpu().numpy(), whole)
    assert np.array_equal(whole, np.stack([W.write_adaptive(_specs_of_pcm(pcm[s])) for s in range(S)]))


@pytest.mark.parametrize("nch", [1, 2])
def test_without_the_flag_the_fixed_writers_bytes(B, nch):
    """the same calls on a context that has just written adaptive frames: the oracle writer's frames"""
    specs, pcm = _specs("mix", nch), _pcm(("mix", "noise"), nch)
    win = np.ascontiguousarray(WIN[:, :, :nch])
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    try:
        enc.write_frames(specs, win, adaptive=True)
        got_w = enc.write_frames(specs, win)
        enc.encode_frames(pcm, adaptive=True)
        enc.reset()
        got_e = enc.encode_frames(pcm)
    finally:
        enc.close()
    assert np.array_equal(got_w, np.stack([at3p_write_frames(specs[s], win[s]) for s in range(S)]))
    assert np.array_equal(got_e, np.stack([at3p_write_frames(_specs_of_pcm(pcm[s])) for s in range(S)]))


@pytest.mark.parametrize("cid", ["small_1", "steep_1", "steep_2", "share_a_2", "loud_2"])
def test_without_the_flag_write_frames_tonal_gives_the_references_bytes(B, cid):
    """k_at3p_write_tonal in the library that also holds the adaptive kernels, on a context that has just written adaptive frames
    with the same records: the reference's frames of tests/golden/at3p_tonal_write.npz (tests/test_at3p_tonal_write_gpu.py's
    cases: one wave, 48 waves, window flags, sharing, loud spectra that lose units to the block)"""
    g = np.load(TW.GOLDEN)
    nch = int(cid.rsplit("_", 1)[1])
    blocks = TW.blocks_from_ints(nch, g[f"{cid}_blocks"])
    flags = g[f"{cid}_flags"] if f"{cid}_flags" in g else None
    specs, recs = TW.case_specs(cid, int(g[f"{cid}_seed"])), B.pack_tonal_blocks(blocks, nch)
    enc = B.At3pHip(n_streams=TW.STREAMS, max_frames=TW.FRAMES, channels=nch)
    try:
        adaptive = enc.write_frames(specs, flags, recs, adaptive=True)
        plain = enc.write_frames(specs, flags, recs)
    finally:
        enc.close()
    assert np.array_equal(plain, g[f"{cid}_frames"])
    assert (adaptive != plain).any(axis=2).all()
    assert np.array_equal(adaptive, _expect(specs, flags, blocks))


@pytest.mark.parametrize("gated,shared", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("nch", [1, 2])
def test_without_the_flag_encode_frames_tonal_gives_the_parents_bytes(B, nch, gated, shared):
    """at3phip_encode_frames_tonal without the flag, after the same call with it: the tone analysis' pipeline (tests/at3p_gha_lib.py)
    around the fixed writer - mono: the oracle's writer with the block spliced in; stereo: at3phip_write_frames_tonal without the
    flag, which prices the block and is pinned to the reference above"""
    pcm = np.stack([G.twin_pcm("tones", F), G.keyed_pcm(F, 2)]) if nch == 2 else np.stack([G.signal_pcm("tones", F, 1), G.keyed_pcm(F, 1)])
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    one = B.At3pHip(n_streams=1, max_frames=F, channels=nch)
    try:
        with_flag = enc.encode_frames_tonal(pcm, gated=gated, shared=shared, adaptive=True)
        enc.reset()
        got = enc.encode_frames_tonal(pcm, gated=gated, shared=shared)
        write = None if nch == 1 else (lambda specs, recs: one.write_frames(specs[None], None, recs[None])[0])
        want = np.stack([G.pipeline(pcm[s], gated, shared, write)[0] for s in range(S)])
    finally:
        enc.close()
        one.close()
    assert np.array_equal(got, want)
    assert (with_flag != got).any()


@pytest.mark.parametrize("nch", [1, 2])
def test_non_finite_spectra_stay_in_their_stream(B, nch):
    """NaN, +-inf and +-FLT_MAX, a unit of nothing but NaN, beside a normal stream: the call returns, the normal stream's frames are
    what they are alone, the odd stream's frames equal the restatement's"""
    normal = W.specs_of("noise", nch, F)
    specs = np.stack([W.odd_specs(nch, F), normal])
    enc = B.At3pHip(n_streams=S, max_frames=F, channels=nch)
    try:
        got = enc.write_frames(specs, adaptive=True)
        alone = enc.write_frames(np.stack([normal, normal]), adaptive=True)
    finally:
        enc.close()
    assert np.array_equal(got[1], alone[0]) and np.array_equal(got[1], W.write_adaptive(normal))
    assert np.array_equal(got[0], W.write_adaptive(specs[0]))


@pytest.mark.parametrize("nch", [1, 2])
def test_decoder_decodes_the_adaptive_frames(B, nch):
    NF = 6
    pcm = _pcm(("mix", "tones"), nch, NF)
    enc = B.At3pHip(n_streams=S, max_frames=NF, channels=nch)
    dec = B.At3pHipDecoder(n_streams=S, channels=nch, max_frames=NF)
    try:
        frames = enc.encode_frames(pcm, adaptive=True)
        out = dec.decode(frames)
        assert sum(dec.counters().values()) == 0
    finally:
        enc.close()
        dec.close()
    for s in range(S):
        want, rej = T.cpu_tonal_decode(frames[s], nch)
        assert rej.sum() == 0 and np.array_equal(out[s].view(np.uint32), want.view(np.uint32))


def _oma_frames(path):
    data = open(path, "rb").read()
    assert data[:3] == b"EA3"
    body = data[96:]
    return np.frombuffer(body[:len(body) // 2048 * 2048], np.uint8).reshape(-1, 2048)


@pytest.mark.parametrize("nch", [1, 2])
def test_cli_adaptive(B, tmp_path, nch):
    NF = 6
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "at3hipenc")
    pcm16 = np.clip(np.rint(G.signal_pcm("mix", NF, nch) * 32767.0), -32768, 32767).astype("<i2")
    wav_in, oma, wav_out = str(tmp_path / "in.wav"), str(tmp_path / "a.oma"), str(tmp_path / "y.wav")
    with wave.open(wav_in, "wb") as w:
        w.setnchannels(nch)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(pcm16.tobytes())
    r = subprocess.run([exe, "-e", "atrac3plus", "-i", wav_in, "-o", oma, "--nostdout", "--adaptive", "--batch", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = _oma_frames(oma)
    # the tool's schedule: the silent frame of the look-ahead, then the input's frames; its reader hands over int16 / 32768
    x = (pcm16.astype(np.float32) / np.float32(32768.0)).reshape(NF, 2048, nch)
    want = np.concatenate([W.write_adaptive(np.zeros((1, nch, 2048), np.float32)), W.write_adaptive(_specs_of_pcm(x))[:NF - 1]])
    assert got.shape == (NF, 2048) and np.array_equal(got, want)
    r = subprocess.run([exe, "-d", "-i", oma, "-o", wav_out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Skipped" not in r.stdout + r.stderr, r.stdout + r.stderr
    r = subprocess.run([exe, "-e", "atrac3", "-i", wav_in, "-o", str(tmp_path / "b.oma"), "--adaptive"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "usage:" in r.stderr and not os.path.exists(str(tmp_path / "b.oma"))
    r = subprocess.run([exe, "-d", "-i", oma, "-o", str(tmp_path / "z.wav"), "--adaptive"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "usage:" in r.stderr   # the flag belongs to the ATRAC3plus encoder alone


@pytest.mark.parametrize("nch,extra", [(1, ["--tones"]), (2, ["--tones", "--gate"]), (2, ["--tones", "--share"]), (2, ["--tones", "--gate", "--share"])],
                         ids=["tones_1", "gate_2", "share_2", "gate_share_2"])
def test_cli_adaptive_with_tones(B, tmp_path, nch, extra):
    """--adaptive with --tones [--gate] [--share] on `keyed` (both channels alike in stereo, so that there are onsets to gate and
    bands to share): the file's frames are the tone analysis' pipeline with the restatement as its frame writer, and decode"""
    NF = 5
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "at3hipenc")
    pcm16 = np.clip(np.rint(G.keyed_pcm(NF, nch) * 32767.0), -32768, 32767).astype("<i2")
    wav_in, oma, wav_out = str(tmp_path / "in.wav"), str(tmp_path / "a.oma"), str(tmp_path / "y.wav")
    with wave.open(wav_in, "wb") as w:
        w.setnchannels(nch)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(pcm16.tobytes())
    r = subprocess.run([exe, "-e", "atrac3plus", "-i", wav_in, "-o", oma, "--nostdout", "--adaptive", *extra, "--batch", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    x = (pcm16.astype(np.float32) / np.float32(32768.0)).reshape(NF, 2048, nch)
    want, blocks, _ = G.pipeline(x, "--gate" in extra, "--share" in extra, lambda specs, recs: W.write_adaptive(specs, blocks=recs))
    assert sum(G.n_waves(b) for b in blocks[:-1]) > 0
    assert np.array_equal(_oma_frames(oma), want)
    r = subprocess.run([exe, "-d", "-i", oma, "-o", wav_out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Skipped" not in r.stdout + r.stderr, r.stdout + r.stderr


def test_largest_shape(B):
    """the create-time limit of tests/test_large_shapes_gpu.py's ATRAC3plus encoder test: mono, 65535 streams x 9 frames
    (gridDim.y = 65535 in the front end, 589815 workgroups in the writer; PCM and spectra 4.83e9 bytes each). The first and the
    last streams' frames against the restatement, a sample of the rest against the copies they are."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 32 << 30:
        pytest.skip(f"needs 32 GiB of free device memory, {free / 2 ** 30:.1f} GiB free")
    big_s, nf, P = 65535, 9, 5
    pcm = _pcm(("mix", "noise", "tones", "silence", "burst"), 1, nf)           # stream s = copy s % P
    small = torch.from_numpy(pcm).cuda()
    big_in = torch.empty((big_s, nf, 2048, 1), dtype=torch.float32, device="cuda")
    for r in range(P):
        big_in[r::P] = small[r]
    out = torch.full((big_s, nf, 2048), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    enc = B.At3pHip(n_streams=big_s, max_frames=nf, channels=1)
    try:
        enc.encode_frames_device(big_in.data_ptr(), nf, out.data_ptr(), adaptive=True)
    finally:
        enc.close()
    want = np.stack([W.write_adaptive(_specs_of_pcm(pcm[r])) for r in range(P)])
    assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[big_s - 1].cpu().numpy(), want[(big_s - 1) % P])
    ref = torch.from_numpy(want).cuda()
    for r in range(P):
        assert bool((out[r::P] == ref[r]).all()), r
    del big_in, out, small, ref
    torch.cuda.empty_cache()
