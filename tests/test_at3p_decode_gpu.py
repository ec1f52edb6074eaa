"""The ATRAC3plus decoder on the GPU (include/at3phip.h, decoder section): goldens bit for bit, seeded fuzzing against the C
restatement, call splits, device tensors and queued calls, s16 output, a long stream, bad arguments, the encoder round trip and
the command line's encode-then-decode."""
import os
import subprocess
import wave

import numpy as np
import pytest

from at3_testlib import at3p_signal, pin_digest
from at3p_decode_lib import DELAY, GOLDEN, REASONS, CpuDecoder, cpu_decode, fuzz_streams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return g, [str(c) for c in g["cases"]]


def _dec(nch, n_streams=1, max_frames=64):
    import atracdenc_amd
    return atracdenc_amd.At3pHipDecoder(n_streams=n_streams, channels=nch, max_frames=max_frames, device_id=0)


def test_goldens_bit_identical(golden):
    g, names = golden
    for nch in (1, 2):
        cases = [n for n in names if int(g[f"{n}_channels"]) == nch]
        nf = max(g[f"{n}_frames"].shape[0] for n in cases)
        # every case of this channel count side by side as its own stream, padded with silence frames past its end
        frames = np.zeros((len(cases), nf, 2048), np.uint8)
        pad = cpu_frames_silence(nch)
        for i, n in enumerate(cases):
            fr = g[f"{n}_frames"]
            frames[i, :fr.shape[0]] = fr
            frames[i, fr.shape[0]:] = pad
        dec = _dec(nch, n_streams=len(cases), max_frames=nf)
        pcm = dec.decode(frames)
        counters = dec.counters()
        dec.close()
        want = np.zeros(len(REASONS), np.int64)
        for i, n in enumerate(cases):
            k = g[f"{n}_frames"].shape[0]
            assert np.array_equal(pin_digest(pcm[i, :k]), g[f"{n}_pcm_sha256"]), n
            if f"{n}_pcm" in g:
                assert np.array_equal(pcm[i, :k].view(np.uint32), g[f"{n}_pcm"].view(np.uint32)), n
            want += g[f"{n}_rejected"]
        assert [counters[r] for r in REASONS] == want.tolist(), (counters, want)


def cpu_frames_silence(nch):
    """one valid silent frame (what the oracle writer makes of a zero spectrum)"""
    from at3_testlib import at3p_write_frames
    return at3p_write_frames(np.zeros((1, nch, 2048), np.float32))[0]


@pytest.mark.parametrize("nch", [1, 2])
def test_fuzz_equals_restatement(golden, nch):
    g, names = golden
    frames = fuzz_streams(g, names, nch)
    dec = _dec(nch, n_streams=frames.shape[0], max_frames=frames.shape[1])
    got = dec.decode(frames)
    counters = dec.counters()
    dec.close()
    total = np.zeros(len(REASONS), np.int64)
    for i in range(frames.shape[0]):
        want, rej = cpu_decode(frames[i], nch)
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), i
        total += rej
    assert [counters[r] for r in REASONS] == total.tolist()


def test_splits_reset_and_counters(golden):
    g, names = golden
    frames = np.concatenate([g["sig_mix_2ch_frames"], g["win_alternating_2ch_frames"], g["crafted_2ch_frames"]])[None]
    dec = _dec(2, max_frames=frames.shape[1])
    whole = dec.decode(frames)
    c_whole = dec.counters(reset=True)
    dec.reset()
    assert all(v == 0 for v in dec.counters().values())
    rng = np.random.default_rng(5)
    for _ in range(3):
        dec.reset()
        cuts = np.sort(rng.choice(np.arange(1, frames.shape[1]), 4, replace=False))
        parts = [dec.decode(frames[:, a:b]) for a, b in zip(np.r_[0, cuts], np.r_[cuts, frames.shape[1]])]
        assert np.array_equal(np.concatenate(parts, axis=1).view(np.uint32), whole.view(np.uint32))
        assert dec.counters(reset=True) == c_whole
    # one frame per call
    dec.reset()
    one = np.concatenate([dec.decode(frames[:, k:k + 1]) for k in range(frames.shape[1])], axis=1)
    assert np.array_equal(one.view(np.uint32), whole.view(np.uint32))
    dec.close()
    want, rej = cpu_decode(frames[0], 2)
    assert np.array_equal(whole[0].view(np.uint32), want.view(np.uint32))
    assert [c_whole[r] for r in REASONS] == rej.tolist()


def test_device_tensors_ordered_and_queued(golden):
    import torch
    g, _ = golden
    frames = np.stack([g["sig_mix_2ch_frames"], g["sig_burst_2ch_frames"]])
    dec = _dec(2, n_streams=2, max_frames=frames.shape[1])
    want = dec.decode(frames)
    dev = torch.device("cuda:0")
    for ordered in (True, False):
        dec.reset()
        src = torch.from_numpy(frames).to(dev)
        out = torch.empty((2, frames.shape[1], 2048, 2), dtype=torch.float32, device=dev)
        if not ordered:
            torch.cuda.synchronize()
        dec.decode_device(src, out, ordered=ordered)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), ordered
    # queued calls, one frame each, behind a side stream
    dec.reset()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        src = torch.from_numpy(frames).to(dev)
        chunks = [src[:, k:k + 1].contiguous() for k in range(frames.shape[1])]
        outs = [torch.empty((2, 1, 2048, 2), dtype=torch.float32, device=dev) for _ in chunks]
        for c, o in zip(chunks, outs):
            dec.decode_device(c, o, asynchronous=True)
        dec.sync()
        side.synchronize()
    got = torch.cat(outs, dim=1).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    dec.close()


def test_s16_output_is_lrintf_of_float(golden):
    g, _ = golden
    frames = np.concatenate([g["sig_stress_2ch_frames"], g["crafted_2ch_frames"]])[None]
    dec = _dec(2, max_frames=frames.shape[1])
    f = dec.decode(frames)
    dec.reset()
    s = dec.decode(frames, s16=True)
    dec.close()
    assert s.dtype == np.int16
    assert np.array_equal(s, np.rint(f * np.float32(32767.0)).astype(np.int16))


def test_long_stream(golden):
    g, _ = golden
    base = np.concatenate([g["sig_mix_2ch_frames"], g["sig_noise_2ch_frames"], g["win_alternating_2ch_frames"]])
    n = 65536
    frames = base[np.arange(n) % base.shape[0]][None]
    dec = _dec(2, max_frames=n)
    got = dec.decode(frames)
    dec.close()
    cpu = CpuDecoder(2)
    head = cpu.decode(frames[0, :40])
    assert np.array_equal(got[0, :40].view(np.uint32), head.view(np.uint32))
    # the pattern repeats every base.shape[0] frames once the stream's start has left the filter memory
    p = base.shape[0]
    q = (n // p - 1) * p
    assert np.array_equal(got[0, q:q + p].view(np.uint32), got[0, 2 * p:3 * p].view(np.uint32))


def test_bad_arguments():
    import atracdenc_amd
    from atracdenc_amd import At3HipError
    for kw in (dict(channels=0), dict(channels=3), dict(n_streams=0), dict(max_frames=0), dict(device_id=-1), dict(device_id=4096)):
        args = dict(n_streams=1, channels=2, max_frames=4, device_id=0)
        args.update(kw)
        with pytest.raises(At3HipError):
            atracdenc_amd.At3pHipDecoder(**args)
    dec = _dec(2, max_frames=4)
    lib = dec.lib
    buf = np.zeros((1, 5, 2048), np.uint8)
    out = np.zeros((1, 5, 2048, 2), np.float32)
    assert lib.at3phip_decode(dec.ctx, buf.ctypes.data, 5, out.ctypes.data, 0) != 0          # more than max_frames
    assert lib.at3phip_decode(dec.ctx, buf.ctypes.data, 0, out.ctypes.data, 0) != 0          # no frames
    assert lib.at3phip_decode(dec.ctx, None, 1, out.ctypes.data, 0) != 0
    assert lib.at3phip_decode(dec.ctx, buf.ctypes.data, 1, None, 0) != 0
    assert lib.at3phip_decode(dec.ctx, buf.ctypes.data, 1, out.ctypes.data, 1 << 20) != 0   # unknown flag
    assert b"bad argument" in lib.at3phip_decoder_last_error(dec.ctx)
    assert lib.at3phip_decode(None, buf.ctypes.data, 1, out.ctypes.data, 0) != 0
    dec.close()


@pytest.mark.parametrize("nch", [1, 2])
def test_encoder_round_trip(nch):
    import atracdenc_amd
    nf = 10
    x = np.stack([at3p_signal("mix", nf, channel=c) for c in range(nch)], axis=-1)[None]
    enc = atracdenc_amd.At3pHip(n_streams=1, max_frames=nf, channels=nch, device_id=0)
    frames = enc.encode_frames(x)
    enc.close()
    dec = _dec(nch, max_frames=nf)
    pcm = dec.decode(frames)
    dec.close()
    want, rej = cpu_decode(frames[0], nch)
    assert not rej.any()
    assert np.array_equal(pcm[0].view(np.uint32), want.view(np.uint32))
    y = pcm[0].reshape(-1, nch)[DELAY:]
    ref = x[0].reshape(-1, nch)[: y.shape[0]]
    snr = 10 * np.log10((ref ** 2).sum() / ((y - ref) ** 2).sum())
    assert snr > (15.0 if nch == 1 else 7.5), snr   # the restatement's floors (test_at3p_decode_cpu.SNR_FLOOR, "mix")


@pytest.mark.parametrize("container", ["oma", "riff"])
@pytest.mark.parametrize("nch", [1, 2])
def test_cli_encode_then_decode(tmp_path, container, nch):
    from atracdenc_amd.binding import LIB_PATH
    exe = os.path.join(os.path.dirname(LIB_PATH), "at3hipenc")
    nf = 8
    x = np.stack([at3p_signal("mix", nf, channel=c) for c in range(nch)], axis=-1).reshape(-1, nch)
    pcm16 = np.clip(np.rint(x * 32767.0), -32768, 32767).astype("<i2")
    wav_in, enc, wav_out = tmp_path / "in.wav", tmp_path / f"x.{'oma' if container == 'oma' else 'at3'}", tmp_path / "y.wav"
    with wave.open(str(wav_in), "wb") as w:
        w.setnchannels(nch)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(pcm16.tobytes())
    r = subprocess.run([exe, "-e", "atrac3plus", "-i", str(wav_in), "-o", str(enc)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "-d", "-i", str(enc), "-o", str(wav_out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Codec: ATRAC3plus" in r.stdout
    data = enc.read_bytes()
    if data[:3] == b"EA3":
        body = data[96:]
    else:
        i = data.index(b"data")
        body = data[i + 8:i + 8 + int.from_bytes(data[i + 4:i + 8], "little")]
    frames = np.frombuffer(body[:len(body) // 2048 * 2048], np.uint8).reshape(-1, 2048)
    dec = _dec(nch, max_frames=frames.shape[0])
    want = dec.decode(frames[None], s16=True)[0].reshape(-1, nch)
    dec.close()
    with wave.open(str(wav_out), "rb") as w:
        assert w.getnchannels() == nch and w.getsampwidth() == 2
        got = np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, nch)
    assert np.array_equal(got, want)
