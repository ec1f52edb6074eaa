"""ATRAC3 decoder on the MI355X (include/at3hip.h decoder section, atracdenc_amd/csrc/at3_decode.hpp): bit-identical to the
goldens (whose synthesis is the reference's own) and to the C restatement (tests/host/at3_decode_cpu.c) on fuzzed frames, across
call splits, resets, device buffers, queued calls, 16-bit output, long streams and the encoder round trip."""
import os

import numpy as np
import pytest

from atracdenc_amd import At3Hip, At3HipDecoder, At3HipError
from at3_decode_lib import GOLDEN, REASONS, ROWS, cpu_ref, fuzz_frames
from at3_testlib import ROOT, SIGNALS, pin_digest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def s16_of(pcm):
    return np.rint(pcm.astype(np.float32) * np.float32(32767.0)).astype(np.int16)


def counts(dec):
    c = dec.counters()
    return [c[r] for r in REASONS]


def test_goldens_bit_identical(golden):
    for name in golden["cases"]:
        fsz, js = (int(v) for v in golden[f"{name}_row"])
        frames = golden[f"{name}_frames"]
        dec = At3HipDecoder(n_streams=1, frame_size=fsz, max_frames=frames.shape[0])
        assert dec.joint_stereo == bool(js)
        got = dec.decode(frames[None])[0]
        c = counts(dec)
        dec.close()
        assert np.array_equal(pin_digest(got), golden[f"{name}_pcm_sha256"]), name
        if f"{name}_pcm" in golden.files:
            assert np.array_equal(bits(got), bits(golden[f"{name}_pcm"])), name
        assert c == golden[f"{name}_rejected"].tolist(), name


@pytest.mark.parametrize("row", ROWS, ids=[str(r[1]) for r in ROWS])
def test_fuzz_equals_restatement(golden, row):
    _, fsz, js = row
    frames = fuzz_frames(golden, fsz, 3, 96, seed=fsz)
    exp, rej = cpu_ref(frames, fsz, js)
    dec = At3HipDecoder(n_streams=3, frame_size=fsz, max_frames=96)
    got = dec.decode(frames)
    c = counts(dec)
    dec.close()
    assert np.array_equal(bits(got), bits(exp)), int((bits(got) != bits(exp)).sum())
    assert c == rej
    assert sum(rej) > 0


def test_splits_reset_and_counters(golden):
    fsz, js = 192, True
    frames = fuzz_frames(golden, fsz, 2, 120, seed=77)
    exp, rej = cpu_ref(frames, fsz, js)
    dec = At3HipDecoder(n_streams=2, frame_size=fsz, max_frames=120)
    rng = np.random.default_rng(5)
    for trial in range(3):
        cuts = np.sort(rng.choice(np.arange(1, 120), 5, replace=False))
        parts = [dec.decode(np.ascontiguousarray(p)) for p in np.split(frames, cuts, axis=1)]
        assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(exp)), trial
        assert counts(dec) == rej
        dec.reset()
        assert counts(dec) == [0] * len(REASONS)
    assert np.array_equal(bits(dec.decode(frames[:, :1])), bits(exp[:, :1]))   # reset returns to the initial state
    dec.close()


def test_device_tensors_ordered_and_queued(golden):
    import torch
    fsz, js = 384, False
    frames = fuzz_frames(golden, fsz, 4, 200, seed=9)
    exp, _ = cpu_ref(frames, fsz, js)
    dec = At3HipDecoder(n_streams=4, frame_size=fsz, max_frames=200)
    src = torch.from_numpy(frames).cuda()
    u = torch.zeros_like(src)
    out = torch.full((4, 200, 1024, 2), float("nan"), device="cuda")
    torch.cuda._sleep(20_000_000)
    u.copy_(src)
    dec.decode_device(u, out)
    assert np.array_equal(bits(out.cpu().numpy()), bits(exp))
    dec.reset()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        u2 = torch.zeros_like(src)
        out2 = torch.full((4, 200, 1024, 2), float("nan"), device="cuda")
        torch.cuda._sleep(20_000_000)
        u2.copy_(src)
        dec.decode_device(u2, out2)
        res = out2.cpu()
    assert np.array_equal(bits(res.numpy()), bits(exp))
    dec.reset()
    pieces = [(0, 50), (50, 51), (51, 52), (52, 200)]
    ins = [u[:, a:b].contiguous() for a, b in pieces]
    outs = [torch.zeros((4, b - a, 1024, 2), device="cuda") for a, b in pieces]
    torch.cuda.synchronize()
    for i, o in zip(ins, outs):
        dec.decode_device(i, o, asynchronous=True)
    dec.sync()
    assert np.array_equal(bits(torch.cat(outs, 1).cpu().numpy()), bits(exp))
    dec.reset()
    o16 = torch.zeros((4, 200, 1024, 2), dtype=torch.int16, device="cuda")
    dec.decode_device(u, o16)
    assert np.array_equal(o16.cpu().numpy(), s16_of(exp))
    dec.close()


def test_s16_output_is_lrintf_of_float(golden):
    for name in ("crafted_192", "burst_384_ch2", "random_1024"):
        fsz = int(golden[f"{name}_row"][0])
        frames = golden[f"{name}_frames"][None]
        dec = At3HipDecoder(n_streams=1, frame_size=fsz, max_frames=frames.shape[1])
        f32 = dec.decode(frames)
        dec.reset()
        got = dec.decode(frames, s16=True)
        dec.close()
        assert np.array_equal(pin_digest(f32[0]), golden[f"{name}_pcm_sha256"]), name
        assert got.dtype == np.int16 and np.array_equal(got, s16_of(f32)), name


def test_long_stream(golden):
    fsz, js = 272, True
    n = 65536
    frames = fuzz_frames(golden, fsz, 1, n, seed=3)
    exp, rej = cpu_ref(frames, fsz, js)
    dec = At3HipDecoder(n_streams=1, frame_size=fsz, max_frames=n)
    got = dec.decode(frames)
    c = counts(dec)
    dec.close()
    assert np.array_equal(bits(got), bits(exp)), int((bits(got) != bits(exp)).sum())
    assert c == rej


def test_bad_arguments():
    for kw in (dict(frame_size=100), dict(frame_size=192, joint_stereo=False), dict(frame_size=384, joint_stereo=True),
               dict(n_streams=0), dict(max_frames=0), dict(n_streams=40000)):
        with pytest.raises(At3HipError):
            At3HipDecoder(**dict(dict(n_streams=1, frame_size=384, max_frames=8), **kw))
    dec = At3HipDecoder(n_streams=1, frame_size=384, max_frames=8)
    with pytest.raises(At3HipError):
        dec.decode(np.zeros((1, 9, 384), np.uint8))
    frames = np.zeros((1, 2, 384), np.uint8)
    out = np.zeros((1, 2, 1024, 2), np.float32)
    lib = dec.lib
    assert lib.at3hip_decode(dec.ctx, frames.ctypes.data, 0, out.ctypes.data, 0) == -1
    assert lib.at3hip_decode(dec.ctx, None, 2, out.ctypes.data, 0) == -1
    assert lib.at3hip_decode(dec.ctx, frames.ctypes.data, 2, None, 0) == -1
    assert lib.at3hip_decode(dec.ctx, frames.ctypes.data, 2, out.ctypes.data, 0x100) == -1
    assert lib.at3hip_decode(None, frames.ctypes.data, 2, out.ctypes.data, 0) == -1
    assert lib.at3hip_decoder_get_counters(dec.ctx, None, 0) == -1
    assert lib.at3hip_decoder_sync(None) == -1 and lib.at3hip_decoder_reset(None) == -1
    assert lib.at3hip_decoder_create(None, None) == -1
    assert dec.decode(frames).shape == (1, 2, 1024, 2)   # still usable
    dec.close()


@pytest.mark.parametrize("row", [ROWS[0], ROWS[3]], ids=["192", "384"])
def test_encoder_round_trip(row):
    br, fsz, js = row
    pcm = np.stack([SIGNALS["mix"](12), SIGNALS["burst"](12)])
    enc = At3Hip(n_streams=2, max_blocks=12, bitrate=br)
    frames = enc.encode(pcm)
    enc.close()
    assert frames.shape == (2, 11, fsz)
    dec = At3HipDecoder(n_streams=2, frame_size=fsz, max_frames=11)
    got = dec.decode(frames)
    c = counts(dec)
    dec.close()
    exp, rej = cpu_ref(frames, fsz, js)
    assert rej == [0] * len(REASONS) and c == rej
    assert np.array_equal(bits(got), bits(exp))


@pytest.mark.parametrize("container", ["oma", "riff"])
def test_cli_encode_then_decode(tmp_path, container):
    """at3hipenc -e atrac3 -> at3hipenc -d on the OMA / RIFF file equals the restatement's PCM16 of the file's frames"""
    import struct
    import subprocess
    from at3_decode_lib import container_frames, row_of
    exe = os.path.join(ROOT, "atracdenc_amd", "at3hipenc")
    assert os.path.exists(exe), "at3hipenc not built"
    rows = set()
    for nch, opts in ((2, ["--bitrate", "128"]), (2, ["--bitrate", "64"]), (1, ["--bitrate", "64"])):
        s16 = (SIGNALS["burst"](9).reshape(-1, 2)[:9000, :nch] * 32768).astype("<i2")
        body = np.ascontiguousarray(s16).tobytes()
        wav = str(tmp_path / "in.wav")
        fmt = struct.pack("<HHIIHH", 1, nch, 44100, 44100 * 2 * nch, 2 * nch, 16)
        open(wav, "wb").write(b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt +
                              b"data" + struct.pack("<I", len(body)) + body)
        enc = str(tmp_path / ("out.oma" if container == "oma" else "out.at3"))
        r = subprocess.run([exe, "-e", "atrac3", "-i", wav, "-o", enc, "--container", container, "--nostdout"] + opts,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        data = open(enc, "rb").read()
        fsz = (int.from_bytes(data[32:36], "big") & 0x3FF) * 8 if container == "oma" else int.from_bytes(data[32:34], "little")
        _, _, js = row_of(fsz)
        rows.add(fsz)
        frames = container_frames(data, fsz)
        exp, rej = cpu_ref(frames[None], fsz, js)
        assert sum(rej) == 0
        out = str(tmp_path / "dec.wav")
        r = subprocess.run([exe, "-d", "-i", enc, "-o", out, "--batch", "3"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f"Codec: ATRAC3, frame size {fsz}" in r.stdout
        got = open(out, "rb").read()
        riff, size, wave, fmt_id, fmt_len, tag, ch, rate, brate, align, bits_, dtag, dlen = struct.unpack("<4sI4s4sIHHIIHH4sI", got[:44])
        assert (riff, wave, fmt_id, fmt_len, tag, ch, rate, bits_, dtag) == (b"RIFF", b"WAVE", b"fmt ", 16, 1, 2, 44100, 16, b"data")
        assert dlen == frames.shape[0] * 1024 * 4 and size == 36 + dlen and len(got) == 44 + dlen
        samples = np.frombuffer(got[44:], "<i2").reshape(-1, 1024, 2)
        assert np.array_equal(samples, s16_of(exp[0]))
    assert rows == {384, 192}
