"""at3hipenc --resample: a 48 kHz WAV encodes to the same file, byte for byte, as the restatement's 44.1 kHz conversion of its
samples (s / 32768, as TWavSource reads them) written as a float WAV and encoded without the flag; every encoder."""
import os
import struct
import subprocess

import numpy as np
import pytest

from resample_lib import CpuResampler

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "atracdenc_amd", "at3hipenc")


def write_wav(path, x, rate):
    """x int16 or float32 [n][channels]"""
    tag, bits = (1, 16) if x.dtype == np.int16 else (3, 32)
    n, ch = x.shape
    data = np.ascontiguousarray(x).tobytes()
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(data), b"WAVE", b"fmt ", 16, tag, ch, rate, rate * ch * bits // 8,
                      ch * bits // 8, bits, b"data", len(data))
    with open(path, "wb") as f:
        f.write(hdr + data)


def run(*args):
    return subprocess.run([CLI, *args, "--nostdout"], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample_cli")
    rng = np.random.RandomState(12)
    T = 48000 + 777
    t = np.arange(T)
    x = np.stack([0.5 * np.sin(2 * np.pi * 997 * t / 48000) + 0.1 * rng.uniform(-1, 1, T),
                  0.4 * np.sin(2 * np.pi * 5000 * t / 48000 + 1) + 0.05 * rng.uniform(-1, 1, T)], axis=-1)
    s16 = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    write_wav(str(d / "in48.wav"), s16, 48000)
    conv = CpuResampler(48000, 44100, 2).whole(s16.astype(np.float32) / np.float32(32768.0))
    assert conv.shape[0] == -(-T * 147 // 160)
    write_wav(str(d / "in44f.wav"), conv.astype(np.float32), 44100)
    return d


@pytest.mark.parametrize("codec,ext", [("atrac1", "aea"), ("atrac3", "oma"), ("atrac3plus", "oma")])
def test_resample_flag_equals_converted_input(inputs, codec, ext):
    a, b = str(inputs / f"a_{codec}.{ext}"), str(inputs / f"b_{codec}.{ext}")
    r = run("-e", codec, "-i", str(inputs / "in48.wav"), "-o", a, "--resample")
    assert r.returncode == 0, r.stderr
    r = run("-e", codec, "-i", str(inputs / "in44f.wav"), "-o", b)
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == open(b, "rb").read()
    # a 44.1 kHz input with the flag is encoded as without it
    c = str(inputs / f"c_{codec}.{ext}")
    r = run("-e", codec, "-i", str(inputs / "in44f.wav"), "-o", c, "--resample")
    assert r.returncode == 0, r.stderr
    assert open(c, "rb").read() == open(b, "rb").read()


def test_without_the_flag_other_rates_are_refused(inputs):
    for codec in ("atrac1", "atrac3", "atrac3plus"):
        r = run("-e", codec, "-i", str(inputs / "in48.wav"), "-o", str(inputs / "refused.oma"))
        assert r.returncode == 1 and "unsupported sample rate" in r.stderr, (codec, r.stderr)


# ---- at3hipenc -d --rate ------------------------------------------------------------------------------------------------------
def _decoded_float(codec, path):
    """the Python decoder's float output [n][channels] for what `at3hipenc -d` decodes of the file, and the tool's exit status
    (an AEA file whose last 4096-sample call runs past its frames ends with status 1, the complete calls written)"""
    from atracdenc_amd import At1HipDecoder, At3HipDecoder, At3pHipDecoder
    from at3_decode_lib import container_frames
    data = open(path, "rb").read()
    status = 0
    if codec == "atrac1":
        nch = data[264]
        units = np.frombuffer(data[2048:], np.uint8)
        units = units[: units.size // (212 * nch) * 212 * nch].reshape(-1, nch, 212)
        frames = units.shape[0]
        calls = max(1, -(-(frames - 5) // 8))   # TAeaInput::GetLengthInSamples and the engine's 4096-sample calls
        n = 8 * min(calls, frames // 8)
        status = 0 if 8 * calls <= frames else 1
        dec = At1HipDecoder(n_streams=1, max_frames=n, channels=nch)
        pcm = dec.decode(units[None, :n])[0]
    elif codec == "atrac3":
        frames = container_frames(data, 384)
        dec = At3HipDecoder(n_streams=1, frame_size=384, max_frames=frames.shape[0])
        pcm = dec.decode(frames[None])[0]
    else:
        frames = container_frames(data, 2048)
        dec = At3pHipDecoder(n_streams=1, channels=2, max_frames=frames.shape[0])
        pcm = dec.decode(frames[None], tones=True)[0]
    dec.close()
    return pcm.reshape(-1, pcm.shape[-1]), status


@pytest.mark.parametrize("codec,ext", [("atrac1", "aea"), ("atrac3", "oma"), ("atrac3plus", "oma")])
@pytest.mark.parametrize("rate", [48000, 22050])
def test_decode_rate_equals_restated_conversion(inputs, codec, ext, rate):
    """-d --rate hz: the Python decoder's float output, converted by the restatement, clamped to [-1, 1] and written as
    lrintf(x * 32767.0f), behind a WAV header at hz"""
    from at1_decode_lib import read_wav, s16_of
    enc = str(inputs / f"d_{codec}.{ext}")
    if not os.path.exists(enc):
        r = run("-e", codec, "-i", str(inputs / "in44f.wav"), "-o", enc)
        assert r.returncode == 0, r.stderr
    wav = str(inputs / f"d_{codec}_{rate}.wav")
    r = run("-d", "-i", enc, "-o", wav, "--rate", str(rate), "--batch", "7")
    pcm, status = _decoded_float(codec, enc)
    assert r.returncode == status, r.stderr
    conv = CpuResampler(44100, rate, pcm.shape[1]).whole(pcm)
    assert conv.shape[0] == -(-pcm.shape[0] * rate // 44100)
    exp = s16_of(np.clip(conv, np.float32(-1), np.float32(1)))
    h, samples = read_wav(wav)
    assert (h["tag"], h["nch"], h["rate"], h["bits"], h["byte_rate"]) == (1, pcm.shape[1], rate, 16, rate * 2 * pcm.shape[1])
    assert h["data_len"] == exp.size * 2 and h["file_len"] == 44 + h["data_len"]
    assert np.array_equal(samples, exp)
    # --rate 44100 is the decoders' own rate: the same file as -d alone
    a, b = str(inputs / f"d_{codec}_plain.wav"), str(inputs / f"d_{codec}_44100.wav")
    assert run("-d", "-i", enc, "-o", a).returncode == status
    assert run("-d", "-i", enc, "-o", b, "--rate", "44100").returncode == status
    assert open(a, "rb").read() == open(b, "rb").read()


def test_decode_rate_refuses_unsupported_rates(inputs):
    enc = str(inputs / "r_atrac3.oma")
    assert run("-e", "atrac3", "-i", str(inputs / "in44f.wav"), "-o", enc).returncode == 0
    for rate in ("12345", "44000", "0x"):
        r = run("-d", "-i", enc, "-o", str(inputs / "r.wav"), "--rate", rate)
        assert r.returncode == 1 and "unsupported output rate" in r.stderr, (rate, r.stderr)
