"""at3hipenc --loudness / --measure: the file written with `--loudness -16 --truepeak` equals, byte for byte, the file the tool
writes without the flag from the samples the Python API scaled (HipResampler for a 48 kHz input, HipLoudness, loudness_gain,
one float32 multiply); the printed line carries the API's numbers; --measure writes nothing; an input above full scale that
makes the ATRAC3 encoder clamp leaves its overflow counters at zero once --loudness has brought it down."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import loudness_lib as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "atracdenc_amd", "at3hipenc")


def write_wav(path, x, rate):
    """x float32 [n][channels] as an IEEE-float WAV"""
    n, ch = x.shape
    data = np.ascontiguousarray(x, np.float32).tobytes()
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(data), b"WAVE", b"fmt ", 16, 3, ch, rate, rate * ch * 4, ch * 4, 32,
                      b"data", len(data))
    with open(path, "wb") as f:
        f.write(hdr + data)


def run(*args, cwd=None):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600, cwd=cwd)


def programme(rate, seconds, seed, scale=1.0):
    """float32 [T][2]: two tones and noise with a quiet second half"""
    rng = np.random.RandomState(seed)
    T = int(rate * seconds) + 777
    t = np.arange(T)
    x = np.stack([0.5 * np.sin(2 * np.pi * 997 * t / rate) + 0.1 * rng.uniform(-1, 1, T),
                  0.4 * np.sin(2 * np.pi * 5000 * t / rate + 1) + 0.05 * rng.uniform(-1, 1, T)], axis=-1)
    x[T // 2:] *= 0.2
    return np.ascontiguousarray(scale * x, np.float32)


def seen_by_the_encoder(x, rate):
    """the 44.1 kHz samples an encoder gets from a float WAV of x: x itself, or the GPU converter's output (process and flush)"""
    if rate == 44100:
        return x
    from atracdenc_amd import HipResampler
    r = HipResampler(rate, 44100, channels=x.shape[1], n_streams=1, max_in=x.shape[0])
    try:
        return np.ascontiguousarray(np.concatenate([r.process(x[None]), r.flush()], axis=1)[0])
    finally:
        r.close()


def api_measure(pcm, true_peak):
    from atracdenc_amd import HipLoudness
    m = HipLoudness(channels=pcm.shape[1], n_streams=1, max_in=pcm.shape[0], max_hops=pcm.shape[0] // L.HOP + 1, true_peak=true_peak)
    try:
        m.process(pcm[None])
        return m.finish()[0]
    finally:
        m.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("loudness_cli")
    for rate in (44100, 48000):
        write_wav(str(d / f"in{rate}.wav"), programme(rate, 3.0, 12), rate)
    return d


@pytest.mark.parametrize("codec,ext", [("atrac3", "oma"), ("atrac1", "aea")])
@pytest.mark.parametrize("rate", [44100, 48000])
def test_loudness_flag_equals_api_scaled_input(inputs, codec, ext, rate):
    from atracdenc_amd import loudness_gain
    src = str(inputs / f"in{rate}.wav")
    extra = ["--resample"] if rate != 44100 else []
    a, b = str(inputs / f"a_{codec}_{rate}.{ext}"), str(inputs / f"b_{codec}_{rate}.{ext}")
    r = run("-e", codec, "-i", src, "-o", a, "--loudness", "-16", "--truepeak", *extra)
    assert r.returncode == 0, r.stderr
    pcm = seen_by_the_encoder(programme(rate, 3.0, 12), rate)
    res = api_measure(pcm, True)
    assert L.results_equal(res, L.measure(pcm, True))
    g = loudness_gain(res, -16.0, -1.0)
    scaled = str(inputs / f"scaled_{codec}_{rate}.wav")
    write_wav(scaled, pcm * g, 44100)
    p = run("-e", codec, "-i", scaled, "-o", b, "--nostdout")
    assert p.returncode == 0, p.stderr
    assert open(a, "rb").read() == open(b, "rb").read()
    # the printed line carries the API's numbers
    line = re.search(r"^loudness: I (\S+) LUFS, peak (\S+) dBFS, gain (\S+) dB$", r.stdout, re.M)
    assert line, r.stdout
    peak = float(max(res.true_peak))
    assert line.groups() == (f"{res.integrated:.2f}", f"{20 * np.log10(peak):.2f}", f"{20 * np.log10(float(g)):.2f}"), line.group(0)
    # --nostdout prints nothing, and without the flags the file is what it was: the plain encode of the unscaled input
    q = run("-e", codec, "-i", src, "-o", a + ".quiet", "--loudness", "-16", "--truepeak", "--nostdout", *extra)
    assert q.returncode == 0 and q.stdout == "" and open(a + ".quiet", "rb").read() == open(a, "rb").read()
    plain_wav = str(inputs / f"plain_{rate}.wav")
    write_wav(plain_wav, pcm, 44100)
    c, d = a + ".plain", b + ".plain"
    assert run("-e", codec, "-i", src, "-o", c, "--nostdout", *extra).returncode == 0
    assert run("-e", codec, "-i", plain_wav, "-o", d, "--nostdout").returncode == 0
    assert open(c, "rb").read() == open(d, "rb").read() != open(a, "rb").read()


def test_sample_peak_ceiling_without_truepeak(inputs):
    """without --truepeak the ceiling holds the sample peak; --peak moves it"""
    from atracdenc_amd import loudness_gain
    src = str(inputs / "in44100.wav")
    pcm = programme(44100, 3.0, 12)
    res = api_measure(pcm, False)
    assert max(res.true_peak) == 0.0
    r = run("-e", "atrac3", "-i", src, "-o", str(inputs / "sp.oma"), "--loudness", "0", "--peak", "-3")
    assert r.returncode == 0, r.stderr
    g = loudness_gain(res, 0.0, -3.0)
    assert abs(20 * np.log10(float(g) * float(max(res.sample_peak))) - (-3.0)) < 1e-4   # ceiling-bound
    line = re.search(r"^loudness: I (\S+) LUFS, peak (\S+) dBFS, gain (\S+) dB$", r.stdout, re.M)
    assert line and line.group(3) == f"{20 * np.log10(float(g)):.2f}", r.stdout
    write_wav(str(inputs / "sp_scaled.wav"), pcm * g, 44100)
    assert run("-e", "atrac3", "-i", str(inputs / "sp_scaled.wav"), "-o", str(inputs / "sp_b.oma"), "--nostdout").returncode == 0
    assert open(inputs / "sp.oma", "rb").read() == open(inputs / "sp_b.oma", "rb").read()


def test_measure_prints_and_writes_nothing(inputs, tmp_path):
    for rate in (44100, 48000):
        extra = ["--resample"] if rate != 44100 else []
        before = sorted(os.listdir(inputs))
        r = run("--measure", "-i", str(inputs / f"in{rate}.wav"), "--truepeak", *extra, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        assert sorted(os.listdir(inputs)) == before and os.listdir(tmp_path) == []
        res = api_measure(seen_by_the_encoder(programme(rate, 3.0, 12), rate), True)
        want = (f"loudness: I {res.integrated:.2f} LUFS, M max {res.momentary_max:.2f} LUFS, S max {res.short_term_max:.2f} LUFS, "
                f"sample peak {20 * np.log10(float(max(res.sample_peak))):.2f} dBFS, true peak {20 * np.log10(float(max(res.true_peak))):.2f} dBFS")
        assert r.stdout.strip() == want
    r = run("--measure", "-i", str(inputs / "in44100.wav"), cwd=str(tmp_path))
    assert r.returncode == 0 and "true peak" not in r.stdout and "sample peak" in r.stdout
    # --measure takes no output file and no codec; a 48 kHz input needs --resample as the encoders do
    assert run("--measure", "-i", str(inputs / "in44100.wav"), "-o", str(tmp_path / "x.oma")).returncode == 1
    assert run("--measure", "-e", "atrac3", "-i", str(inputs / "in44100.wav")).returncode == 1
    r = run("--measure", "-i", str(inputs / "in48000.wav"))
    assert r.returncode == 1 and "unsupported sample rate" in r.stderr
    assert os.listdir(tmp_path) == []
    # --peak and --truepeak without --loudness are refused
    assert run("-e", "atrac3", "-i", str(inputs / "in44100.wav"), "-o", str(tmp_path / "y.oma"), "--truepeak").returncode == 1
    assert run("-e", "atrac3", "-i", str(inputs / "in44100.wav"), "-o", str(tmp_path / "y.oma"), "--peak", "-2").returncode == 1


def test_loudness_removes_the_clipping(inputs):
    """An input far above full scale (a float WAV can hold one) makes TScaler::Scale clamp (at3hip_get_counters counts it); with --loudness -23 --peak -1
    the counters the tool prints are zero, and so are the API's for the same scaled samples."""
    from atracdenc_amd import At3Hip, loudness_gain
    hot = programme(44100, 3.0, 21, scale=60.0)   # (the encoder's spectra pass MAX_SCALE some 30 dB above full scale)
    src = str(inputs / "hot.wav")
    write_wav(src, hot, 44100)
    nb = hot.shape[0] // 1024
    enc = At3Hip(n_streams=1, max_blocks=nb)
    try:
        enc.encode(hot[: nb * 1024].reshape(1, nb, 1024, 2))
        without = enc.counters(reset=True)
        assert without["clipped_values"] > 0, without
        g = loudness_gain(api_measure(hot, False), -23.0, -1.0)
        enc.reset()
        enc.encode((hot * g)[: nb * 1024].reshape(1, nb, 1024, 2))
        assert enc.counters() == {"scale_overflow": 0, "clipped_values": 0}
    finally:
        enc.close()
    r = run("-e", "atrac3", "-i", src, "-o", str(inputs / "hot.oma"), "--loudness", "-23", "--peak", "-1")
    assert r.returncode == 0, r.stderr
    assert re.search(r"^clipping: 0 blocks, 0 values$", r.stdout, re.M), r.stdout
    write_wav(str(inputs / "hot_scaled.wav"), hot * g, 44100)
    assert run("-e", "atrac3", "-i", str(inputs / "hot_scaled.wav"), "-o", str(inputs / "hot_b.oma"), "--nostdout").returncode == 0
    assert open(inputs / "hot.oma", "rb").read() == open(inputs / "hot_b.oma", "rb").read()
