"""at3hipenc --loudness LUFS --limit: the file written from a WAV with clicks equals, byte for byte, the file the tool writes
without the flags from the samples the C restatement limited (tests/host/limiter_cpu.c on the gain to the target alone), also
behind --resample; the printed `limiter:` line carries the restatement's statistics; the result reaches the target loudness
where the one constant gain cannot; --limit without --loudness is a usage error."""
import re

import numpy as np
import pytest

import limiter_lib as LM
import loudness_lib as L
from test_loudness_cli_gpu import run, seen_by_the_encoder, write_wav

pytestmark = pytest.mark.gpu

TARGET = -16.0


def clicks(rate):
    """float32 [T][2]: a -26 dBFS 1 kHz tone, 4 s and a bit, with a full-scale click of one sample every two seconds"""
    x = L.tone_segments([(-26.0, 4.0)], rate=rate)
    x = np.concatenate([x, x[:777]])
    x[rate // 2::2 * rate] = 1.0
    return np.ascontiguousarray(x, np.float32)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("limiter_cli")
    for rate in (44100, 48000):
        write_wav(str(d / f"in{rate}.wav"), clicks(rate), rate)
    return d


@pytest.mark.parametrize("rate", [44100, 48000])
def test_limit_flag_equals_restatement_limited_input(inputs, rate):
    src = str(inputs / f"in{rate}.wav")
    extra = ["--resample"] if rate != 44100 else []
    a, b = str(inputs / f"a_{rate}.oma"), str(inputs / f"b_{rate}.oma")
    r = run("-e", "atrac3", "-i", src, "-o", a, "--loudness", str(TARGET), "--limit", "--truepeak", *extra)
    assert r.returncode == 0, r.stderr
    pcm = seen_by_the_encoder(clicks(rate), rate)
    res = L.measure(pcm, True)
    g = L.gain(res, TARGET, 400.0)              # the gain to the target alone
    capped = L.gain(res, TARGET, -1.0)          # what --loudness applies without --limit
    assert g > 2 * capped
    y, S, _, (min_s, n_lim) = LM.restate(pcm, g, LM.CEIL, True)
    limited = str(inputs / f"limited_{rate}.wav")
    write_wav(limited, y, 44100)
    p = run("-e", "atrac3", "-i", limited, "-o", b, "--nostdout")
    assert p.returncode == 0, p.stderr
    assert open(a, "rb").read() == open(b, "rb").read()
    # the printed lines: the gain to the target, then the restatement's statistics
    line = re.search(r"^loudness: I (\S+) LUFS, peak (\S+) dBFS, gain (\S+) dB$", r.stdout, re.M)
    assert line and line.group(3) == f"{20 * np.log10(float(g)):.2f}", r.stdout
    line = re.search(r"^limiter: max reduction (\S+) dB, limited (\S+) %$", r.stdout, re.M)
    assert line, r.stdout
    assert 0 < n_lim < len(S)
    assert line.groups() == (f"{-20 * np.log10(min_s / LM.FULL):.2f}", f"{100.0 * n_lim / len(S):.2f}"), line.group(0)
    # what the flag is for: the limited file is at the target, the capped constant gain leaves it far below
    at_target, constant = L.measure(y, True).integrated, L.measure(pcm * capped, True).integrated
    assert abs(at_target - TARGET) < 0.5 and constant < TARGET - 5.0, (at_target, constant)
    # --nostdout prints nothing and writes the same file; without --limit the file is another one
    q = run("-e", "atrac3", "-i", src, "-o", a + ".quiet", "--loudness", str(TARGET), "--limit", "--truepeak", "--nostdout", *extra)
    assert q.returncode == 0 and q.stdout == "" and open(a + ".quiet", "rb").read() == open(a, "rb").read()
    c = run("-e", "atrac3", "-i", src, "-o", a + ".const", "--loudness", str(TARGET), "--truepeak", *extra)
    assert c.returncode == 0 and "limiter:" not in c.stdout and open(a + ".const", "rb").read() != open(a, "rb").read()


def test_sample_detector_and_peak_option(inputs):
    """without --truepeak the detector reads the samples; --peak sets the ceiling"""
    src = str(inputs / "in44100.wav")
    a, b = str(inputs / "sp.aea"), str(inputs / "sp_b.aea")
    r = run("-e", "atrac1", "-i", src, "-o", a, "--loudness", str(TARGET), "--limit", "--peak", "-3")
    assert r.returncode == 0, r.stderr
    pcm = clicks(44100)
    g = L.gain(L.measure(pcm, False), TARGET, 400.0)
    y, S, _, (min_s, n_lim) = LM.restate(pcm, g, np.float32(10.0 ** (-3.0 / 20.0)), False)
    write_wav(str(inputs / "sp_limited.wav"), y, 44100)
    assert run("-e", "atrac1", "-i", str(inputs / "sp_limited.wav"), "-o", b, "--nostdout").returncode == 0
    assert open(a, "rb").read() == open(b, "rb").read()
    line = re.search(r"^limiter: max reduction (\S+) dB, limited (\S+) %$", r.stdout, re.M)
    assert line and line.groups() == (f"{-20 * np.log10(min_s / LM.FULL):.2f}", f"{100.0 * n_lim / len(S):.2f}"), r.stdout


def test_limit_needs_loudness(inputs, tmp_path):
    src = str(inputs / "in44100.wav")
    r = run("-e", "atrac3", "-i", src, "-o", str(tmp_path / "x.oma"), "--limit")
    assert r.returncode == 1 and "usage" in r.stderr
    assert run("--measure", "-i", src, "--limit").returncode == 1
    assert list(tmp_path.iterdir()) == []
