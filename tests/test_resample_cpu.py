"""The sample-rate converter's definition on the host (include/at3hip_resample.h; no GPU): the library's table equals the C
restatement's bit for bit for every supported pair, the shapes, the filter's response, and the restatement's streaming rules."""
import subprocess

import numpy as np
import pytest

import atracdenc_amd
from atracdenc_amd import binding
from resample_lib import PAIRS, CpuResampler, n_outputs, shape, table

RESAMPLER_SYMBOLS = ["at3hip_resampler_create", "at3hip_resampler_destroy", "at3hip_resampler_last_error", "at3hip_resampler_reset",
                     "at3hip_resampler_max_out", "at3hip_resampler_process", "at3hip_resampler_flush", "at3hip_resampler_sync",
                     "at3hip_resampler_set_stream", "at3hip_resampler_shape", "at3hip_resampler_host_tables"]


@pytest.fixture(scope="module", autouse=True)
def _library():
    import os
    if not os.path.exists(atracdenc_amd.LIB_PATH):
        atracdenc_amd.build_library()


def test_library_exports_the_resampler():
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in RESAMPLER_SYMBOLS:
        assert s in names and s in binding.SYMBOLS, s


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_host_tables_equal_the_restatement(pair):
    got = atracdenc_amd.resampler_host_tables(*pair)
    exp = table(*pair)
    assert got.shape == exp.shape == shape(*pair)[::2]
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_shapes():
    expect = {(48000, 44100): (147, 160, 158), (44100, 48000): (160, 147, 144), (32000, 44100): (441, 320, 144),
              (192000, 44100): (147, 640, 628), (44100, 8000): (80, 441, 794), (88200, 44100): (1, 2, 288),
              (44100, 22050): (1, 2, 288), (11025, 44100): (4, 1, 144)}
    for pair, lmk in expect.items():
        assert shape(*pair) == lmk, pair
        assert binding.resampler_shape(*pair) == lmk, pair
    for pair in PAIRS:
        assert binding.resampler_shape(*pair) == shape(*pair)


@pytest.mark.parametrize("pair", [(44100, 44100), (48000, 32000), (44000, 44100), (44100, 12000), (0, 44100), (-48000, 44100)])
def test_unsupported_pairs(pair):
    with pytest.raises(atracdenc_amd.At3HipError):
        binding.resampler_shape(*pair)
    with pytest.raises(atracdenc_amd.At3HipError):
        atracdenc_amd.resampler_host_tables(*pair)
    with pytest.raises(ValueError):
        shape(*pair)


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_filter_response(pair):
    """The float table's prototype on the fine grid (d = k - (K/2 - 1) - p / L): flat passband, deep stopband, unit DC gain
    per phase."""
    in_rate, out_rate = pair
    hp = table(*pair).astype(np.float64)
    L, K = hp.shape
    f_lo = min(pair)
    h = np.zeros(L * K + L)
    for p in range(L):
        h[np.arange(K) * L - p + L - 1] = hp[p]
    n = 1 << 20
    mag = np.abs(np.fft.rfft(h, n)) / L
    f = np.arange(mag.size) * L / n          # cycles per input sample
    db = 20 * np.log10(np.maximum(mag, 1e-30))
    passband = db[f <= 0.4535 * f_lo / in_rate]
    assert passband.min() > -0.001 and passband.max() < 0.001, (passband.min(), passband.max())
    assert db[f >= 0.5 * f_lo / in_rate].max() <= -99.0
    assert np.abs(hp.sum(axis=1) - 1).max() < 1e-5


@pytest.mark.parametrize("pair", [(48000, 44100), (44100, 48000), (192000, 44100), (8000, 44100), (44100, 8000), (88200, 44100)])
@pytest.mark.parametrize("channels", [1, 2])
def test_restatement_counts_and_split_invariance(pair, channels):
    rng = np.random.RandomState(sum(pair) + channels)
    T = 3001
    x = rng.uniform(-1, 1, (T, channels)).astype(np.float32)
    whole = CpuResampler(*pair, channels).whole(x)
    assert whole.shape == (n_outputs(T, *pair), channels)
    L, M, K = shape(*pair)
    r = CpuResampler(*pair, channels)
    parts, at = [], 0
    for cut in sorted(rng.randint(0, T, 6)) + [T]:
        got = r.process(x[at:cut])
        # every output whose last tap is in: i + K/2 <= T - 1
        a = cut - K // 2
        assert sum(p.shape[0] for p in parts) + got.shape[0] == (-(-a * L // M) if a > 0 else 0)
        parts.append(got)
        at = cut
    parts.append(r.flush())
    split = np.concatenate(parts)
    assert np.array_equal(split.view(np.uint32), whole.view(np.uint32))
    # the flush leaves the start state
    again = r.whole(x)
    assert np.array_equal(again.view(np.uint32), whole.view(np.uint32))


def test_restatement_centred_and_exact_at_dc():
    """A constant stays (close to) that constant away from the edges; output n sits at time n / out: a sine converts to the
    same sine sampled at the new rate."""
    r = CpuResampler(48000, 44100, 1)
    t = np.arange(48000)
    y = r.whole(np.sin(2 * np.pi * 997 * t / 48000).astype(np.float32)[:, None])[:, 0]
    n = np.arange(y.size)
    ref = np.sin(2 * np.pi * 997 * n / 44100)
    L, M, K = shape(48000, 44100)
    edge = K * L // M
    err = y[edge:-edge] - ref[edge:-edge]
    snr = 10 * np.log10(np.sum(ref[edge:-edge] ** 2) / np.sum(err ** 2))
    assert snr >= 90, snr
