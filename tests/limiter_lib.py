"""Helpers of the look-ahead limiter's tests (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * the C restatement tests/host/limiter_cpu.c (the definition in include/at3hip_loudness.h, "The look-ahead limiter"), compiled
    on first use with gcc -O2 -ffp-contract=off -fno-fast-math; the converter's table comes from the meter's restatement.
  * the signals of the property tests, and the batch, the cuts and the driver that the GPU tests and the SIMT-harness driver
    share: a run through binding.HipLoudness against the restatement of every stream alone.
"""
import concurrent.futures
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import loudness_lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
CPU_SRC = os.path.join(HERE, "host", "limiter_cpu.c")
A, H = 220, 2205
FULL = (A + 1) << 30
TILE = 2048                                  # outputs per workgroup of k_limit_gain
CEIL = np.float32(10.0 ** (-1.0 / 20.0))     # -1 dBFS
RATE = 44100

_cpu_so = None
_table = None


def cpu_lib():
    global _cpu_so
    if _cpu_so is None:
        so = os.path.join(tempfile.mkdtemp(prefix="limiter_"), "liblimiter_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *L.CFLAGS, "-shared", "-o", so, CPU_SRC, "-lm"])
        _cpu_so = so
    lib = ctypes.CDLL(_cpu_so)
    vp = ctypes.c_void_p
    lib.lim_run.argtypes = [vp, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_float, vp, vp, vp, vp, vp]
    return lib


def tp_table():
    """the 44100 -> 176400 table float32 [4][144] of the meter's restatement"""
    global _table
    if _table is None:
        _table = np.zeros((4, 144), np.float32)
        L.cpu_lib().ld_tp_table(_table.ctypes.data)
        _table.setflags(write=False)
    return _table


def delay(true_peak):
    return A + (72 if true_peak else 0)


def restate(x, g, c=CEIL, true_peak=False):
    """the restatement over the whole stream x [T][C]: (y float32 [T][C], S int64 [T], r float64 [T], (min S, limited count))"""
    x = L._pcm(x)
    T, C = x.shape
    y = np.zeros((T, C), np.float32)
    S = np.zeros(T, np.int64)
    r = np.zeros(T, np.float64)
    stats = np.zeros(2, np.int64)
    hp = tp_table().ctypes.data if true_peak else None
    cpu_lib().lim_run(x.ctypes.data, T, C, np.float32(g), np.float32(c), hp, y.ctypes.data, S.ctypes.data, r.ctypes.data, stats.ctypes.data)
    return y, S, r, (int(stats[0]), int(stats[1]))


# ---- the signals of the property tests: float32 [n][channels] --------------------------------------------------------------------
KINDS = ("clicks", "burst", "noise", "fs4", "tone40")


def signal(kind, n=2 * RATE, channels=2, seed=1):
    rng = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64)
    if kind == "clicks":      # sparse full-scale clicks of one to three samples over a noise floor
        x = 0.02 * rng.uniform(-1, 1, (n, channels))
        at = 1500 + 7000 * np.arange(n // 7000) + rng.randint(0, 3000, n // 7000)
        for a in at[at < n - 3]:
            w = rng.randint(1, 4)
            x[a:a + w] = rng.choice([-1.0, 1.0], (w, 1)) * rng.uniform(0.9, 1.0, (w, channels))
    elif kind == "burst":     # bench.py's `burst`: a 3 kHz sine whose amplitude toggles 0.02 / 0.6 every 3000 samples
        amp = np.where((t // 3000) % 2 == 0, 0.02, 0.6)
        left = amp * np.sin(2 * np.pi * 3000.0 * t / RATE)
        x = np.stack([left, 0.5 * left], axis=-1)[:, :channels]
    elif kind == "noise":
        x = rng.uniform(-1, 1, (n, channels))
    elif kind == "fs4":       # fs / 4 at 45 degrees: every sample 0.707 of the peak between the samples
        x = np.stack([0.9 * np.sin(2 * np.pi * 0.25 * t + np.pi / 4 + 0.1 * c) for c in range(channels)], axis=-1)
    elif kind == "tone40":
        x = np.stack([0.8 * np.sin(2 * np.pi * 40.0 * t / RATE + c) for c in range(channels)], axis=-1)
    elif kind == "tone997":
        x = np.stack([0.5 * np.sin(2 * np.pi * 997.0 * t / RATE + c) for c in range(channels)], axis=-1)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, np.float32)


def leveling_example(seconds=15):
    """a -26 dBFS 1 kHz stereo tone (loudness_lib.tone_segments) with a full-scale click of one sample every three seconds: the
    clicks set the peak and carry about 1 % of the K-weighted energy (a limiter removes the clicks' own energy, so an example in
    which they carried much of the loudness could not land on the target by any limiter)"""
    x = L.tone_segments([(-26.0, float(seconds))]).copy()
    for k in range(0, seconds, 3):
        x[k * RATE + 20000] = 1.0
    return x


# ---- the batch of the parity tests -----------------------------------------------------------------------------------------------
T_GPU = 2 * TILE + 1237
GAINS = np.array([4.0, 0.25, 4.0], np.float32)   # stream 1 is never limited


def batch(channels, true_peak):
    """float32 [3][T_GPU][channels]: clicks and burst (limited between a tenth and 0.95 of the time at g = 4) and a quiet stream,
    with extra peaks on the last output of the first gain-kernel tile, on the first of the next one, within A of the start
    and within A of the end. All values are multiples of 2^-15, so that the 16-bit calls see the same samples."""
    xs = np.stack([signal("clicks", T_GPU, channels, 5), signal("noise", T_GPU, channels, 6), signal("burst", T_GPU, channels, 7)])
    xs[0, TILE - 1, 0] = 0.97
    xs[0, TILE, channels - 1] = -0.95
    xs[0, 100] = 0.93
    xs[0, T_GPU - 50, 0] = -0.99
    xs[2, T_GPU - 1] = 0.9
    xs[2, 0] = -0.9
    # (+ 0.0: a 16-bit zero has no sign)
    return np.ascontiguousarray(np.round(np.clip(xs, -1.0, 32767.0 / 32768.0) * 32768.0) / 32768.0 + 0.0, np.float32)


SEVEN = (("clicks", 4.0), ("noise", 0.25), ("burst", 4.0), ("fs4", 1.0), ("tone40", 2.0), ("tone997", 3.0), ("clicks", 1.5))
SEVEN_FIRST = 3400


def seven(T, channels):
    """(xs float32 [7][T][channels], gains [7]): seven distinct streams of any length for the tests that choose their own sizes,
    samples 3400 .. 3400 + T of signal()'s stereo form, mono taking its channel 0 (the first click of `clicks` falls near sample
    600 and `burst` is loud up to 2600, so that stream 0 of 3000 samples is limited, and not everywhere); stream 1 is never
    limited"""
    n = max(SEVEN_FIRST + T, 2 * RATE)   # (signal() places its clicks by the length it is asked for)
    xs = np.stack([signal(kind, n, 2, 5 + i)[SEVEN_FIRST:SEVEN_FIRST + T, :channels] for i, (kind, _) in enumerate(SEVEN)])
    return np.ascontiguousarray(xs), np.array([g for _, g in SEVEN], np.float32)


def restate_all(xs, gains, c, true_peak):
    """the restatement of every stream alone: (ys [S][T][C], [(min S, limited count)]). The streams run side by side on up to
    eight threads (the C call holds no lock): the naive window minimum is 2426 steps per sample."""
    cpu_lib(), tp_table()   # compiled and loaded before the threads start
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():   # (the SIMT-harness drivers run as children of one core each)
        cores = min(cores, int(os.environ["OMP_NUM_THREADS"]))
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(8, cores, xs.shape[0]))) as pool:
        res = list(pool.map(lambda i: restate(xs[i], gains[i], c, true_peak), range(xs.shape[0])))
    return np.stack([r[0] for r in res]), [r[3] for r in res]


def cuts_for(rng, T, true_peak):
    """sorted call ends, the last one T: an empty call, calls of 1 and of 71 samples, cuts on both sides of the input positions
    at which an output tile ends (outputs lag the input by the delay), and random ones"""
    d = delay(true_peak)
    cuts = {1, 72, TILE + d - 1, TILE + d, TILE + d + 1, TILE, TILE + 1, T}
    cuts |= set(rng.randint(1, T + 1, 4).tolist())
    return sorted([0, TILE] + [c for c in cuts if c <= T])   # (0 and the second TILE are empty calls)


def run_engine(m, xs, gains, c, true_peak, cuts, s16=False):
    """xs [S][T][C] through HipLoudness `m` in calls ending at `cuts`, then the flush: (y [S][T][C], [(min S, limited)] per stream)"""
    m.limit_start(gains, c, true_peak)
    pieces, at = [], 0
    for cut in cuts:
        piece = xs[:, at:cut]
        if s16:
            piece = np.round(piece * 32768.0).astype(np.int16)
            assert np.array_equal(piece.astype(np.float32) / np.float32(32768.0), xs[:, at:cut])
        pieces.append(m.limit_s16(piece) if s16 else m.limit(piece))
        at = cut
        assert sum(p.shape[1] for p in pieces) == max(0, at - delay(true_peak)), (at, [p.shape for p in pieces])
    pieces.append(m.limit_flush())
    st = m.limit_stats()
    assert all(s.n_out == xs.shape[1] for s in st)
    return np.concatenate(pieces, axis=1), [(s.min_sum, s.n_limited) for s in st]


_expect = {}


def expect(channels, true_peak):
    """the restatement of every stream of batch() alone, computed once: (ys [3][T][C], stats)"""
    key = (channels, true_peak)
    if key not in _expect:
        xs = batch(channels, true_peak)
        res = [restate(xs[i], GAINS[i], CEIL, true_peak) for i in range(xs.shape[0])]
        ys = np.stack([r[0] for r in res])
        ys.setflags(write=False)
        _expect[key] = (ys, [r[3] for r in res])
    return _expect[key]


def bad_streams(y, stats, want_y, want_stats):
    """streams whose samples (as bit patterns, a NaN matching a NaN) or statistics differ"""
    import float_domain_lib as FD
    if y.shape != want_y.shape:
        return list(range(want_y.shape[0]))
    return [i for i in range(want_y.shape[0]) if FD.floats_match(y[i], want_y[i]).any() or tuple(stats[i]) != tuple(want_stats[i])]
