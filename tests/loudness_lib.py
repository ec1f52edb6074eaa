"""Helpers of the loudness meter's tests (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * the C restatement tests/host/loudness_cpu.c (the definition of include/at3hip_loudness.h), compiled on first use into a
    temporary directory with gcc -O2 -ffp-contract=off -fno-fast-math: hops, peaks, gate, gain, measure.
  * prototype(): the analogue prototype the header quotes, evaluated with numpy at any rate.
  * the signals and call patterns that the GPU tests and the SIMT-harness driver share.
"""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPU_SRC = os.path.join(HERE, "host", "loudness_cpu.c")
HEADER = os.path.join(ROOT, "include", "at3hip_loudness.h")
CFLAGS = ["-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]
HOP = 4410

_cpu_so = None


class Result(ctypes.Structure):
    """at3hip_loudness_result / ld_result"""
    _fields_ = [("integrated", ctypes.c_double), ("momentary_max", ctypes.c_double), ("short_term_max", ctypes.c_double),
                ("sample_peak", ctypes.c_float * 2), ("true_peak", ctypes.c_float * 2), ("n_samples", ctypes.c_int64),
                ("n_hops", ctypes.c_int32), ("n_blocks_kept", ctypes.c_int32)]


FIELDS = [n for n, _ in Result._fields_]


def cpu_lib(outdir=None):
    """ctypes handle of the restatement (built once per process)."""
    global _cpu_so
    if _cpu_so is None:
        d = str(outdir or tempfile.mkdtemp(prefix="loudness_"))
        so = os.path.join(d, "libloudness_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, CPU_SRC, "-lm"])
        _cpu_so = so
    lib = ctypes.CDLL(_cpu_so)
    vp, i64, i32, resp = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(Result)
    lib.ld_coeffs.argtypes = [vp]
    lib.ld_hops.argtypes = [vp, i64, ctypes.c_int, vp]
    lib.ld_hops_warm.argtypes = [vp, i64, ctypes.c_int, vp, ctypes.c_int]
    lib.ld_hops_continuous.argtypes = [vp, i64, ctypes.c_int, vp]
    lib.ld_sample_peak.argtypes = [vp, i64, ctypes.c_int, vp]
    lib.ld_true_peak.argtypes = [vp, i64, ctypes.c_int, vp]
    lib.ld_tp_table.argtypes = [vp]
    lib.ld_gate.argtypes = [vp, i32, i32, resp]
    lib.ld_gate_opt.argtypes = [vp, i32, i32, resp, ctypes.c_int]
    lib.ld_gain.argtypes = [resp, ctypes.c_double, ctypes.c_double]
    lib.ld_gain.restype = ctypes.c_float
    lib.ld_measure.argtypes = [vp, i64, ctypes.c_int, ctypes.c_int, resp]
    return lib


def _pcm(x):
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 2 and x.shape[1] in (1, 2), x.shape
    return x


def coeffs():
    """the restatement's coefficients, float64 [2][5]: {b0, b1, b2, a1, a2} per stage"""
    out = np.zeros((2, 5), np.float64)
    cpu_lib().ld_coeffs(out.ctypes.data)
    return out


def header_coeffs():
    """the decimal literals of AT3HIP_KW_STAGE1 / AT3HIP_KW_STAGE2 in the header, float64 [2][5]"""
    text = open(HEADER).read()
    rows = []
    for name in ("AT3HIP_KW_STAGE1", "AT3HIP_KW_STAGE2"):
        body = re.search(r"#define " + name + r" \{([^}]*)\}", text).group(1)
        rows.append([float(v) for v in body.split(",")])
    return np.array(rows, np.float64)


def prototype(fs):
    """the analogue prototype of the header's comment at sample rate fs, float64 [2][5]"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    s1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
          (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    d = 1.0 + K / Q + K * K
    s2 = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d]
    return np.array([s1, s2], np.float64)


def hops(x, warm=2):
    """z float64 [T // 4410][C] of x [T][C]; warm = hops of warm-up (the definition: 2)"""
    x = _pcm(x)
    z = np.zeros((x.shape[0] // HOP, x.shape[1]), np.float64)
    cpu_lib().ld_hops_warm(x.ctypes.data, x.shape[0], x.shape[1], z.ctypes.data, int(warm))
    return z


def hops_continuous(x):
    x = _pcm(x)
    z = np.zeros((x.shape[0] // HOP, x.shape[1]), np.float64)
    cpu_lib().ld_hops_continuous(x.ctypes.data, x.shape[0], x.shape[1], z.ctypes.data)
    return z


def gate(z, relative=True):
    z = np.ascontiguousarray(z, np.float64)
    r = Result()
    cpu_lib().ld_gate_opt(z.ctypes.data, z.shape[0], z.shape[1], ctypes.byref(r), int(relative))
    return r


def gain(r, target, ceiling_db=-1.0):
    return np.float32(cpu_lib().ld_gain(ctypes.byref(r), float(target), float(ceiling_db)))


def measure(x, true_peak=False):
    """the restatement's result for the whole stream x [T][C]"""
    x = _pcm(x)
    r = Result()
    cpu_lib().ld_measure(x.ctypes.data, x.shape[0], x.shape[1], int(true_peak), ctypes.byref(r))
    return r


def result_bits(r):
    """every field of a result as raw bytes, by name (ctypes structures of either module)"""
    out = {}
    for n in FIELDS:
        v = getattr(r, n)
        if n in ("sample_peak", "true_peak"):
            out[n] = np.array(v[:], np.float32).tobytes()
        elif n in ("integrated", "momentary_max", "short_term_max"):
            out[n] = np.float64(v).tobytes()
        else:
            out[n] = int(v)
    return out


def results_equal(a, b):
    return result_bits(a) == result_bits(b)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- EBU Tech 3341 ------------------------------------------------------------------------------------------------------------
def tone_segments(segments, freq=1000.0, rate=44100):
    """in-phase stereo sine of `freq`, float32 [T][2]: segments [(dBFS of the amplitude, seconds)], one continuous phase"""
    n = [int(round(sec * rate)) for _, sec in segments]
    t = np.arange(sum(n), dtype=np.float64)
    amp = np.concatenate([np.full(k, 10.0 ** (db / 20.0)) for (db, _), k in zip(segments, n)])
    x = amp * np.sin(2.0 * np.pi * freq * t / rate)
    return np.ascontiguousarray(np.stack([x, x], axis=-1), np.float32)


EBU_3341 = [([(-23.0, 20.0)], -23.0),
            ([(-33.0, 20.0)], -33.0),
            ([(-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0)], -23.0),
            ([(-72.0, 10.0), (-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0), (-72.0, 10.0)], -23.0),
            ([(-26.0, 20.0), (-20.0, 20.1), (-26.0, 20.0)], -23.0)]


# ---- the inputs and call patterns of the GPU tests and of the SIMT-harness tests ----------------------------------------------
KINDS = ("noise", "sweep", "silence", "subnormal", "tone_dc")


def signal(kind, n, channels, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(n)
    if kind == "noise":
        x = rng.uniform(-1, 1, (n, channels))
    elif kind == "sweep":   # 20 Hz up to Nyquist, above full scale at its loudest
        f = 20 * (22050 / 20) ** (t / max(n, 1))
        ph = 2 * np.pi * np.cumsum(f) / 44100
        x = np.stack([1.2 * np.sin(ph + c) for c in range(channels)], axis=-1)
    elif kind == "silence":
        x = np.zeros((n, channels))
    elif kind == "subnormal":   # subnormals, signed zeros and the smallest normals
        x = rng.choice(np.array([1e-39, -1e-40, 1.4e-45, -0.0, 0.0, 1.2e-38, -3e-39], np.float32), (n, channels))
        x = x * rng.uniform(0.5, 1.5, (n, channels)).astype(np.float32)
    elif kind == "tone_dc":
        x = np.stack([0.3 * np.sin(2 * np.pi * (440.0 + 110.0 * c) * t / 44100) + 0.25 + 0.02 * rng.uniform(-1, 1, n)
                      for c in range(channels)], axis=-1)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, np.float32)


def random_cuts(rng, T, n):
    """sorted call ends in (0, T], the last one T; hop boundaries and their neighbours among them when they fit"""
    cuts = set(rng.randint(1, T + 1, n).tolist())
    for c in (HOP - 1, HOP, HOP + 1, 2 * HOP, 3 * HOP + 7):
        if c < T and rng.rand() < 0.5:
            cuts.add(c)
    cuts.add(T)
    return sorted(cuts)


def run_split(meter, xs, cuts):
    """xs [S][T][C] through `meter` (a HipLoudness) in calls ending at `cuts`; returns (hops [S][H][C], results)"""
    at = 0
    for cut in cuts:
        meter.process(xs[:, at:cut])
        at = cut
    z = meter.hops()
    return z, meter.finish()
