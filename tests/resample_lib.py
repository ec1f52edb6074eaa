"""Helpers of the resampler's tests (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module).

  * CpuResampler: one stream of the C restatement tests/host/resample_cpu.c (the definition of include/at3hip_resample.h),
    compiled on first use into a temporary directory with gcc -O2 -ffp-contract=off -fno-fast-math.
  * PAIRS: every supported (in, out) pair; shape / table: the restatement's (L, M, K) and hp[L][K].
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CPU_SRC = os.path.join(HERE, "host", "resample_cpu.c")
CFLAGS = ["-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]
OTHER_RATES = (8000, 11025, 16000, 22050, 24000, 32000, 48000, 88200, 96000, 176400, 192000)
PAIRS = [(r, 44100) for r in OTHER_RATES] + [(44100, r) for r in OTHER_RATES]

_cpu_so = None


def cpu_lib(outdir=None):
    """ctypes handle of the restatement (built once per process)."""
    global _cpu_so
    if _cpu_so is None:
        d = str(outdir or tempfile.mkdtemp(prefix="resample_"))
        so = os.path.join(d, "libresample_cpu.so")
        subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, CPU_SRC, "-lm"])
        _cpu_so = so
    lib = ctypes.CDLL(_cpu_so)
    i32p = ctypes.POINTER(ctypes.c_int32)
    lib.rs_shape.argtypes = [ctypes.c_int, ctypes.c_int, i32p, i32p, i32p]
    lib.rs_table.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.rs_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.rs_create.restype = ctypes.c_void_p
    lib.rs_destroy.argtypes = [ctypes.c_void_p]
    lib.rs_reset.argtypes = [ctypes.c_void_p]
    lib.rs_process.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.rs_process.restype = ctypes.c_int64
    lib.rs_flush.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.rs_flush.restype = ctypes.c_int64
    return lib


def shape(in_rate, out_rate):
    lib = cpu_lib()
    L, M, K = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    if lib.rs_shape(in_rate, out_rate, ctypes.byref(L), ctypes.byref(M), ctypes.byref(K)) != 0:
        raise ValueError(f"unsupported pair {in_rate} -> {out_rate}")
    return L.value, M.value, K.value


def table(in_rate, out_rate):
    L, _, K = shape(in_rate, out_rate)
    hp = np.zeros((L, K), np.float32)
    assert cpu_lib().rs_table(in_rate, out_rate, hp.ctypes.data) == 0
    return hp


def n_outputs(T, in_rate, out_rate):
    """ceil(T L / M): the outputs of a whole stream of T input samples"""
    L, M, _ = shape(in_rate, out_rate)
    return -(-T * L // M)


class CpuResampler:
    """One stream of the restatement; state carries across process() calls."""

    def __init__(self, in_rate, out_rate, channels):
        self.lib = cpu_lib()
        self.L, self.M, self.K = shape(in_rate, out_rate)
        self.channels = int(channels)
        self.h = self.lib.rs_create(in_rate, out_rate, self.channels)
        self._pending = 0   # input samples received since the start (bounds the output of the next call)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.rs_destroy(self.h)
            self.h = None

    def process(self, x):
        """x float32 [n][channels] -> the outputs this call emits, [m][channels]"""
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.channels)
        self._pending += x.shape[0]
        out = np.zeros((self._pending * self.L // self.M + 2, self.channels), np.float32)
        n = self.lib.rs_process(self.h, x.ctypes.data, x.shape[0], out.ctypes.data)
        return out[:n].copy()

    def flush(self):
        out = np.zeros((self._pending * self.L // self.M + 2, self.channels), np.float32)
        n = self.lib.rs_flush(self.h, out.ctypes.data)
        self._pending = 0
        return out[:n].copy()

    def whole(self, x):
        """the converted stream: one call and the flush"""
        a = self.process(x)
        return np.concatenate([a, self.flush()])


# ---- the inputs and call patterns of the GPU tests and of the SIMT-harness tests ----------------------------------------------
def signal(kind, n, channels, seed, rate=48000):
    rng = np.random.RandomState(seed)
    t = np.arange(n)
    if kind == "noise":
        x = rng.uniform(-1, 1, (n, channels))
    elif kind == "sweep":   # full scale, 20 Hz up to the rate's Nyquist
        f = 20 * (rate / 2 / 20) ** (t / n)
        ph = 2 * np.pi * np.cumsum(f) / rate
        x = np.stack([np.sin(ph + c) for c in range(channels)], axis=-1)
    elif kind == "silence":
        x = np.zeros((n, channels))
    elif kind == "subnormal":   # subnormals, signed zeros and the smallest normals
        x = rng.choice(np.array([1e-39, -1e-40, 1.4e-45, -0.0, 0.0, 1.2e-38, -3e-39], np.float32), (n, channels))
        x = x * rng.uniform(0.5, 1.5, (n, channels)).astype(np.float32)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, np.float32)


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def run_split(r, xs, cuts):
    """xs [S][T][C] through r in calls ending at `cuts`, then flush; checks n_out against the host-computed count"""
    L, M, K = r.L, r.M, r.K
    parts, at = [], 0
    for cut in cuts:
        got = r.process(xs[:, at:cut])
        a = cut - K // 2
        emitted = sum(p.shape[1] for p in parts)
        assert got.shape[1] == (-(-a * L // M) if a > 0 else 0) - emitted
        parts.append(got)
        at = cut
    tail = r.flush()
    assert tail.shape[1] == n_outputs(at, r.in_rate, r.out_rate) - sum(p.shape[1] for p in parts)
    parts.append(tail)
    return np.concatenate(parts, axis=1)
