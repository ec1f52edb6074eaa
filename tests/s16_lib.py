"""Inputs and comparisons of the 16-bit PCM input tests (TEST INFRASTRUCTURE: nothing under atracdenc_amd/ imports this module);
tools/emu/run_emu_s16.py uses the same inputs."""
import numpy as np


def widen(p16):
    """the definition of the 16-bit entry points: a sample s is the float (float)s * 0x1p-15f (exact, = s / 32768.0f)"""
    return np.ascontiguousarray(p16.astype(np.float32) * np.float32(2.0 ** -15))


def pcm16(n_streams, n, channels, seed, quiet=None):
    """int16 [n_streams][n][channels] from a fixed seed: noise over the full range with -32768 and 32767 planted in every stream
    and channel; with quiet=(a, b) the samples [a, b) of every stream are silence and a full-scale square burst of 200 samples
    follows them (what a transient detector reacts to)."""
    rng = np.random.RandomState(seed)
    x = rng.randint(-32768, 32768, size=(n_streams, n, channels)).astype(np.int16)
    x[:, 1 % n] = -32768
    x[:, 2 % n] = 32767
    if quiet is not None:
        a, b = quiet
        x[:, a:b] = 0
        t = np.arange(b, min(n, b + 200))
        x[:, b:b + 200] = np.where((t // 8) % 2 == 0, 32767, -32768).astype(np.int16)[None, :, None]
    return x


def square16(n, channels, period=6):
    """a full-scale square wave int16 [n][channels]: a band-limiting filter overshoots 1.0 on it"""
    t = np.arange(n)
    return np.repeat(np.where((t // (period // 2)) % 2 == 0, 32767, -32768).astype(np.int16)[:, None], channels, axis=1)


def out_s16_of(y):
    """the resampler's 16-bit output rule (AT3HIP_RESAMPLE_OUT_S16) of its float output y"""
    return np.rint(np.clip(y, np.float32(-1), np.float32(1)) * np.float32(32767)).astype(np.int16)


def same_bits(a, b):
    """equal shape, dtype and bit pattern"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()


def result_mismatches(a, b):
    """names of the fields in which two LoudnessResult differ (floats and doubles by bit pattern)"""
    bad = []
    for name, ctype in type(a)._fields_:
        x, y = getattr(a, name), getattr(b, name)
        if bytes(ctype(*x[:]) if hasattr(x, "__len__") else ctype(x)) != bytes(ctype(*y[:]) if hasattr(y, "__len__") else ctype(y)):
            bad.append(name)
    return bad
